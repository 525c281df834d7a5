"""The loop guard, the parts that need no GPU: the rule restated (loop_guard.first_loop) on named cases, trimmed, the
limits of LoopRule, the engine calls the scheduler makes for a request with a rule (over a fake engine that runs the rule), the server's
`loop_guard` field, and RowStage with ROW_LOOP against tests/loop_stage_model.cpp — a stand-alone program compiled with
-fsanitize=address,undefined and run directly."""
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

from dots_ocr_amd.config import DotsConfig
from dots_ocr_amd.engine import LogitRules, SamplingParams
from dots_ocr_amd.loop_guard import LoopRule, as_rule, first_loop, last_loop, trimmed
from dots_ocr_amd.row_features import FEATURES, ROW_FEATURES, rows_holding
from test_parallel_sampling_cpu import ForkEngine

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "dots_ocr_amd" / "csrc"


# ---------------------------------------------------------------------------------------------------- the rule

def _plant(head, block, copies):
    return list(head) + list(block) * copies


def test_period_one_two_and_three():
    rule = LoopRule(1, 8, 3, 0)
    assert first_loop(_plant([7, 8], [5], 10), rule) == (4, 1, 3)             # 7 8 5 5 5: the third 5
    assert first_loop(_plant([7, 8], [5, 6], 10), rule) == (7, 2, 6)
    assert first_loop(_plant([7, 8], [4, 5, 6], 10), rule) == (10, 3, 9)
    assert first_loop([1, 2, 3, 4, 5, 6, 7, 8, 9], rule) is None
    assert first_loop([], rule) is None


def test_min_span_dominating_and_repeats_dominating():
    ids = _plant([9], [1, 2], 40)
    assert first_loop(ids, LoopRule(1, 4, 3, 20)) == (20, 2, 20)             # L(2) = max(6, 20): twenty tokens of the cycle
    assert first_loop(ids, LoopRule(1, 4, 3, 4)) == (6, 2, 6)                # L(2) = max(6, 4): three copies
    assert first_loop(ids, LoopRule(1, 4, 3, 6)) == (6, 2, 6)                # equal
    # an odd span over an even period: the window need not hold whole copies
    assert first_loop(ids, LoopRule(1, 4, 2, 7)) == (7, 2, 7)
    assert LoopRule(1, 4, 3, 20).span(2) == 20 and LoopRule(1, 4, 3, 4).span(2) == 6


def test_a_break_at_any_position_of_the_window_delays_the_hit():
    rule = LoopRule(1, 3, 3, 0)
    clean = _plant([], [1, 2, 3], 8)
    assert first_loop(clean, rule) == (8, 3, 9)
    for at in range(9):                                                        # the window of the clean hit is [0, 8]
        ids = list(clean)
        ids[at] = 50
        hit = first_loop(ids, rule)
        # the cycle has to stand again behind the break: nine clean tokens from at + 1 on
        assert hit == (at + 9, 3, 9), (at, hit)
        assert first_loop(ids[:at + 9], rule) is None


def test_n_plus_one_equals_the_span_exactly():
    rule = LoopRule(1, 4, 2, 8)
    ids = [3, 4, 3, 4, 3, 4, 3, 4]
    assert first_loop(ids, rule) == (7, 2, 8) and first_loop(ids[:7], rule) is None
    assert first_loop([3] * 8, rule) == (7, 1, 8) and first_loop([3] * 7, rule) is None


def test_the_smallest_period_is_reported():
    ids = [1, 2] * 12
    assert first_loop(ids, LoopRule(1, 8, 2, 8)) == (7, 2, 8)                # periods 2 and 4 both fire at index 7 (L = 8 for both)
    assert first_loop(ids, LoopRule(3, 8, 2, 8)) == (7, 4, 8)                # without period 2: its multiple
    assert first_loop([5] * 20, LoopRule(2, 8, 3, 0)) == (5, 2, 6)            # a constant run under min_period 2


def test_last_loop_is_first_loop_at_the_row_s_end():
    g = np.random.default_rng(4)
    rule = LoopRule(1, 6, 2, 6)
    seen = 0
    for _ in range(200):
        ids = g.integers(0, 2, 40).tolist()
        hit = first_loop(ids, rule)
        if hit is None:
            assert last_loop(ids, rule) is None
            continue
        seen += 1
        assert last_loop(ids[:hit[0] + 1], rule) == hit
        assert all(last_loop(ids[:n + 1], rule) is None for n in range(hit[0]))
    assert seen > 100


def test_trimmed_keeps_one_copy_of_the_cycle():
    ids = _plant([9, 8], [1, 2, 3], 5)
    hit = first_loop(ids, LoopRule(1, 4, 3, 0))
    assert hit == (10, 3, 9)
    assert trimmed(ids[:11], hit) == [9, 8, 1, 2, 3]
    assert trimmed(ids, None) == ids
    hit = first_loop(_plant([9], [1, 2], 40), LoopRule(1, 4, 3, 21))          # a span that is no multiple of the period
    assert hit == (21, 2, 21) and trimmed(_plant([9], [1, 2], 40)[:22], hit) == [9, 1, 2]
    assert trimmed(np.asarray([5] * 12), (11, 1, 12)) == [5]


@pytest.mark.parametrize("bad", [(0, 4, 2, 0), (5, 4, 2, 0), (1, 1025, 2, 0), (1, 4, 1, 0), (1, 4, 65, 0), (1, 4, 2, -1), (1, 4, 2, 65536),
                                 (1, 4, 2.5, 0), (1, True, 2, 0), ("1", 4, 2, 0)])
def test_bad_rules_are_a_value_error(bad):
    with pytest.raises(ValueError):
        LoopRule(*bad)


def test_limits_are_inclusive_and_the_defaults_stand():
    LoopRule(1, 1, 2, 0)
    LoopRule(1024, 1024, 64, 65535)
    d = LoopRule()
    assert (d.min_period, d.max_period, d.repeats, d.min_span) == (1, 512, 4, 256)
    assert as_rule(True) == d and as_rule(None) is None and as_rule(False) is None and as_rule(d) is d
    assert as_rule({"max_period": 8, "min_span": 0}) == LoopRule(1, 8, 4, 0)
    for bad in ("yes", 3, {"period": 3}, {"repeats": 1}, [1, 2, 3, 4]):
        with pytest.raises(ValueError):
            as_rule(bad)
    # thirty empty cells of a legitimate table row: a cycle of three tokens over ninety, which the defaults let pass
    assert first_loop(_plant([1, 2, 3], [10, 11, 12], 30), d) is None


# ---------------------------------------------------------------------------------------------------- header, binding, feature table

def test_header_binding_and_feature_table_agree():
    from dots_ocr_amd import engine, loop_guard
    txt = (ROOT / "include" / "dots_ocr_hip.h").read_text()
    assert int(re.search(r"#define DOTS_MAX_LOOP_PERIOD (\d+)", txt).group(1)) == loop_guard.MAX_LOOP_PERIOD == 1024
    body = re.search(r"typedef struct DotsLoopRule \{(.*?)\} DotsLoopRule;", txt, re.S).group(1)
    fields = re.findall(r"int32_t (\w+);", body)
    assert fields == [n for n, _ in engine.CDotsLoopRule._fields_] == ["min_period", "max_period", "repeats", "min_span"]
    for name in ("dots_set_row_loop", "dots_row_loop_hit", "dots_loop_probe"):
        assert name in engine.EXPORTED_SYMBOLS
    for m in ("set_row_loop", "row_loop_hit", "loop_probe"):
        assert hasattr(engine.Engine, m)
    f = FEATURES["loop"]
    assert f.setter == "set_row_loop" and f.noun == "a loop guard" and f.off == (None,) and not f.token_bytes
    assert len(ROW_FEATURES) == 8
    stage = (CSRC / "row_stage.h").read_text()
    assert re.search(r"enum RowFeature \{[^}]*ROW_STOP, ROW_FEATURES, ROW_LOOP = ROW_FEATURES, ROW_ALL_FEATURES \}", stage)


# ---------------------------------------------------------------------------------------------------- the scheduler over a fake engine

class LoopEngine(ForkEngine):
    """ForkEngine + the loop guard as the engine defines it: the commit of a token that is no EOS checks the row's rule at that token and
    finishes the row at a hit; prefill and fork start the window over, a fork hands the source's rule to its children, release and reset
    clear the row.  Every set_row_loop, row_loop_hit, slots_prefill and slot_release is recorded in `trace`."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.loops, self.trace = {}, []

    def set_row_loop(self, row, rule):
        self.trace.append(("set_row_loop", row, rule))
        if rule is None:
            self.loops.pop(row, None)
        else:
            assert isinstance(rule, LoopRule)
            self.loops[row] = dict(rule=rule, hit=None)

    def set_row_logit_rules(self, row, rules):
        pass

    def row_loop_hit(self, row):
        self.trace.append(("row_loop_hit", row))
        return self.loops[row]["hit"] if row in self.loops else None

    def _advance(self, st):
        was = st["done"]
        super()._advance(st)
        slot = next((s for s, v in self.slots.items() if v is st), None)
        rl = self.loops.get(slot)
        if was or rl is None or st["out"][-1] in self.eos:
            return
        hit = last_loop(st["out"], rl["rule"])
        if hit is not None:
            rl["hit"] = hit
            st["done"] = True

    def _restart(self, s):
        if s in self.loops:
            self.loops[s]["hit"] = None
        super()._restart(s)

    def slots_prefill(self, slots, ids, lens, caps):
        self.trace.append(("slots_prefill", tuple(int(s) for s in slots)))
        super().slots_prefill(slots, ids, lens, caps)

    def slots_fork(self, src, dst):
        for d in dst:
            if src in self.loops:
                self.loops[d] = dict(self.loops[src], hit=None)
        super().slots_fork(src, dst)

    def slot_release(self, s):
        self.trace.append(("slot_release", int(s)))
        self.loops.pop(s, None)
        super().slot_release(s)

    def slots_reset(self):
        super().slots_reset()
        self.loops = {}


EOS = 9
RULE = LoopRule(1, 4, 3, 6)


def _script(prompt):
    """a prompt of 2s cycles over two ids to its cap; one of 3s says three tokens and ends; any other counts up and ends"""
    if prompt[0] == 2:
        return [30, 31] * 40
    if prompt[0] == 3:
        return [40, 41, 42, EOS]
    return list(range(50, 62)) + [EOS]


def _req(first, cap=40, **kw):
    from dots_ocr_amd.scheduler import Request
    return Request(np.full(5, first, np.int32), max_new_tokens=cap, **kw)


def _batcher(max_batch=2):
    from dots_ocr_amd.scheduler import ContinuousBatcher
    eng = LoopEngine(_script, 64, max_batch=max_batch, max_prefill_tokens=1024, max_seq_len=1024)
    return eng, ContinuousBatcher(eng, eos_ids=[EOS], chunk=4)


def test_the_batcher_sets_the_rule_before_the_prefill_and_reads_the_hit_before_the_release():
    eng, cb = _batcher()
    a, b = _req(2, loop=RULE), _req(4)
    outs = cb.run([a, b])
    assert outs[0].tolist() == [30, 31] * 3 and a.loop_hit == (5, 2, 6) == first_loop([30, 31] * 40, RULE)
    assert outs[1].tolist() == list(range(50, 62)) + [EOS] and not hasattr(b, "loop_hit")
    t = eng.trace
    slot = t[0][1]
    assert t[0] == ("set_row_loop", slot, RULE) and t[1][0] == "slots_prefill" and slot in t[1][1]       # set, then prefill
    hit_at, clear_at, rel_at = t.index(("row_loop_hit", slot)), t.index(("set_row_loop", slot, None)), t.index(("slot_release", slot))
    assert hit_at < clear_at < rel_at                                                                     # read, then cleared, then released
    assert [x for x in t if x[0] == "set_row_loop"] == [("set_row_loop", slot, RULE), ("set_row_loop", slot, None)]
    assert eng.loops == {} and rows_holding(cb._rows, "loop") == [] and not eng.slots
    # a request that ends by EOS before its rule could fire carries None; a slot reused without the rule holds none
    c, d = _req(3, loop=RULE), _req(2, cap=10)
    outs = cb.run([c, d])
    assert c.loop_hit is None and outs[0].tolist() == [40, 41, 42, EOS] and outs[1].tolist() == [30, 31] * 5 and not hasattr(d, "loop_hit")


def test_n_2_reports_one_hit_per_sequence():
    eng, cb = _batcher(max_batch=3)
    r = _req(2, loop=RULE, n=2, sampling=SamplingParams(temperature=1.0, seed=3))
    cb.run([r])
    assert r.loop_hit == [(5, 2, 6), (5, 2, 6)] and [o.tolist() for o in r.outputs] == [[30, 31] * 3] * 2
    assert eng.loops == {} and not eng.slots


def test_a_cancel_clears_the_row():
    eng, cb = _batcher()
    never = LoopRule(1, 4, 3, 500)
    rid = cb.submit(_req(2, cap=64, loop=never))
    cb.step()
    slot = next(iter(cb.running))
    assert eng.loops[slot]["rule"] == never and rows_holding(cb._rows, "loop") == [slot]
    assert cb.cancel(rid)
    done = cb.step()
    assert [r.cancelled for _, r, _ in done] == [True]
    assert eng.loops == {} and rows_holding(cb._rows, "loop") == [] and not eng.slots
    sets = [x for x in eng.trace if x[0] == "set_row_loop"]
    assert sets[0] == ("set_row_loop", slot, never) and sets[-1] == ("set_row_loop", slot, None)


def test_submit_refuses_what_cannot_be_honoured():
    from dots_ocr_amd.scheduler import ContinuousBatcher, RequestRejected
    from fakes import FakePagedEngine
    with pytest.raises(ValueError, match="set_row_loop"):
        ContinuousBatcher(FakePagedEngine(lambda p: [1], 8), chunk=2).submit(_req(2, loop=RULE))
    eng, cb = _batcher()
    eng.slots_score = eng.slots_extend = lambda *a, **k: None
    with pytest.raises(RequestRejected, match="loop guard"):
        cb.submit(_req(2, loop=RULE, score=[[5, 6]]))
    eng.slots_beam = lambda *a, **k: None
    with pytest.raises(RequestRejected, match="loop guard"):
        cb.submit(_req(2, loop=RULE, num_beams=2))


# ---------------------------------------------------------------------------------------------------- the server over a fake engine

TEXTS = {0: "ab" * 30, 1: "no cycle here."}


class _LoopModel:
    """a completion spells TEXTS[seed % 2] and ends by EOS; generate() is the static path's: it honours loop_guard as the engine would"""

    def __init__(self, proc, cfg):
        self.config, self.proc = cfg, proc
        model = self

        def script(prompt):
            e = model.engine
            p = e.rows.get(e.cur)
            return proc.tokenizer.encode(TEXTS[(0 if p is None else p.seed) % 2]) + [cfg.eos_token_ids[0]]
        self.engine = LoopEngine(script, 256, max_batch=3, max_patches=4096, max_prefill_tokens=4096, max_seq_len=2048)
        self.engine.slots_drain = None                     # present: the streaming path is refused for other reasons on this fake
        del self.engine.slots_drain
        self.generate_kw = []

    def generate(self, input_ids=None, seed=0, loop_guard=None, max_new_tokens=40, **kw):
        self.generate_kw.append(dict(kw, loop_guard=loop_guard))
        new = (self.proc.tokenizer.encode(TEXTS[seed % 2]) + [self.config.eos_token_ids[0]])[:max_new_tokens]
        hit = first_loop(new[:-1], loop_guard) if loop_guard is not None else None
        if hit is not None:
            new = new[:hit[0] + 1] + [self.config.pad_token_id] * (len(new) - hit[0] - 1)
        return torch.cat([input_ids, torch.tensor(new)[None].repeat(input_ids.shape[0], 1)], dim=1)


def _payload(**kw):
    body = {"model": "model", "messages": [{"role": "user", "content": "Read this."}], "max_completion_tokens": 80, "temperature": 0.8, "seed": 10}
    body.update(kw)
    return body


def _app(**kw):
    pytest.importorskip("fastapi")
    from dots_ocr_amd.processing import DotsOcrProcessor
    from dots_ocr_amd.server import create_app
    cfg = DotsConfig.tiny()
    proc = DotsOcrProcessor(cfg)
    model = _LoopModel(proc, cfg)
    return model, proc, create_app(model, proc, model_name="model", max_batch=3, **kw)


GUARD = {"max_period": 4, "repeats": 3, "min_span": 8}


@pytest.mark.parametrize("continuous", [True, False])
def test_server_reports_repetition(continuous):
    from fastapi.testclient import TestClient
    model, proc, app = _app(continuous=continuous)
    with TestClient(app) as c:
        r = c.post("/v1/chat/completions", json=_payload(loop_guard=GUARD))
        assert r.status_code == 200, r.text
        d = r.json()
        ch = d["choices"][0]
        assert ch["finish_reason"] == "repetition" and ch["repetition"] == {"period": 2, "span": 8}
        assert ch["message"]["content"] == "ab" * 4 and d["usage"]["completion_tokens"] == 8
        d = c.post("/v1/chat/completions", json=_payload(loop_guard=GUARD, seed=11)).json()       # no cycle: the EOS ends it
        ch = d["choices"][0]
        assert ch["finish_reason"] == "stop" and "repetition" not in ch and ch["message"]["content"] == TEXTS[1]
        d = c.post("/v1/chat/completions", json=_payload(loop_guard=True)).json()                 # the defaults: 256 tokens, never reached
        assert d["choices"][0]["finish_reason"] == "stop" and d["choices"][0]["message"]["content"] == TEXTS[0]
        plain = c.post("/v1/chat/completions", json=_payload()).json()                            # without the field: today's keys
        assert sorted(plain["choices"][0]) == ["finish_reason", "index", "message"] and plain["choices"][0]["message"]["content"] == TEXTS[0]
        for off in (None, False):
            assert sorted(c.post("/v1/chat/completions", json=_payload(loop_guard=off)).json()["choices"][0]) == ["finish_reason", "index", "message"]
        for bad in ("yes", 3, {"period": 3}, {"repeats": 1}, {"max_period": 1025}, {"min_span": -1}, {"min_period": 5, "max_period": 4}, [1]):
            r = c.post("/v1/chat/completions", json=_payload(loop_guard=bad))
            assert r.status_code == 400 and "loop_guard" in r.text, (bad, r.text)
    if continuous:
        assert not model.engine.slots and model.engine.loops == {} and model.engine.kv_pool_info() == (256, 256)
    else:
        assert model.generate_kw[0]["loop_guard"] == LoopRule(1, 4, 3, 8) and model.generate_kw[3]["loop_guard"] is None


def test_server_refuses_the_field_with_beam_and_score_by_name():
    from fastapi.testclient import TestClient
    from dots_ocr_amd.server import BEAM_FORBIDDEN, SCORE_FORBIDDEN
    assert "loop_guard" in BEAM_FORBIDDEN and "loop_guard" in SCORE_FORBIDDEN
    model, proc, app = _app()
    model.engine.slots_beam = model.engine.slots_score = model.engine.slots_extend = lambda *a, **k: None
    with TestClient(app) as c:
        r = c.post("/v1/chat/completions", json=_payload(loop_guard=True, use_beam_search=True, n=2, temperature=0.0))
        assert r.status_code == 400 and "loop_guard" in r.text and "beam" in r.text
        r = c.post("/v1/chat/completions", json=_payload(loop_guard=GUARD, score_candidates=["ab"]))
        assert r.status_code == 400 and "loop_guard" in r.text and "score" in r.text


def test_server_n_2_reports_each_choice_s_own_end():
    from fastapi.testclient import TestClient
    model, proc, app = _app()
    with TestClient(app) as c:
        d = c.post("/v1/chat/completions", json=_payload(loop_guard=GUARD, n=2)).json()          # seeds 10 and 11: one cycles, one does not
        a, b = d["choices"]
        assert (a["message"]["content"], a["finish_reason"], a["repetition"]) == ("ab" * 4, "repetition", {"period": 2, "span": 8})
        assert (b["message"]["content"], b["finish_reason"]) == (TEXTS[1], "stop") and "repetition" not in b
    assert not model.engine.slots and model.engine.loops == {}


# ---------------------------------------------------------------------------------------------------- generate() and the parser

def test_generate_and_parser_take_the_keyword():
    import inspect
    from dots_ocr_amd.modeling import CallSettings, DotsOcrHipForCausalLM
    from dots_ocr_amd.parser import DotsOCRParser, PageText
    assert inspect.signature(DotsOcrHipForCausalLM.generate).parameters["loop_guard"].default is None
    assert CallSettings().loop is None
    assert inspect.signature(DotsOCRParser.__init__).parameters["loop_guard"].default is None

    class _Tok:
        pad_token_id = 0

    class _Proc:
        tokenizer = _Tok()
    p = DotsOCRParser.__new__(DotsOCRParser)
    p.loop_guard, p.processor = LoopRule(1, 4, 3, 6), _Proc()
    rows = [torch.tensor([7, 1, 2, 1, 2, 1, 2, 0, 0]), torch.tensor([7, 8, 9, 10, 11, 12, 13, 14, 0])]
    cut, hits = p._cut_loops(rows)
    assert hits == [(6, 2, 6), None] and cut[0].tolist() == [7, 1, 2] and cut[1] is rows[1]
    marked = p._mark_loops(["x", "y"], hits)
    assert isinstance(marked[0], PageText) and marked[0].repetition == {"period": 2, "span": 6} and marked[0] == "x"
    assert type(marked[1]) is str
    assert p._loop_field() == {"loop_guard": {"min_period": 1, "max_period": 4, "repeats": 3, "min_span": 6}}
    p.loop_guard = None
    assert p._loop_field() == {} and p._cut_loops(rows) == (rows, [None, None])
    with pytest.raises(ValueError):
        DotsOCRParser(loop_guard=True, num_beams=2, model=object(), processor=_Proc())
    with pytest.raises(ValueError):
        DotsOCRParser(loop_guard={"repeats": 1}, model=object(), processor=_Proc())


# ---------------------------------------------------------------------------------------------------- RowStage with ROW_LOOP

def test_a_loop_row_never_speculates(tmp_path):
    cxx = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    assert cxx, "no C++ compiler (c++, g++ or clang++) on PATH"
    max_batch = re.search(r"^#define DOTS_MAX_BATCH (\d+)", (CSRC / "kernels.h").read_text(), re.M).group(1)
    exe = tmp_path / "loop_stage_model"
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", f"-DDOTS_MAX_BATCH={max_batch}",
           f"-I{CSRC}", str(ROOT / "tests" / "loop_stage_model.cpp"), "-o", str(exe)]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert re.search(r"(\d+) cases, 0 failures", p.stdout) and int(re.search(r"(\d+) cases", p.stdout).group(1)) >= 3 * 2 * 64 * 2 * 64
