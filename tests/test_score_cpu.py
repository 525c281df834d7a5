"""Scoring given tokens without a GPU: the row plan (csrc/score_plan.h) held to the brute-force statement of
tests/score_plan_model.cpp, the scheduler's Request(score=...) over a fake paged engine that forks, extends and scores, the server's
`score_candidates` field, the parser's score_image, the Python binding's packing and the C-ABI symbols."""
import ctypes as C
import math
import re
import shutil
import subprocess
import types
from pathlib import Path

import numpy as np
import pytest

from dots_ocr_amd.config import DotsConfig
from dots_ocr_amd.engine import SamplingParams
from fakes import FakePagedEngine

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "dots_ocr_amd" / "csrc"
EOS = 9
K = 20


# ---------------------------------------------------------------------------------------------------- the row plan

@pytest.mark.parametrize("flags", [(), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g")], ids=["plain", "asan-ubsan"])
def test_row_plan_matches_the_brute_force_statement(tmp_path, flags):
    cxx = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    assert cxx, "no C++ compiler (c++, g++ or clang++) on PATH"
    exe = tmp_path / "score_plan_model"
    cmd = [cxx, "-std=c++17", "-O1", "-Wall", "-Werror", *flags, f"-I{CSRC}", str(ROOT / "tests" / "score_plan_model.cpp"), "-o", str(exe)]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    m = re.search(r"(\d+) checks, 0 mismatches", p.stdout)
    assert m and int(m.group(1)) > 100000, p.stdout                    # 2 x (10 + 100 + 1000) calls, every row of each


# ---------------------------------------------------------------------------------------------------- the fake engine

def _fake_scores(fed, top_n):
    """what the fake engine records for one fed list: values that spell the target ids, so that an order or a split gone wrong shows"""
    m = len(fed) - 1
    tok = np.asarray([-(int(t) % 97) / 8.0 - 0.25 for t in fed[1:]], np.float32)
    ids = np.full((m, K), -1, np.int32)
    top = np.full((m, K), np.nan, np.float32)
    for j in range(m):
        ids[j, :top_n] = np.arange(top_n) + int(fed[j + 1])
        top[j, :top_n] = -np.arange(top_n, dtype=np.float32) / 4
    return tok, ids, top


class ScoreEngine(FakePagedEngine):
    """FakePagedEngine + slots_fork / slots_extend / slots_score as the engine defines them.  A fork child shares the source's
    floor(L / 64) full prompt pages; an extend or a score appends ids behind the slot's prompt, grows the slot to the admission reserve of
    the longer prompt and restarts its output; a score also returns one record per slot."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.rows, self.fresh, self.groups, self.spec_k = {}, set(), {}, 0

    def set_row_sampling(self, row, params):
        if params is None:
            self.rows.pop(row, None)
        else:
            self.rows[row] = params

    def _admit(self, prompt, cap):
        return (min(prompt + min(cap, 64), self.max_seq_len) + 63) // 64

    def _restart(self, s):
        st = self.slots[s]
        st.update(plan=list(self.script(st["prompt"])), out=[], done=False)
        self._advance(st)

    def slots_reset(self):
        super().slots_reset()
        self.fresh, self.groups = set(), {}

    def slots_prefill(self, slots, ids, lens, caps):
        super().slots_prefill(slots, ids, lens, caps)
        self.fresh = set(slots)

    def slots_decode(self, n):
        self.fresh = set()
        super().slots_decode(n)

    def slots_fork(self, src, dst):
        assert src in self.fresh and src in self.slots, "only a freshly prefilled sequence can be forked"
        assert len(set(dst)) == len(dst) and all(0 <= d < self.max_batch and d not in self.slots for d in dst)
        p = self.slots[src]
        L, shared = len(p["prompt"]), len(p["prompt"]) // 64
        own = self._admit(L, p["limit"] - L) - shared
        if own * len(dst) > self.free:
            raise RuntimeError("KV pool exhausted")
        key = p.setdefault("group", ("group", src, len(self.log)))
        self.groups[key] = self.groups.get(key, 1) + len(dst)
        for d in dst:
            self.slots[d] = dict(prompt=p["prompt"].copy(), cap=p["limit"] - L, pages=shared + own, limit=p["limit"], ctx=L, group=key, shared=shared)
            self.free -= own
            self._restart(d)
        p["shared"] = shared
        self.log.append(("fork", src, tuple(dst)))

    def _extend(self, kind, slots, ids_list, keep_pending, max_new_tokens):
        assert not keep_pending
        assert len(set(slots)) == len(slots) == len(ids_list) and all(s in self.slots for s in slots) and all(len(x) >= 1 for x in ids_list)
        lacking = [max(0, self._admit(len(self.slots[s]["prompt"]) + len(x), max_new_tokens) - self.slots[s]["pages"]) for s, x in zip(slots, ids_list)]
        if sum(lacking) > self.free:
            raise RuntimeError("KV pool exhausted")
        before = tuple(tuple(int(t) for t in self.slots[s]["prompt"]) for s in slots)
        for s, x, more in zip(slots, ids_list, lacking):
            st = self.slots[s]
            st["prompt"] = np.concatenate([st["prompt"], np.asarray(x, st["prompt"].dtype)])
            st.update(pages=st["pages"] + more, cap=int(max_new_tokens), limit=len(st["prompt"]) + int(max_new_tokens), ctx=len(st["prompt"]))
            self.free -= more
            self._restart(s)
        self.fresh = set()
        self.log.append((kind, tuple(slots), tuple(tuple(x) for x in ids_list), before))

    def slots_extend(self, slots, ids_list, keep_pending=False, max_new_tokens=1):
        self._extend("extend", slots, ids_list, keep_pending, max_new_tokens)

    def slots_score(self, slots, ids_list, top_n=0, keep_pending=False, max_new_tokens=1):
        assert 0 <= int(top_n) <= K
        self._extend("score", slots, ids_list, keep_pending, max_new_tokens)
        self.log[-1] = self.log[-1] + (int(top_n), self.kv_pool_info()[1])
        return [_fake_scores(x, int(top_n)) for x in ids_list]

    def slot_release(self, s):
        st = self.slots[s]
        key = st.get("group")
        if key is not None:
            self.groups[key] -= 1
            if self.groups[key] > 0:
                self.free -= st["shared"]            # other rows still hold the shared pages: they stay out of the pool
        self.rows.pop(s, None)
        self.log.append(("release", s))
        super().slot_release(s)


def _seq(prompt):
    return [int(prompt[-1]) * 1000 + len(prompt)] * 3 + [EOS]


def _engine(pool_pages=64, max_batch=8, cls=ScoreEngine, **kw):
    return cls(_seq, pool_pages, max_batch=max_batch, max_prefill_tokens=1024, max_seq_len=1024, **kw)


def _req(first, L=70, cap=40, **kw):
    from dots_ocr_amd.scheduler import Request
    return Request(np.full(L, first, np.int32), max_new_tokens=cap, **kw)


def _same(a, b):
    return all(np.array_equal(x, y, equal_nan=True) and x.dtype == y.dtype for x, y in zip(a, b))


# ---------------------------------------------------------------------------------------------------- scheduler

def test_a_score_request_takes_one_prefill_one_fork_one_score_and_no_decode_step():
    from dots_ocr_amd.scheduler import ContinuousBatcher
    eng = _engine()
    cands = [[11, 12, 13], [21], [31, 32, 33, 34, 35]]
    r = _req(7, score=cands, score_top_logprobs=4)
    r.pixel_values, r.grid_thw = np.zeros((16, 4), np.float32), np.array([[1, 4, 4]], np.int64)
    cb = ContinuousBatcher(eng, eos_ids=(EOS,), chunk=2)
    outs = cb.run([r])
    kinds = [ev[0] for ev in eng.log]
    assert kinds == ["vit", "prefill", "fork", "score", "release", "release", "release"]      # one of each and no decode step at all
    assert eng.log[1] == ("prefill", (0,)) and eng.log[2] == ("fork", 0, (1, 2))
    sc = eng.log[3]
    assert sc[1] == (0, 1, 2) and sc[2] == tuple(tuple(c) for c in cands) and sc[4] == 4
    assert all(len(p) == 70 for p in sc[3])                            # every slot held the prefix alone
    assert len(r.scores_out) == 3
    for got, c in zip(r.scores_out, cands):                            # in candidate order
        assert _same(got, _fake_scores(c, 4)) and got[0].shape == (len(c) - 1,)
    assert [o.tolist() for o in r.outputs] == [[], [], []] and outs[0].tolist() == []
    assert r.max_new_tokens == 1 and r.kv_truncated is False
    assert cb.admissions == 1 and cb.decode_steps == 0 and cb.idle
    assert eng.kv_pool_info() == (64, 64) and not eng.slots and not cb.running


def test_one_candidate_needs_no_fork_and_runs_beside_a_generating_request():
    from dots_ocr_amd.scheduler import ContinuousBatcher
    eng = _engine()
    alone = ContinuousBatcher(eng, eos_ids=(EOS,), chunk=2).run([_req(5, L=10)])[0].tolist()
    eng.log.clear()
    r, other = _req(7, score=[[41, 42]]), _req(5, L=10)
    cb = ContinuousBatcher(eng, eos_ids=(EOS,), chunk=2)
    outs = cb.run([r, other])
    kinds = [ev[0] for ev in eng.log]
    assert "fork" not in kinds and kinds.count("score") == 1
    assert kinds.index("score") < kinds.index("release") < kinds.index("decode")      # the scored slot is back before anything decodes
    assert eng.log[kinds.index("release")] == ("release", 0)
    assert _same(r.scores_out[0], _fake_scores([41, 42], 0))
    assert outs[0].tolist() == [] and outs[1].tolist() == alone == _seq([5] * 10)      # the generating request is undisturbed
    assert eng.kv_pool_info() == (64, 64) and not eng.slots


def test_page_accounting_is_that_of_suffixes_with_one_new_token():
    from dots_ocr_amd.scheduler import ContinuousBatcher
    # prefix 70 (one full page shared), cap forced to 1: candidates of 3 / 58 / 60 tokens end at 73 / 128 / 130 -> + 1 ahead: 2 / 3 / 3 pages
    cands = [[1] * 3, [2] * 58, [3] * 60]
    eng = _engine(pool_pages=6)
    cb = ContinuousBatcher(eng, eos_ids=(EOS,), chunk=2)
    r = _req(7, cap=500, score=cands)
    cb.submit(r)
    assert r.max_new_tokens == 1
    assert cb._group_pages(r) == 2 + 3 + 3 - 2 == 6
    assert cb._worst_pages(r) == (74 + 63) // 64 + (129 + 63) // 64 + (131 + 63) // 64 - 2 == 6
    same = _req(7, cap=1, suffixes=cands)
    cb2 = ContinuousBatcher(_engine(pool_pages=6), eos_ids=(EOS,))
    cb2.submit(same)
    assert cb2._group_pages(same) == cb._group_pages(r) and cb2._worst_pages(same) == cb._worst_pages(r)
    cb.step()
    sc = [ev for ev in eng.log if ev[0] == "score"][0]
    assert sc[5] == 0                                                  # all six pages were in use when the score ran
    assert cb.idle and eng.kv_pool_info() == (6, 6)
    with pytest.raises(ValueError, match="KV pages"):                  # a pool one page short never admits it
        ContinuousBatcher(_engine(pool_pages=5), eos_ids=(EOS,)).submit(_req(7, score=cands))


def test_score_refusals_are_raised_at_submit_and_name_the_setting():
    from dots_ocr_amd.engine import LogitRules, NgramRule
    from dots_ocr_amd.scheduler import ContinuousBatcher, RequestRejected
    eng = _engine()
    cb = ContinuousBatcher(eng, eos_ids=(EOS,))
    one = [[1, 2]]
    for kw, what in ((dict(score=one, n=2), "n > 1"), (dict(score=one, num_beams=2), "num_beams"),
                     (dict(score=one, suffixes=[[1], [2]]), "suffixes"),
                     (dict(score=one, sampling=SamplingParams(temperature=0.7)), "sampling parameters"),
                     (dict(score=one, sampling=SamplingParams(repetition_penalty=1.2)), "sampling parameters"),
                     (dict(score=one, guide=3), "a guide"), (dict(score=one, rules=LogitRules(stop=(5,))), "logit rules"),
                     (dict(score=one, ngram=NgramRule(3)), "n-gram rule"), (dict(score=one, stop=["x"]), "stop strings"),
                     (dict(score=one, logprobs=2), "logprobs"), (dict(score=one, score_top_logprobs=21), r"\[0, 20\]"),
                     (dict(score=one, score_top_logprobs=-1), r"\[0, 20\]"), (dict(score=one, score_top_logprobs=True), r"\[0, 20\]"),
                     (dict(score=[[1], []]), "empty"), (dict(score=[]), "1 .. 8"), (dict(score=[[1]] * 9), "1 .. 8")):
        with pytest.raises(RequestRejected, match=what):
            cb.submit(_req(7, **kw))
    assert not cb.pending and not eng.log
    eng.spec_k = 2
    with pytest.raises(RequestRejected, match="speculates"):
        ContinuousBatcher(eng, eos_ids=(EOS,)).submit(_req(7, score=one))
    eng.spec_k = 0
    with pytest.raises(RequestRejected, match="static batching"):      # no slots_score: static batching
        ContinuousBatcher(_engine(cls=FakePagedEngine), eos_ids=(EOS,)).submit(_req(7, score=one))
    eng.cfg = types.SimpleNamespace(vocab_size=4000)
    with pytest.raises(RequestRejected, match="outside"):
        ContinuousBatcher(eng, eos_ids=(EOS,)).submit(_req(7, score=[[1], [4000]]))
    with pytest.raises(ValueError, match="max_seq_len"):
        ContinuousBatcher(eng, eos_ids=(EOS,)).submit(_req(7, L=1000, score=[[1] * 30]))
    cb.submit(_req(7, score=one, score_top_logprobs=20))               # and the plain one goes in
    assert len(cb.pending) == 1


def test_a_failed_score_gives_its_slots_back():
    from dots_ocr_amd.scheduler import ContinuousBatcher

    class Failing(ScoreEngine):
        def slots_score(self, *a, **kw):
            raise RuntimeError("score failed")
    eng = _engine(cls=Failing)
    cb = ContinuousBatcher(eng, eos_ids=(EOS,))
    cb.submit(_req(7, score=[[1, 2], [3]]))
    with pytest.raises(RuntimeError, match="score failed"):
        cb.step()
    assert not eng.slots and eng.kv_pool_info() == (64, 64) and len(cb.pending) == 1 and not cb.running


# ---------------------------------------------------------------------------------------------------- binding and C ABI

def test_engine_slots_score_packs_its_lists_and_reads_the_entries():
    from dots_ocr_amd import engine
    calls, reads = [], []

    def score(h, slots, n, ids, lens, keep, cap, top):
        tot = sum(lens[i] for i in range(n))
        calls.append(([slots[i] for i in range(n)], [ids[i] for i in range(tot)], [lens[i] for i in range(n)], [keep[i] for i in range(n)],
                      [cap[i] for i in range(n)], [top[i] for i in range(n)]))
        return 0

    def scores(h, slot, pos0, n, tok, ids, top, n_out):
        reads.append((slot, pos0, n))
        n_out._obj.value = 3
        for j in range(n):
            tok[j] = -1.0 - slot - j
            for k in range(K):
                ids[j * K + k], top[j * K + k] = slot * 100 + j, -0.5 * k
        return 0
    e = engine.Engine.__new__(engine.Engine)
    e.lib, e.h = types.SimpleNamespace(dots_slots_score=score, dots_slot_scores=scores), None
    out = e.slots_score([4, 1], [[7, 8, 9, 6], [5, 2, 3, 4]], top_n=[3, 0], keep_pending=False, max_new_tokens=24)
    assert calls[0] == ([4, 1], [7, 8, 9, 6, 5, 2, 3, 4], [4, 4], [0, 0], [24, 24], [3, 0])
    assert reads == [(4, 0, 0), (4, 0, 3), (1, 0, 0), (1, 0, 3)]       # first how many, then the entries
    assert len(out) == 2 and out[0][0].tolist() == [-5.0, -6.0, -7.0] and out[1][1].shape == (3, K) and out[1][1][2, 0] == 102
    e.slots_score([2], [[1]], top_n=5, keep_pending=True)
    assert calls[1] == ([2], [1], [1], [1], [1], [5])
    reads.clear()
    tok, ids, top = e.slot_scores(6, n=2, pos0=1)
    assert reads == [(6, 1, 2)] and tok.shape == (2,) and ids.shape == (2, K) and top.shape == (2, K)


def test_score_symbols_are_exported_and_declared():
    from dots_ocr_amd import _lib, engine
    lib = _lib.load()
    header = (ROOT / "include" / "dots_ocr_hip.h").read_text()
    for sym in ("dots_slots_score", "dots_slot_scores"):
        assert sym in engine.EXPORTED_SYMBOLS and hasattr(lib, sym)
        assert re.search(rf"^int {sym}\(DotsEngine\* e,", header, re.M)
    assert "Refused with nothing changed, as dots_slots_extend" in header and "top_n outside [0, 20]" in header
    i32p = C.POINTER(C.c_int32)
    lib.dots_slots_score.restype = C.c_int32
    lib.dots_slots_score.argtypes = [C.c_void_p, i32p, C.c_int32, i32p, i32p, i32p, i32p, i32p]
    one = (C.c_int32 * 1)(0)
    assert lib.dots_slots_score(None, one, 1, one, one, one, one, one) == -1               # no engine: refused before anything is touched
    lib.dots_slot_scores.restype = C.c_int32
    lib.dots_slot_scores.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, i32p]
    assert lib.dots_slot_scores(None, 0, 0, 0, None, None, None, one) == -1
    kernels = (CSRC / "kernels.h").read_text()
    src = (CSRC / "score.hip").read_text()
    for k in ("score_logprob_partial_kernel", "score_logprob_final_kernel", "lp_partial_chunk(", "lp_final_entry("):
        assert k in src
    assert "launch_score_logprob_partial" in kernels and "launch_score_logprob_final" in kernels
    assert (CSRC / "score_plan.h").exists() and '#include "score_plan.h"' in (CSRC / "slots.hip").read_text()
    # the shared reductions are called, not restated: score.hip holds no reduction of its own
    assert "expf" not in src and "__shfl" not in src and "logf" not in src
    # one routine serves the extend and the score
    slots = (CSRC / "slots.hip").read_text()
    assert slots.count("extend_slots(e, \"dots_slots_") == 2


# ---------------------------------------------------------------------------------------------------- server

fastapi = pytest.importorskip("fastapi")


class _SlotModel:
    def __init__(self, cfg, cls=ScoreEngine):
        self.config = cfg
        self.engine = cls(lambda prompt: [65, 66, cfg.eos_token_ids[0]], 4096, max_batch=8, max_patches=4096, max_prefill_tokens=4096, max_seq_len=2048)


def _payload(page, **kw):
    from dots_ocr_amd.image_utils import PILimage_to_base64
    body = {"model": "model", "messages": [{"role": "user", "content": [
        {"type": "image_url", "image_url": {"url": PILimage_to_base64(page)}},
        {"type": "text", "text": "<|img|><|imgpad|><|endofimg|>Which language is this page in?"}]}]}
    body.update(kw)
    return body


def test_server_score_candidates_field():
    from fastapi.testclient import TestClient
    from dots_ocr_amd.processing import DotsOcrProcessor
    from dots_ocr_amd.server import create_app
    from dots_ocr_amd.synthetic import synth_page
    cfg = DotsConfig.tiny()
    proc = DotsOcrProcessor(cfg)
    model = _SlotModel(cfg)
    eng = model.engine
    page = synth_page(0, (140, 84))
    n_img = (84 // 14) * (140 // 14) // 4
    cands = ["en", "de-CH", "zh"]
    P = proc(text=[proc.apply_chat_template([{"role": "user", "content": [{"type": "image", "image": page},
                                                                          {"type": "text", "text": "Which language is this page in?"}]}],
                                            tokenize=False, add_generation_prompt=True)], images=[page])["input_ids"][0].tolist()
    eos = cfg.eos_token_ids[0]
    with TestClient(create_app(model, proc, model_name="model", max_batch=8)) as c:
        r = c.post("/v1/chat/completions", json=_payload(page, score_candidates=cands, top_logprobs=2))
        assert r.status_code == 200, r.text
        d = r.json()
        kinds = [ev[0] for ev in eng.log if ev[0] in ("vit", "prefetch", "prefill", "fork", "score", "extend", "decode")]
        assert kinds.count("prefill") == 1 and kinds.count("fork") == 1 and kinds.count("score") == 1 and "decode" not in kinds and "extend" not in kinds
        assert kinds.count("vit") + kinds.count("prefetch") == 1       # the page went through the tower once
        sc = [ev for ev in eng.log if ev[0] == "score"][0]
        fed = [[P[-1]] + list(c_.encode()) + [eos] for c_ in cands]    # the synthetic tokenizer's ids are the UTF-8 bytes
        assert [list(x) for x in sc[2]] == fed and sc[4] == 2
        assert all(list(p) == P[:-1] for p in sc[3])                   # the prefix is P[:-1]: every image token lies in it
        assert P[:-1].count(cfg.image_token_id) == n_img and not eng.slots
        # one choice per candidate, in order, in the shape the server emits for generated tokens
        assert [ch["index"] for ch in d["choices"]] == [0, 1, 2]
        for ch, cand, x in zip(d["choices"], cands, fed):
            want = _fake_scores(x, 2)
            assert ch["message"] == {"role": "assistant", "content": cand} and ch["finish_reason"] == "scored"
            content = ch["logprobs"]["content"]
            assert len(content) == len(cand.encode()) + 1              # every candidate token and the EOS
            assert [e["bytes"] for e in content[:-1]] == [[b] for b in cand.encode()]
            assert content[-1]["token"] == proc.tokenizer.decode([eos], skip_special_tokens=False)
            assert [e["logprob"] for e in content] == [float(v) for v in want[0]]
            assert all(set(e) == {"token", "logprob", "bytes", "top_logprobs"} and len(e["top_logprobs"]) == 2 for e in content)
            assert [t["logprob"] for t in content[0]["top_logprobs"]] == [0.0, -0.25]
            assert ch["cumulative_logprob"] == float(want[0].astype(np.float64).sum())
        assert d["usage"] == {"prompt_tokens": len(P) - 1 + sum(len(x) for x in fed), "completion_tokens": 0,
                              "total_tokens": len(P) - 1 + sum(len(x) for x in fed)}
        # score_eos: false, one candidate, no top lists
        eng.log.clear()
        d = c.post("/v1/chat/completions", json=_payload(page, score_candidates=["en"], score_eos=False)).json()
        sc = [ev for ev in eng.log if ev[0] == "score"][0]
        assert [list(x) for x in sc[2]] == [[P[-1]] + list(b"en")] and sc[4] == 0 and not [ev for ev in eng.log if ev[0] == "fork"]
        assert len(d["choices"]) == 1 and len(d["choices"][0]["logprobs"]["content"]) == 2 and d["choices"][0]["logprobs"]["content"][0]["top_logprobs"] == []
        assert math.isclose(d["choices"][0]["cumulative_logprob"], sum(e["logprob"] for e in d["choices"][0]["logprobs"]["content"]))
        # every conflicting field is a 400 that names it
        for kw, what in ((dict(stream=True), "streaming"), (dict(n=2), "n"), (dict(use_beam_search=True), "use_beam_search"),
                         (dict(prompts=["a", "b"]), "prompts"), (dict(temperature=0), "temperature"), (dict(temperature=0.7), "temperature"),
                         (dict(top_p=0.9), "top_p"), (dict(top_k=5), "top_k"), (dict(seed=1), "seed"),
                         (dict(repetition_penalty=1.3), "repetition_penalty"), (dict(presence_penalty=0.4), "presence_penalty"),
                         (dict(frequency_penalty=0.4), "frequency_penalty"), (dict(guided_regex="a+"), "guided_regex"),
                         (dict(guided_choice=["a"]), "guided_choice"), (dict(guided_json={"type": "object"}), "guided_json"),
                         (dict(response_format={"type": "json_schema"}), "response_format"), (dict(logit_bias={"5": 1.0}), "logit_bias"),
                         (dict(allowed_token_ids=[1]), "allowed_token_ids"), (dict(min_tokens=1), "min_tokens"),
                         (dict(stop_token_ids=[1]), "stop_token_ids"), (dict(ignore_eos=True), "ignore_eos"),
                         (dict(no_repeat_ngram_size=3), "no_repeat_ngram_size"), (dict(stop=["x"]), "stop"),
                         (dict(top_logprobs=21), "top_logprobs"), (dict(top_logprobs=-1), "top_logprobs"), (dict(logprobs=False, top_logprobs=1), "logprobs"),
                         (dict(score_eos="yes"), "score_eos")):
            bad = c.post("/v1/chat/completions", json=_payload(page, score_candidates=cands, **kw))
            assert bad.status_code == 400 and what in bad.json()["detail"], (kw, bad.text)
        for value in ([], "a string", ["", "x"], ["x"] * 9, [1, 2]):
            assert c.post("/v1/chat/completions", json=_payload(page, score_candidates=value)).status_code == 400
        bad = c.post("/v1/chat/completions", json=_payload(page, score_candidates=["<|imgpad|>"]))
        assert bad.status_code == 400 and "image token" in bad.json()["detail"]
        assert c.post("/v1/chat/completions", json=_payload(page, score_candidates=cands, logprobs=True)).status_code == 200
        eng.spec_k = 2
        bad = c.post("/v1/chat/completions", json=_payload(page, score_candidates=cands))
        assert bad.status_code == 400 and "--speculative-ngram" in bad.json()["detail"]
        eng.spec_k = 0
    with TestClient(create_app(model, proc, model_name="model", max_batch=8, continuous=False)) as c:
        bad = c.post("/v1/chat/completions", json=_payload(page, score_candidates=cands))
        assert bad.status_code == 400 and "--static-batching" in bad.json()["detail"]


# ---------------------------------------------------------------------------------------------------- parser

def test_score_image_issues_one_request(tmp_path, monkeypatch):
    import dots_ocr.model.inference as inf
    from dots_ocr_amd.parser import DotsOCRParser
    from dots_ocr_amd.synthetic import synth_page
    page_path = tmp_path / "page.png"
    synth_page(0, (280, 168)).save(page_path)
    calls = []

    def score(image, prompt, candidates, **kw):
        calls.append((image.size, prompt, list(candidates), kw))
        return [{"index": i, "message": {"content": c}, "finish_reason": "scored", "cumulative_logprob": -1.5 * len(c),
                 "logprobs": {"content": [{"token": ch, "logprob": -1.5, "bytes": [ord(ch)], "top_logprobs": [{"token": ch, "logprob": -0.5, "bytes": []}]}
                                          for ch in c]}} for i, c in enumerate(candidates)]
    monkeypatch.setattr(inf, "score_with_vllm", score)
    parser = DotsOCRParser(output_dir=str(tmp_path / "out"))
    res = parser.score_image(str(page_path), ["abc", "de"], prompt_mode="prompt_ocr", top_logprobs=1)
    assert len(calls) == 1 and calls[0][2] == ["abc", "de"] and calls[0][3]["top_logprobs"] == 1
    assert [r["text"] for r in res] == ["abc", "de"] and res[0]["tokens"] == ["a", "b", "c"]
    assert res[0]["token_logprobs"] == [-1.5] * 3 and res[0]["cumulative_logprob"] == -4.5 and res[1]["mean_logprob"] == -1.5
    assert set(res[0]) == {"text", "tokens", "token_logprobs", "cumulative_logprob", "mean_logprob", "top_logprobs"}
    assert res[0]["top_logprobs"][0] == [("a", -0.5)]
    assert set(parser.score_image(str(page_path), ["x"], prompt_mode="prompt_ocr")[0]) == {"text", "tokens", "token_logprobs", "cumulative_logprob",
                                                                                           "mean_logprob"}
    for bad in ([], ["x"] * 9, ["", "y"], [3]):
        with pytest.raises(ValueError):
            parser.score_image(str(page_path), bad)


def test_score_image_through_the_in_process_model(tmp_path):
    from dots_ocr_amd.parser import DotsOCRParser
    from dots_ocr_amd.processing import DotsOcrProcessor, process_vision_info
    from dots_ocr_amd.synthetic import synth_page
    cfg = DotsConfig.tiny()
    proc = DotsOcrProcessor(cfg)
    page_path = tmp_path / "page.png"
    synth_page(0, (280, 168)).save(page_path)
    seen = []

    class Model:
        config = cfg
        engine = types.SimpleNamespace()

        def score(self, input_ids, pixel_values, image_grid_thw, candidates=None, top_logprobs=0):
            seen.append((input_ids[0].tolist(), [list(c) for c in candidates], top_logprobs))
            return [_fake_scores(c, top_logprobs) for c in candidates]
    parser = DotsOCRParser(output_dir=str(tmp_path / "out"), model=Model(), processor=proc)
    parser.process_vision_info = process_vision_info
    res = parser.score_image(str(page_path), ["ab", "c"], prompt_mode="prompt_ocr", top_logprobs=2)
    prefix, fed, top = seen[0]
    eos = cfg.eos_token_ids[0]
    assert top == 2 and [x[1:] for x in fed] == [list(b"ab") + [eos], list(b"c") + [eos]] and fed[0][0] == fed[1][0]
    assert cfg.image_token_id in prefix and cfg.image_token_id not in fed[0]
    assert res[0]["tokens"][:2] == ["a", "b"] and len(res[0]["token_logprobs"]) == 3 and len(res[1]["token_logprobs"]) == 2
    assert res[0]["cumulative_logprob"] == float(_fake_scores(fed[0], 2)[0].astype(np.float64).sum())
    assert math.isclose(res[0]["mean_logprob"], res[0]["cumulative_logprob"] / 3)
    assert len(res[0]["top_logprobs"]) == 3 and len(res[0]["top_logprobs"][0]) == 2
