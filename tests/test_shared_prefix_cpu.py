"""Shared-prefix decode attention without a GPU: the host planner (csrc/share_plan.h through dots_plan_shared_prefix) held to
a restatement written here — by hand and over seeded random block tables — and the switch's way from the server, the batcher, generate() and
the parser to the engine, over the fakes."""
import inspect
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from dots_ocr_amd.config import DotsConfig
from test_parallel_sampling_cpu import EOS, ForkEngine, _by_seed, _seq

ROOT = Path(__file__).resolve().parents[1]
WAVES = 4


@pytest.fixture(scope="module")
def plan():
    from dots_ocr_amd import build
    from dots_ocr_amd.engine import plan_shared_prefix
    build.build(verbose=False)
    return plan_shared_prefix


# ---------------------------------------------------------------------------------------------------- 1. the planner

def restated(active, table, static_pages, n_splits, waves=WAVES):
    """the rule in plain words: per split, the active rows whose static pages cover it, classed by their page ids; classes of two or more"""
    table = np.asarray(table)
    rows, max_pages = table.shape
    items, masks = [], [0] * rows
    if n_splits * waves < max_pages:
        return items, masks
    for s in range(n_splits):
        classes = {}
        for b in range(rows):
            if active[b] and waves * (s + 1) <= static_pages[b]:
                classes.setdefault(tuple(int(x) for x in table[b, waves * s:waves * (s + 1)]), []).append(b)
        for members in sorted((m for m in classes.values() if len(m) > 1), key=lambda m: m[0]):
            items.append((s, members))
            for b in members:
                masks[b] |= 1 << s
    return items, masks


def check_plan(items, masks, active, static_pages, rows):
    """what holds of every plan, whatever the tables"""
    seen = set()
    for s, members in items:
        assert len(members) >= 2 and members == sorted(set(members))          # ascending, no row twice
        for b in members:
            assert active[b] and WAVES * (s + 1) <= static_pages[b]
            assert (b, s) not in seen                                         # at most one item per row and split
            seen.add((b, s))
    assert [sum(1 << s for s in range(64) if (b, s) in seen) for b in range(rows)] == masks      # items and masks agree


def _table(rows, max_pages, fill=None):
    t = np.arange(rows * max_pages, dtype=np.int32).reshape(rows, max_pages) + 1000      # every page its own
    return t if fill is None else np.full_like(t, fill)


def test_hand_cases(plan):
    # three forked rows over 9 shared pages of 12: two full splits; row 3 is independent, row 4 shares but is inactive
    t = _table(5, 12)
    for b in (1, 2, 4):
        t[b, :9] = t[0, :9]
    active, static = [1, 1, 1, 1, 0], [9, 9, 9, 9, 9]
    items, masks = plan(active, t, static, 3)
    assert items == [(0, [0, 1, 2]), (1, [0, 1, 2])] and masks == [3, 3, 3, 0, 0]
    check_plan(items, masks, active, static, 5)
    # static_pages = 4 s + 3 is one page short of split s
    items, masks = plan([1, 1, 1, 1, 0], t, [9, 7, 3, 9, 9], 3)
    assert items == [(0, [0, 1]), ] and masks == [1, 1, 0, 0, 0]
    items, masks = plan([1, 1, 1, 1, 0], t, [9, 8, 4, 9, 9], 3)
    assert items == [(0, [0, 1, 2]), (1, [0, 1])] and masks == [3, 3, 1, 0, 0]
    # one row alone never makes an item, nor do two rows that agree on three of the four pages
    t2 = _table(2, 8)
    t2[1, :3] = t2[0, :3]
    assert plan([1, 1], t2, [8, 8], 2) == ([], [0, 0])
    assert plan([1], _table(1, 8), [8], 2) == ([], [0])


def test_the_tree_case(plan):
    """a prefix-cache tree: three rows agree on 2 splits, two of them on 1 more — classes are formed per split"""
    t = _table(3, 16)
    t[1, :12] = t[0, :12]
    t[2, :8] = t[0, :8]
    items, masks = plan([1, 1, 1], t, [16, 14, 13], 4)
    assert items == [(0, [0, 1, 2]), (1, [0, 1, 2]), (2, [0, 1])] and masks == [7, 7, 3]
    # two classes in one split, in the order of their lowest member
    t = _table(5, 4)
    t[3] = t[0]
    t[4] = t[1]
    assert plan([1] * 5, t, [4] * 5, 1)[0] == [(0, [0, 3]), (0, [1, 4])]


def test_empty_when_a_wave_walks_more_than_one_page(plan):
    t = _table(4, 257, fill=7)                                                # every row names the same pages
    assert plan([1] * 4, t, [257] * 4, 64) == ([], [0] * 4)                  # 64 splits x 4 < 257 pages: contexts above 16 k
    items, masks = plan([1] * 4, t[:, :256], [256] * 4, 64)
    assert len(items) == 64 and masks == [2 ** 64 - 1] * 4


@pytest.mark.parametrize("seed", range(6))
def test_random_tables_against_the_restatement(plan, seed):
    rng = np.random.default_rng(100 + seed)
    for _ in range(60):
        rows, n_splits = int(rng.integers(1, 17)), int(rng.integers(1, 5))
        max_pages = int(rng.integers(max(1, WAVES * (n_splits - 1) + 1), WAVES * n_splits + 1))
        # page ids from a small pool, and prefixes copied between rows, so that classes form
        t = rng.integers(0, 3, (rows, max_pages)).astype(np.int32)
        for b in range(1, rows):
            if rng.random() < 0.6:
                k = int(rng.integers(0, max_pages + 1))
                t[b, :k] = t[int(rng.integers(0, b)), :k]
        active = [int(rng.random() < 0.8) for _ in range(rows)]
        static = [int(rng.integers(0, max_pages + 1)) for _ in range(rows)]
        items, masks = plan(active, t, static, n_splits)
        assert (items, masks) == restated(active, t, static, n_splits)
        check_plan(items, masks, active, static, rows)


def test_the_planner_is_host_code_and_exported():
    from dots_ocr_amd import _lib, build, engine
    src = (ROOT / "dots_ocr_amd" / "csrc" / "share_plan.h").read_text()
    assert "hip" not in src.lower().replace("ship", "")                       # plain C++: a host program can include it
    build.build(verbose=False)
    lib = _lib.load()
    header = (ROOT / "include" / "dots_ocr_hip.h").read_text()
    for sym in ("dots_set_shared_prefix_attention", "dots_shared_prefix_info", "dots_plan_shared_prefix", "dots_op_decode_attn_shared"):
        assert hasattr(lib, sym) and sym in engine.EXPORTED_SYMBOLS and re.search(r"^int " + sym + r"\(", header, re.M), sym
    for method in ("set_shared_prefix_attention", "shared_prefix_info", "op_decode_attn_shared"):
        assert callable(getattr(engine.Engine, method))


# ---------------------------------------------------------------------------------------------------- 2. the switch's way to the engine

class ShareEngine(ForkEngine):
    """ForkEngine + the switch and its counter: a decode chunk with the switch on `reads` 12 pages less per step and forked row"""

    def __init__(self, *a, spec_k=0, **kw):
        super().__init__(*a, **kw)
        self.share_calls, self.share_on, self.saved, self.spec_k = [], False, 0, spec_k

    def set_shared_prefix_attention(self, on=True):
        self.share_calls.append(bool(on))
        self.share_on = bool(on)

    def shared_prefix_info(self):
        return {"items": 0, "rows": 0, "pairs": 0, "pages_not_read": self.saved}

    def slots_decode(self, n):
        if self.share_on and not self.spec_k:                                 # inert while the engine speculates
            self.saved += 12 * n * sum(1 for st in self.slots.values() if st.get("group") is not None)
        super().slots_decode(n)


def _engine(max_batch=4, **kw):
    box = []
    e = ShareEngine(_by_seed(box), 64, max_batch=max_batch, max_prefill_tokens=1024, max_seq_len=1024, **kw)
    box.append(e)
    return e


def _req(first, L=5, cap=40, **kw):
    from dots_ocr_amd.scheduler import Request
    return Request(np.full(L, first, np.int32), max_new_tokens=cap, **kw)


def test_the_batcher_sets_the_switch_and_counts():
    from dots_ocr_amd.engine import SamplingParams
    from dots_ocr_amd.scheduler import ContinuousBatcher
    e = _engine()
    ContinuousBatcher(e, eos_ids=[EOS], chunk=2)
    assert e.share_calls == []                                                # the default leaves the engine alone
    e.saved = 1000                                                            # an earlier batcher's
    cb = ContinuousBatcher(e, eos_ids=[EOS], chunk=2, shared_prefix_attention=True)
    assert e.share_calls == [True] and cb.shared_prefix_attention and cb.shared_pages_not_read == 0
    outs = cb.run([_req(3, n=3, sampling=SamplingParams(temperature=1.0, seed=1))])
    assert e.saved > 1000 and cb.shared_pages_not_read == e.saved - 1000
    want = ContinuousBatcher(_engine(), eos_ids=[EOS], chunk=2).run([_req(3, n=3, sampling=SamplingParams(temperature=1.0, seed=1))])
    assert [o.tolist() for o in outs] == [o.tolist() for o in want]           # and changes no token
    ContinuousBatcher(e, eos_ids=[EOS], shared_prefix_attention=False)
    assert e.share_calls == [True, False]


def test_the_batcher_needs_an_engine_with_the_switch_only_when_on():
    from dots_ocr_amd.scheduler import ContinuousBatcher
    from fakes import FakePagedEngine
    plain = FakePagedEngine(lambda p: [1, EOS], 16)
    ContinuousBatcher(plain, shared_prefix_attention=False)
    ContinuousBatcher(plain)
    with pytest.raises(ValueError, match="shared-prefix"):
        ContinuousBatcher(plain, shared_prefix_attention=True)


def test_inert_and_not_refused_with_speculation():
    from dots_ocr_amd.scheduler import ContinuousBatcher
    e = _engine(spec_k=3)
    cb = ContinuousBatcher(e, eos_ids=[EOS], chunk=2, shared_prefix_attention=True)      # accepted ...
    assert e.share_calls == [True]
    outs = cb.run([_req(2, n=2)])
    assert len(outs) == 1 and cb.shared_pages_not_read == 0                              # ... and nothing is shared
    from dots_ocr_amd.server import build_arg_parser, speculation_args
    a = build_arg_parser().parse_args(["--shared-prefix-attention", "--speculative-ngram", "3"])
    assert a.shared_prefix_attention and speculation_args(a) is not None
    assert build_arg_parser().parse_args(["--shared-prefix-attention", "--static-batching"]).shared_prefix_attention
    assert build_arg_parser().parse_args([]).shared_prefix_attention is False


def test_generate_passes_the_switch_for_the_call():
    from dots_ocr_amd.modeling import CallSettings, DotsOcrHipForCausalLM
    assert inspect.signature(DotsOcrHipForCausalLM.generate).parameters["shared_prefix_attention"].default is False
    assert CallSettings().shared_prefix_attention is False
    cfg = DotsConfig.tiny()
    e = _engine()
    e.max_patches = 4096
    m = object.__new__(DotsOcrHipForCausalLM)
    m.config, m.engine, m.max_batch, m.max_seq_len, m.max_patches = cfg, e, 4, 1024, 4096
    m.generation_config = {"do_sample": False}
    ids = torch.tensor([[1, 1, 1]])
    kw = dict(max_new_tokens=16, do_sample=True, temperature=0.7, top_p=0.9, seed=10, num_return_sequences=3, eos_token_id=[EOS], pad_token_id=0)
    want = m.generate(ids, **kw)
    assert e.share_calls == [] and e.saved == 0                               # without the keyword the call is what it was
    got = m.generate(ids, shared_prefix_attention=True, **kw)
    assert e.share_calls == [True, False] and e.saved > 0                     # on for the call's run, off behind it
    assert torch.equal(got, want)
    for j in range(3):
        w = _seq(1, 10 + j)
        assert got[j].tolist()[3:3 + len(w)] == w


class RecModel:
    def __init__(self):
        self.engine = object()
        self.kw = None

    def generate(self, **kw):
        self.kw = kw
        raise StopIteration                                                   # the keywords are all this test wants


class FakeInputs(dict):
    def to(self, device):
        return self


def test_the_parser_passes_the_switch():
    from dots_ocr_amd.parser import DotsOCRParser
    for on in (True, False):
        p = DotsOCRParser(model=RecModel(), processor=object(), shared_prefix_attention=on)
        p._build_inputs = lambda images, prompts: FakeInputs(input_ids=None)
        with pytest.raises(StopIteration):
            p._inference_batch_with_hf([None], ["x"])
        assert p.model.kw.get("shared_prefix_attention", False) is on and (on or "shared_prefix_attention" not in p.model.kw)
        assert p._chunk_kw() == ({"shared_prefix_attention": True} if on else {})
    assert DotsOCRParser(shared_prefix_attention=True, speculative_ngram=3).shared_prefix_attention      # accepted beside speculation
    assert DotsOCRParser(prefill_chunk=64, enable_prefix_caching=True, shared_prefix_attention=True)._chunk_kw() == \
        {"prefill_chunk": 64, "shared_prefix_attention": True, "prefix_caching": True}


def test_the_server_hands_the_switch_to_its_batchers_and_counts():
    pytest.importorskip("fastapi")
    from fastapi.testclient import TestClient
    from dots_ocr_amd.processing import DotsOcrProcessor
    from dots_ocr_amd.server import BatchingWorker, ContinuousWorker, create_app
    cfg = DotsConfig.tiny()
    proc = DotsOcrProcessor(cfg)

    class Model:
        config = cfg

    model = Model()

    def script(prompt):
        p = model.engine.rows.get(model.engine.cur)
        return proc.tokenizer.encode(f"seed={-1 if p is None else p.seed}|") + [cfg.eos_token_ids[0]]

    model.engine = ShareEngine(script, 256, max_batch=3, max_patches=4096, max_prefill_tokens=4096, max_seq_len=2048)
    body = {"model": "model", "messages": [{"role": "user", "content": "Read this."}], "max_completion_tokens": 24, "temperature": 0.8, "n": 3, "seed": 4}
    app = create_app(model, proc, model_name="model", max_batch=3)
    assert app.state.worker._chunk_kw() == {} and app.state.worker.counters["shared_pages_not_read"] == 0
    with TestClient(app) as c:
        off = c.post("/v1/chat/completions", json=body)
        assert off.status_code == 200 and model.engine.share_calls == [] and app.state.worker.counters["shared_pages_not_read"] == 0
    app = create_app(model, proc, model_name="model", max_batch=3, shared_prefix_attention=True)
    assert isinstance(app.state.worker, ContinuousWorker) and app.state.worker._chunk_kw() == {"shared_prefix_attention": True}
    with TestClient(app) as c:
        on = c.post("/v1/chat/completions", json=body)
        assert on.status_code == 200 and model.engine.share_calls and all(model.engine.share_calls)
        assert [ch["message"]["content"] for ch in on.json()["choices"]] == [ch["message"]["content"] for ch in off.json()["choices"]]
        assert app.state.worker.counters["shared_pages_not_read"] == model.engine.saved > 0      # beside preemptions / swapped_pages
    # static batching: accepted and inert
    app = create_app(model, proc, model_name="model", max_batch=3, continuous=False, shared_prefix_attention=True)
    assert isinstance(app.state.worker, BatchingWorker) and not isinstance(app.state.worker, ContinuousWorker)
