"""Per-row sampling parameters above the kernels, on CPU: SamplingParams, the C struct mirror, the scheduler's
set_row_sampling calls, the server's request fields and running set, modeling.generate's per-row path."""
import ctypes
import re
import threading
import time
from pathlib import Path

import numpy as np
import pytest
import torch

from dots_ocr_amd.config import DotsConfig
from dots_ocr_amd.engine import CDotsSamplingParams, SamplingParams
from dots_ocr_amd.row_features import rows_holding

ROOT = Path(__file__).resolve().parent.parent


def test_sampling_params_validate_and_normalise():
    p = SamplingParams(temperature=0.5, top_p=3.0, top_k=-1, seed=-1)
    assert (p.top_p, p.top_k, p.seed) == (1.0, 0, 2 ** 64 - 1)
    assert not SamplingParams().has_penalty and SamplingParams(presence_penalty=0.1).has_penalty
    for bad in (dict(temperature=-0.1), dict(temperature=float("inf")), dict(top_p=0.0), dict(top_p=float("nan")),
                dict(repetition_penalty=0.0), dict(repetition_penalty=-1.0), dict(frequency_penalty=2.5), dict(presence_penalty=-2.01),
                dict(top_k=1.5)):
        with pytest.raises(ValueError):
            SamplingParams(**bad)
    # top_k is an int32 in the engine: larger values mean "keep everything" and are clamped, never wrapped
    assert SamplingParams(top_k=2 ** 31).to_c().top_k == SamplingParams(top_k=2 ** 32 + 5).to_c().top_k == 2 ** 31 - 1
    # the float fields are checked as the fp32 values the engine receives
    for bad in (dict(temperature=1e39), dict(repetition_penalty=1e-50), dict(repetition_penalty=1e39)):
        with pytest.raises(ValueError):
            SamplingParams(**bad)
    c = SamplingParams(temperature=0.1, top_p=0.9, top_k=50, repetition_penalty=1.1, frequency_penalty=0.2, presence_penalty=-0.3, seed=7).to_c()
    assert (c.top_k, c.seed) == (50, 7) and abs(c.top_p - 0.9) < 1e-7 and abs(c.presence_penalty + 0.3) < 1e-7


def test_sampling_params_mirror_matches_header():
    txt = (ROOT / "include" / "dots_ocr_hip.h").read_text()
    body = re.search(r"typedef struct DotsSamplingParams \{(.*?)\} DotsSamplingParams;", txt, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    cmap = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64, "float": ctypes.c_float, "double": ctypes.c_double}
    want = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ty, rest = decl.split(None, 1)
            want += [(n.strip(), cmap[ty]) for n in rest.split(",")]
    assert want == list(CDotsSamplingParams._fields_)
    assert ctypes.sizeof(CDotsSamplingParams) == 32


# ---------------------------------------------------------------------------------------------------- scheduler
def _row_engine(base):
    class RowEngine(base):
        """fake slot engine + per-row parameters: records every set_row_sampling and the row state each prefill sees"""

        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            self.rows, self.row_calls, self.prefill_rows = {}, [], []

        def set_row_sampling(self, row, params):
            self.row_calls.append((row, params))
            if params is None:
                self.rows.pop(row, None)
            else:
                self.rows[row] = params

        def slots_prefill(self, slots, ids, lens, caps):
            off = 0
            for s, n in zip(slots, lens):
                self.prefill_rows.append((s, int(ids[off]), self.rows.get(s)))
                off += n
            super().slots_prefill(slots, ids, lens, caps)

        def slot_release(self, s):           # the engine clears the row with the slot (dots_slot_release)
            self.rows.pop(s, None)
            super().slot_release(s)
    return RowEngine


def test_scheduler_sets_row_parameters_before_the_prefill_that_admits_them():
    from fakes import FakeSlotEngine
    from dots_ocr_amd.scheduler import ContinuousBatcher, Request
    eng = _row_engine(FakeSlotEngine)(lambda prompt: [5] * (3 + int(prompt[0]) % 4), max_batch=2, max_prefill_tokens=64)
    sps = [SamplingParams(temperature=0.3, seed=1), None, SamplingParams(repetition_penalty=1.2), None, None,
           SamplingParams(top_k=4, temperature=1.0, seed=9)]
    reqs = [Request(np.array([10 + i, 1, 2], np.int32), max_new_tokens=4 + i, sampling=sp) for i, sp in enumerate(sps)]
    outs = ContinuousBatcher(eng, chunk=2).run(reqs)
    assert len(outs) == len(reqs) and len(eng.prefill_rows) == len(reqs)
    for slot, first, row in eng.prefill_rows:
        assert row == sps[first - 10], (slot, first)         # the request's own parameters, or a cleared row
    # a request without parameters on a slot that had them: cleared explicitly
    eng2 = _row_engine(FakeSlotEngine)(lambda prompt: [5] * 6, max_batch=1, max_prefill_tokens=64)
    eng2.slot_release = FakeSlotEngine.slot_release.__get__(eng2)       # an engine that keeps the entry until told otherwise
    ContinuousBatcher(eng2, chunk=2).run([Request(np.array([1, 2], np.int32), max_new_tokens=3, sampling=SamplingParams(temperature=0.5)),
                                          Request(np.array([3, 4], np.int32), max_new_tokens=3)])
    assert [c[1] for c in eng2.row_calls] == [SamplingParams(temperature=0.5), None]
    assert eng2.prefill_rows[1][2] is None


def test_scheduler_clears_row_parameters_when_the_prefill_fails():
    from fakes import FakeSlotEngine
    from dots_ocr_amd.scheduler import ContinuousBatcher, Request
    eng = _row_engine(FakeSlotEngine)(lambda prompt: [5] * 4, max_batch=2, max_prefill_tokens=64)
    fail = {"on": True}
    real = eng.slots_prefill

    def flaky(*a):
        if fail["on"]:
            raise RuntimeError("KV pool exhausted")
        return real(*a)
    eng.slots_prefill = flaky
    cb = ContinuousBatcher(eng, chunk=2)
    cb.submit(Request(np.array([1, 2], np.int32), max_new_tokens=3, sampling=SamplingParams(temperature=0.4, seed=2)))
    with pytest.raises(RuntimeError):
        cb.step()
    assert eng.rows == {} and rows_holding(cb._rows, "sampling") == []          # no entry left on a slot that was never occupied
    assert eng.row_calls[-1][1] is None


def test_scheduler_without_parameters_makes_no_row_calls():
    from fakes import FakeSlotEngine
    from dots_ocr_amd.scheduler import ContinuousBatcher, Request
    eng = _row_engine(FakeSlotEngine)(lambda prompt: [5] * 4, max_batch=2, max_prefill_tokens=64)
    ContinuousBatcher(eng, chunk=2).run([Request(np.array([1 + i, 2], np.int32), max_new_tokens=3) for i in range(5)])
    assert eng.row_calls == []


# ---------------------------------------------------------------------------------------------------- server

class _RowSlotModel:
    """model with an engine that selects per row: each completion spells out the parameters of its own slot"""

    def __init__(self, proc, cfg, per_row=True):
        from fakes import FakeSlotEngine
        self.config = cfg
        model = self

        class Eng(FakeSlotEngine):
            def slots_prefill(self, slots, ids, lens, caps):
                off = 0
                for s, n, c in zip(slots, lens, caps):
                    self.cur = s
                    super().slots_prefill([s], ids[off:off + n], [n], [c])
                    off += n

            def slots_decode(self, n):
                time.sleep(0.005)            # keep a request running while the next ones arrive
                super().slots_decode(n)

        def script(prompt):
            e = model.engine
            p = getattr(e, "rows", {}).get(e.cur)
            t, tp, k, r, seed = (e.sampling[0], e.sampling[1], 0, 1.0, e.sampling[2]) if p is None else \
                (p.temperature, p.top_p, p.top_k, p.repetition_penalty, p.seed)
            return proc.tokenizer.encode(f"{t:g}|{tp:g}|{k}|{r:g}|{seed}|" + "x" * 200) + [cfg.eos_token_ids[0]]
        base = _row_engine(Eng) if per_row else Eng
        self.engine = base(script, max_batch=3, max_patches=4096, max_prefill_tokens=4096, max_seq_len=2048)


def _text_payload(**kw):
    body = {"model": "model", "messages": [{"role": "user", "content": "Read this."}], "max_completion_tokens": 48}
    body.update(kw)
    return body


def test_server_serves_mixed_parameters_in_one_running_set():
    pytest.importorskip("fastapi")
    from fastapi.testclient import TestClient
    from dots_ocr_amd.processing import DotsOcrProcessor
    from dots_ocr_amd.server import ContinuousWorker, create_app
    cfg = DotsConfig.tiny()
    proc = DotsOcrProcessor(cfg)
    model = _RowSlotModel(proc, cfg)
    app = create_app(model, proc, model_name="model", max_batch=3)
    asks = [dict(temperature=0.1, top_p=0.9, seed=5), dict(temperature=0.9, top_k=40, repetition_penalty=1.1),
            dict(temperature=0.5, top_p=0.8, frequency_penalty=0.5, presence_penalty=0.5, seed=77)]
    with TestClient(app) as c:
        w = app.state.worker
        assert isinstance(w, ContinuousWorker) and w.per_row
        w.chunk = 2
        res = [None] * 3

        def go(i):
            res[i] = c.post("/v1/chat/completions", json=_text_payload(**asks[i]))
        th = [threading.Thread(target=go, args=(i,)) for i in range(3)]
        [t.start() for t in th]
        [t.join() for t in th]
        for ask, r in zip(asks, res):
            assert r.status_code == 200, r.text
            t, tp, k, rp, seed, _ = r.json()["choices"][0]["message"]["content"].split("|")
            assert float(t) == ask["temperature"] and float(tp) == ask.get("top_p", 1.0) and int(k) == ask.get("top_k", 0)
            assert float(rp) == pytest.approx(ask.get("repetition_penalty", 1.0))
            if "seed" in ask:
                assert int(seed) == ask["seed"]
        assert max(w.batches) == 3                     # all three decoded together: no drain between parameter sets
        for bad in (dict(repetition_penalty=0), dict(frequency_penalty=3), dict(presence_penalty=-2.5), dict(top_k=1.5), dict(seed="x"),
                    dict(repetition_penalty="high")):
            assert c.post("/v1/chat/completions", json=_text_payload(**bad)).status_code == 400, bad
        # a top_k beyond int32 (a client's "keep everything") is clamped: it neither wraps nor fails the request running beside it
        res = [None] * 2

        def go2(i, body):
            res[i] = c.post("/v1/chat/completions", json=_text_payload(**body))
        th = [threading.Thread(target=go2, args=(0, dict(temperature=0.7, seed=3))),
              threading.Thread(target=go2, args=(1, dict(temperature=0.7, top_k=3_000_000_000, seed=4)))]
        [t.start() for t in th]
        [t.join() for t in th]
        assert [r.status_code for r in res] == [200, 200], [r.text for r in res]
        assert int(res[1].json()["choices"][0]["message"]["content"].split("|")[2]) == 2 ** 31 - 1
        assert c.post("/v1/chat/completions", json=_text_payload(temperature=1e39)).status_code == 400
        # a greedy request without knobs takes the engine-wide greedy path
        d = c.post("/v1/chat/completions", json=_text_payload(temperature=0)).json()
        assert d["choices"][0]["message"]["content"].startswith("0|1|0|1|0|")


def test_server_refuses_knobs_an_engine_cannot_honour():
    pytest.importorskip("fastapi")
    from fastapi.testclient import TestClient
    from dots_ocr_amd.processing import DotsOcrProcessor
    from dots_ocr_amd.server import create_app
    cfg = DotsConfig.tiny()
    proc = DotsOcrProcessor(cfg)
    model = _RowSlotModel(proc, cfg, per_row=False)
    app = create_app(model, proc, model_name="model", max_batch=3)
    with TestClient(app) as c:
        assert not app.state.worker.per_row
        for ask in (dict(repetition_penalty=1.2), dict(top_k=5), dict(frequency_penalty=0.1), dict(presence_penalty=0.1)):
            assert c.post("/v1/chat/completions", json=_text_payload(**ask)).status_code == 400, ask
        r = c.post("/v1/chat/completions", json=_text_payload(temperature=0.3, seed=4))
        assert r.status_code == 200 and r.json()["choices"][0]["message"]["content"].startswith("0.3|1|0|1|")


# ---------------------------------------------------------------------------------------------------- modeling
class _GenEngine:
    def __init__(self):
        self.calls = []
        self.rows = {}

    def set_sampling(self, t, p, seed):
        self.calls.append(("sampling", t, p, seed))

    def set_row_sampling(self, row, params):
        self.calls.append(("row", row, params))
        if params is None:
            self.rows.pop(row, None)
        else:
            self.rows[row] = params

    def generate(self, packed, lens, pix, grid, max_new, eos, *a, **kw):
        self.calls.append(("generate", len(lens), dict(self.rows)))
        return np.full((len(lens), max_new), 7, np.int32), np.full(len(lens), max_new, np.int32)


def _fake_model():
    from dots_ocr_amd.modeling import DotsOcrHipForCausalLM
    cfg = DotsConfig.tiny()
    m = object.__new__(DotsOcrHipForCausalLM)
    m.config, m.engine, m.max_batch, m.max_seq_len, m.max_patches = cfg, _GenEngine(), 4, 256, 4096
    m.generation_config = {"do_sample": False}
    return m


def test_generate_passes_top_k_and_repetition_penalty_as_row_parameters():
    m = _fake_model()
    ids = torch.tensor([[1, 2, 3], [4, 5, 6]])
    m.generate(ids, max_new_tokens=3, do_sample=True, temperature=0.7, top_p=0.9, seed=10, top_k=20, repetition_penalty=1.2)
    gen = [c for c in m.engine.calls if c[0] == "generate"]
    assert len(gen) == 1
    rows = gen[0][2]
    assert sorted(rows) == [0, 1]
    for b in (0, 1):
        assert rows[b] == SamplingParams(temperature=0.7, top_p=0.9, top_k=20, repetition_penalty=1.2, seed=10 + b)
    assert m.engine.rows == {}                         # cleared afterwards
    # without the new keys: the engine-wide path only, no row call
    m2 = _fake_model()
    m2.generate(ids, max_new_tokens=3, do_sample=True, temperature=0.7, top_p=0.9, seed=10)
    assert [c for c in m2.engine.calls if c[0] == "row"] == []
    assert ("sampling", 0.7, 0.9, 10) in m2.engine.calls
