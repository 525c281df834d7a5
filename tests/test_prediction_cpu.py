"""Predicted outputs without a GPU: the drafting rule and the replay on the host, the C ABI's names, the scheduler's calls
around a slot's prefill, and the server's `prediction` field."""
import json
import re
from pathlib import Path

import numpy as np
import pytest

from dots_ocr_amd import engine
from dots_ocr_amd.config import DotsConfig
from dots_ocr_amd.engine import ngram_draft, predicted_draft, predicted_run
from dots_ocr_amd.processing import DotsOcrProcessor
from dots_ocr_amd.scheduler import ContinuousBatcher, Request, RequestRejected
from fakes import FakePagedEngine

ROOT = Path(__file__).resolve().parent.parent


# ---------------------------------------------------------------------------------------------------- 1. the rule

def _brute(out, pred, cur, at, k, min_n, max_n):
    """the rule of the header, with explicit loops and no slicing"""
    L, P = len(out), len(pred)
    es = cur + (L - at)
    e = None
    m = min(min_n, L, es)
    if m >= 1 and es < P:
        same = True
        for j in range(m):
            if pred[es - m + j] != out[L - m + j]:
                same = False
        if same:
            e = es
    if e is None:
        n = min(max_n, L)
        while n >= min_n and e is None:
            best = None
            for i in range(0, P):
                if i + n >= P:
                    break
                hit = True
                for j in range(n):
                    if pred[i + j] != out[L - n + j]:
                        hit = False
                        break
                if not hit:
                    continue
                c = i + n
                if best is None or abs(c - es) < abs(best - es) or (abs(c - es) == abs(best - es) and c > best):
                    best = c
            e = best
            n -= 1
    if e is None:
        return None, cur, at
    d = []
    for j in range(k):
        if e + j < P:
            d.append(pred[e + j])
    return d, e, L


def test_rule_equals_brute_force_on_small_alphabets():
    rng = np.random.default_rng(7)
    found = missed = 0
    for case in range(1500):
        a = int(rng.integers(2, 6))
        out = [int(t) for t in rng.integers(0, a, int(rng.integers(0, 40)))]
        pred = [int(t) for t in rng.integers(0, a, int(rng.integers(0, 60)))]
        at = int(rng.integers(0, len(out) + 1))
        cur = int(rng.integers(0, len(pred) + 1))
        k, lo = int(rng.integers(1, 8)), int(rng.integers(1, 4))
        hi = lo + int(rng.integers(0, 5))
        got = predicted_draft(out, pred, cur, at, k, lo, hi)
        assert got == _brute(out, pred, cur, at, k, lo, hi), (case, out, pred, cur, at, k, lo, hi)
        found += got[0] is not None
        missed += got[0] is None
    assert found > 300 and missed > 100


def test_rule_planted_cases():
    d = lambda *a: predicted_draft(*a, 3, 2, 4)                      # noqa: E731
    assert d([1, 2, 3, 4], [1, 2, 3, 4, 5, 6, 7, 8], 0, 0) == ([5, 6, 7], 4, 4)                        # anchor hit
    assert d([1, 2, 3, 4, 5], [0, 1, 2, 3, 4, 5, 6, 7, 8], 3, 2) == ([6, 7, 8], 6, 5)                  # ... from a moved alignment: e* = 3 + (5 - 2)
    assert d([1, 2, 9, 4, 5], [1, 2, 3, 4, 5, 6, 7, 8], 0, 0) == ([6, 7, 8], 5, 5)                     # anchor hit on the last two
    assert d([1, 2, 3, 9, 5], [1, 2, 3, 4, 5, 6, 7, 8], 0, 0) == (None, 0, 0)                          # anchor miss, nothing to find
    assert d([4, 5], [1, 2, 3, 4, 5, 6, 7, 8], 0, 0) == ([6, 7, 8], 5, 2)                              # anchor miss, then the search
    assert d([7, 8], [7, 8, 20, 21, 7, 8, 30, 31], 4, 2) == ([30, 31], 6, 2)                           # a tie: the larger e
    assert d([7, 8], [7, 8, 20, 21, 22, 23, 7, 8, 30, 7, 8, 40], 9, 2) == ([30, 7, 8], 8, 2)           # the nearest, not the last
    assert d([7, 8], [7, 8, 20, 21, 22, 23, 7, 8, 30, 7, 8, 40], 10, 2) == ([40], 11, 2)
    assert d([5, 6, 7, 8, 9, 10], [5, 6, 7, 8], 0, 0) == (None, 0, 0)                                  # e* >= P and no key to find
    assert d([5, 6, 7], [5, 6, 7, 8], 2, 0) == ([8], 3, 3)                                             # e* >= P, the search still finds
    assert d([1, 2, 3], [1, 2, 3, 4, 5], 0, 0) == ([4, 5], 3, 3)                                       # fewer than k left
    assert d([1, 2, 3], [], 0, 0) == (None, 0, 0)                                                      # empty prediction
    assert d([1], [1, 2, 3], 0, 0) == ([2, 3], 1, 1) and d([2], [1, 2, 3], 0, 0) == (None, 0, 0)       # L < min_n: the anchor alone
    assert d([], [1, 2, 3], 0, 0) == (None, 0, 0)
    assert d([50, 51, 52], [1, 2, 3, 4, 5, 6], 1, 1) == (None, 1, 1)                                   # no match: cur and at untouched
    assert d([1, 2, 3, 4, 5, 6], [3, 4, 5, 6, 9, 4, 5, 6, 8], 0, 0) == ([9, 4, 5], 4, 6)               # the longest key first: n = 4 has one candidate
    with pytest.raises(ValueError):
        predicted_draft([1], [1], 0, 0, 0, 2, 4)


# ---------------------------------------------------------------------------------------------------- 2. the replay

T = list(range(100, 130))            # 30 distinct tokens: the own-output rule never finds anything


def _run(pred, tokens=T, k=3, cap=None):
    return predicted_run(tokens, pred, k, 2, 4, cap)


def test_replay_perfect_prediction():
    r = _run(T)
    # the prefill's token, one plain step, then k + 1 tokens per step
    assert r["n_steps"] == 1 + -(-(len(T) - 2) // 4) == 8
    assert r["steps"][0] == {"drafts": [], "source": None, "live": 0, "accepted": 0}
    assert all(s["source"] == "prediction" and s["accepted"] == s["live"] for s in r["steps"][1:])
    assert r["pred_accepted"] == r["accepted"] == len(T) - 1 - r["n_steps"] and r["pred_drafted"] == r["drafted"]
    assert _run([])["n_steps"] == len(T) - 1 and _run([])["drafted"] == 0


def test_replay_one_substitution():
    pred = list(T)
    pred[10] = 999
    r = _run(pred)
    wrong = [s for s in r["steps"] if s["accepted"] < s["live"]]
    assert len(wrong) == 1 and 999 in wrong[0]["drafts"]
    # behind the wrong token the anchor fails until min_n right tokens lie behind it: two plain steps, then it drafts again
    assert r["pred_drafted"] - r["pred_accepted"] == wrong[0]["live"] - wrong[0]["accepted"] and r["n_steps"] < len(T) // 2
    i = r["steps"].index(wrong[0])
    assert [s["source"] for s in r["steps"][i + 1:i + 4]] == [None, None, "prediction"]


def test_replay_deletion_insertion_and_swap():
    base = _run(T)["n_steps"]
    for name, pred in (("deleted", T[:12] + T[15:]), ("inserted", T[:12] + [999] + T[12:]),
                       ("swapped", T[:4] + T[12:20] + T[4:12] + T[20:])):
        r = _run(pred)
        assert base < r["n_steps"] < len(T) // 2, name                # it re-synchronises: a few steps lost, not the prediction
        assert r["steps"][-1]["source"] == "prediction", name
        assert r["pred_drafted"] > r["pred_accepted"] > len(T) // 2, name


def test_replay_short_prediction_and_the_cap_cut():
    r = _run(T[:10])
    assert r["pred_accepted"] == 6 and r["n_steps"] == 1 + 2 + (len(T) - 10)      # the prediction runs out: plain steps to the end
    assert all(s["source"] is None for s in r["steps"][3:])
    # the cap cuts the drafts a step verifies: a step at L tokens may commit 1 + (cap - L - 1) more.  10 tokens at cap 10 fit three steps
    r = _run(T, tokens=T[:10], cap=10)
    assert [s["live"] for s in r["steps"]] == [0, 3, 3] and [len(s["drafts"]) for s in r["steps"]] == [0, 3, 3]
    assert r["drafted"] == 6 and r["accepted"] == 6
    r = _run(T, tokens=T[:7], cap=7)                                 # the last step holds three drafts and verifies none
    assert [s["live"] for s in r["steps"]] == [0, 3, 0] and [len(s["drafts"]) for s in r["steps"]] == [0, 3, 3] and r["pred_drafted"] == 3
    r = _run(T, tokens=T[:9], cap=9)
    assert [s["live"] for s in r["steps"]] == [0, 3, 2] and r["pred_drafted"] == 5 and r["pred_accepted"] == 5
    # without a cap given the tokens ended otherwise (an EOS): a step that finishes mid-walk accepts what it committed
    r = _run(T, tokens=T[:9], cap=40)
    assert [(s["live"], s["accepted"]) for s in r["steps"]] == [(0, 0), (3, 3), (3, 2)]


def test_replay_falls_back_to_own_output():
    toks = [1, 2, 3, 4, 1, 2, 3, 4, 1, 2, 3, 4]
    r = predicted_run(toks, [900, 901, 902], 3, 2, 4)
    assert r["pred_drafted"] == 0 and r["accepted"] > 0 and {s["source"] for s in r["steps"]} == {None, "own"}
    own = [ngram_draft(toks[:n], 3, 2, 4) for n in range(2, len(toks))]
    assert any(own)


# ---------------------------------------------------------------------------------------------------- 3. the C ABI's names

def test_symbols_are_declared_and_listed():
    header = (ROOT / "include" / "dots_ocr_hip.h").read_text()
    for sym in ("dots_set_row_prediction", "dots_row_prediction_stats", "dots_op_predict_draft"):
        assert sym in engine.EXPORTED_SYMBOLS and re.search(r"^int " + sym + r"\(", header, re.M), sym
    for word in ("anchor", "search", "DOTS_E_CAPACITY: n > max_seq_len", "dots_slot_release and dots_slots_reset clear"):
        assert word in header, word
    kernels = (ROOT / "dots_ocr_amd" / "csrc" / "kernels.h").read_text()
    assert "launch_predict_draft" in kernels and "struct PredictState" in kernels
    assert "predict_draft_kernel" in (ROOT / "dots_ocr_amd" / "csrc" / "predict.hip").read_text()
    assert re.search(r"struct StepKey \{[^}]*\bpred\b", (ROOT / "dots_ocr_amd" / "csrc" / "engine.h").read_text())
    for name in ("set_row_prediction", "row_prediction_stats", "predict_draft_op"):
        assert callable(getattr(engine.Engine, name))


# ---------------------------------------------------------------------------------------------------- 4. the scheduler

class PredEngine(FakePagedEngine):
    """FakePagedEngine + predictions: the calls are logged; a speculating one (spec_k > 0) counts the positions at which the prediction
    held the token the row committed.  The tokens never depend on it."""

    def __init__(self, script, pool_pages=64, spec_k=3, **kw):
        super().__init__(script, pool_pages, **kw)
        self.spec_k, self.preds, self.streams, self.cursor = spec_k, {}, set(), {}

    def set_row_prediction(self, row, ids):
        self.log.append(("prediction", row, tuple(ids) if ids else None))
        self.preds.pop(row, None) if not ids else self.preds.__setitem__(row, list(ids))

    def row_prediction_stats(self, row):
        pred, out = self.preds.get(row), self.slots[row]["out"]
        if not pred or not self.spec_k:
            return {"drafted": 0, "accepted": 0}
        n = min(len(pred), len(out))
        return {"drafted": n, "accepted": sum(int(pred[i] == out[i]) for i in range(n))}

    def slot_release(self, s):
        self.log.append(("release", s))
        self.preds.pop(s, None)
        self.streams.discard(s)
        super().slot_release(s)

    # streaming: everything new, once
    def set_row_stream(self, row, on=True):
        self.streams.add(row) if on else self.streams.discard(row)

    def slots_prefill(self, slots, ids, lens, caps):
        super().slots_prefill(slots, ids, lens, caps)
        for s in slots:
            self.cursor[s] = 0

    def slots_drain(self):
        fin, lens = self.slots_poll()
        deltas = {}
        for s in sorted(self.slots):
            out = self.slots[s]["out"]
            if s in self.streams and len(out) > self.cursor[s]:
                deltas[s] = (np.asarray(out[self.cursor[s]:], np.int32), None)
                self.cursor[s] = len(out)
        return fin, lens, deltas


def _engine(spec_k=3, **kw):
    return PredEngine(lambda p: [10, 11, 12, 13, 14, 15], spec_k=spec_k, max_batch=2, max_patches=64, max_prefill_tokens=256, max_seq_len=128, **kw)


def _req(**kw):
    return Request(np.arange(1, 9, dtype=np.int32), max_new_tokens=6, **kw)


def _calls(e, *kinds):
    return [c for c in e.log if c[0] in kinds]


def test_scheduler_sets_before_the_prefill_and_clears_for_the_next_request():
    e = _engine()
    cb = ContinuousBatcher(e, chunk=4)
    a = _req(prediction=[10, 11, 99, 13])
    (out_a,) = cb.run([a])
    assert out_a.tolist() == [10, 11, 12, 13, 14, 15]
    assert _calls(e, "prediction", "prefill", "release") == [("prediction", 0, (10, 11, 99, 13)), ("prefill", (0,)), ("release", 0)]
    assert a.prediction_stats == {"drafted": 4, "accepted": 3}       # read before the release cleared it
    # the slot is admitted again without one: an explicit clear before its prefill; then no call at all
    e.log.clear()
    b = _req()
    cb.run([b])
    assert _calls(e, "prediction", "prefill", "release") == [("prediction", 0, None), ("prefill", (0,)), ("release", 0)]
    assert not hasattr(b, "prediction_stats")
    e.log.clear()
    cb.run([_req()])
    assert _calls(e, "prediction") == []
    # two at once: each slot its own
    e.log.clear()
    cb.run([_req(prediction=[1]), _req(prediction=[2, 3])])
    assert _calls(e, "prediction", "prefill") == [("prediction", 0, (1,)), ("prediction", 1, (2, 3)), ("prefill", (0, 1))]


def test_scheduler_refusals_name_the_prediction():
    e = _engine()
    e.slots_fork = e.slots_beam = e.slots_extend = e.slots_score = lambda *a, **k: None
    cb = ContinuousBatcher(e)
    for kw in (dict(n=2), dict(num_beams=2), dict(score=[[1, 2]]), dict(suffixes=[[1], [2]])):
        with pytest.raises(RequestRejected, match="prediction"):
            cb.submit(_req(prediction=[1, 2], **kw))
    for bad in ([-1], ["x"], 5, [0] * 129):
        with pytest.raises(RequestRejected, match="prediction"):
            cb.submit(_req(prediction=bad))
    assert not cb.pending and _calls(e, "prediction") == []
    # an engine without the call: static batching's stand-in
    plain = FakePagedEngine(lambda p: [10], 64, max_batch=2, max_patches=64, max_prefill_tokens=256, max_seq_len=128)
    with pytest.raises(RequestRejected, match="prediction"):
        ContinuousBatcher(plain).submit(_req(prediction=[1]))


def test_scheduler_inert_on_a_non_speculating_engine():
    outs = {}
    for k in (0, 3):
        e = _engine(spec_k=k)
        r = _req(prediction=[10, 11, 12])
        outs[k] = (ContinuousBatcher(e).run([r])[0].tolist(), r.prediction_stats, _calls(e, "prediction"))
    assert outs[0][0] == outs[3][0] and outs[0][2] == outs[3][2] == [("prediction", 0, (10, 11, 12))]      # validated and stored either way
    assert outs[0][1] == {"drafted": 0, "accepted": 0} and outs[3][1] == {"drafted": 3, "accepted": 3}
    e = _engine(spec_k=0)
    assert ContinuousBatcher(e).run([_req(prediction=[])])[0].tolist() == outs[0][0] and _calls(e, "prediction") == []


def test_row_features_table_is_unchanged():
    from dots_ocr_amd.row_features import ROW_FEATURES
    assert len(ROW_FEATURES) == 8 and "prediction" not in {f.name for f in ROW_FEATURES}
    assert "prediction" in (ROOT / "dots_ocr_amd" / "row_features.py").read_text().split('"""')[1]


# ---------------------------------------------------------------------------------------------------- 5. the server

fastapi = pytest.importorskip("fastapi")
from fastapi.testclient import TestClient  # noqa: E402

TEXT = "total 42 EUR"


class _Model:
    def __init__(self, proc, cfg, engine):
        self.config, self.engine = cfg, engine


def _payload(**kw):
    body = {"model": "model", "messages": [{"role": "user", "content": "read"}], "max_completion_tokens": 64, "temperature": 0}
    body.update(kw)
    return body


@pytest.fixture()
def served():
    from dots_ocr_amd.server import create_app
    cfg = DotsConfig.tiny()
    proc = DotsOcrProcessor(cfg)
    e = PredEngine(lambda p: proc.tokenizer.encode(TEXT) + [cfg.eos_token_ids[0]], 4096, max_batch=4, max_patches=4096, max_prefill_tokens=4096,
                   max_seq_len=2048)
    app = create_app(_Model(proc, cfg, e), proc, model_name="model", max_batch=4, look_ahead=0)
    with TestClient(app) as c:
        yield c, e, proc


def test_server_takes_both_content_shapes(served):
    c, e, proc = served
    plain = c.post("/v1/chat/completions", json=_payload()).json()
    assert "completion_tokens_details" not in plain["usage"] and _calls(e, "prediction") == []
    assert sorted(plain["usage"]) == ["completion_tokens", "prompt_tokens", "total_tokens"]      # byte for byte what it was
    n = len(proc.tokenizer.encode(TEXT))
    for content, ids, acc in ((TEXT, proc.tokenizer.encode(TEXT), n),
                              ([{"type": "text", "text": "total 4"}, {"type": "text", "text": "3 EUR"}], proc.tokenizer.encode("total 43 EUR"), n - 1)):
        e.log.clear()
        r = c.post("/v1/chat/completions", json=_payload(prediction={"type": "content", "content": content}))
        assert r.status_code == 200, r.text
        body = r.json()
        assert body["choices"] == plain["choices"]
        assert _calls(e, "prediction")[0] == ("prediction", 0, tuple(ids))
        assert body["usage"] == {**plain["usage"], "completion_tokens_details": {"accepted_prediction_tokens": acc, "rejected_prediction_tokens": n - acc}}
    r = c.post("/v1/chat/completions", json=_payload(prediction=None))
    assert r.status_code == 200 and r.json()["usage"] == plain["usage"]


def test_server_400s(served):
    c, e, proc = served
    for bad in ("text", {"type": "content"}, {"type": "tokens", "content": "a"}, {"type": "content", "content": "a", "extra": 1},
                {"type": "content", "content": 5}, {"type": "content", "content": [{"type": "image", "text": "a"}]},
                {"type": "content", "content": [{"type": "text", "text": 1}]}, {"type": "content", "content": []},
                {"type": "content", "content": "x" * 2049}):          # longer than max_seq_len: refused, not cut
        r = c.post("/v1/chat/completions", json=_payload(prediction=bad))
        assert r.status_code == 400 and "prediction" in r.json()["detail"], bad
    ok = {"type": "content", "content": "a"}
    for kw in (dict(n=2), dict(use_beam_search=True), dict(score_candidates=["a"]), dict(prompts=["a", "b"])):
        r = c.post("/v1/chat/completions", json=_payload(prediction=ok, **kw))
        assert r.status_code == 400 and "prediction" in r.json()["detail"], kw
    assert _calls(e, "prediction") == []


def test_server_static_batching_is_a_400():
    from dots_ocr_amd.server import create_app
    cfg = DotsConfig.tiny()
    proc = DotsOcrProcessor(cfg)
    e = PredEngine(lambda p: [65, cfg.eos_token_ids[0]], 4096, max_batch=4, max_patches=4096, max_prefill_tokens=4096, max_seq_len=2048)
    with TestClient(create_app(_Model(proc, cfg, e), proc, continuous=False)) as c:
        r = c.post("/v1/chat/completions", json=_payload(prediction={"type": "content", "content": "a"}))
        assert r.status_code == 400 and "prediction" in r.json()["detail"] and "static" in r.json()["detail"]


def test_server_streams_the_details_in_the_usage_chunk(served):
    c, e, proc = served
    pred = {"type": "content", "content": TEXT}
    plain = c.post("/v1/chat/completions", json=_payload(prediction=pred)).json()
    r = c.post("/v1/chat/completions", json=_payload(prediction=pred, stream=True, stream_options={"include_usage": True}))
    assert r.status_code == 200 and r.headers["content-type"].startswith("text/event-stream")
    data = [ln[6:] for block in r.text.split("\n\n") for ln in block.split("\n") if ln.startswith("data: ")]
    assert data[-1] == "[DONE]"
    chunks = [json.loads(d) for d in data[:-1]]
    assert "".join(ch["choices"][0]["delta"].get("content", "") for ch in chunks if ch["choices"]) == TEXT
    assert chunks[-1]["choices"] == [] and chunks[-1]["usage"] == plain["usage"]
    assert chunks[-1]["usage"]["completion_tokens_details"]["accepted_prediction_tokens"] == len(proc.tokenizer.encode(TEXT))
    # a streamed request without the field: its usage chunk has no details
    r = c.post("/v1/chat/completions", json=_payload(stream=True, stream_options={"include_usage": True}))
    last = [json.loads(ln[6:]) for block in r.text.split("\n\n") for ln in block.split("\n") if ln.startswith("data: ") and ln[6:] != "[DONE]"][-1]
    assert "completion_tokens_details" not in last["usage"]
