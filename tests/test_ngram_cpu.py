"""No-repeat n-gram blocking, the parts that need no GPU: the host restatement of the ban against transformers' processor,
the window and whitelist by hand, NgramRule validation, the scheduler's routing and the server's fields."""
import time

import numpy as np
import pytest

from dots_ocr_amd.config import DotsConfig
from dots_ocr_amd.engine import MAX_NGRAM_SIZE, MAX_NGRAM_WHITELIST, NgramRule, banned_ngram_ids
from dots_ocr_amd.row_features import rows_holding


# ---------------------------------------------------------------------------------------------------- the definition

def test_restatement_equals_transformers_processor():
    """window 0, no whitelist: exactly what NoRepeatNGramLogitsProcessor(n) bans when it is given the generated tokens as input_ids"""
    import torch
    from transformers.generation.logits_process import NoRepeatNGramLogitsProcessor
    rng = np.random.default_rng(0)
    non_empty = 0
    for case in range(3000):
        V = int(rng.integers(2, 6))
        L = int(rng.integers(0, 40))
        n = int(rng.integers(1, 6))
        out = rng.integers(0, V, size=L)
        scores = NoRepeatNGramLogitsProcessor(n)(torch.from_numpy(out.astype(np.int64))[None, :], torch.zeros(1, V))
        want = set(torch.nonzero(torch.isinf(scores[0])).flatten().tolist())
        got = banned_ngram_ids(out, n)
        assert got == want, (case, V, L, n, out.tolist())
        non_empty += bool(want)
    assert non_empty > 1500, non_empty                     # the comparison is not one of empty sets


def test_window_and_whitelist_by_hand():
    # the bigram (7, 8) sits at i = 1 of L = 6 tokens; the last token is 7 again, so n = 2 bans 8
    out = [1, 7, 8, 2, 3, 7]
    assert banned_ngram_ids(out, 2) == {8}
    assert banned_ngram_ids(out, 2, window=5) == {8}       # i = 1 = L - W: the first token of the match is the oldest one in the window
    assert banned_ngram_ids(out, 2, window=4) == set()     # i = 1 = L - W - 1: just outside
    # the last possible match, i = L - n: the n-gram ends at the last token but one
    assert banned_ngram_ids([4, 5, 5], 2) == {5}
    assert banned_ngram_ids([4, 5, 5], 2, window=2) == {5}
    assert banned_ngram_ids([3, 4, 9, 3, 4], 3) == {9}
    # L = n - 2: there is no full prefix yet; L = n - 1: a prefix, but no earlier n-gram
    assert banned_ngram_ids([1], 3) == set() and banned_ngram_ids([1, 1], 3) == set() and banned_ngram_ids([], 2) == set()
    # n = 1: every token of the window is banned
    assert banned_ngram_ids([5, 6, 7, 6], 1) == {5, 6, 7}
    assert banned_ngram_ids([5, 6, 7, 6], 1, window=2) == {6, 7}
    assert banned_ngram_ids([], 1) == set()
    # a whitelisted continuation stays
    assert banned_ngram_ids(out, 2, whitelist=[8]) == set()
    assert banned_ngram_ids([5, 6, 7, 6], 1, whitelist=[6]) == {5, 7}
    # two matches ban two different ids; the window drops the older one
    two = [7, 8, 0, 7, 9, 0, 7]
    assert banned_ngram_ids(two, 2) == {8, 9}
    assert banned_ngram_ids(two, 2, window=4) == {9}
    assert banned_ngram_ids(two, 2, whitelist=[9]) == {8}


# ---------------------------------------------------------------------------------------------------- NgramRule

def test_ngram_rule_normalises():
    r = NgramRule(np.int64(3), 8, [5, 4], vocab_size=10, max_seq_len=64)
    assert (r.size, r.window, r.whitelist) == (3, 8, (5, 4)) and isinstance(r.size, int)
    assert NgramRule(1).window == 0 and NgramRule(MAX_NGRAM_SIZE).size == MAX_NGRAM_SIZE
    NgramRule(4, 4)                                          # a window of exactly one n-gram
    NgramRule(2, whitelist=range(MAX_NGRAM_WHITELIST))
    with pytest.raises(Exception):
        r.size = 4                                           # frozen
    c = NgramRule(3, 8, [5, 4]).to_c()
    assert (c.size, c.window, c.n_whitelist) == (3, 8, 2) and list(c.whitelist)[:3] == [5, 4, 0]


@pytest.mark.parametrize("bad", [dict(size=0), dict(size=-1), dict(size=MAX_NGRAM_SIZE + 1), dict(size=2.0), dict(size=True), dict(size="3"),
                                 dict(size=3, window=2), dict(size=3, window=-1), dict(size=3, window=1.5), dict(size=3, window=65, max_seq_len=64),
                                 dict(size=2, whitelist=[1, 1]), dict(size=2, whitelist=[-1]), dict(size=2, whitelist=[1.5]),
                                 dict(size=2, whitelist=[10], vocab_size=10), dict(size=2, whitelist=list(range(MAX_NGRAM_WHITELIST + 1)))])
def test_ngram_rule_rejects(bad):
    with pytest.raises(ValueError):
        NgramRule(**bad)


# ---------------------------------------------------------------------------------------------------- scheduler

def _ngram_engine(base):
    """a slot engine with set_row_ngram: a log of the calls in order, and the rule each row held when it was prefilled"""
    class NgramEngine(base):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            self.ngram, self.calls, self.prefill_ngram = {}, [], []

        def set_row_ngram(self, row, rule):
            self.calls.append(("set", row, rule))
            if rule is None:
                self.ngram.pop(row, None)
            else:
                self.ngram[row] = rule

        def slots_prefill(self, slots, ids, lens, caps):
            off = 0
            for s, n in zip(slots, lens):
                self.prefill_ngram.append((s, int(ids[off]), self.ngram.get(s)))
                off += n
            super().slots_prefill(slots, ids, lens, caps)

        def slot_release(self, s):
            self.calls.append(("release", s, self.ngram.get(s)))
            super().slot_release(s)
    return NgramEngine


def test_scheduler_sets_the_rule_before_the_prefill_and_clears_it_on_release():
    from fakes import FakeSlotEngine
    from dots_ocr_amd.scheduler import ContinuousBatcher, Request
    eng = _ngram_engine(FakeSlotEngine)(lambda prompt: [5, 6, 7, 8], max_batch=2, max_prefill_tokens=64)
    rules = [NgramRule(2), None, NgramRule(3, 8, [5]), None, None]
    reqs = [Request(np.array([10 + i, 1, 2], np.int32), max_new_tokens=4, ngram=r) for i, r in enumerate(rules)]
    cb = ContinuousBatcher(eng, chunk=2)
    outs = cb.run(reqs)
    assert [list(o) for o in outs] == [[5, 6, 7, 8]] * 5
    assert len(eng.prefill_ngram) == len(reqs)
    for slot, first, seen in eng.prefill_ngram:              # every request was prefilled with its own rule on its row, or with none
        assert seen is rules[first - 10], (slot, first)
    # a rule is taken off its row before the slot is released: no release ever sees one, and none is left at the end
    assert [c for c in eng.calls if c[0] == "release" and c[2] is not None] == []
    assert sum(1 for c in eng.calls if c[0] == "release") == len(reqs)
    assert [c[2] for c in eng.calls if c[0] == "set" and c[2] is not None] == [rules[0], rules[2]]
    assert eng.ngram == {} and rows_holding(cb._rows, "ngram") == []


def test_scheduler_without_a_rule_makes_no_ngram_calls():
    from fakes import FakeSlotEngine
    from dots_ocr_amd.scheduler import ContinuousBatcher, Request
    eng = _ngram_engine(FakeSlotEngine)(lambda prompt: [5] * 4, max_batch=2, max_prefill_tokens=64)
    ContinuousBatcher(eng, chunk=2).run([Request(np.array([1 + i, 2], np.int32), max_new_tokens=3) for i in range(4)])
    assert [c for c in eng.calls if c[0] == "set"] == []


def test_scheduler_clears_the_rule_when_the_prefill_fails():
    from fakes import FakeSlotEngine
    from dots_ocr_amd.scheduler import ContinuousBatcher, Request
    eng = _ngram_engine(FakeSlotEngine)(lambda prompt: [5] * 4, max_batch=2, max_prefill_tokens=64)

    def fail(*a):
        raise RuntimeError("KV pool exhausted")
    eng.slots_prefill = fail
    cb = ContinuousBatcher(eng, chunk=2)
    r = NgramRule(2)
    cb.submit(Request(np.array([1, 2], np.int32), max_new_tokens=3, ngram=r))
    with pytest.raises(RuntimeError):
        cb.step()
    assert eng.ngram == {} and rows_holding(cb._rows, "ngram") == []
    assert eng.calls == [("set", 0, r), ("set", 0, None)]


def test_scheduler_refuses_a_rule_on_an_engine_without_the_call():
    from fakes import FakeSlotEngine
    from dots_ocr_amd.scheduler import ContinuousBatcher, Request
    cb = ContinuousBatcher(FakeSlotEngine(lambda prompt: [5] * 4, max_batch=2, max_prefill_tokens=64), chunk=2)
    with pytest.raises(ValueError):
        cb.submit(Request(np.array([1, 2], np.int32), max_new_tokens=3, ngram=NgramRule(2)))
    cb.submit(Request(np.array([1, 2], np.int32), max_new_tokens=3))


# ---------------------------------------------------------------------------------------------------- server

class _Model:
    def __init__(self, cfg, proc, ngram=True):
        from fakes import FakeSlotEngine

        class Eng(FakeSlotEngine):
            def slots_decode(self, n):
                time.sleep(0.002)
                super().slots_decode(n)
        script = lambda prompt: proc.tokenizer.encode("ok then") + [cfg.eos_token_ids[0]] + proc.tokenizer.encode("more")     # noqa: E731
        self.config = cfg
        self.engine = (_ngram_engine(Eng) if ngram else Eng)(script, max_batch=2, max_patches=4096, max_prefill_tokens=4096, max_seq_len=2048)


def _payload(**kw):
    body = {"model": "model", "messages": [{"role": "user", "content": "Read this."}], "max_completion_tokens": 32}
    body.update(kw)
    return body


def _app(ngram=True, continuous=True):
    pytest.importorskip("fastapi")
    from dots_ocr_amd.processing import DotsOcrProcessor
    from dots_ocr_amd.server import create_app
    cfg = DotsConfig.tiny()
    proc = DotsOcrProcessor(cfg)
    return cfg, proc, create_app(_Model(cfg, proc, ngram), proc, model_name="model", max_batch=2, continuous=continuous)


def test_server_parses_the_fields_and_rejects_bad_values():
    from fastapi.testclient import TestClient
    cfg, _, app = _app()
    V = cfg.vocab_size
    eng = app.state.worker.model.engine
    with TestClient(app) as c:
        for bad in (dict(no_repeat_ngram_size=-1), dict(no_repeat_ngram_size=1.5), dict(no_repeat_ngram_size=True), dict(no_repeat_ngram_size="3"),
                    dict(no_repeat_ngram_size=MAX_NGRAM_SIZE + 1),
                    dict(no_repeat_ngram_size=3, no_repeat_ngram_window=2), dict(no_repeat_ngram_size=3, no_repeat_ngram_window=-1),
                    dict(no_repeat_ngram_size=3, no_repeat_ngram_window=2049), dict(no_repeat_ngram_size=3, no_repeat_ngram_window="8"),
                    dict(no_repeat_ngram_size=2, no_repeat_ngram_whitelist=[V]), dict(no_repeat_ngram_size=2, no_repeat_ngram_whitelist=[-1]),
                    dict(no_repeat_ngram_size=2, no_repeat_ngram_whitelist=[1, 1]), dict(no_repeat_ngram_size=2, no_repeat_ngram_whitelist=7),
                    dict(no_repeat_ngram_size=2, no_repeat_ngram_whitelist=[1.5]),
                    dict(no_repeat_ngram_size=2, no_repeat_ngram_whitelist=list(range(MAX_NGRAM_WHITELIST + 1))),
                    dict(no_repeat_ngram_window=8), dict(no_repeat_ngram_whitelist=[3]), dict(no_repeat_ngram_size=0, no_repeat_ngram_window=8)):
            r = c.post("/v1/chat/completions", json=_payload(**bad))
            assert r.status_code == 400 and "n-gram" in r.text, (bad, r.text)
        assert [x for x in eng.calls if x[0] == "set"] == []
        # no_repeat_ngram_size = 0 is "off", as in Hugging Face: no rule travels
        assert c.post("/v1/chat/completions", json=_payload(no_repeat_ngram_size=0)).status_code == 200
        assert c.post("/v1/chat/completions", json=_payload()).status_code == 200
        assert [x for x in eng.calls if x[0] == "set"] == []
        r = c.post("/v1/chat/completions", json=_payload(no_repeat_ngram_size=3, no_repeat_ngram_window=8, no_repeat_ngram_whitelist=[5, 4]))
        assert r.status_code == 200 and r.json()["choices"][0]["message"]["content"] == "ok then"
    sets = [x[2] for x in eng.calls if x[0] == "set"]
    assert sets[0] == NgramRule(3, 8, (5, 4), vocab_size=V, max_seq_len=2048) and sets[1:] == [None]
    assert eng.prefill_ngram[-1][2] is sets[0]


def test_server_refuses_the_fields_where_the_worker_cannot_honour_them():
    from fastapi.testclient import TestClient
    _, _, app = _app(continuous=False)                       # static batches through model.generate
    with TestClient(app) as c:
        r = c.post("/v1/chat/completions", json=_payload(no_repeat_ngram_size=3))
        assert r.status_code == 400 and "no_repeat_ngram_size" in r.text and "continuous batching" in r.text, r.text
    _, _, app = _app(ngram=False)                            # slots, but an engine without set_row_ngram
    with TestClient(app) as c:
        r = c.post("/v1/chat/completions", json=_payload(no_repeat_ngram_size=3))
        assert r.status_code == 400 and "Engine.set_row_ngram" in r.text, r.text
        assert c.post("/v1/chat/completions", json=_payload()).status_code == 200


# ---------------------------------------------------------------------------------------------------- parser

def test_parser_sends_the_fields_only_when_they_are_set(monkeypatch):
    import dots_ocr.model.inference as inf
    from dots_ocr_amd.parser import DotsOCRParser
    seen = []
    monkeypatch.setattr(inf, "inference_with_vllm", lambda image, prompt, **kw: seen.append(kw) or "x")
    DotsOCRParser(output_dir="/tmp")._inference_with_vllm(None, "p")
    assert "extra_body" not in seen[-1]                      # the default: the request is what it always was
    DotsOCRParser(output_dir="/tmp", no_repeat_ngram_size=30, no_repeat_ngram_window=90, no_repeat_ngram_whitelist=[7, 8])._inference_with_vllm(None, "p")
    assert seen[-1]["extra_body"] == {"no_repeat_ngram_size": 30, "no_repeat_ngram_window": 90, "no_repeat_ngram_whitelist": [7, 8]}

    class M:
        def generate(self, **kw):
            seen.append(kw)
            import torch
            return torch.zeros(1, 3, dtype=torch.long)

    class P:
        def batch_decode(self, t, **kw):
            return ["x"]
    for kw, want in ((dict(), {}), (dict(no_repeat_ngram_size=4), {"no_repeat_ngram_size": 4})):
        p = DotsOCRParser(output_dir="/tmp", model=M(), processor=P(), **kw)
        import torch
        monkeypatch.setattr(p, "_build_inputs", lambda images, prompts: type("I", (dict,), {"input_ids": torch.zeros(1, 2, dtype=torch.long)})())
        p._inference_batch_with_hf([None], ["p"])
        assert {k: v for k, v in seen[-1].items() if k != "max_new_tokens"} == want
