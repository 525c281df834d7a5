"""Per-request logit rules above the kernels, on CPU: validation of engine.LogitRules, the scheduler's
set_row_logit_rules calls around a slot's life, and the server's logit_bias / allowed_token_ids / min_tokens / stop_token_ids /
ignore_eos fields."""
import math
import time

import numpy as np
import pytest

from dots_ocr_amd.config import DotsConfig
from dots_ocr_amd.engine import MAX_LOGIT_BIAS, MAX_STOP_IDS, LogitRules
from dots_ocr_amd.row_features import rows_holding


# ---------------------------------------------------------------------------------------------------- LogitRules

def test_logit_rules_normalises_and_reports_empty():
    assert LogitRules().empty
    r = LogitRules(bias={7: 1.5, 3: -math.inf}, allowed=[9, 3, 7, 7], min_tokens=2, stop=[4, 5], ignore_eos=1, vocab_size=16)
    assert not r.empty
    assert r.bias == ((7, 1.5), (3, -math.inf)) and r.allowed == (3, 7, 9) and r.stop == (4, 5)
    assert r.min_tokens == 2 and r.ignore_eos is True
    assert LogitRules(bias=[(1, 0.1)]).bias[0][1] == np.float32(0.1)            # the fp32 value the engine receives
    for one in (dict(bias={1: 0.0}), dict(allowed=[1]), dict(min_tokens=1), dict(stop=[1]), dict(ignore_eos=True)):
        assert not LogitRules(**one).empty
    with pytest.raises(Exception):                                             # frozen
        r.min_tokens = 3


@pytest.mark.parametrize("bad", [
    dict(bias={1: math.nan}), dict(bias={1: math.inf}), dict(bias=[(1, 0.5), (1, 0.25)]), dict(bias={-1: 0.5}), dict(bias={1.5: 0.5}),
    dict(bias={i: 0.0 for i in range(MAX_LOGIT_BIAS + 1)}),
    dict(allowed=[]), dict(allowed=[-2]), dict(allowed=[True]),
    dict(min_tokens=-1), dict(min_tokens=1.5), dict(min_tokens=True),
    dict(stop=list(range(MAX_STOP_IDS + 1))), dict(stop=[-1]),
    dict(bias={16: 1.0}, vocab_size=16), dict(allowed=[3, 16], vocab_size=16), dict(stop=[16], vocab_size=16),
])
def test_logit_rules_rejects(bad):
    with pytest.raises(ValueError):
        LogitRules(**bad)


def test_logit_rules_rejects_what_could_never_select_a_token():
    with pytest.raises(ValueError):
        LogitRules(allowed=[2, 3], bias={2: -math.inf, 3: -math.inf})
    with pytest.raises(ValueError):
        LogitRules(allowed=[2, 3], stop=[3, 2, 9], min_tokens=1)
    with pytest.raises(ValueError):
        LogitRules(allowed=[2, 3], bias={2: -math.inf}, stop=[3], min_tokens=4)
    LogitRules(allowed=[2, 3], stop=[3, 2])                                    # without min_tokens a stop id can be selected
    LogitRules(allowed=[2, 3], bias={2: -math.inf}, stop=[2], min_tokens=4)
    LogitRules(bias={2: -math.inf}, stop=[3], min_tokens=4)                    # no allowed list: the rest of the vocabulary remains


def test_logit_rules_to_c_layout():
    r = LogitRules(bias={7: 1.5, 3: -math.inf}, allowed=[9, 3], min_tokens=2, stop=[4, 5], ignore_eos=True)
    c = r.to_c()
    assert c.n_bias == 2 and [c.bias_ids[j] for j in range(2)] == [7, 3]
    assert c.bias_values[0] == 1.5 and c.bias_values[1] == -math.inf
    assert c.n_allowed == 2 and [c.allowed_ids[j] for j in range(2)] == [3, 9]
    assert (c.min_tokens, c.n_stop, c.ignore_eos) == (2, 2, 1) and list(c.stop_ids)[:2] == [4, 5]
    c = LogitRules(min_tokens=1).to_c()
    assert not c.bias_ids and not c.allowed_ids and c.n_bias == 0 and c.n_allowed == 0


# ---------------------------------------------------------------------------------------------------- scheduler

def _rules_engine(base):
    """a slot engine with set_row_logit_rules: a log of the calls, and a row's stop ids / ignore_eos honoured as the device does"""
    class RulesEngine(base):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            self.rules, self.rule_calls, self.prefill_rules = {}, [], []

        def set_row_logit_rules(self, row, rules):
            self.rule_calls.append((row, rules))
            if rules is None:
                self.rules.pop(row, None)
            else:
                self.rules[row] = rules

        def _advance(self, st):
            if st["done"]:
                return
            r = st.get("rules")
            tok = st["plan"][len(st["out"])] if len(st["out"]) < len(st["plan"]) else 0
            st["out"].append(int(tok))
            eos = set() if (r is not None and r.ignore_eos) else set(self.eos)
            eos |= set(r.stop) if r is not None else set()
            st["done"] = tok in eos or len(st["out"]) >= st["cap"]

        def slots_prefill(self, slots, ids, lens, caps):
            off = 0
            for s, n in zip(slots, lens):
                self.prefill_rules.append((s, int(ids[off]), self.rules.get(s)))
                off += n
            real = self._advance
            self._advance = lambda st: None                  # attach the row's rules before its first token is selected
            try:
                super().slots_prefill(slots, ids, lens, caps)
            finally:
                self._advance = real
            for s in slots:
                self.slots[s]["rules"] = self.rules.get(s)
                self._advance(self.slots[s])

        def slot_release(self, s):                           # the engine clears the row with the slot (dots_slot_release)
            self.rules.pop(s, None)
            super().slot_release(s)
    return RulesEngine


def test_scheduler_sets_rules_before_the_prefill():
    from fakes import FakeSlotEngine
    from dots_ocr_amd.scheduler import ContinuousBatcher, Request
    eng = _rules_engine(FakeSlotEngine)(lambda prompt: [5, 6, 7, 8, 9, 10], max_batch=2, max_prefill_tokens=64)
    rules = [LogitRules(stop=[7]), None, LogitRules(min_tokens=2), None, LogitRules(stop=[5]), None]
    reqs = [Request(np.array([10 + i, 1, 2], np.int32), max_new_tokens=6, rules=r) for i, r in enumerate(rules)]
    outs = ContinuousBatcher(eng, chunk=2).run(reqs)
    assert len(eng.prefill_rules) == len(reqs)
    for slot, first, seen in eng.prefill_rules:
        assert seen is rules[first - 10], (slot, first)
    assert [list(o) for o in outs] == [[5, 6, 7], [5, 6, 7, 8, 9, 10], [5, 6, 7, 8, 9, 10], [5, 6, 7, 8, 9, 10], [5], [5, 6, 7, 8, 9, 10]]


def test_scheduler_clears_rules_on_reuse_by_a_request_without_rules():
    from fakes import FakeSlotEngine
    from dots_ocr_amd.scheduler import ContinuousBatcher, Request
    eng = _rules_engine(FakeSlotEngine)(lambda prompt: [5] * 6, max_batch=1, max_prefill_tokens=64)
    eng.slot_release = FakeSlotEngine.slot_release.__get__(eng)          # an engine that keeps the rules until told otherwise
    r = LogitRules(stop=[9])
    ContinuousBatcher(eng, chunk=2).run([Request(np.array([1, 2], np.int32), max_new_tokens=3, rules=r),
                                         Request(np.array([3, 4], np.int32), max_new_tokens=3)])
    assert eng.rule_calls == [(0, r), (0, None)]
    assert [p[2] for p in eng.prefill_rules] == [r, None]


def test_scheduler_clears_rules_when_the_prefill_fails():
    from fakes import FakeSlotEngine
    from dots_ocr_amd.scheduler import ContinuousBatcher, Request
    eng = _rules_engine(FakeSlotEngine)(lambda prompt: [5] * 4, max_batch=2, max_prefill_tokens=64)

    def fail(*a):
        raise RuntimeError("KV pool exhausted")
    eng.slots_prefill = fail
    cb = ContinuousBatcher(eng, chunk=2)
    r = LogitRules(min_tokens=2)
    cb.submit(Request(np.array([1, 2], np.int32), max_new_tokens=3, rules=r))
    with pytest.raises(RuntimeError):
        cb.step()
    assert eng.rules == {} and rows_holding(cb._rows, "rules") == []
    assert eng.rule_calls == [(0, r), (0, None)]


def test_scheduler_without_rules_makes_no_rule_calls():
    from fakes import FakeSlotEngine
    from dots_ocr_amd.scheduler import ContinuousBatcher, Request
    eng = _rules_engine(FakeSlotEngine)(lambda prompt: [5] * 4, max_batch=2, max_prefill_tokens=64)
    ContinuousBatcher(eng, chunk=2).run([Request(np.array([1 + i, 2], np.int32), max_new_tokens=3) for i in range(4)])
    assert eng.rule_calls == []


def _refusing(base, bad_first_ids):
    """an engine whose set_row_logit_rules refuses the rules of some requests (told apart by min_tokens), as the C check would"""
    class Refusing(_rules_engine(base)):
        def set_row_logit_rules(self, row, rules):
            if rules is not None and rules.min_tokens in bad_first_ids:
                self.rule_calls.append((row, "refused"))
                raise RuntimeError("logit rules: refused by the engine")
            super().set_row_logit_rules(row, rules)
    return Refusing


def test_a_request_the_engine_refuses_fails_alone():
    from fakes import FakeSlotEngine
    from dots_ocr_amd.engine import SamplingParams
    from dots_ocr_amd.scheduler import ContinuousBatcher, Request, RequestRejected
    eng = _refusing(FakeSlotEngine, {77})(lambda prompt: [5, 6, 7, 8], max_batch=2, max_prefill_tokens=64)
    eng.set_row_sampling = lambda row, p: eng.rule_calls.append((row, "sampling", p))
    cb = ContinuousBatcher(eng, chunk=2)
    good = [Request(np.array([10 + i, 1], np.int32), max_new_tokens=4, rules=LogitRules(stop=[7]) if i == 2 else None) for i in range(4)]
    bad = Request(np.array([99, 1], np.int32), max_new_tokens=4, rules=LogitRules(min_tokens=77), sampling=SamplingParams(temperature=0.5))
    ids = [cb.submit(r) for r in good[:1] + [bad] + good[1:]]
    done = {}
    while not cb.idle:
        for rid, req, toks in cb.step():
            done[rid] = (req, list(toks))
    assert set(done) == set(ids)
    req, toks = done[ids[1]]
    assert req is bad and toks == [] and isinstance(req.error, RequestRejected) and "refused" in str(req.error)
    for i, r in zip([ids[0]] + ids[2:], good):               # every other request finished with its own tokens
        assert getattr(done[i][0], "error", None) is None
        assert done[i][1] == ([5, 6, 7] if r.rules is not None else [5, 6, 7, 8])
    # nothing of the refused request stayed on its slot: its sampling entry was taken back, no rules are left anywhere
    assert eng.rules == {} and rows_holding(cb._rows, "rules") == [] and rows_holding(cb._rows, "sampling") == []
    assert (1, "sampling", None) in eng.rule_calls
    assert not any(first == 99 for _, first, _ in eng.prefill_rules)          # it never reached the prefill
    with pytest.raises(RequestRejected):                     # run(): the others finish, then the refusal is raised
        ContinuousBatcher(eng, chunk=2).run([Request(np.array([1, 2], np.int32), max_new_tokens=2),
                                             Request(np.array([3, 2], np.int32), max_new_tokens=2, rules=LogitRules(min_tokens=77))])


def test_submit_refuses_rules_that_the_batchers_eos_ids_make_unselectable():
    from fakes import FakeSlotEngine
    from dots_ocr_amd.scheduler import ContinuousBatcher, Request, RequestRejected
    eng = _rules_engine(FakeSlotEngine)(lambda prompt: [5] * 4, max_batch=2, max_prefill_tokens=64)
    cb = ContinuousBatcher(eng, eos_ids=[8, 9], chunk=2)
    for bad in (LogitRules(allowed=[8], min_tokens=1), LogitRules(allowed=[8, 9, 3], stop=[3], min_tokens=2),
                LogitRules(allowed=[8, 4], bias={4: -math.inf}, min_tokens=1)):
        with pytest.raises(RequestRejected):
            cb.submit(Request(np.array([1, 2], np.int32), max_new_tokens=3, rules=bad))
    assert not cb.pending and eng.rule_calls == []
    r = LogitRules(allowed=[8, 4], min_tokens=1)
    cb.submit(Request(np.array([1, 2], np.int32), max_new_tokens=3, rules=r))
    assert cb.pending[0][1].rules is r                       # checked, not replaced
    with pytest.raises(ValueError):
        LogitRules(allowed=[8], min_tokens=1, eos_ids=[8, 9])
    LogitRules(allowed=[8], min_tokens=0, eos_ids=[8, 9])


def test_scheduler_refuses_rules_on_an_engine_without_the_call():
    from fakes import FakeSlotEngine
    from dots_ocr_amd.scheduler import ContinuousBatcher, Request
    cb = ContinuousBatcher(FakeSlotEngine(lambda prompt: [5] * 4, max_batch=2, max_prefill_tokens=64), chunk=2)
    with pytest.raises(ValueError):
        cb.submit(Request(np.array([1, 2], np.int32), max_new_tokens=3, rules=LogitRules(min_tokens=1)))


# ---------------------------------------------------------------------------------------------------- server

class _Model:
    def __init__(self, cfg, proc, rules=True):
        from fakes import FakeSlotEngine

        class Eng(FakeSlotEngine):
            def slots_decode(self, n):
                time.sleep(0.002)
                super().slots_decode(n)
        script = lambda prompt: proc.tokenizer.encode("ok then") + [cfg.eos_token_ids[0]] + proc.tokenizer.encode("more")     # noqa: E731
        self.config = cfg
        self.engine = (_rules_engine(Eng) if rules else Eng)(script, max_batch=2, max_patches=4096, max_prefill_tokens=4096, max_seq_len=2048)


def _payload(**kw):
    body = {"model": "model", "messages": [{"role": "user", "content": "Read this."}], "max_completion_tokens": 32}
    body.update(kw)
    return body


def _app(rules=True, continuous=True):
    pytest.importorskip("fastapi")
    from dots_ocr_amd.processing import DotsOcrProcessor
    from dots_ocr_amd.server import create_app
    cfg = DotsConfig.tiny()
    proc = DotsOcrProcessor(cfg)
    return cfg, proc, create_app(_Model(cfg, proc, rules), proc, model_name="model", max_batch=2, continuous=continuous)


def test_server_rejects_bad_rule_fields():
    from fastapi.testclient import TestClient
    cfg, _, app = _app()
    V = cfg.vocab_size
    with TestClient(app) as c:
        for bad in (dict(logit_bias=[1, 2]), dict(logit_bias={"x": 1}), dict(logit_bias={"1": 101}), dict(logit_bias={"1": -100.5}),
                    dict(logit_bias={"1": "2"}), dict(logit_bias={"1": True}), dict(logit_bias={str(V): 1}), dict(logit_bias={"-1": 1}),
                    dict(logit_bias={"1": 1, "01": 2}),
                    dict(allowed_token_ids=[]), dict(allowed_token_ids=[V]), dict(allowed_token_ids="12"), dict(allowed_token_ids=[1.5]),
                    dict(allowed_token_ids=[3], logit_bias={"3": -100}, min_tokens=1, stop_token_ids=[3]),
                    dict(min_tokens=-1), dict(min_tokens=1.5), dict(min_tokens=True), dict(min_tokens=33),
                    dict(stop_token_ids=[V]), dict(stop_token_ids=7), dict(stop_token_ids=list(range(MAX_STOP_IDS + 1))),
                    dict(ignore_eos="yes"), dict(ignore_eos=1)):
            r = c.post("/v1/chat/completions", json=_payload(**bad))
            assert r.status_code == 400, (bad, r.text)
        assert c.post("/v1/chat/completions", json=_payload(min_tokens=32)).status_code == 200


def test_server_refuses_rules_where_the_worker_cannot_honour_them():
    from fastapi.testclient import TestClient
    fields = (dict(logit_bias={"5": 2}), dict(allowed_token_ids=[5, 6]), dict(min_tokens=2), dict(stop_token_ids=[5]), dict(ignore_eos=True))
    _, _, app = _app(continuous=False)                       # static batches through model.generate
    with TestClient(app) as c:
        for f in fields:
            r = c.post("/v1/chat/completions", json=_payload(**f))
            assert r.status_code == 400 and "logit" in r.text, (f, r.text)
    _, _, app = _app(rules=False)                            # slots, but an engine without set_row_logit_rules
    with TestClient(app) as c:
        for f in fields:
            assert c.post("/v1/chat/completions", json=_payload(**f)).status_code == 400, f
        assert c.post("/v1/chat/completions", json=_payload()).status_code == 200


def test_server_answers_400_for_rules_the_eos_ids_make_unselectable():
    from fastapi.testclient import TestClient
    cfg, _, app = _app()
    E = list(cfg.eos_token_ids)
    with TestClient(app) as c:
        for bad in (dict(allowed_token_ids=[E[0]], min_tokens=1), dict(allowed_token_ids=E + [70], stop_token_ids=[70], min_tokens=3)):
            r = c.post("/v1/chat/completions", json=_payload(**bad))
            assert r.status_code == 400 and "logit rules" in r.text, (bad, r.text)
        assert app.state.worker.model.engine.rule_calls == []
        assert c.post("/v1/chat/completions", json=_payload(allowed_token_ids=E + [70], min_tokens=3)).status_code == 200


def test_server_engine_refusal_is_a_400_for_that_request_and_the_others_finish():
    import threading
    from fakes import FakeSlotEngine
    from fastapi.testclient import TestClient
    pytest.importorskip("fastapi")
    from dots_ocr_amd.processing import DotsOcrProcessor
    from dots_ocr_amd.server import create_app
    cfg = DotsConfig.tiny()
    proc = DotsOcrProcessor(cfg)
    model = _Model(cfg, proc)

    class Slow(_refusing(FakeSlotEngine, {5}).__mro__[0]):
        def slots_decode(self, n):
            time.sleep(0.005)
            super().slots_decode(n)
    model.engine = Slow(model.engine.script, max_batch=2, max_patches=4096, max_prefill_tokens=4096, max_seq_len=2048)
    app = create_app(model, proc, model_name="model", max_batch=2, continuous=True)
    with TestClient(app) as c:
        res = {}

        def go(key, body):
            res[key] = c.post("/v1/chat/completions", json=_payload(**body))
        asks = {"a": dict(), "bad": dict(min_tokens=5), "b": dict(stop_token_ids=[32]), "c": dict()}
        th = [threading.Thread(target=go, args=(k, b)) for k, b in asks.items()]
        [t.start() for t in th]
        [t.join() for t in th]
        assert res["bad"].status_code == 400 and "refused" in res["bad"].text, res["bad"].text
        for k in ("a", "b", "c"):
            assert res[k].status_code == 200, (k, res[k].text)
            assert res[k].json()["choices"][0]["finish_reason"] == "stop"
        assert res["a"].json()["choices"][0]["message"]["content"] == "ok then"


def test_server_stop_id_finishes_with_stop_and_plain_requests_are_untouched():
    from fastapi.testclient import TestClient
    cfg, proc, app = _app()
    tk = proc.tokenizer
    ids = tk.encode("ok then")
    with TestClient(app) as c:
        plain = c.post("/v1/chat/completions", json=_payload())
        assert plain.status_code == 200
        d = plain.json()
        assert set(d) == {"id", "object", "created", "model", "choices", "usage"}
        assert d["choices"] == [{"index": 0, "message": {"role": "assistant", "content": "ok then"}, "finish_reason": "stop"}]
        assert d["usage"]["completion_tokens"] == len(ids) + 1                 # the EOS id included
        assert app.state.worker.model.engine.rule_calls == []                  # no rule call for a request without rules
        # an explicit null / false is a request without rules too
        same = c.post("/v1/chat/completions", json=_payload(logit_bias=None, ignore_eos=False, min_tokens=0, stop_token_ids=[])).json()
        assert same["choices"] == d["choices"] and same["usage"] == d["usage"]
        assert app.state.worker.model.engine.rule_calls == []

        r = c.post("/v1/chat/completions", json=_payload(stop_token_ids=[ids[2]]))
        assert r.status_code == 200, r.text
        d = r.json()
        assert d["choices"][0]["finish_reason"] == "stop" and d["usage"]["completion_tokens"] == 3
        assert d["choices"][0]["message"]["content"] == "ok "

        r = c.post("/v1/chat/completions", json=_payload(ignore_eos=True, max_completion_tokens=len(ids) + 3))
        d = r.json()
        assert d["choices"][0]["finish_reason"] == "length" and d["usage"]["completion_tokens"] == len(ids) + 3

        r = c.post("/v1/chat/completions", json=_payload(logit_bias={"65": -100, "66": 3.5}, allowed_token_ids=[65, 66, 67], min_tokens=2))
        assert r.status_code == 200, r.text
        calls = app.state.worker.model.engine.rule_calls
        sent = [x for _, x in calls if x is not None][-1]
        assert sent.bias == ((65, -100.0), (66, 3.5)) and sent.allowed == (65, 66, 67) and sent.min_tokens == 2
