"""Beam search without a GPU: the host model against exhaustive search and hand-computed cases, the exact early stop against
brute force, and the scheduler's and the server's handling of a beam request on stand-in engines."""
import itertools

import numpy as np
import pytest

from dots_ocr_amd.beam import backtrace, beam_search_host, may_stop, rank_hypotheses
from dots_ocr_amd.scheduler import ContinuousBatcher, Request, RequestRejected
from fakes import FakePagedEngine

V, DEPTH, EOS = 6, 4, 5
f32 = np.float32


def table_lm(seed, eos_bias=0.0):
    """a language model over 6 tokens given as a table: seeded logits per prefix, returned as the sorted top list of its log-softmax"""
    def top_fn(prefix):
        rng = np.random.default_rng([seed, len(prefix)] + [int(t) + 1 for t in prefix])
        logits = rng.normal(0, 2, V)
        logits[EOS] += eos_bias
        lp = (logits - np.log(np.exp(logits).sum())).astype(f32)
        order = sorted(range(V), key=lambda t: (-float(lp[t]), t))
        return np.array(order, np.int32), lp[order]
    return top_fn


def exhaustive(top_fn, max_new):
    """every hypothesis of the table model: non-EOS tokens ended by an EOS, or max_new non-EOS tokens; cum summed in fp32 in token order"""
    out = []

    def walk(prefix, cum):
        ids, lps = top_fn(prefix)
        for t, lp in zip(ids, lps):
            s = f32(cum + lp)
            if t == EOS:
                out.append((list(prefix) + [EOS], s, len(prefix)))
            elif len(prefix) + 1 == max_new:
                out.append((list(prefix) + [int(t)], s, max_new))
            else:
                walk(prefix + (int(t),), s)
    walk((), f32(0))
    return out


# ---------------------------------------------------------------------------------------------------- the host model
@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("penalty", [0.0, 1.0])
def test_a_wide_enough_group_is_exhaustive_search(seed, penalty):
    top_fn = table_lm(seed)
    completed, tr = beam_search_host(top_fn, V ** 3, DEPTH, [EOS])
    got = rank_hypotheses(completed, tr["parents"], tr["tokens"], tr["cum"][-1], DEPTH, penalty, 10 ** 6)
    want = exhaustive(top_fn, DEPTH)
    assert len(want) == sum(5 ** k for k in range(DEPTH)) + 5 ** DEPTH
    # every hypothesis that ends in an EOS is found; of the 5 ** 4 that reach the cap the group keeps its B best by cum, which — they have
    # one length — are the B best by score: the best B hypotheses overall are therefore exact
    assert sorted(tuple(h["tokens"]) for h in got if h["finish_reason"] == "stop") == sorted(tuple(h[0]) for h in want if h[0][-1] == EOS)
    score = lambda h: float(h[1]) / max(1, h[2]) ** penalty                              # noqa: E731
    want.sort(key=lambda h: -score(h))
    for g, w in zip(got[:V ** 3], want[:V ** 3]):            # no two of these seeds' scores tie
        assert g["tokens"] == w[0] and f32(g["cum"]) == w[1] and g["score"] == score(w)


def dict_lm(table):
    def top_fn(prefix):
        assert prefix in table, f"prefix {prefix} is asked for but no live beam holds it"
        ids, lps = table[prefix]
        return np.array(ids, np.int32), np.array(lps, f32)
    return top_fn


def test_eos_at_rank_one_and_at_the_last_rank():
    a, b, c, d, E = 1, 2, 3, 4, 9
    lm = dict_lm({(): ([a, E, b, c], [-0.5, -1.0, -2.0, -3.0]),
                  (a,): ([c, d, a, E], [-0.25, -0.5, -1.0, -4.0]),
                  (b,): ([a, b, c, d], [-0.125, -0.25, -3.0, -4.0])})
    completed, tr = beam_search_host(lm, 2, 2, [E])
    assert completed == [(0, 0, E, f32(-1.0)), (1, 0, E, f32(-4.5))]
    assert tr["parents"].tolist() == [[0, 0], [0, 0]] and tr["tokens"].tolist() == [[a, c], [b, d]]
    assert tr["cum"].tolist() == [[-0.5, -2.0], [-0.75, -1.0]]


def test_a_dead_beam_offers_nothing_not_even_an_eos():
    a, b, E = 1, 2, 9
    asked = []

    def lm(prefix):
        asked.append(prefix)
        return dict_lm({(): ([a, -1, -1, -1], [-0.5, 0, 0, 0]), (a,): ([E, b, -1, -1], [-0.25, -1.0, 0, 0]), (a, b): ([E, a, b, -1], [-1.0, -2.0, -2.0, 0])})(prefix)
    completed, tr = beam_search_host(lm, 2, 3, [E])
    assert asked == [(), (a,), (a, b)]                       # beam 1 is dead throughout: its list is never read
    assert completed == [(1, 0, E, f32(-0.75)), (2, 0, E, f32(-2.5))]
    assert tr["parents"].tolist() == [[0, 0, 0], [-1, -1, 0]] and tr["tokens"].tolist() == [[a, b, a], [-1, -1, b]]
    assert np.isneginf(tr["cum"][:2, 1]).all() and tr["cum"][2].tolist() == [-3.5, -3.5]


def test_a_tie_is_broken_by_beam_then_by_rank():
    a, b, x, y = 1, 2, 3, 4
    lm = dict_lm({(): ([a, b, -1, -1], [-1.0, -1.0, 0, 0]),
                  (a,): ([x, y, a, b], [-0.5, -0.5, -0.5, -0.5]), (b,): ([x, y, a, b], [-0.5, -0.5, -0.5, -0.5])})
    _, tr = beam_search_host(lm, 2, 2, [9])
    assert tr["parents"][:, 1].tolist() == [0, 0] and tr["tokens"][:, 1].tolist() == [x, y]
    lm = dict_lm({(): ([a, b, -1, -1], [-1.0, -1.0, 0, 0]),
                  (a,): ([x, y, a, b], [-0.75, -1.0, -2.0, -2.0]), (b,): ([y, x, a, b], [-0.5, -0.75, -2.0, -2.0])})
    _, tr = beam_search_host(lm, 2, 2, [9])                  # (b, y) wins alone; (a, x) and (b, x) tie: the lower beam
    assert tr["parents"][:, 1].tolist() == [1, 0] and tr["tokens"][:, 1].tolist() == [y, x]


def test_length_penalty_flips_the_winner():
    E = 9
    parents = np.array([[0, 0, 0, 0, 0], [0, 1, 1, 1, 1]], np.int32)
    tokens = np.array([[1, 2, 3, 4, 5], [6, 6, 6, 6, 6]], np.int32)
    completed = [(1, 0, E, f32(-1.0)), (4, 0, E, f32(-2.0))]
    dead = np.full(2, -np.inf, f32)
    short, long_ = [1, E], [1, 2, 3, 4, E]
    r0 = rank_hypotheses(completed, parents, tokens, dead, 5, 0.0, 2)        # -1 against -2
    r1 = rank_hypotheses(completed, parents, tokens, dead, 5, 1.0, 2)        # -1 / 1 against -2 / 4
    assert [h["tokens"] for h in r0] == [short, long_] and [h["score"] for h in r0] == [-1.0, -2.0]
    assert [h["tokens"] for h in r1] == [long_, short] and [h["score"] for h in r1] == [-0.5, -1.0]
    assert [h["finish_reason"] for h in r1] == ["stop", "stop"] and [h["cum"] for h in r1] == [-2.0, -1.0]
    live = rank_hypotheses([], parents, tokens, np.array([-3.0, -2.5], f32), 5, 1.0, 2)
    assert [(h["tokens"], h["finish_reason"]) for h in live] == [([6, 6, 6, 6, 6], "length"), ([1, 2, 3, 4, 5], "length")]


def test_backtrace_round_trips():
    completed, tr = beam_search_host(table_lm(7), 3, DEPTH, [EOS])
    held = [()] * 3
    for t in range(tr["tokens"].shape[1]):
        held = [held[tr["parents"][j, t]] + (int(tr["tokens"][j, t]),) if tr["parents"][j, t] >= 0 else None for j in range(3)]
        for j in range(3):
            if held[j] is not None:
                assert tuple(backtrace(tr["parents"], tr["tokens"], t, j)) == held[j]
    assert backtrace(tr["parents"], tr["tokens"], -1, 0) == []


def test_may_stop_never_changes_what_is_returned():
    fired = 0
    for seed, B, n_ret, penalty in itertools.product(range(40), (2, 3), (1, 2), (0.0, 1.0, 2.0)):
        lm = table_lm(seed, eos_bias=2.0)
        completed, tr = beam_search_host(lm, B, DEPTH, [EOS])
        steps = tr["tokens"].shape[1]
        final = rank_hypotheses(completed, tr["parents"], tr["tokens"], tr["cum"][-1], steps, penalty, n_ret)
        for t in range(1, steps):
            so_far = [r for r in completed if r[0] < t]
            assert not may_stop(so_far, tr["cum"][t - 1], DEPTH, -1.0, n_ret)
            if may_stop(so_far, tr["cum"][t - 1], DEPTH, penalty, n_ret):
                fired += 1
                early = rank_hypotheses(so_far, tr["parents"], tr["tokens"], np.full(B, -np.inf, f32), t, penalty, n_ret)
                assert [(h["tokens"], h["cum"]) for h in early] == [(h["tokens"], h["cum"]) for h in final], (seed, B, n_ret, penalty, t)
    assert fired > 50                                        # the test is not vacuous


# ---------------------------------------------------------------------------------------------------- scheduler
class FakeBeamEngine(FakePagedEngine):
    """FakePagedEngine + beam groups as the engine keeps them (slots.hip / beam.hip): full reservation when the group is made, one trace
    per group from the host model over a table LM seeded by the prompt, all slots released together"""

    def __init__(self, script, pool_pages, eos_bias=0.0, **kw):
        super().__init__(script, pool_pages, **kw)
        self.groups, self.eos_bias, self.spec_k = {}, eos_bias, 0

    def slots_beam(self, src, dst):
        st = self.slots[src]
        L, cap, B = len(st["prompt"]), st["cap"], 1 + len(dst)
        assert all(0 <= d < self.max_batch and d not in self.slots for d in dst) and len(st["out"]) == 1
        shared = L // 64
        own = (L + cap + 63) // 64 - shared
        need = own - (st["pages"] - shared) + 1 + len(dst) * (own + 1)
        if need > self.free:
            raise RuntimeError("KV pool exhausted")
        self.free -= need
        completed, tr = beam_search_host(table_lm(int(st["prompt"].sum()), self.eos_bias), B, cap, [EOS])
        g = dict(slots=[src] + list(dst), pages=st["pages"] + need, completed=completed, tr=tr, steps=1, total=tr["tokens"].shape[1])
        for s in g["slots"]:
            self.slots[s] = dict(prompt=st["prompt"], cap=cap, plan=[], out=[], done=False, pages=0, limit=L + cap, ctx=L, group=g)
        self.log.append(("beam", tuple(g["slots"])))
        self.last_prompt = st["prompt"]

    def slots_decode(self, n):
        for g in {id(st["group"]): st["group"] for st in self.slots.values() if "group" in st}.values():
            g["steps"] = min(g["steps"] + n, g["total"])
        plain = {s: st for s, st in self.slots.items() if "group" not in st}
        every, self.slots = self.slots, plain
        try:
            if plain:
                super().slots_decode(n)
            else:
                self.log.append(("decode", n, ()))
        finally:
            every.update(self.slots)
            self.slots = every

    def slots_poll(self):
        fin, lens = super().slots_poll()
        for s, st in self.slots.items():
            if "group" in st:
                fin[s], lens[s] = int(st["group"]["steps"] >= st["group"]["total"]), st["group"]["steps"]
        return fin, lens

    def beam_read(self, s):
        g = self.slots[s]["group"]
        n = g["steps"]
        return {"B": len(g["slots"]), "steps": n, "cum": g["tr"]["cum"][n - 1].copy(), "tokens": g["tr"]["tokens"][:, :n].copy(),
                "parents": g["tr"]["parents"][:, :n].copy(), "completed": [r for r in g["completed"] if r[0] < n]}

    def slot_release(self, s):
        g = self.slots[s].get("group")
        if g is None:
            return super().slot_release(s)
        self.free += g["pages"]
        for k in g["slots"]:
            del self.slots[k]
        self.log.append(("release_group", tuple(g["slots"])))


def _prompt(n, seed=0):
    return np.random.default_rng(seed).integers(10, 90, n).astype(np.int32)


def _engine(pool=64, max_batch=4, **kw):
    return FakeBeamEngine(lambda p: [7] * 400, pool, max_batch=max_batch, max_prefill_tokens=4096, max_seq_len=1024, **kw)


def test_a_beam_request_takes_b_slots_its_full_pages_and_is_reported_once_best_first():
    eng = _engine()
    cb = ContinuousBatcher(eng, eos_ids=[EOS], chunk=2)
    ids = _prompt(70)
    rid = cb.submit(Request(ids, max_new_tokens=DEPTH, num_beams=3, num_return=2, length_penalty=-1.0))      # a negative penalty: to the cap
    out = cb.step()
    assert not out and sorted(cb.running) == [0, 1, 2] and ("beam", (0, 1, 2)) in eng.log
    # one shared prompt page; per beam ceil(74 / 64) - 1 = 1 page and a spare
    assert eng.kv_pool_info() == (64, 64 - (1 + 3 * 2)) == (64, 64 - cb._beam_pages(cb.running[0][1]))
    done = []
    while not cb.idle:
        done += cb.step()
    assert [r for r, _, _ in done] == [rid] and not eng.slots and eng.kv_pool_info() == (64, 64)
    assert ("release_group", (0, 1, 2)) in eng.log
    req = done[0][1]
    completed, tr = beam_search_host(table_lm(int(ids.sum())), 3, DEPTH, [EOS])
    want = rank_hypotheses(completed, tr["parents"], tr["tokens"], tr["cum"][-1], tr["tokens"].shape[1], -1.0, 2)
    assert [o.tolist() for o in req.outputs] == [h["tokens"] for h in want] and done[0][2].tolist() == want[0]["tokens"]
    assert req.cumulative_logprobs == [h["cum"] for h in want] and req.finish_reasons == [h["finish_reason"] for h in want]
    assert req.beam_scores == sorted(req.beam_scores, reverse=True)


def test_the_head_of_the_queue_waits_for_its_slots_and_nothing_overtakes_it():
    eng = _engine(max_batch=4)
    cb = ContinuousBatcher(eng, eos_ids=[EOS], chunk=4)
    a = cb.submit(Request(_prompt(20, 1), max_new_tokens=9))
    b = cb.submit(Request(_prompt(21, 2), max_new_tokens=5))
    g = cb.submit(Request(_prompt(30, 3), max_new_tokens=DEPTH, num_beams=3, length_penalty=-1.0))
    c = cb.submit(Request(_prompt(22, 4), max_new_tokens=3))
    order = []
    while not cb.idle:
        order += [rid for rid, _, _ in cb.step()]
        if any(rid == g for rid, _ in cb.running.values()):
            assert a not in [rid for rid, _ in cb.running.values()] or len(cb.running) == 4
    pre = [e[1] for e in eng.log if e[0] in ("prefill", "beam")]
    assert pre[0] == (0, 1)                                  # a and b; two slots are free, the group of three waits and c behind it
    assert ("beam", (0, 2, 3)) in eng.log or ("beam", (1, 2, 3)) in eng.log
    assert order.index(b) < order.index(g) < order.index(c) and sorted(order) == [a, b, g, c]
    assert not eng.slots and eng.kv_pool_info() == (64, 64)


def test_a_group_waits_for_its_pages():
    eng = _engine(pool=8)
    cb = ContinuousBatcher(eng, eos_ids=[EOS], chunk=4, headroom_pages=0)
    a = cb.submit(Request(_prompt(100, 1), max_new_tokens=40))                 # 3 pages
    g = cb.submit(Request(_prompt(70, 2), max_new_tokens=DEPTH, num_beams=3, length_penalty=-1.0))      # 7 pages
    cb.step()
    assert [rid for rid, _ in cb.running.values()] == [a] and [rid for rid, _ in cb.pending] == [g]
    order = []
    while not cb.idle:
        order += [rid for rid, _, _ in cb.step()]
    assert order == [a, g]
    with pytest.raises(ValueError):                          # a group the whole pool could not hold
        cb.submit(Request(_prompt(70, 2), max_new_tokens=DEPTH, num_beams=4))


def test_a_group_ends_early_only_where_that_is_exact():
    ids = _prompt(40, 5)
    runs = {}
    for penalty in (1.0, -1.0):
        eng = _engine(eos_bias=4.0)
        cb = ContinuousBatcher(eng, eos_ids=[EOS], chunk=1)
        cb.submit(Request(ids, max_new_tokens=60, num_beams=2, length_penalty=penalty))
        done = []
        while not cb.idle:
            done += cb.step()
        runs[penalty] = (cb.decode_steps, done[0][1])
    completed, tr = beam_search_host(table_lm(int(ids.sum()), 4.0), 2, 60, [EOS])
    for penalty, (steps, req) in runs.items():
        want = rank_hypotheses(completed, tr["parents"], tr["tokens"], tr["cum"][-1], tr["tokens"].shape[1], penalty, 1)
        assert [o.tolist() for o in req.outputs] == [want[0]["tokens"]] and req.cumulative_logprobs == [want[0]["cum"]]
    total = tr["tokens"].shape[1]
    first = next(t for t in range(1, total + 1) if may_stop([r for r in completed if r[0] < t], tr["cum"][t - 1], 60, 1.0, 1))
    assert runs[1.0][0] == first - 1 < total - 1              # ended at the first poll where it was exact, well before the cap
    assert runs[-1.0][0] == total - 1                         # a negative penalty: to the cap


def _refused(cb, **kw):
    with pytest.raises(RequestRejected):
        cb.submit(Request(_prompt(20), max_new_tokens=4, **{"num_beams": 3, **kw}))
    assert not cb.pending


def test_every_forbidden_combination_is_refused():
    from dots_ocr_amd.engine import LogitRules, NgramRule, SamplingParams
    eng = _engine()
    for name in ("set_row_sampling", "set_row_logprobs", "set_row_logit_rules", "set_row_guide", "set_row_ngram", "set_row_stop"):
        setattr(eng, name, lambda *a, **k: None)
    cb = ContinuousBatcher(eng, eos_ids=[EOS])
    for sp in (SamplingParams(temperature=0.7), SamplingParams(temperature=0.0, top_k=4), SamplingParams(temperature=0.0, top_p=0.5),
               SamplingParams(temperature=0.0, repetition_penalty=1.2), SamplingParams(temperature=0.0, frequency_penalty=0.5),
               SamplingParams(temperature=0.0, presence_penalty=0.5)):
        _refused(cb, sampling=sp)
    _refused(cb, rules=LogitRules(allowed=[3]))
    _refused(cb, guide=0)
    _refused(cb, ngram=NgramRule(2))
    _refused(cb, stop=["ab"])
    _refused(cb, logprobs=0)
    _refused(cb, n=2)
    _refused(cb, num_return=4)
    _refused(cb, num_return=0)
    _refused(cb, num_beams=1)
    _refused(cb, num_beams=9)
    _refused(cb, length_penalty=float("nan"))
    eng.spec_k = 2
    _refused(cb)
    eng.spec_k = 0
    cb.submit(Request(_prompt(20), max_new_tokens=4, num_beams=3, sampling=SamplingParams(temperature=0.0)))      # plain greedy says nothing
    assert len(cb.pending) == 1
    plain = FakePagedEngine(lambda p: [7], 64)
    with pytest.raises(ValueError):                          # an engine without beam groups
        ContinuousBatcher(plain).submit(Request(_prompt(20), max_new_tokens=4, num_beams=2))


# ---------------------------------------------------------------------------------------------------- server
fastapi = pytest.importorskip("fastapi")


class _BeamModel:
    def __init__(self, cfg, beams=True):
        self.config = cfg
        self.engine = _engine(eos_bias=1.0) if beams else FakePagedEngine(lambda p: [7, cfg.eos_token_ids[0]], 64, max_batch=4, max_prefill_tokens=4096,
                                                                          max_seq_len=1024)


@pytest.fixture()
def served():
    from fastapi.testclient import TestClient
    from dots_ocr_amd.config import DotsConfig
    from dots_ocr_amd.processing import DotsOcrProcessor
    from dots_ocr_amd.server import create_app
    cfg = DotsConfig.tiny()
    cfg.eos_token_ids = [EOS]
    proc = DotsOcrProcessor(cfg)
    model = _BeamModel(cfg)
    with TestClient(create_app(model, proc, model_name="model", max_batch=4)) as c:
        yield c, model, proc


def _body(**kw):
    return {"messages": [{"role": "user", "content": "read this"}], "max_tokens": DEPTH, "temperature": 0, "use_beam_search": True, **kw}


def test_server_returns_the_hypotheses_best_first(served):
    c, model, proc = served
    r = c.post("/v1/chat/completions", json=_body(n=2, beam_width=3, length_penalty=0.5))
    assert r.status_code == 200, r.text
    d = r.json()
    ids = model.engine.last_prompt                           # the chat template's prompt, as the engine was given it
    completed, tr = beam_search_host(table_lm(int(ids.sum()), 1.0), 3, DEPTH, [EOS])
    steps = tr["tokens"].shape[1]
    want = rank_hypotheses(completed, tr["parents"], tr["tokens"], tr["cum"][-1], steps, 0.5, 2)
    assert [ch["index"] for ch in d["choices"]] == [0, 1]
    assert [ch["finish_reason"] for ch in d["choices"]] == [h["finish_reason"] for h in want]
    assert [ch["cumulative_logprob"] for ch in d["choices"]] == [h["cum"] for h in want]
    assert d["usage"]["completion_tokens"] == sum(len(h["tokens"]) for h in want) and d["usage"]["prompt_tokens"] == len(ids)
    assert not model.engine.slots
    one = c.post("/v1/chat/completions", json=_body(beam_width=3, length_penalty=0.5)).json()      # n absent: the best hypothesis alone
    assert len(one["choices"]) == 1 and one["choices"][0]["cumulative_logprob"] == want[0]["cum"]
    assert one["choices"][0]["message"]["content"] == d["choices"][0]["message"]["content"]
    assert c.post("/v1/chat/completions", json=_body()).status_code == 400      # beam_width defaults to n = 1: no group


@pytest.mark.parametrize("field", [{"temperature": 0.5}, {"top_p": 0.9}, {"top_k": 5}, {"repetition_penalty": 1.1}, {"frequency_penalty": 0.1},
                                   {"presence_penalty": 0.1}, {"seed": 3}, {"logprobs": True}, {"top_logprobs": 2}, {"logit_bias": {"3": 1.0}},
                                   {"allowed_token_ids": [3]}, {"min_tokens": 2}, {"stop_token_ids": [4]}, {"ignore_eos": True},
                                   {"guided_regex": "a+"}, {"guided_choice": ["a"]}, {"no_repeat_ngram_size": 2}, {"stop": ["ab"]},
                                   {"early_stopping": True}, {"beam_width": 9}, {"beam_width": 1}, {"n": 3, "beam_width": 2},
                                   {"length_penalty": "x"}])
def test_server_refuses_what_a_beam_row_cannot_honour(served, field):
    c, model, _ = served
    r = c.post("/v1/chat/completions", json=_body(**{"beam_width": 2, **field}))
    assert r.status_code == 400, (field, r.text)
    assert not model.engine.slots


def test_server_refuses_beam_fields_without_beam_search_and_servers_that_cannot_run_a_group(served):
    from fastapi.testclient import TestClient
    from dots_ocr_amd.processing import DotsOcrProcessor
    from dots_ocr_amd.server import create_app
    c, model, proc = served
    assert c.post("/v1/chat/completions", json={**_body(beam_width=2), "use_beam_search": False}).status_code == 400
    model.engine.spec_k = 2                                  # a speculating server
    assert c.post("/v1/chat/completions", json=_body(beam_width=2)).status_code == 400
    model.engine.spec_k = 0
    assert c.post("/v1/chat/completions", json=_body(beam_width=2)).status_code == 200
    plain = _BeamModel(model.config, beams=False)           # an engine without beam groups
    with TestClient(create_app(plain, proc, model_name="model", max_batch=4)) as c2:
        assert c2.post("/v1/chat/completions", json=_body(beam_width=2)).status_code == 400

    class Static:                                            # no engine slots at all: the static batching worker
        config = model.config
    with TestClient(create_app(Static(), proc, model_name="model", max_batch=4, continuous=False)) as c3:
        assert c3.post("/v1/chat/completions", json=_body(beam_width=2)).status_code == 400
