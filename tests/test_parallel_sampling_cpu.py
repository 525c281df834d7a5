"""Parallel sampling (`n` > 1) without a GPU: the scheduler's admission, page arithmetic, seeds and reporting over a fake
paged engine that forks with reference counts; the server's `n` field; modeling.generate's num_return_sequences."""
import numpy as np
import pytest
import torch

from dots_ocr_amd.config import DotsConfig
from dots_ocr_amd.engine import SamplingParams
from fakes import FakePagedEngine


class ForkEngine(FakePagedEngine):
    """FakePagedEngine + per-row parameters + slots_fork as the engine defines it: only a sequence of the most recent prefill, before any
    decode step; a child shares the source's floor(L / 64) full prompt pages (counted once in the pool, returned by the last holder)
    and takes the rest of the admission reserve for itself.  `script` may read self.cur / self.rows: the slot it is asked about."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.rows, self.row_calls, self.cur, self.fresh, self.groups = {}, [], None, set(), {}

    def set_row_sampling(self, row, params):
        self.row_calls.append((row, params))
        if params is None:
            self.rows.pop(row, None)
        else:
            self.rows[row] = params

    def _restart(self, s):
        st = self.slots[s]
        self.cur = s
        st.update(plan=list(self.script(st["prompt"])), out=[], done=False)
        self._advance(st)

    def slots_reset(self):
        super().slots_reset()
        self.fresh, self.groups = set(), {}

    def slots_prefill(self, slots, ids, lens, caps):
        super().slots_prefill(slots, ids, lens, caps)
        for s in slots:
            self._restart(s)
        self.fresh = set(slots)

    def slots_decode(self, n):
        self.fresh = set()
        super().slots_decode(n)

    def slots_fork(self, src, dst):
        assert src in self.fresh and src in self.slots, "only a freshly prefilled sequence can be forked"
        assert len(set(dst)) == len(dst) and all(0 <= d < self.max_batch and d not in self.slots for d in dst)
        p = self.slots[src]
        L, shared = len(p["prompt"]), len(p["prompt"]) // 64
        own = (min(L + min(p["limit"] - L, 64), self.max_seq_len) + 63) // 64 - shared
        if own * len(dst) > self.free:
            raise RuntimeError("KV pool exhausted")
        key = p.setdefault("group", ("group", src, len(self.log)))
        self.groups[key] = self.groups.get(key, 1) + len(dst)
        for d in dst:
            self.slots[d] = dict(prompt=p["prompt"].copy(), cap=p["limit"] - L, pages=shared + own, limit=p["limit"], ctx=L, group=key, shared=shared)
            self.free -= own
            self._restart(d)
        p["shared"] = shared
        self.log.append(("fork", src, tuple(dst), tuple(self.rows.get(s) for s in [src] + list(dst))))

    def slot_release(self, s):
        st = self.slots[s]
        key = st.get("group")
        if key is not None:
            self.groups[key] -= 1
            if self.groups[key] > 0:
                self.free -= st["shared"]            # other rows still hold the shared pages: they stay out of the pool
        self.rows.pop(s, None)
        super().slot_release(s)


EOS = 9


def _seq(first, seed):
    """what a sequence generates: 2 + 4 * (seed % 3) tokens that spell its first prompt id and its seed, then the EOS"""
    return [int(first) * 100 + seed] * (2 + 4 * (seed % 3)) + [EOS]


def _by_seed(eng):
    def script(prompt):
        sp = eng[0].rows.get(eng[0].cur)
        return _seq(prompt[0], 0 if sp is None else sp.seed)
    return script


def _engine(pool_pages=64, max_batch=4, **kw):
    box = []
    e = ForkEngine(_by_seed(box), pool_pages, max_batch=max_batch, max_prefill_tokens=1024, max_seq_len=1024, **kw)
    box.append(e)
    return e


def _req(first, L=5, cap=40, **kw):
    from dots_ocr_amd.scheduler import Request
    return Request(np.full(L, first, np.int32), max_new_tokens=cap, **kw)


# ---------------------------------------------------------------------------------------------------- scheduler

def test_a_request_with_n_waits_for_n_slots_in_fifo_order():
    from dots_ocr_amd.scheduler import ContinuousBatcher
    eng = _engine()
    sp = lambda seed: SamplingParams(temperature=1.0, seed=seed)      # noqa: E731
    a, b = _req(1, sampling=sp(2)), _req(2, sampling=sp(0))           # a runs 11 tokens, b 3: two of four slots are taken
    c, d = _req(3, sampling=sp(3), n=3), _req(4, sampling=sp(0))      # c needs three slots; d must not overtake it
    cb = ContinuousBatcher(eng, eos_ids=(EOS,), chunk=2)
    outs = cb.run([a, b, c, d])
    starts = [ev for ev in eng.log if ev[0] in ("prefill", "fork")]
    assert starts[0] == ("prefill", (0, 1))
    assert starts[1] == ("prefill", (1,)) and starts[2][:3] == ("fork", 1, (2, 3))       # c, once b has left: a still holds slot 0
    assert starts[3][0] == "prefill" and len(starts) == 4                                  # d afterwards
    # the children ran under seed + i, everything else as the request says
    assert starts[2][3] == (sp(3), sp(4), sp(5))
    assert [o.tolist() for o in c.outputs] == [_seq(3, 3), _seq(3, 4), _seq(3, 5)]
    assert outs[2].tolist() == _seq(3, 3) and outs[3].tolist() == _seq(4, 0)
    assert eng.kv_pool_info() == (64, 64) and not eng.slots and eng.rows == {}


@pytest.mark.parametrize("L,cap", [(130, 80), (64, 10), (65, 200), (127, 1)])
def test_page_need_follows_the_formula_and_the_pool_returns_to_full(L, cap):
    from dots_ocr_amd.scheduler import ContinuousBatcher
    admit = (min(L + min(cap, 64), 1024) + 63) // 64
    need = admit + 2 * (admit - L // 64)
    for pool, fits in ((need, True), (need - 1, False)):
        eng = _engine(pool_pages=pool)
        cb = ContinuousBatcher(eng, eos_ids=(EOS,), chunk=4, headroom_pages=0)
        r = _req(7, L=L, cap=cap, sampling=SamplingParams(temperature=1.0, seed=1), n=3)
        assert cb._group_pages(r) == need
        if not fits:
            with pytest.raises(ValueError, match="KV pages"):
                cb.submit(r)
            continue
        cb.submit(r)
        cb._admit(cb.plan_admission())
        assert eng.kv_pool_info() == (pool, 0) and sorted(eng.slots) == [0, 1, 2]
        while not cb.idle:
            cb.step()
        assert eng.kv_pool_info() == (pool, pool)
    # full reservation counts the worst case the same way: shared prompt pages once
    eng = _engine(pool_pages=64)
    cb = ContinuousBatcher(eng, chunk=4, headroom_pages=None)
    worst = (min(L + cap, 1024) + 63) // 64
    assert cb._worst_pages(_req(7, L=L, cap=cap, n=3)) == worst + 2 * (worst - L // 64)


def test_the_parent_may_finish_first_and_the_request_is_reported_once():
    from dots_ocr_amd.scheduler import ContinuousBatcher
    eng = _engine(max_batch=3)
    r = _req(5, sampling=SamplingParams(temperature=1.0, seed=0), logprobs=None, n=3)      # 3, 7 and 11 tokens
    nxt = _req(6)
    cb = ContinuousBatcher(eng, eos_ids=(EOS,), chunk=1)
    cb.submit(r)
    cb.submit(nxt)
    reported = []
    seen_reuse = False
    while not cb.idle:
        done = cb.step()
        reported += [id(req) for _, req, _ in done]
        if id(r) not in reported and 0 in eng.slots and int(eng.slots[0]["prompt"][0]) == 6:
            seen_reuse = True                         # the parent's slot serves the next request while its children still run
    assert seen_reuse
    assert reported == [id(nxt), id(r)]               # once, when its last sequence has finished
    assert [o.tolist() for o in r.outputs] == [_seq(5, 0), _seq(5, 1), _seq(5, 2)]
    assert r.kv_truncated is False and r.kv_truncated_each == [False] * 3


def test_submit_refuses_a_bad_n():
    from dots_ocr_amd.scheduler import ContinuousBatcher
    cb = ContinuousBatcher(_engine(max_batch=4), chunk=2)
    for bad in (0, -1, 2.0, "2", True, 5):
        with pytest.raises(ValueError):
            cb.submit(_req(1, n=bad))
    plain = FakePagedEngine(lambda p: [1, 2, 3], 64, max_batch=4)
    cb = ContinuousBatcher(plain, chunk=2)
    with pytest.raises(ValueError, match="slots_fork"):
        cb.submit(_req(1, n=2))
    cb.submit(_req(1, n=1))


def test_requests_with_n_1_make_the_calls_they_make_today():
    from dots_ocr_amd.scheduler import ContinuousBatcher
    script = lambda p: [int(p[0])] * (2 + int(p[0]) % 5)              # noqa: E731
    logs = []
    for cls in (FakePagedEngine, ForkEngine):
        eng = cls(script, 12, max_batch=3, max_prefill_tokens=1024, max_seq_len=1024)
        reqs = [_req(1 + i, L=20 + 30 * i, cap=6 + i) for i in range(7)]
        outs = ContinuousBatcher(eng, chunk=2).run(reqs)
        logs.append((eng.log, [o.tolist() for o in outs]))
        assert all(not hasattr(r, "outputs") for r in reqs)
    assert logs[0] == logs[1]
    assert not any(ev[0] == "fork" for ev in logs[1][0])


# ---------------------------------------------------------------------------------------------------- server

class _ForkModel:
    """each completion spells out the seed of its own slot; an even seed ends by EOS, an odd one runs into max_tokens"""

    def __init__(self, proc, cfg, fork=True):
        self.config = cfg
        model = self

        def script(prompt):
            e = model.engine
            p = e.rows.get(e.cur)
            seed = -1 if p is None else p.seed
            body = proc.tokenizer.encode(f"seed={seed}|")
            return body + [cfg.eos_token_ids[0]] if seed % 2 == 0 else body + proc.tokenizer.encode("x" * 300)
        if fork:
            self.engine = ForkEngine(script, 256, max_batch=3, max_patches=4096, max_prefill_tokens=4096, max_seq_len=2048)
        else:
            class NoFork(ForkEngine):
                slots_fork = property()              # an engine without the call
            self.engine = NoFork(script, 256, max_batch=3, max_patches=4096, max_prefill_tokens=4096, max_seq_len=2048)


def _payload(**kw):
    body = {"model": "model", "messages": [{"role": "user", "content": "Read this."}], "max_completion_tokens": 24, "temperature": 0.8}
    body.update(kw)
    return body


def _app(**kw):
    pytest.importorskip("fastapi")
    from dots_ocr_amd.processing import DotsOcrProcessor
    from dots_ocr_amd.server import create_app
    cfg = DotsConfig.tiny()
    proc = DotsOcrProcessor(cfg)
    model = _ForkModel(proc, cfg, **{k: v for k, v in kw.items() if k == "fork"})
    return model, proc, create_app(model, proc, model_name="model", max_batch=3, **{k: v for k, v in kw.items() if k != "fork"})


def test_server_validates_n():
    from fastapi.testclient import TestClient
    model, _, app = _app()
    with TestClient(app) as c:
        for bad in (0, -2, 1.5, "2", True, 4):                       # 4: the worker runs three sequences at a time
            r = c.post("/v1/chat/completions", json=_payload(n=bad))
            assert r.status_code == 400, (bad, r.text)
        assert c.post("/v1/chat/completions", json=_payload(n=3, seed=2)).status_code == 200
    _, _, static = _app(continuous=False)
    with TestClient(static) as c:
        assert c.post("/v1/chat/completions", json=_payload(n=2)).status_code == 400
    m, _, nofork = _app(fork=False)
    assert not hasattr(m.engine, "slots_fork")
    with TestClient(nofork) as c:
        assert c.post("/v1/chat/completions", json=_payload(n=2)).status_code == 400
        assert c.post("/v1/chat/completions", json=_payload(n=1, seed=2)).status_code == 200


def test_server_returns_n_choices_with_their_own_finish_reasons_and_summed_usage():
    from fastapi.testclient import TestClient
    model, proc, app = _app()
    with TestClient(app) as c:
        app.state.worker.chunk = 4
        r = c.post("/v1/chat/completions", json=_payload(n=3, seed=10))
        assert r.status_code == 200, r.text
        d = r.json()
        assert [ch["index"] for ch in d["choices"]] == [0, 1, 2]
        assert [ch["message"]["content"].split("|")[0] for ch in d["choices"]] == ["seed=10", "seed=11", "seed=12"]
        assert [ch["finish_reason"] for ch in d["choices"]] == ["stop", "length", "stop"]
        alone = [c.post("/v1/chat/completions", json=_payload(seed=10 + i)).json() for i in range(3)]
        assert [a["choices"][0]["message"]["content"] for a in alone] == [ch["message"]["content"] for ch in d["choices"]]
        assert d["usage"]["prompt_tokens"] == alone[0]["usage"]["prompt_tokens"]          # counted once
        assert alone[1]["usage"]["completion_tokens"] == 24
        assert d["usage"]["completion_tokens"] == sum(a["usage"]["completion_tokens"] for a in alone)
        assert d["usage"]["total_tokens"] == d["usage"]["prompt_tokens"] + d["usage"]["completion_tokens"]
        assert all("logprobs" not in ch for ch in d["choices"])
        # exactly today's keys for n = 1, given or not
        for body in (_payload(seed=10), _payload(seed=10, n=1)):
            one = c.post("/v1/chat/completions", json=body).json()
            assert sorted(one) == ["choices", "created", "id", "model", "object", "usage"]
            assert len(one["choices"]) == 1 and sorted(one["choices"][0]) == ["finish_reason", "index", "message"]
            assert one["choices"][0]["index"] == 0 and one["choices"][0]["message"]["content"] == "seed=10|"
            assert sorted(one["usage"]) == ["completion_tokens", "prompt_tokens", "total_tokens"]
        assert not model.engine.slots and model.engine.kv_pool_info() == (256, 256)


def test_an_unseeded_request_takes_n_values_of_the_seed_counter():
    from fastapi.testclient import TestClient
    _, _, app = _app()
    with TestClient(app) as c:
        w = app.state.worker
        s0 = w.seed
        d = c.post("/v1/chat/completions", json=_payload(n=3)).json()
        assert [ch["message"]["content"].split("|")[0] for ch in d["choices"]] == [f"seed={s0 + 1 + i}" for i in range(3)]
        assert w.seed == s0 + 3
        d = c.post("/v1/chat/completions", json=_payload()).json()
        assert d["choices"][0]["message"]["content"].startswith(f"seed={s0 + 4}|") and w.seed == s0 + 4
        c.post("/v1/chat/completions", json=_payload(n=2, seed=99))
        assert w.seed == s0 + 4                                        # a seeded request leaves the counter alone


# ---------------------------------------------------------------------------------------------------- modeling

def test_generate_lays_out_num_return_sequences_as_hf_does():
    from dots_ocr_amd.modeling import DotsOcrHipForCausalLM
    cfg = DotsConfig.tiny()
    eng = _engine(max_batch=4)
    eng.max_patches = 4096
    m = object.__new__(DotsOcrHipForCausalLM)
    m.config, m.engine, m.max_batch, m.max_seq_len, m.max_patches = cfg, eng, 4, 1024, 4096
    m.generation_config = {"do_sample": False}
    ids = torch.tensor([[1, 1, 1], [2, 2, 2], [3, 3, 3]])
    out = m.generate(ids, max_new_tokens=16, do_sample=True, temperature=0.7, top_p=0.9, seed=10, num_return_sequences=2, eos_token_id=[EOS],
                     pad_token_id=0)
    assert out.shape[0] == 6
    for i in range(3):
        for j in range(2):
            row, want = out[i * 2 + j].tolist(), _seq(i + 1, 10 + i * 2 + j)
            assert row[:3] == [i + 1] * 3 and row[3:3 + len(want)] == want and set(row[3 + len(want):]) <= {0}
    assert sum(1 for ev in eng.log if ev[0] == "fork") == 3 and sum(len(ev[1]) for ev in eng.log if ev[0] == "prefill") == 3
    assert eng.rows == {} and eng.kv_pool_info() == (64, 64)
    with pytest.raises(ValueError, match="continuous"):
        m.generate(ids, max_new_tokens=4, num_return_sequences=2, continuous=False)
    with pytest.raises(ValueError):
        m.generate(ids, max_new_tokens=4, num_return_sequences=0)
    one = m.generate(ids[:1], max_new_tokens=16, do_sample=False, continuous=True, eos_token_id=[EOS], pad_token_id=0)
    assert one.tolist() == [[1, 1, 1] + _seq(1, 0)]                   # n = 1: one row per prompt, as before
