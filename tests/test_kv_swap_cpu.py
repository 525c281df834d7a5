"""Swap preemption without a GPU: the scheduler's policy against a fake engine that keeps the real engine's page
accounting, the new C-ABI symbols and their ctypes signatures, and the server's flag validation."""
import ctypes as C
import random

import numpy as np
import pytest

from dots_ocr_amd.engine import E_CAPACITY, E_STATE, DotsEngineError
from dots_ocr_amd.scheduler import ContinuousBatcher, Request
from fakes import FakePagedEngine


def _err(code, what):
    e = DotsEngineError(f"{what} failed ({code})")
    e.code = code
    return e


class FakeSwapEngine(FakePagedEngine):
    """FakePagedEngine + the suspend / resume surface of the real engine (slots.hip): a suspended slot gives all its pages back, parks the
    ceil(context / 64) pages that hold positions in the host space, takes no decode step and polls as 2."""

    def __init__(self, script, pool_pages, **kw):
        super().__init__(script, pool_pages, **kw)
        self.swap_total = self.swap_free = 0
        self.beam_rows = set()

    def _parked(self):
        return {s: st for s, st in self.slots.items() if st.get("parked") is not None}

    def kv_swap_reserve(self, pages):
        if self._parked():
            raise _err(E_STATE, "dots_kv_swap_reserve")
        self.swap_total = self.swap_free = int(pages)

    def kv_swap_info(self):
        return self.swap_total, self.swap_free

    def slots_reset(self):
        super().slots_reset()
        self.swap_free = self.swap_total

    def slot_suspend(self, s):
        st = self.slots.get(s)
        if st is None or st["done"] or st.get("parked") is not None or s in self.beam_rows:
            raise _err(E_STATE, "dots_slot_suspend")
        data = (st["ctx"] + 63) // 64
        if data > self.swap_free:
            raise _err(E_CAPACITY, "dots_slot_suspend")
        self.swap_free -= data
        self.free += st["pages"]
        st.update(parked=data, pages=0)
        self.log.append(("suspend", s))

    def slot_resume(self, s):
        st = self.slots.get(s)
        if st is None or st.get("parked") is None:
            raise _err(E_STATE, "dots_slot_resume")
        if st["parked"] > self.free:
            raise _err(E_CAPACITY, "dots_slot_resume")
        self.free -= st["parked"]
        self.swap_free += st["parked"]
        st.update(pages=st["parked"], parked=None)
        self.log.append(("resume", s))

    def slots_pages_short(self, n):
        lack = 0
        for st in self.slots.values():
            if st["done"] or st.get("parked") is not None:
                continue
            want = min(st["ctx"] + n, st["limit"] - 1)
            lack += max(0, (want + 63) // 64 - st["pages"])
        return max(0, lack - self.free)

    def slots_decode(self, n):
        parked = self._parked()
        for s in parked:
            del self.slots[s]
        try:
            super().slots_decode(n)
        finally:
            self.slots.update(parked)

    def slots_poll(self):
        fin, lens = super().slots_poll()
        for s in self._parked():
            fin[s] = 2
        return fin, lens

    def slot_release(self, s):
        st = self.slots[s]
        if st.get("parked") is not None:
            self.swap_free += st["parked"]
        super().slot_release(s)


def _engine(pool_pages=12, **kw):
    args = dict(max_batch=4, max_patches=100, max_prefill_tokens=2048, max_seq_len=640)
    args.update(kw)
    return FakeSwapEngine(lambda prompt: [1 + int(prompt[0]) % 7] * 1000, pool_pages, **args)


def _req(L=100, cap=200, first=0, **kw):
    ids = np.full(L, 3, np.int32)
    ids[0] = first
    return Request(ids, max_new_tokens=cap, **kw)


def _events(e, kinds):
    return [ev for ev in e.log if ev[0] in kinds]


# ---------------------------------------------------------------------------------------------------- policy

def test_default_batcher_truncates_where_swap_does_not():
    """four sequences of five pages each at their caps on twelve pages: today's policy ends some early, swap ends none"""
    e = _engine()
    plain = ContinuousBatcher(e, chunk=16, headroom_pages=0)
    out = plain.run([_req(first=i) for i in range(4)])
    assert plain.kv_truncated >= 1 and any(len(o) < 200 for o in out)
    assert not _events(e, ("suspend", "resume"))                       # preemption=None never touches the new calls

    e = _engine()
    cb = ContinuousBatcher(e, chunk=16, headroom_pages=0, preemption="swap")
    assert e.kv_swap_info() == (12, 12)                                # default host space: as many pages as the pool
    out = cb.run([_req(first=i) for i in range(4)])
    assert cb.kv_truncated == 0 and e.capped == 0
    assert [o.tolist() for o in out] == [[1 + i] * 200 for i in range(4)]
    assert cb.preemptions == cb.resumes > 0 and cb.swapped_pages > 0
    assert e.kv_pool_info() == (12, 12) and e.kv_swap_info() == (12, 12)


def test_victims_are_the_most_recent_and_resumes_the_oldest_suspension():
    e = _engine()
    cb = ContinuousBatcher(e, chunk=16, headroom_pages=0, preemption="swap")
    ids = [cb.submit(_req(first=i)) for i in range(5)]                 # four slots: the fifth request waits
    done = {}
    steps = 0
    while not cb.idle:
        for rid, _, toks in cb.step():
            done[rid] = toks
        if cb.suspended:                                               # nothing is admitted while anything is suspended
            assert len(cb.pending) == 1 and len(cb.free_slots()) <= 2
        steps += 1
        assert steps < 200
    assert sorted(done) == ids and all(len(t) == 200 for t in done.values())
    sus, res = [s for k, s in _events(e, ("suspend",))], [s for k, s in _events(e, ("resume",))]
    assert sus[:2] == [3, 2]                                           # admitted in slot order: the latest goes first
    assert res[:2] == [3, 2]                                           # and the one suspended longest comes back first
    # the fifth request's prefill comes after the resumes of the first round: the suspended sequences are older than the queue
    log = e.log
    second_prefill = [i for i, ev in enumerate(log) if ev[0] == "prefill"][1]
    assert max([i for i, ev in enumerate(log) if ev[0] == "resume"][:2]) < second_prefill


def _manual(cb, e, reqs):
    """prefill the requests into slots 0 .. and register them as running, as an admission would"""
    for s, r in enumerate(reqs):
        e.slots_prefill([s], r.input_ids, [len(r.input_ids)], [r.max_new_tokens])
        cb.running[s] = (s, r)
        cb._admit_seq[s] = s + 1


def test_the_last_running_sequence_is_never_suspended():
    e = _engine(pool_pages=40)
    cb = ContinuousBatcher(e, chunk=16, headroom_pages=0, preemption="swap", swap_pages=40)
    _manual(cb, e, [_req(first=i) for i in range(3)])
    e.slots_pages_short = lambda n: 1                                  # an engine that is short whatever is suspended
    cb._preempt()
    assert cb.suspended == [2, 1] and cb._active() == [0]
    assert e.slots_poll()[0].tolist() == [0, 2, 2, -1]


def test_a_beam_group_is_never_chosen():
    e = _engine(pool_pages=40)
    cb = ContinuousBatcher(e, chunk=16, headroom_pages=0, preemption="swap", swap_pages=40)
    reqs = [_req(first=0), _req(first=1), _req(first=2), _req(first=3)]
    reqs[2].num_beams = reqs[3].num_beams = 2                          # the two rows of a group: the most recently admitted
    _manual(cb, e, reqs)
    e.beam_rows = {2, 3}
    e.slots_pages_short = lambda n: 1
    cb._preempt()
    assert cb.suspended == [1, 0]                                      # every ordinary row, no group row: the group keeps running
    assert e.slots_poll()[0].tolist() == [2, 2, 0, 0]


def test_full_host_space_falls_back_to_capping():
    e = _engine()
    cb = ContinuousBatcher(e, chunk=16, headroom_pages=0, preemption="swap", swap_pages=0)
    out = cb.run([_req(first=i) for i in range(4)])
    assert cb.preemptions == 0 and cb.kv_truncated >= 1 and e.capped >= 1
    assert any(len(o) < 200 for o in out)

    e = _engine()                                                      # two host pages: nothing that needs three can be parked
    cb = ContinuousBatcher(e, chunk=16, headroom_pages=0, preemption="swap", swap_pages=2)
    cb.run([_req(first=i) for i in range(4)])
    assert cb.preemptions == 0 and cb.kv_truncated >= 1


def test_a_request_that_cannot_finish_alone_is_refused_at_submit():
    e = _engine(pool_pages=6)
    cb = ContinuousBatcher(e, chunk=16, preemption="swap")
    with pytest.raises(ValueError, match="fit the pool alone"):
        cb.submit(_req(L=100, cap=400))                                # 500 tokens: eight pages
    cb.submit(_req(L=100, cap=280))                                    # 380 tokens: six
    ContinuousBatcher(_engine(pool_pages=6), chunk=16).submit(_req(L=100, cap=400))        # the default policy takes it, and may truncate


@pytest.mark.parametrize("seed", range(12))
def test_a_random_closed_set_drains_without_truncation(seed):
    g = random.Random(seed)
    pool = g.choice([8, 10, 12, 16])
    e = _engine(pool_pages=pool, max_batch=g.choice([2, 3, 4]))
    cb = ContinuousBatcher(e, chunk=g.choice([8, 16, 32]), headroom_pages=g.choice([0, 1, 2]), preemption="swap", swap_pages=4 * pool)
    reqs = []
    for i in range(g.randint(4, 10)):
        L = g.randint(5, 300)
        cap = g.randint(1, min(640 - L, pool * 64 - L))
        reqs.append(_req(L=L, cap=cap, first=i))
    ids = [cb.submit(r) for r in reqs]
    done, steps = {}, 0
    while not cb.idle:
        for rid, _, toks in cb.step():
            done[rid] = toks
        steps += 1
        assert steps < 2000, "the set does not drain"
    assert sorted(done) == ids                                         # no request starves
    for rid, r in zip(ids, reqs):
        assert done[rid].tolist() == [1 + rid % 7] * r.max_new_tokens
    assert cb.kv_truncated == 0 and e.capped == 0 and cb.resumes == cb.preemptions
    assert e.kv_pool_info() == (pool, pool) and e.kv_swap_info() == (4 * pool, 4 * pool)


# ---------------------------------------------------------------------------------------------------- refusals at construction

def test_batcher_refuses_what_it_cannot_honour():
    with pytest.raises(ValueError, match="None or 'swap'"):
        ContinuousBatcher(_engine(), preemption="recompute")
    with pytest.raises(ValueError, match="needs preemption"):
        ContinuousBatcher(_engine(), swap_pages=4)
    spec = _engine()
    spec.spec_k = 2
    with pytest.raises(ValueError, match="speculating"):
        ContinuousBatcher(spec, preemption="swap")
    with pytest.raises(ValueError, match="slot_suspend"):
        ContinuousBatcher(FakePagedEngine(lambda p: [1] * 10, 12), preemption="swap")


# ---------------------------------------------------------------------------------------------------- C ABI

def test_new_symbols_and_their_signatures():
    from dots_ocr_amd import _lib, build, engine
    build.build(verbose=False)
    lib = _lib.load()
    engine._prototypes(lib)
    vp, i32, P = C.c_void_p, C.c_int32, C.POINTER
    want = {
        "dots_kv_swap_reserve": [vp, i32],
        "dots_kv_swap_info": [vp, P(i32), P(i32)],
        "dots_slot_suspend": [vp, i32],
        "dots_slot_resume": [vp, i32],
        "dots_slots_pages_short": [vp, i32, P(i32)],
    }
    for name, args in want.items():
        fn = getattr(lib, name)
        assert fn.restype is i32 and list(fn.argtypes) == args, name
        assert name in engine.EXPORTED_SYMBOLS
    for method in ("kv_swap_reserve", "kv_swap_info", "slot_suspend", "slot_resume", "slots_pages_short"):
        assert callable(getattr(engine.Engine, method))
    t, f = i32(7), i32(7)                                              # a null engine is refused, not dereferenced
    assert lib.dots_kv_swap_info(None, C.byref(t), C.byref(f)) == -1
    assert lib.dots_slot_suspend(None, 0) == -1 and lib.dots_slot_resume(None, 0) == -1
    assert lib.dots_kv_swap_reserve(None, 1) == -1 and lib.dots_slots_pages_short(None, 1, C.byref(t)) == -1


# ---------------------------------------------------------------------------------------------------- server flags

def test_server_flag_validation():
    from dots_ocr_amd.config import DotsConfig
    from dots_ocr_amd.server import build_arg_parser, main, preemption_args, swap_pages_for
    ap = build_arg_parser()
    assert preemption_args(ap.parse_args([])) is None                  # the default: today's behaviour
    assert preemption_args(ap.parse_args(["--preemption", "swap"])) == ("swap", None)
    assert preemption_args(ap.parse_args(["--preemption", "swap", "--swap-space-gib", "4"])) == ("swap", 4.0)
    for bad in (["--swap-space-gib", "4"], ["--preemption", "swap", "--static-batching"], ["--preemption", "swap", "--speculative-ngram", "2"],
                ["--preemption", "swap", "--swap-space-gib", "0"], ["--preemption", "swap", "--swap-space-gib", "-1"],
                ["--preemption", "swap", "--swap-space-gib", "nan"]):
        with pytest.raises(ValueError):
            preemption_args(ap.parse_args(bad))
    with pytest.raises(SystemExit):
        ap.parse_args(["--preemption", "recompute"])
    with pytest.raises(SystemExit):                                    # refused at server start, before anything is loaded
        main(["--preemption", "swap", "--static-batching"])
    cfg = DotsConfig()
    per_page = cfg.num_hidden_layers * cfg.num_key_value_heads * 2 * 8192 * 2
    assert swap_pages_for(cfg, 4.0) == (4 << 30) // per_page
    assert swap_pages_for(cfg, 4.0, "fp8") == (4 << 30) // (per_page // 2)                 # an e4m3 page is half the bytes
