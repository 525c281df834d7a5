"""Chunked prefill without a GPU.

1. The probes of tests/chunk_probes.py judged as test_attention_probes_cpu.py judges its probes: the bf16-emulated oracle lies inside the
   tolerance of the float64 reference on every probe (the tolerance is the reference's, not a kernel's), the reference alone excludes
   (almost) nothing, and every mutant — a causal limit off by one either way, a dropped prefix page, two exchanged pages, a page read
   unmasked to its 64th slot — lies >= MUTANT_FACTOR x the tolerance away.  Run with -s for the table.
2. The scheduler's policy over a fake engine that fills in passes: at most one pass per step with a decode chunk between passes, fills in
   FIFO order, prompts longer than the workspace, a filling request never a swap victim, a group's fork right behind the completing pass.
3. The server's flags and that prefill_chunk reaches the batcher.
"""
import threading

import numpy as np
import pytest

import attention_probes as ap
import chunk_probes as cp
from dots_ocr_amd.engine import E_CAPACITY, E_STATE, DotsEngineError
from dots_ocr_amd.scheduler import ContinuousBatcher, Request
from fakes import FakePagedEngine
from test_attention_probes_cpu import emulated

# ---------------------------------------------------------------------------------------------------- 1. the probes

POOLS = [None, "unit", "per_head"]
PROBES = [(c, m, s) for c, m in cp.SHAPES + [cp.BIG_SHAPE] for s in POOLS]


def _probe(c, m, scales):
    big = (c, m) == cp.BIG_SHAPE
    return cp.suffix_probe(c, m, None if scales is None else ap.KV8_SCALES[scales], **(dict(Hq=12, Hkv=2) if big else {}))


@pytest.mark.parametrize("c,m,scales", PROBES, ids=[f"{c}+{m}-{s or 'bf16'}" for c, m, s in PROBES])
def test_probe_is_pinned_to_fp64_and_sees_every_mutant(c, m, scales):
    seq = _probe(c, m, scales)
    pos = cp.positions(seq)
    assert seq.causal and seq.nq == m and seq.n == c + m and pos.tolist() == [c + r for r in seq.rows]
    assert {0, m - 1} <= set(seq.rows) and all(b - c in seq.rows and b - c - 1 in seq.rows for b in range((c // 64 + 1) * 64, c + m, 64))
    best = {}
    for code in ap.CODES:
        ref = seq.reference(code)
        ratio, excluded, rel = ap.deviation(emulated(seq, code), ref)
        print(f"\n{seq.name} {scales or 'bf16'} {code}: emulated oracle vs fp64 {rel:.5f} relative = {ratio:.2f} x the tolerance, excluded {excluded:.4f}")
        assert ratio <= 1.0, f"{seq.name} {code}: the emulated oracle is {ratio:.2f} x the tolerance from fp64"
        assert excluded <= ap.MAX_EXCLUDED
        for name in cp.MUTANTS:
            out = cp.mutant_output(seq, code, name)
            if out is not None:
                best[name] = max(best.get(name, 0.0), ap.deviation(out, ref)[0])
    for name, d in best.items():
        print(f"  | {seq.name} {scales or 'bf16'} | {name} | {min(d, 9999.0):.1f}")
        assert d >= ap.MUTANT_FACTOR, f"{seq.name}: mutant '{name}' is only {d:.2f} x the tolerance away: the probe would not see it"
    # which mutants a shape must see: all of them wherever they can exist at all
    want = {"causal limit +1", "causal limit -1", "the last page read unmasked to 64"}
    if c >= 64:
        want |= {"a prefix page dropped", "two pages exchanged"}
    assert want <= set(best), (want - set(best), "mutants this shape did not try")


def test_every_mutant_is_seen_by_some_probe():
    seen = set()
    for c, m in cp.SHAPES:
        seq = cp.suffix_probe(c, m)
        seen |= {name for name in cp.MUTANTS if cp.mutant_output(seq, "lane", name) is not None}
    assert seen == set(cp.MUTANTS)


# ---------------------------------------------------------------------------------------------------- 2. the scheduler

def _err(code, what):
    e = DotsEngineError(f"{what} failed ({code})")
    e.code = code
    return e


class ChunkEngine(FakePagedEngine):
    """FakePagedEngine + the resumable prefill of the real engine: begin reserves the admission pages of every slot (all or nothing) and
    leaves it filling (poll 3, no decode step touches it); advance fills up to n positions, oldest begin first, every cut on a multiple of
    64 positions of its sequence or at its end; a completed slot is what slots_prefill leaves and may be forked until the next step.  Also
    the suspend / resume surface, as tests/test_kv_swap_cpu.py's fake has it."""

    def __init__(self, script, pool_pages, **kw):
        super().__init__(script, pool_pages, **kw)
        self.fills, self.fresh, self.order = {}, set(), 0
        self.swap_total = self.swap_free = 0

    def _need(self, n, c):
        return (min(n + min(c, 64), self.max_seq_len) + 63) // 64

    def slots_reset(self):
        super().slots_reset()
        self.fills, self.fresh = {}, set()
        self.swap_free = self.swap_total

    def slots_prefill(self, slots, ids, lens, caps):
        assert not set(slots) & set(self.fills)
        super().slots_prefill(slots, ids, lens, caps)
        self.fresh = set(slots)

    def slots_prefill_begin(self, slots, ids, lens, caps):
        assert sum(lens) == len(ids)                                       # bounded by the pool, not by max_prefill_tokens
        need = [self._need(n, c) for n, c in zip(lens, caps)]
        if sum(need) > self.free:
            raise RuntimeError("KV pool exhausted")
        off = 0
        for s, n, c, p in zip(slots, lens, caps, need):
            assert 0 <= s < self.max_batch and s not in self.slots and s not in self.fills
            self.order += 1
            self.fills[s] = dict(prompt=np.asarray(ids[off:off + n]).copy(), cap=int(c), cursor=0, pages=p, order=self.order)
            self.free -= p
            off += n
        self.log.append(("begin", tuple(slots)))

    def slots_prefill_advance(self, n):
        assert n > 0 and n % 64 == 0 and n <= self.max_prefill_tokens
        budget, taken, done = n, [], []
        for s in sorted(self.fills, key=lambda k: self.fills[k]["order"]):
            f = self.fills[s]
            left = len(f["prompt"]) - f["cursor"]
            take = min(left, budget)
            if take < left:
                take = take // 64 * 64
            if take <= 0:
                break
            assert f["cursor"] % 64 == 0
            f["cursor"] += take
            budget -= take
            taken.append((s, take))
            if f["cursor"] == len(f["prompt"]):
                done.append(s)
        for s in done:
            f = self.fills.pop(s)
            L = len(f["prompt"])
            self.slots[s] = dict(prompt=f["prompt"], cap=f["cap"], plan=list(self.script(f["prompt"])), out=[], done=False, pages=f["pages"],
                                 limit=L + f["cap"], ctx=L)
            self._advance(self.slots[s])
        self.fresh = set(done)
        self.log.append(("advance", n, tuple(taken)))
        return sum(len(f["prompt"]) - f["cursor"] for f in self.fills.values())

    def slots_fork(self, src, dst):
        assert src in self.fresh and src in self.slots, "only a freshly prefilled sequence can be forked"
        p = self.slots[src]
        L = len(p["prompt"])
        own = self._need(L, p["limit"] - L)
        if own * len(dst) > self.free:
            raise RuntimeError("KV pool exhausted")
        for d in dst:
            assert d not in self.slots and d not in self.fills
            self.slots[d] = dict(prompt=p["prompt"].copy(), cap=p["cap"], plan=list(self.script(p["prompt"])), out=[], done=False, pages=own,
                                 limit=p["limit"], ctx=L)
            self.free -= own
            self._advance(self.slots[d])
        self.log.append(("fork", src, tuple(dst)))

    def _parked(self):
        return {s: st for s, st in self.slots.items() if st.get("parked") is not None}

    def slots_decode(self, n):
        self.fresh = set()
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
        for s in self.fills:
            fin[s] = 3
        return fin, lens

    def slot_release(self, s):
        if s in self.fills:
            self.free += self.fills.pop(s)["pages"]
            self.log.append(("release_filling", s))
            return
        if self.slots[s].get("parked") is not None:
            self.swap_free += self.slots[s]["parked"]
        super().slot_release(s)

    # suspend / resume
    def kv_swap_reserve(self, pages):
        self.swap_total = self.swap_free = int(pages)

    def kv_swap_info(self):
        return self.swap_total, self.swap_free

    def slot_suspend(self, s):
        st = self.slots.get(s)
        if st is None or st["done"] or st.get("parked") is not None:      # a filling slot is not in `slots`: refused, as the engine does
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
            lack += max(0, (min(st["ctx"] + n, st["limit"] - 1) + 63) // 64 - st["pages"])
        return max(0, lack - self.free)


def _engine(pool_pages=40, **kw):
    args = dict(max_batch=4, max_patches=100, max_prefill_tokens=128, max_seq_len=640)
    args.update(kw)
    return ChunkEngine(lambda prompt: [1 + int(prompt[0]) % 7] * 1000, pool_pages, **args)


def _req(L=100, cap=20, first=0, **kw):
    ids = np.full(L, 3, np.int32)
    ids[0] = first
    return Request(ids, max_new_tokens=cap, **kw)


def _steps(cb, e, limit=500):
    """run to idle -> ({request id: tokens}, the engine's log cut per step)"""
    done, per_step = {}, []
    while not cb.idle:
        mark = len(e.log)
        for rid, _, toks in cb.step():
            done[rid] = toks.tolist()
        per_step.append(e.log[mark:])
        assert len(per_step) < limit, "the set does not drain"
    return done, per_step


def test_one_pass_per_step_with_a_decode_chunk_between_passes():
    e = _engine()
    cb = ContinuousBatcher(e, chunk=4, prefill_chunk=64, headroom_pages=0)
    short = cb.submit(_req(60, 40, first=1))
    done, steps = _steps(cb, e)                                            # alone first: its fill is one pass
    assert done[short] == [2] * 40
    cb = ContinuousBatcher(e, chunk=4, prefill_chunk=64, headroom_pages=0)
    short, long_ = cb.submit(_req(60, 40, first=1)), cb.submit(_req(300, 8, first=2))
    done, steps = _steps(cb, e)
    assert done == {short: [2] * 40, long_: [3] * 8}
    assert not any(ev[0] == "prefill" for st in steps for ev in st)        # with chunking on, nothing is prefilled in one pass
    passes = [i for i, st in enumerate(steps) if any(ev[0] == "advance" for ev in st)]
    assert len(passes) == 1 + 5                                            # 60 -> one pass; 300 -> 64 x 4 + 44
    for i, st in enumerate(steps):
        kinds = [ev[0] for ev in st]
        assert kinds.count("advance") <= 1 and kinds.count("decode") <= 1
        if "advance" in kinds and i > passes[0]:                           # from the second pass on the short request is running:
            assert kinds.index("advance") < kinds.index("decode")          # the pass, then this step's decode chunk — never two passes in a row
    adv = [ev for st in steps for ev in st if ev[0] == "advance"]
    assert [ev[1] for ev in adv] == [64] * 6
    assert adv[0][2] == ((0, 60),) and [ev[2] for ev in adv[1:]] == [((1, 64),)] * 4 + [((1, 44),)]
    assert cb.fill_passes == 6 and e.kv_pool_info() == (40, 40)


def test_fills_are_served_in_begin_order():
    e = _engine(max_prefill_tokens=256)
    cb = ContinuousBatcher(e, chunk=2, prefill_chunk=128, headroom_pages=0, admit_group=1)
    a, b = cb.submit(_req(200, 30, first=1)), cb.submit(_req(150, 30, first=2))
    done, steps = _steps(cb, e)
    assert done == {a: [2] * 30, b: [3] * 30}
    begins = [ev for st in steps for ev in st if ev[0] == "begin"]
    assert begins == [("begin", (0,)), ("begin", (1,))]                    # admitted one per step (admit_group=1)
    adv = [ev[2] for st in steps for ev in st if ev[0] == "advance"]
    # the older fill first; the younger gets what a pass has left only in whole pages of 64, so nothing here: then its own passes
    assert adv == [((0, 128),), ((0, 72),), ((1, 128),), ((1, 22),)]


def test_a_prompt_longer_than_the_workspace_needs_chunking():
    e = _engine()
    with pytest.raises(ValueError, match="max_prefill_tokens"):
        ContinuousBatcher(e).submit(_req(300, 8))                          # off: today's refusal
    cb = ContinuousBatcher(e, chunk=4, prefill_chunk=128, headroom_pages=0)
    rid = cb.submit(_req(300, 8, first=4))
    done, _ = _steps(cb, e)
    assert done[rid] == [5] * 8
    with pytest.raises(ValueError, match="max_seq_len"):
        cb.submit(_req(640, 8))                                            # max_seq_len still bounds a prompt
    with pytest.raises(ValueError, match="KV pages"):
        ContinuousBatcher(_engine(pool_pages=4), prefill_chunk=64).submit(_req(300, 8))      # and so does the pool


def test_batcher_refuses_what_it_cannot_honour():
    for bad in (0, 63, 100, -64, 64.0, True):
        with pytest.raises(ValueError, match="multiple of 64"):
            ContinuousBatcher(_engine(), prefill_chunk=bad)
    with pytest.raises(ValueError, match="max_prefill_tokens"):
        ContinuousBatcher(_engine(), prefill_chunk=192)                    # the fake's workspace holds 128
    with pytest.raises(ValueError, match="slots_prefill_begin"):
        ContinuousBatcher(FakePagedEngine(lambda p: [1] * 10, 12, max_prefill_tokens=128), prefill_chunk=64)
    spec = _engine()
    spec.spec_k = 2
    with pytest.raises(ValueError, match="speculating"):
        ContinuousBatcher(spec, prefill_chunk=64)


def test_a_filling_request_is_never_a_swap_victim():
    e = _engine(pool_pages=17)
    cb = ContinuousBatcher(e, chunk=16, prefill_chunk=64, headroom_pages=0, preemption="swap", swap_pages=40)
    a, b, c = cb.submit(_req(180, 300, first=1)), cb.submit(_req(180, 300, first=2)), cb.submit(_req(500, 60, first=3))
    seen = []
    done = {}
    for _ in range(400):
        if cb.idle:
            break
        mark = len(e.log)
        for rid, _, toks in cb.step():
            done[rid] = toks.tolist()
        for ev in e.log[mark:]:
            if ev[0] == "suspend":
                seen.append((ev[1], sorted(e.fills), sorted(cb.running)))
    assert cb.idle and done == {a: [2] * 300, b: [3] * 300, c: [4] * 60}
    assert cb.preemptions >= 1 and cb.resumes == cb.preemptions and cb.kv_truncated == 0 and e.capped == 0
    victim, filling, running = seen[0]
    assert filling == [2] and victim == 1 and running == [0, 1]            # the pool ran short while slot 2 was filling: the youngest RUNNING row went
    assert all(v not in f for v, f, _ in seen)
    assert e.kv_pool_info() == (17, 17)


def test_a_groups_fork_follows_the_completing_pass_in_the_same_step():
    e = _engine()
    cb = ContinuousBatcher(e, chunk=4, prefill_chunk=64, headroom_pages=0)
    other, group = cb.submit(_req(60, 30, first=1)), _req(150, 6, first=2, n=3)
    gid = cb.submit(group)
    done, steps = _steps(cb, e)
    assert done[other] == [2] * 30 and [o.tolist() for o in group.outputs] == [[3] * 6] * 3
    (i,) = [i for i, st in enumerate(steps) if any(ev[0] == "fork" for ev in st)]
    kinds = [ev[0] for ev in steps[i]]
    assert kinds == ["advance", "fork", "decode"]                          # the pass that completed the fill, its fork, this step's decode chunk
    assert steps[i][0][2] == ((1, 22),) and steps[i][1] == ("fork", 1, (2, 3))
    assert all("fork" not in [ev[0] for ev in st] for j, st in enumerate(steps) if j != i)
    # while the group's source was filling, the slots of its children were held for it
    assert cb.admissions == 1 and e.kv_pool_info() == (40, 40)


def test_a_release_while_filling_returns_the_pages():
    e = _engine()
    cb = ContinuousBatcher(e, chunk=4, prefill_chunk=64, headroom_pages=0)
    cb.submit(_req(300, 8))
    cb.step()
    assert e.slots_poll()[0][0] == 3 and e.kv_pool_info() == (40, 40 - 5) and cb.filling and not cb.idle
    e.slot_release(0)
    assert e.kv_pool_info() == (40, 40) and e.slots_poll()[0][0] == -1
    cb2 = ContinuousBatcher(e, chunk=4, prefill_chunk=64)                  # a new batcher starts from an empty engine: fills are dropped too
    cb2.submit(_req(300, 8))
    cb2.step()
    ContinuousBatcher(e, chunk=4)
    assert e.kv_pool_info() == (40, 40) and not e.fills


def test_nothing_moves_when_off():
    """without prefill_chunk the batcher makes exactly the calls it made before the feature existed: the list below was recorded from the
    scheduler of the commit before it, on this scenario"""
    e = _engine(max_prefill_tokens=512)
    cb = ContinuousBatcher(e, chunk=4, headroom_pages=0)
    assert cb.prefill_chunk is None and cb.filling == []
    reqs = [_req(60, 6, first=1), _req(300, 11, first=2), _req(100, 3, first=3), _req(90, 7, first=4), _req(70, 5, first=5)]
    ids = [cb.submit(r) for r in reqs]
    done, steps = _steps(cb, e)
    assert done == {i: [2 + k] * r.max_new_tokens for k, (i, r) in enumerate(zip(ids, reqs))}
    assert [ev for st in steps for ev in st] == [("prefill", (0, 1, 2)), ("decode", 4, (0, 1, 2)), ("prefill", (2, 3)), ("decode", 4, (0, 1, 2, 3)),
                                                 ("decode", 4, (1, 2))]
    assert cb.admissions == 2 and cb.fill_passes == 0


# ---------------------------------------------------------------------------------------------------- 3. the server

def test_server_flag_validation():
    from dots_ocr_amd.server import build_arg_parser, chunked_prefill_args, main
    ap_ = build_arg_parser()
    assert chunked_prefill_args(ap_.parse_args([])) is None                # the default: today's behaviour
    assert chunked_prefill_args(ap_.parse_args(["--enable-chunked-prefill"])) == 2048
    assert chunked_prefill_args(ap_.parse_args(["--enable-chunked-prefill", "--max-num-batched-tokens", "4096"])) == 4096
    for bad in (["--max-num-batched-tokens", "1024"], ["--enable-chunked-prefill", "--static-batching"],
                ["--enable-chunked-prefill", "--speculative-ngram", "2"], ["--enable-chunked-prefill", "--max-num-batched-tokens", "100"],
                ["--enable-chunked-prefill", "--max-num-batched-tokens", "0"], ["--enable-chunked-prefill", "--max-num-batched-tokens", "-64"]):
        with pytest.raises(ValueError):
            chunked_prefill_args(ap_.parse_args(bad))
    for argv in (["--enable-chunked-prefill", "--static-batching"], ["--enable-chunked-prefill", "--speculative-ngram", "2"]):
        with pytest.raises(SystemExit):                                    # refused at server start, before anything is loaded
            main(argv)


def test_prefill_chunk_reaches_the_batcher_through_the_server():
    from fastapi.testclient import TestClient
    from dots_ocr_amd.config import DotsConfig
    from dots_ocr_amd.processing import DotsOcrProcessor
    from dots_ocr_amd.server import ContinuousWorker, create_app
    from dots_ocr_amd.synthetic import synth_page
    from test_server_cpu import _payload
    cfg = DotsConfig.tiny()
    proc = DotsOcrProcessor(cfg)

    class Model:
        config = cfg

    model = Model()
    model.engine = ChunkEngine(lambda prompt: proc.tokenizer.encode("ok") + [cfg.eos_token_ids[0]], 200, max_batch=3, max_patches=4096,
                               max_prefill_tokens=4096, max_seq_len=2048)
    with pytest.raises(ValueError, match="continuous"):
        create_app(model, proc, model_name="model", max_batch=3, continuous=False, prefill_chunk=64)
    app = create_app(model, proc, model_name="model", max_batch=3, prefill_chunk=64)
    with TestClient(app) as c:
        assert isinstance(app.state.worker, ContinuousWorker) and app.state.worker.prefill_chunk == 64
        results = [None] * 3

        def go(i):
            results[i] = c.post("/v1/chat/completions", json=_payload(synth_page(i, (112, 84 + 28 * i))))
        th = [threading.Thread(target=go, args=(i,)) for i in range(3)]
        [t.start() for t in th]
        [t.join() for t in th]
        for r in results:
            assert r.status_code == 200, r.text
            assert r.json()["choices"][0]["message"]["content"] == "ok"
    kinds = [ev[0] for ev in model.engine.log]
    assert "begin" in kinds and "prefill" not in kinds
    assert all(ev[1] == 64 for ev in model.engine.log if ev[0] == "advance") and kinds.count("advance") >= 3
    # off: the worker hands the batcher nothing new
    app = create_app(model, proc, model_name="model", max_batch=3)
    assert app.state.worker.prefill_chunk is None and app.state.worker._chunk_kw() == {}
    app.state.worker.close()
