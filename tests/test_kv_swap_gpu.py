"""Suspend and resume on the GPU: Engine.slot_suspend parks a running sequence in its slot and moves the KV pages it holds
alone to pinned host memory; Engine.slot_resume brings it back on whatever pages are free then.  The contract is exact — a resumed row
generates, bit for bit, the tokens and logprobs of the undisturbed run — so every comparison here is for equality, and each test checks
that what it compares is not trivially equal (sampled rows differ from one another, greedy rows are not constant, KV is not all zero)."""
import numpy as np
import pytest

from dots_ocr_amd import guided as G
from dots_ocr_amd.config import DotsConfig
from dots_ocr_amd.engine import DotsEngineError, LogitRules, NgramRule, SamplingParams
from dots_ocr_amd.stop_strings import first_stop
from dots_ocr_amd.weights import random_state_dict

pytestmark = pytest.mark.gpu

SEED = 5200
CHUNK = 16
SWAP_CHUNK_PAGES = 32                # csrc/kernels.h KV_SWAP_CHUNK_PAGES
E_STATE, E_CAPACITY = -3, -4


def _cfg():
    return DotsConfig.tiny(layers=3, v_layers=3, vocab=1024)


def _token_table(V):
    """256 single bytes, then two letters of "abc " per token: what the guide and the stop strings of the feature test are written over"""
    toks = [bytes([i]) for i in range(256)] + [bytes([97 + i % 3, 32 if i % 5 == 0 else 97 + (i // 3) % 3]) for i in range(256, V)]
    return toks


def _engine(**kw):
    from dots_ocr_amd.engine import Engine
    cfg = _cfg()
    args = dict(max_batch=8, max_seq_len=640, max_patches=4096, max_prefill_tokens=2048)
    args.update(kw)
    e = Engine(cfg, **args)
    e.load_state_dict(random_state_dict(cfg, seed=11))
    return cfg, e


@pytest.fixture(scope="module")
def eng():
    """the default pool (every slot at max_seq_len): nothing runs dry here"""
    cfg, e = _engine()
    e.set_token_bytes(G.TokenBytes(_token_table(cfg.vocab_size), range(cfg.vocab_size - 8, cfg.vocab_size)))
    yield cfg, e
    e.close()


@pytest.fixture(scope="module")
def small():
    """12 pages: the LIFO free list hands a freed page straight out again"""
    cfg, e = _engine(kv_pool_tokens=12 * 64)
    yield cfg, e
    e.close()


def _prompt(cfg, L, seed=0):
    return np.random.default_rng(9000 + 13 * L + seed).integers(0, cfg.vocab_size - 8, L).astype(np.int32)


def _sampled(i):
    return SamplingParams(temperature=1.0, top_p=0.95, seed=SEED + i)


def _start(e, swap_pages=None):
    e.set_sampling(0.0, 1.0, 0)
    e.slots_reset()
    e.set_eos([])
    if swap_pages is not None:
        e.kv_swap_reserve(swap_pages)


def _decode_to_end(e, slots, limit=400):
    steps = 0
    while steps < limit:
        fin, _ = e.slots_poll()
        if all(fin[s] == 1 for s in slots):
            return
        e.slots_decode(CHUNK)
        steps += CHUNK
    raise AssertionError(f"slots {slots} did not finish within {limit} steps: {e.slots_poll()}")


def _read(e, s, lp=True):
    _, lens = e.slots_poll()
    n = int(lens[s])
    return e.slot_read(s, n).tolist(), (e.row_logprobs(s, n) if lp else None)


def _same_lp(a, b):
    return all(x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))


def _solo(e, slot, ids, n_new, sp=None, lp=5):
    """the uninterrupted run of one sequence in `slot`"""
    _start(e)
    if sp is not None:
        e.set_row_sampling(slot, sp)
    e.set_row_logprobs(slot, lp)
    e.slots_prefill([slot], ids, [len(ids)], [n_new])
    _decode_to_end(e, [slot])
    out = _read(e, slot)
    e.slot_release(slot)
    return out


def _kv(cfg, e, slot, n):
    """K and V of every layer over positions [0, n) of the row"""
    return [e.read_kv(layer, slot, 0, n, which) for layer in range(cfg.num_hidden_layers) for which in ("k", "v")]


def _same_kv(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and np.array_equal(x, y) for x, y in zip(a, b))


# ---------------------------------------------------------------------------------------------------- 1. exact resume on other physical pages

def test_resumed_row_equals_the_uninterrupted_run(small):
    cfg, e = small
    L, n_new, Lb, nb = 100, 80, 130, 40                               # L + 16 + 12 = 128: the second suspension sits on a page boundary
    a, b = _prompt(cfg, L), _prompt(cfg, Lb, seed=3)
    want_a = _solo(e, 1, a, n_new, _sampled(0))
    want_b = _solo(e, 3, b, nb, _sampled(1))
    assert len(set(want_a[0])) > 8 and want_a[0][:nb] != want_b[0]     # a sampled reading, and not the other sequence's

    _start(e, swap_pages=6)
    e.set_row_sampling(1, _sampled(0))
    e.set_row_logprobs(1, 5)
    e.slots_prefill([1], a, [L], [n_new])
    e.slots_decode(CHUNK)
    pages = e.slot_capacity(1)[0]
    assert e.kv_pool_info() == (12, 12 - pages)
    e.slot_suspend(1)
    assert e.kv_pool_info() == (12, 12) and e.kv_swap_info() == (6, 6 - (L + CHUNK + 63) // 64)
    fin, lens = e.slots_poll()
    assert fin[1] == 2 and lens[1] == CHUNK + 1
    # a second sequence on the pages just freed, run to its end beside the idle row
    e.set_row_sampling(3, _sampled(1))
    e.set_row_logprobs(3, 5)
    e.slots_prefill([3], b, [Lb], [nb])
    _decode_to_end(e, [3])
    got_b = _read(e, 3)
    fin, lens = e.slots_poll()
    assert fin[1] == 2 and lens[1] == CHUNK + 1                        # the idle row grew by nothing
    assert e.slot_read(1, CHUNK + 1).tolist() == want_a[0][:CHUNK + 1]
    e.slot_release(3)
    e.slot_resume(1)
    assert e.kv_swap_info() == (6, 6)
    e.slots_decode(12)                                                 # context 128: an exact multiple of 64
    fin, lens = e.slots_poll()
    assert fin[1] == 0 and L + int(lens[1]) - 1 == 128
    e.slot_suspend(1)
    assert e.kv_swap_info() == (6, 4) and e.kv_pool_info() == (12, 12)
    e.slot_resume(1)
    _decode_to_end(e, [1])
    got_a = _read(e, 1)
    assert got_a[0] == want_a[0] and _same_lp(got_a[1], want_a[1])
    assert got_b[0] == want_b[0] and _same_lp(got_b[1], want_b[1])
    e.slots_reset()
    assert e.kv_pool_info() == (12, 12)


# ---------------------------------------------------------------------------------------------------- 2. raw KV round trip

def _check_kv_round_trip(cfg, e):
    """The pool accounting proves that the row comes back on other pages: with the pool full, the row's three pages are the only free ones
    after its suspension; a new sequence takes exactly those; the filler's release then frees nine OTHER pages, which the resume draws from."""
    La, na, Lc, nc, Lb, nb = 150, 40, 500, 64, 130, 20
    a, c, b = _prompt(cfg, La), _prompt(cfg, Lc, seed=1), _prompt(cfg, Lb, seed=2)
    want = _solo(e, 1, a, na, _sampled(5))[0]
    assert len(set(want)) > 8

    _start(e, swap_pages=3)
    e.set_row_sampling(1, _sampled(5))
    e.slots_prefill([1, 2], np.concatenate([a, c]), [La, Lc], [na, nc])
    assert e.kv_pool_info() == (12, 0)
    e.slots_decode(8)
    ctx = La + 8
    before = _kv(cfg, e, 1, ctx)
    assert all(x.any() for x in before)
    e.slot_suspend(1)
    assert e.kv_pool_info() == (12, 3) and e.kv_swap_info() == (3, 0)
    with pytest.raises(DotsEngineError):
        e.read_kv(0, 1, 0, 1, "k")                                     # nothing of the row is in the cache
    e.slots_prefill([3], b, [Lb], [nb])                                # exactly the three pages the row gave back
    assert e.kv_pool_info() == (12, 0)
    e.slot_release(2)
    assert e.kv_pool_info() == (12, 9)
    e.slot_resume(1)                                                   # from the filler's pages: slot 3 still holds the row's old ones
    assert e.kv_pool_info() == (12, 6) and e.kv_swap_info() == (3, 3)
    after = _kv(cfg, e, 1, ctx)
    assert _same_kv(before, after)
    _decode_to_end(e, [1, 3])
    assert _read(e, 1, lp=False)[0] == want
    e.slots_reset()


def test_kv_round_trip_bf16(small):
    cfg, e = small
    _check_kv_round_trip(cfg, e)


def test_kv_round_trip_fp8():
    cfg, e = _engine(kv_pool_tokens=12 * 64, kv_cache_dtype="fp8")
    try:
        _check_kv_round_trip(cfg, e)
    finally:
        e.close()


# ---------------------------------------------------------------------------------------------------- 3. more than one staging chunk

def test_a_sequence_longer_than_the_staging_buffer():
    cfg, e = _engine(max_batch=2, max_seq_len=2560, max_prefill_tokens=2304)
    try:
        L, n_new = 2150, 40
        ids, other = _prompt(cfg, L), _prompt(cfg, 200, seed=4)
        want = _solo(e, 0, ids, n_new, _sampled(2))
        assert len(set(want[0])) > 8
        _start(e, swap_pages=40)
        e.set_row_sampling(0, _sampled(2))
        e.set_row_logprobs(0, 5)
        e.slots_prefill([0], ids, [L], [n_new])
        e.slots_decode(CHUNK)
        ctx = L + CHUNK
        n_pages = (ctx + 63) // 64
        assert n_pages > SWAP_CHUNK_PAGES and n_pages % SWAP_CHUNK_PAGES          # two chunks, the second a partial one
        before = _kv(cfg, e, 0, ctx)
        assert all(x.any() for x in before)
        total, free = e.kv_pool_info()
        e.slot_suspend(0)
        assert e.kv_swap_info() == (40, 40 - n_pages) and e.kv_pool_info() == (total, total)
        e.slots_prefill([1], other, [len(other)], [8])                 # takes the top of the free list: the row comes back on other pages
        e.slot_resume(0)
        assert e.kv_swap_info() == (40, 40)
        assert _same_kv(before, _kv(cfg, e, 0, ctx))
        e.slot_release(1)
        _decode_to_end(e, [0])
        got = _read(e, 0)
        assert got[0] == want[0] and _same_lp(got[1], want[1])
    finally:
        e.close()


# ---------------------------------------------------------------------------------------------------- 4. every row feature across a suspension

FEATURE_SLOTS = [1, 4, 2, 6, 0, 5]   # penalties, logit rules, guide, n-gram rule, stop string, logprobs: neither ascending nor adjacent
FEATURE_NEW = 64
_FEATURES = {}


def _feature_rows(cfg, e, stop):
    allowed = tuple(range(300, 324))
    return [
        dict(sp=SamplingParams(temperature=0.9, top_p=0.95, seed=SEED + 10, repetition_penalty=1.2, frequency_penalty=0.3, presence_penalty=0.2), lp=2),
        dict(sp=SamplingParams(temperature=1.5, seed=SEED + 11), rules=LogitRules(allowed=allowed, min_tokens=40, stop=allowed[:8]), lp=2),
        dict(sp=SamplingParams(temperature=0.8, top_p=0.95, seed=SEED + 12), guide=e.create_guide(G.compile_regex(r"[a-c ]*")), lp=2),
        dict(sp=SamplingParams(temperature=0.7, seed=SEED + 13), ngram=NgramRule(3), lp=2),
        dict(sp=SamplingParams(temperature=1.0, seed=SEED + 14), rules=LogitRules(allowed=tuple(range(256, cfg.vocab_size - 8))), stop=stop, lp=2),
        dict(lp=5),
    ]


def _feature_run(cfg, e, stop, suspend=()):
    """the six rows of one batch; `suspend`: the slots parked after the first chunk for two chunks while the others run"""
    rows = _feature_rows(cfg, e, stop)
    prompts = [_prompt(cfg, 40 + 7 * i, seed=20 + i) for i in range(6)]
    prompts[2][:20] = np.arange(97, 117)
    _start(e, swap_pages=8)
    for s, r in zip(FEATURE_SLOTS, rows):
        if "sp" in r:
            e.set_row_sampling(s, r["sp"])
        if "rules" in r:
            e.set_row_logit_rules(s, r["rules"])
        if "guide" in r:
            e.set_row_guide(s, r["guide"])
        if "ngram" in r:
            e.set_row_ngram(s, r["ngram"])
        if r.get("stop"):
            e.set_row_stop(s, e.create_stop(list(r["stop"])), 0)
        e.set_row_logprobs(s, r["lp"])
    e.slots_prefill(FEATURE_SLOTS, np.concatenate(prompts), [len(p) for p in prompts], [FEATURE_NEW] * 6)
    e.slots_decode(CHUNK)
    if suspend:
        _, lens0 = e.slots_poll()
        states = {s: (e.row_guide_state(s), e.row_stop_hit(s)) for s in suspend}
        for s in suspend:
            e.slot_suspend(s)
        e.slots_decode(2 * CHUNK)
        fin, lens = e.slots_poll()
        for s in suspend:                                              # parked: no token, no automaton step, no logprob position
            assert fin[s] == 2 and lens[s] == lens0[s] == CHUNK + 1
            assert (e.row_guide_state(s), e.row_stop_hit(s)) == states[s]
            assert e.row_logprobs(s, FEATURE_NEW)[0].shape[0] == CHUNK + 1
        assert all(lens[s] > lens0[s] for s in FEATURE_SLOTS if s not in suspend and not fin[s])
        for s in reversed(suspend):
            e.slot_resume(s)
    _decode_to_end(e, FEATURE_SLOTS)
    out = []
    for s in FEATURE_SLOTS:
        toks, lp = _read(e, s)
        out.append(dict(toks=toks, lp=lp, hit=e.row_stop_hit(s), state=e.row_guide_state(s)))
    e.slots_reset()
    for r in rows:
        if "guide" in r:
            e.destroy_guide(r["guide"])
    return out


def _features(eng):
    """the uninterrupted batch, computed once: first without a stop string, to pick one from the row's own bytes whose match begins before
    the suspension (17 tokens exist then) and ends after it"""
    cfg, e = eng
    if not _FEATURES:
        table = _token_table(cfg.vocab_size)
        chunks = [table[t] for t in _feature_run(cfg, e, None)[4]["toks"]]
        n_susp = CHUNK + 1
        pick = None
        for first in range(n_susp - 3, n_susp):
            for last in range(n_susp, n_susp + 3):
                s = b"".join(chunks[first:last + 1]).decode()
                hit = first_stop(chunks, [s])
                if pick is None and hit is not None and hit[0] == last and hit[1] == len(chunks[last]):
                    pick = ([s], hit)
        assert pick is not None, "the seeded row offers no stop string that straddles the suspension: a test error, choose another seed"
        _FEATURES.update(stop=pick[0], hit=pick[1], want=_feature_run(cfg, e, pick[0]))
    return _FEATURES


@pytest.mark.parametrize("half", [0, 1])
def test_every_row_feature_survives_a_suspension(eng, half):
    cfg, e = eng
    f = _features(eng)
    want = f["want"]
    # the reference itself: the stop row ends at the picked match, past the suspension point; the rule row ends on a stop id after
    # min_tokens; rows differ from one another; the greedy row is not constant
    assert want[4]["hit"] == f["hit"] and CHUNK + 1 <= f["hit"][0] < FEATURE_NEW - 1 and len(want[4]["toks"]) == f["hit"][0] + 1
    assert 40 < len(want[1]["toks"]) < FEATURE_NEW and want[1]["toks"][-1] in range(300, 308)
    assert len({tuple(w["toks"][:30]) for w in want}) == 6 and len(set(want[5]["toks"])) > 2
    assert want[2]["state"] >= 0 and all(w["state"] == -1 for i, w in enumerate(want) if i != 2)
    got = _feature_run(cfg, e, f["stop"], suspend=FEATURE_SLOTS[half::2])
    for i, (g, w) in enumerate(zip(got, want)):
        assert g["toks"] == w["toks"], i
        assert _same_lp(g["lp"], w["lp"]), i
        assert g["hit"] == w["hit"] and g["state"] == w["state"], i


# ---------------------------------------------------------------------------------------------------- 5. forked siblings

def test_a_suspended_fork_child_leaves_the_shared_pages_resident(small):
    cfg, e = small
    L, n_new, slots = 130, 48, [1, 4, 2]
    ids = _prompt(cfg, L)

    def fork():
        _start(e, swap_pages=4)
        for i, s in enumerate(slots):
            e.set_row_sampling(s, _sampled(20 + i))
            e.set_row_logprobs(s, 5)
        e.slots_prefill(slots[:1], ids, [L], [n_new])
        e.slots_fork(slots[0], slots[1:])
        e.slots_decode(CHUNK)

    fork()
    _decode_to_end(e, slots)
    want = [_read(e, s) for s in slots]
    assert len({tuple(w[0]) for w in want}) == 3

    fork()
    shared = L // 64
    total, free = e.kv_pool_info()
    owned = e.slot_capacity(4)[0]
    assert owned > shared
    e.slot_suspend(4)
    assert e.kv_pool_info() == (total, free + owned - shared)          # exactly the pages it held alone
    assert e.slot_capacity(4)[0] == shared                             # the prompt pages stay, and stay counted for this row
    assert e.kv_swap_info() == (4, 4 - (owned - shared))
    e.slots_decode(CHUNK)
    fin, lens = e.slots_poll()
    assert fin[4] == 2 and lens[4] == CHUNK + 1 and lens[1] == lens[2] == 2 * CHUNK + 1      # the siblings decode on
    e.slot_resume(4)
    assert e.slot_capacity(4)[0] >= shared + 1
    _decode_to_end(e, slots)
    for s, w in zip(slots, want):
        got = _read(e, s)
        assert got[0] == w[0] and _same_lp(got[1], w[1]), s
    for s in slots:
        e.slot_release(s)
    assert e.kv_pool_info() == (total, total) and e.kv_swap_info() == (4, 4)


# ---------------------------------------------------------------------------------------------------- 6. accounting and refusals

def _state(e):
    return e.kv_pool_info(), e.kv_swap_info(), e.slots_poll()[0].tolist(), e.slots_poll()[1].tolist()


def _refused(e, call, code):
    before = _state(e)
    with pytest.raises(DotsEngineError) as err:
        call()
    assert err.value.code == code, err.value
    assert _state(e) == before


def test_refusals_change_nothing(small):
    cfg, e = small
    a, short, beam, big = _prompt(cfg, 130), _prompt(cfg, 100, seed=1), _prompt(cfg, 70, seed=2), _prompt(cfg, 250, seed=3)
    want = _solo(e, 0, a, 40, _sampled(6))[0]
    assert len(set(want)) > 8

    _start(e, swap_pages=4)
    e.set_row_sampling(0, _sampled(6))
    e.slots_prefill([0, 5], np.concatenate([a, short]), [130, 100], [40, 4])
    e.slots_prefill([2], beam, [70], [8])
    e.slots_beam(2, [3])
    e.slots_decode(4)
    fin, _ = e.slots_poll()
    assert [int(fin[s]) for s in (0, 5, 2, 3, 7)] == [0, 1, 0, 0, -1]
    _refused(e, lambda: e.slot_suspend(7), E_STATE)                    # a free slot
    _refused(e, lambda: e.slot_suspend(5), E_STATE)                    # a finished slot
    _refused(e, lambda: e.slot_suspend(2), E_STATE)                    # the rows of a beam group
    _refused(e, lambda: e.slot_suspend(3), E_STATE)
    _refused(e, lambda: e.slot_resume(0), E_STATE)                     # not suspended
    e.slot_release(2)
    e.slot_release(5)
    e.slot_suspend(0)
    assert e.kv_pool_info() == (12, 12) and e.kv_swap_info() == (4, 1)
    _refused(e, lambda: e.slot_suspend(0), E_STATE)                    # already suspended
    _refused(e, lambda: e.kv_swap_reserve(8), E_STATE)                 # the host space is in use
    _refused(e, lambda: e.set_speculation(1), E_STATE)
    e.slots_prefill([6, 7], np.concatenate([big, big]), [250, 250], [64, 64])      # 2 x 5 pages: two are left, the row needs three
    assert e.kv_pool_info() == (12, 2)
    _refused(e, lambda: e.slot_resume(0), E_CAPACITY)                  # a dry pool
    e.slot_release(6)
    e.slot_release(7)
    e.slot_resume(0)
    e.kv_swap_reserve(2)
    _refused(e, lambda: e.slot_suspend(0), E_CAPACITY)                 # a full host space: the row needs three host pages
    _decode_to_end(e, [0])
    assert _read(e, 0, lp=False)[0] == want                            # none of it left a trace

    # a speculating engine
    e.slots_reset()
    e.set_speculation(1)
    try:
        e.set_eos([])
        e.slots_prefill([0], a, [130], [40])
        _refused(e, lambda: e.slot_suspend(0), E_STATE)
    finally:
        e.slots_reset()
        e.set_speculation(0)


def test_release_and_reset_return_the_host_pages(small):
    cfg, e = small
    a = _prompt(cfg, 130)
    _start(e, swap_pages=8)
    e.slots_prefill([0, 1], np.concatenate([a, a]), [130, 130], [40, 40])
    e.slots_decode(4)
    e.slot_suspend(0)
    e.slot_suspend(1)                                                  # context 134: three pages each
    assert e.kv_swap_info() == (8, 2) and e.kv_pool_info() == (12, 12)
    e.slot_release(0)
    assert e.kv_swap_info() == (8, 5) and e.slots_poll()[0].tolist()[:2] == [-1, 2]
    e.slots_reset()
    assert e.kv_swap_info() == (8, 8) and e.kv_pool_info() == (12, 12)
    assert e.slots_poll()[0].tolist() == [-1] * 8
    e.kv_swap_reserve(0)
    assert e.kv_swap_info() == (0, 0)


def test_pages_short_agrees_with_what_decode_does(small):
    cfg, e = small
    a, b = _prompt(cfg, 120), _prompt(cfg, 400, seed=1)
    _start(e, swap_pages=0)
    e.slots_prefill([0, 1], np.concatenate([a, b]), [120, 400], [300, 200])        # 3 + 8 pages: one is free
    assert e.kv_pool_info() == (12, 1)
    limits = [120 + 300, 400 + 200]

    def caps():
        return [e.slot_capacity(s)[1] for s in (0, 1)]

    assert e.slots_pages_short(64) == 0                                # both are covered by what they hold
    e.slots_decode(64)
    assert caps() == limits and e.kv_pool_info() == (12, 1)
    assert e.slots_pages_short(64) == 1                                # each lacks one page, one is free
    assert e.slots_pages_short(1) == 0                                 # but neither for one more step
    e.slots_decode(64)
    got = caps()
    assert got[0] == limits[0] and got[1] < limits[1] and e.kv_pool_info() == (12, 0)      # one row was capped, as the call said
    assert e.slots_pages_short(64) == 1                                # the capped row asks for nothing more; the other lacks a page
    e.slots_decode(64)
    assert caps()[0] < limits[0] and caps()[1] == got[1]
    e.slots_reset()


# ---------------------------------------------------------------------------------------------------- 7. through the scheduler

def test_swap_preemption_through_the_scheduler(eng, small):
    from dots_ocr_amd.scheduler import ContinuousBatcher, Request
    cfg, big = eng
    _, e = small

    def requests():
        return [Request(_prompt(cfg, 100, seed=30 + i), max_new_tokens=200, sampling=_sampled(30 + i), logprobs=2) for i in range(3)]

    big.set_sampling(0.0, 1.0, 0)
    e.set_sampling(0.0, 1.0, 0)
    ref = requests()
    want = [o.tolist() for o in ContinuousBatcher(big, chunk=CHUNK, headroom_pages=0).run(ref)]
    assert all(len(w) == 200 for w in want) and len({tuple(w) for w in want}) == 3

    # today's behaviour on 12 pages: three sequences of five pages each at their caps, admitted together, and one runs dry
    plain = ContinuousBatcher(e, chunk=CHUNK, headroom_pages=0)
    cut = plain.run(requests())
    assert plain.kv_truncated >= 1 and any(len(c) < 200 for c in cut)

    cb = ContinuousBatcher(e, chunk=CHUNK, headroom_pages=0, preemption="swap")
    reqs = requests()
    got = [o.tolist() for o in cb.run(reqs)]
    assert cb.kv_truncated == 0 and cb.preemptions > 0 and cb.resumes == cb.preemptions and cb.swapped_pages > 0
    assert got == want
    for r, w in zip(reqs, ref):
        assert not r.kv_truncated and _same_lp(r.logprobs_out, w.logprobs_out)
    assert e.kv_pool_info() == (12, 12) and e.kv_swap_info() == (12, 12)
