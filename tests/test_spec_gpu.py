"""N-gram speculative decoding on the GPU.  Every comparison is exact: a speculating engine must commit the tokens of the
unspeculated engine, only in fewer steps.

`ref` is an engine that never speculates; its token lists are computed once per (prompt, cap) and shared.  The accept path is driven
deterministically through Engine.set_row_drafts (no built-in drafter: max_n = 0), the drafter kernel alone through
Engine.ngram_draft_op against the host rule engine.ngram_draft, and both together through the ContinuousBatcher."""
import numpy as np
import pytest

from dots_ocr_amd.config import DotsConfig
from dots_ocr_amd.engine import DotsEngineError, NgramRule, SamplingParams, ngram_draft
from dots_ocr_amd.weights import random_state_dict

pytestmark = pytest.mark.gpu

SEQ = 640


def _engine(max_batch, kv_cache_dtype=None):
    from dots_ocr_amd.engine import Engine
    cfg = DotsConfig.tiny(layers=3, v_layers=3, vocab=1024)
    e = Engine(cfg, max_batch=max_batch, max_seq_len=SEQ, max_patches=4096, max_prefill_tokens=2048, kv_cache_dtype=kv_cache_dtype)
    e.load_state_dict(random_state_dict(cfg, seed=11))
    return cfg, e


@pytest.fixture(scope="module")
def ref():
    """the unspeculated engine and its token lists, keyed by (prompt seed, prompt length, cap, eos)"""
    cfg, e = _engine(16)
    cache = {}

    def tokens(seed, length, cap, eos=()):
        key = (seed, length, cap, tuple(eos))
        if key not in cache:
            cache[key] = _plain_run(e, [_prompt(cfg, seed, length)], [cap], eos)[0]
        return list(cache[key])
    yield cfg, e, tokens
    e.close()


@pytest.fixture(scope="module")
def spec():
    cfg, e = _engine(16)
    yield cfg, e
    e.close()


def _prompt(cfg, seed, length):
    return np.random.default_rng(seed).integers(0, cfg.vocab_size - 8, length).astype(np.int32)


def _plain_run(e, prompts, caps, eos=(), chunk=16):
    """prefill into slots 0 .. and decode to the end without speculation: token lists"""
    e.set_sampling(0.0, 1.0, 0)
    e.slots_reset()
    e.set_eos(list(eos))
    slots = list(range(len(prompts)))
    e.slots_prefill(slots, np.concatenate(prompts), [len(p) for p in prompts], caps)
    for _ in range(-(-max(caps) // chunk)):
        e.slots_decode(chunk)
    fin, lens = e.slots_poll()
    assert all(fin[s] == 1 for s in slots)
    toks = [e.slot_read(s, int(lens[s])).tolist() for s in slots]
    for s in slots:
        e.slot_release(s)
    return toks


def _fresh(e, k, min_n=2, max_n=4, eos=()):
    e.set_sampling(0.0, 1.0, 0)
    e.slots_reset()
    e.set_speculation(k, min_n, max_n)
    e.set_eos(list(eos))


# ---------------------------------------------------------------------------------------------------- 1. the drafter kernel

def _histories():
    rng = np.random.default_rng(9)
    far = [int(t) for t in rng.integers(4, 1000, 4096)]             # L = 4096; the only match of the last 4 tokens starts at i = 3000,
    far[3000:3004] = far[-4:]                                        # far past a thread's first stride (256 threads)
    far[2999], far[3004] = 1001, 1002
    full_vs_recent = [7, 8, 11, 12, 13, 7, 8, 21, 7, 8]
    return {
        "longest_n": [1, 2, 3, 4, 50, 9, 3, 4, 60, 1, 2, 3, 4],
        "recent_full": [7, 8, 11, 12, 13, 7, 8, 21, 22, 23, 7, 8],
        "full_over_recent": full_vs_recent,
        "run": [5, 5, 5, 5],
        "L_eq_min_n": [4, 4],
        "L_min_n_plus_1": [4, 4, 4],
        "one": [4],
        "no_match": list(range(100, 140)),
        "unigrams_only": [1, 2, 3, 1, 3, 2, 2, 1],
        "k_over_rest": [1, 2, 3, 1, 2],
        "far": far,
        "period_300": [int(t) for t in rng.integers(4, 1000, 300)] * 5,     # many matches in every thread's stride: the most recent full one
    }


@pytest.mark.parametrize("k,min_n,max_n", [(3, 2, 4), (4, 2, 2), (1, 1, 3), (15, 2, 4), (7, 1, 64)])
def test_drafter_kernel_equals_the_host_rule(spec, k, min_n, max_n):
    _, e = spec
    H = _histories()
    names = sorted(H)
    want = {nm: ngram_draft(H[nm], k, min_n, max_n) for nm in names}
    # every history as a launch of its own, then all of them (different lengths) in one launch
    for nm in names:
        assert e.ngram_draft_op([H[nm]], k, min_n, max_n) == [want[nm]], nm
    got = e.ngram_draft_op([H[nm] for nm in names], k, min_n, max_n)
    assert got == [want[nm] for nm in names], [nm for nm, g in zip(names, got) if g != want[nm]]
    if (k, min_n, max_n) == (3, 2, 4):                              # the planted cases are what they are meant to be
        assert want["far"] == [1002] + H["far"][3005:3007] and want["run"] == [5] and want["no_match"] == [] and want["L_eq_min_n"] == []
        assert want["full_over_recent"] == [21, 7, 8] and want["longest_n"] == [50, 9, 3]
    if (k, min_n, max_n) == (4, 2, 2):
        assert want["full_over_recent"] == [11, 12, 13, 7]


def test_drafter_kernel_on_random_histories(spec):
    """64 rows of a small alphabet (matches everywhere, ties between positions) in one launch"""
    _, e = spec
    rng = np.random.default_rng(21)
    hist = [[int(t) for t in rng.integers(0, 3 + b % 5, 1 + (37 * b) % 700)] for b in range(64)]
    for k, lo, hi in ((3, 2, 4), (15, 1, 8)):
        assert e.ngram_draft_op(hist, k, lo, hi) == [ngram_draft(h, k, lo, hi) for h in hist]


# ---------------------------------------------------------------------------------------------------- 2. the accept path, planted drafts

P_LEN = 61          # rows 0 .. 3 of the first step sit at positions 61 .. 64: they straddle the 64-token page boundary
P_CAP = 43          # 42 decode tokens: the last step of the 4-per-step run is cut by the cap


def _fresh_at_draft_1(T):
    """the first position p = L + 2 of a step of the all-true run (L = 1, 5, 9, ...) whose token T[p] occurs nowhere before it, or None"""
    return next((q for q in range(3, P_CAP - 3, 4) if T[q] not in T[:q]), None)


@pytest.fixture(scope="module")
def p_seed(ref):
    """The prompt of the accept-path tests.  A random-weight model often falls into repeating one token; the tests want a continuation that
    varies (a wrong draft must differ from the true one for a reason other than the +1, and the EOS test needs a token that is new at draft
    index 1), so the prompt seed is the first whose reference tokens hold at least 12 distinct ids and such a token."""
    _, _, tokens = ref
    for seed in range(3, 64):
        T = tokens(seed, P_LEN, P_CAP)
        if len(set(T)) >= 12 and _fresh_at_draft_1(T) is not None:
            print(f"accept-path prompt seed {seed}: {len(set(T))} distinct ids among {len(T)} reference tokens")
            return seed
    raise AssertionError("no prompt seed in [3, 64) gives a varied reference continuation")


def _wrong(t, cfg):
    return (t + 1) % (cfg.vocab_size - 8)


def _planted_run(e, cfg, seed, T, k, cap, make_drafts, slot=0):
    """One row driven step by step with host drafts; after every step out_lens must be what the host's walk of `T` predicts.
    Returns (tokens, steps, drafted, accepted) with the host's expected counters."""
    prompt = _prompt(cfg, seed, P_LEN)
    e.slots_prefill([slot], prompt, [len(prompt)], [cap])
    end = len(T)                                                     # where the reference run stopped (cap or EOS)
    L, steps, drafted, accepted = 1, 0, 0, 0
    while L < end:
        drafts = make_drafts(L)
        e.set_row_drafts(slot, drafts)
        e.slots_decode(1)
        # the host's walk: row 0 commits T[L]; while the row is not finished (T ends where the reference finished: cap or EOS) and
        # draft `acc` is the token just committed, the next token of T is committed too.  The cap cuts the drafts that are verified
        live = max(0, min(len(drafts), cap - L - 1))
        n, acc = L + 1, 0
        while acc < live and n < end and drafts[acc] == T[n - 1]:
            acc, n = acc + 1, n + 1
        steps, drafted, accepted = steps + 1, drafted + live, accepted + acc
        L = n
        fin, lens = e.slots_poll()
        assert int(lens[slot]) == L, (steps, int(lens[slot]), L)
        assert int(fin[slot]) == (1 if L >= end else 0)
    toks = e.slot_read(slot, SEQ).tolist()
    st = e.spec_stats(slot)
    e.slot_release(slot)
    return toks, st, {"steps": steps, "drafted": drafted, "accepted": accepted}


@pytest.mark.parametrize("case,per_step", [("true", 4), ("second_wrong", 2), ("all_wrong", 1), ("none", 1)])
def test_accept_path_commits_exactly_the_sequential_tokens(ref, spec, p_seed, case, per_step):
    cfg, _, tokens = ref
    _, e = spec
    cap = P_CAP
    T = tokens(p_seed, P_LEN, cap)
    assert len(T) == cap
    pad = T + [0] * 4

    def make(L):
        if case == "none":
            return []
        d = pad[L:L + 3][:max(0, cap - L)]
        if case == "second_wrong" and len(d) > 1:
            d[1] = _wrong(d[1], cfg)
        if case == "all_wrong":
            d = [_wrong(t, cfg) for t in d]
        return d
    _fresh(e, 3, max_n=0)
    toks, st, want = _planted_run(e, cfg, p_seed, T, 3, cap, make)
    assert toks == T
    assert st == want
    assert want["steps"] == -(-(cap - 1) // per_step)
    if case == "true":
        assert want["accepted"] == cap - 1 - want["steps"] and want["drafted"] == want["accepted"]
    if case in ("all_wrong", "none"):
        assert want["accepted"] == 0
    assert e.spec_stats() == want                                     # the engine's totals: this row is all that ran since set_speculation


# ---------------------------------------------------------------------------------------------------- 3. EOS and the cap inside a draft

def test_eos_at_draft_index_1_finishes_the_row_there(ref, spec, p_seed):
    cfg, _, tokens = ref
    _, e = spec
    T = tokens(p_seed, P_LEN, P_CAP)
    # steps of the all-true run start at L = 1, 5, 9, ...; draft index 1 is verified by committing T[L + 2]
    p = _fresh_at_draft_1(T)
    eos = [T[p]]
    Te = tokens(p_seed, P_LEN, P_CAP, eos)
    assert Te == T[:p + 1]                                            # the unspeculated engine stops there too
    _fresh(e, 3, max_n=0, eos=eos)
    total, free = e.kv_pool_info()
    assert free == total
    toks, st, want = _planted_run(e, cfg, p_seed, Te, 3, P_CAP, lambda L: (T + [0] * 4)[L:L + 3])
    assert toks == Te and st == want
    assert want["steps"] == (p - 3) // 4 + 1 and want["accepted"] == p - want["steps"]
    assert e.kv_pool_info() == (total, total)


def test_cap_at_draft_index_1_ends_the_row_at_the_cap(ref, spec, p_seed):
    cfg, _, tokens = ref
    _, e = spec
    cap = 8                                                           # the step at L = 5 may commit T[5], T[6], T[7]: draft index 2 is past the cap
    T = tokens(p_seed, P_LEN, cap)
    long = tokens(p_seed, P_LEN, P_CAP)
    assert T == long[:cap]
    _fresh(e, 3, max_n=0)
    total, _ = e.kv_pool_info()
    toks, st, want = _planted_run(e, cfg, p_seed, T, 3, cap, lambda L: long[L:L + 3])      # three true drafts every step, the cap must cut them
    assert toks == T and len(toks) == cap
    assert st == want and want == {"steps": 2, "drafted": 3 + 2, "accepted": 3 + 2}
    assert e.kv_pool_info() == (total, total)


# ---------------------------------------------------------------------------------------------------- 4. the built-in drafter, end to end

REQS = [(101, 7, 40), (102, 61, 33), (103, 30, 50), (104, 64, 17), (105, 100, 64), (106, 15, 25)]      # (prompt seed, prompt length, cap)


def _batched(e, cfg, chunk, eos):
    from dots_ocr_amd.scheduler import ContinuousBatcher, Request
    cb = ContinuousBatcher(e, eos_ids=eos, chunk=chunk)
    outs = cb.run([Request(_prompt(cfg, s, n), max_new_tokens=cap) for s, n, cap in REQS])
    return [o.tolist() for o in outs], cb


@pytest.fixture(scope="module")
def e2e_ref(ref):
    """the six requests on the unspeculated engine, with an EOS id that ends one of them early"""
    cfg, e, tokens = ref
    long = tokens(105, 100, 64)
    eos = [next(t for i, t in enumerate(long) if i >= 20 and t not in long[:i])]
    want = [tokens(s, n, cap, eos) for s, n, cap in REQS]
    assert len(want[4]) < 64
    return eos, want


@pytest.mark.parametrize("chunk", [1, 16])
def test_builtin_drafter_end_to_end(ref, spec, e2e_ref, chunk):
    cfg, _, _ = ref
    _, e = spec
    eos, want = e2e_ref
    _fresh(e, 3)
    got, cb = _batched(e, cfg, chunk, eos)
    assert cb.n_slots == 4
    assert got == want
    st = e.spec_stats()
    # every decode token is row 0 of a step or an accepted draft
    assert st["steps"] + st["accepted"] == sum(len(t) - 1 for t in want)
    assert 0 <= st["accepted"] <= st["drafted"]
    total, free = e.kv_pool_info()
    assert free == total


def test_builtin_drafter_under_the_partition_plan(ref, spec, e2e_ref):
    cfg, _, _ = ref
    _, e = spec
    eos, want = e2e_ref
    _fresh(e, 3)
    e.set_decode_plan(1)
    try:
        got, _ = _batched(e, cfg, 16, eos)
    finally:
        e.set_decode_plan(0)
    assert got == want


def test_builtin_drafter_with_the_fp8_kv_cache():
    cfg, plain = _engine(16, "fp8")
    _, e = _engine(16, "fp8")
    try:
        want = [_plain_run(plain, [_prompt(cfg, s, n)], [cap])[0] for s, n, cap in REQS]
        _fresh(e, 3)
        got, _ = _batched(e, cfg, 16, [])
        assert got == want
        st = e.spec_stats()
        assert st["steps"] + st["accepted"] == sum(len(t) - 1 for t in want)
    finally:
        plain.close()
        e.close()


# ---------------------------------------------------------------------------------------------------- 5. more than 16 rows

def test_eight_slots_of_five_rows(ref):
    """max_batch = 40, k = 4: 8 slots, 40 rows (the wide and two-tile kernels), true drafts on every slot"""
    cfg, _, tokens = ref
    _, e = _engine(40)
    try:
        cap = 31                                                      # 30 decode tokens = 6 steps of 5
        seeds = [(200 + b, 20 + 9 * b) for b in range(8)]             # prompt lengths 20 .. 83: page boundaries at different steps
        T = [tokens(s, n, cap) for s, n in seeds]
        _fresh(e, 4, max_n=0)
        assert e.usable_slots == 8
        prompts = [_prompt(cfg, s, n) for s, n in seeds]
        e.slots_prefill(list(range(8)), np.concatenate(prompts), [len(p) for p in prompts], [cap] * 8)
        for step in range(6):
            L = 1 + 5 * step
            for b in range(8):
                e.set_row_drafts(b, T[b][L:L + 4])
            e.slots_decode(1)
            fin, lens = e.slots_poll()
            assert lens[:8].tolist() == [L + 5] * 8, step
        assert fin[:8].tolist() == [1] * 8
        assert [e.slot_read(b, SEQ).tolist() for b in range(8)] == T
        assert e.spec_stats() == {"steps": 48, "drafted": 192, "accepted": 192}
    finally:
        e.close()


# ---------------------------------------------------------------------------------------------------- 6. coexistence

def _mixed_run(e, cfg, cap=40, chunk=4):
    """slot 0 sampled, slot 1 with an n-gram rule, slot 2 with logprobs, slot 3 plain greedy: (tokens, logprobs of slot 2, spec stats)"""
    e.set_row_sampling(0, SamplingParams(temperature=0.8, seed=1234))
    e.set_row_ngram(1, NgramRule(2))
    e.set_row_logprobs(2, 5)
    prompts = [_prompt(cfg, 300 + b, 12 + 17 * b) for b in range(4)]
    e.slots_prefill([0, 1, 2, 3], np.concatenate(prompts), [len(p) for p in prompts], [cap] * 4)
    for _ in range(cap // chunk):
        e.slots_decode(chunk)
    fin, lens = e.slots_poll()
    assert fin[:4].tolist() == [1] * 4 and lens[:4].tolist() == [cap] * 4
    toks = [e.slot_read(b, SEQ).tolist() for b in range(4)]
    lp = e.row_logprobs(2, cap)
    stats = [e.spec_stats(b) for b in range(4)]
    for b in range(4):
        e.slot_release(b)
    return toks, lp, stats


def test_sampled_ruled_and_logprob_rows_decode_unspeculated_beside_a_speculating_row(ref, spec):
    cfg, plain, _ = ref
    _, e = spec
    plain.set_sampling(0.0, 1.0, 0)
    plain.slots_reset()
    plain.set_eos([])
    want, want_lp, _ = _mixed_run(plain, cfg)
    _fresh(e, 3)
    got, got_lp, stats = _mixed_run(e, cfg)
    assert got == want
    for a, b in zip(got_lp, want_lp):
        assert a.tobytes() == b.tobytes()
    for b in range(3):
        assert stats[b]["drafted"] == 0 and stats[b]["accepted"] == 0 and stats[b]["steps"] == 39, (b, stats[b])
    assert stats[3]["steps"] + stats[3]["accepted"] == 39
    # host drafts on a row that does not speculate are ignored: the sampled row with its own true continuation planted
    _fresh(e, 3, max_n=0)
    e.set_row_sampling(0, SamplingParams(temperature=0.8, seed=1234))
    p0 = _prompt(cfg, 300, 12)
    e.slots_prefill([0], p0, [len(p0)], [10])
    e.set_row_drafts(0, want[0][1:4])
    e.slots_decode(1)
    _, lens = e.slots_poll()
    assert int(lens[0]) == 2 and e.spec_stats(0) == {"steps": 1, "drafted": 0, "accepted": 0}
    e.slot_release(0)


# ---------------------------------------------------------------------------------------------------- 7. guards

def _code(excinfo):
    return str(excinfo.value)


def test_guards(ref, spec):
    cfg, _, tokens = ref
    _, e = spec
    _fresh(e, 3, max_n=0)
    p = _prompt(cfg, 3, P_LEN)
    with pytest.raises(DotsEngineError) as ei:                        # slot 16 // 4 = 4 is the first one a speculating engine refuses
        e.slots_prefill([4], p, [len(p)], [8])
    assert "(-4)" in _code(ei) and "max_batch / (k + 1)" in _code(ei)
    assert e.kv_pool_info()[0] == e.kv_pool_info()[1]
    e.slots_prefill([3], p, [len(p)], [8])
    with pytest.raises(DotsEngineError) as ei:
        e.set_speculation(2)
    assert "(-3)" in _code(ei)
    with pytest.raises(DotsEngineError) as ei:
        e.set_speculation(0)
    assert "(-3)" in _code(ei)
    with pytest.raises(DotsEngineError) as ei:
        e.set_row_drafts(3, [1, 2, 3, 4])                             # n > k
    assert "(-1)" in _code(ei)
    with pytest.raises(DotsEngineError) as ei:
        e.set_row_drafts(3, [1, cfg.vocab_size])
    assert "(-1)" in _code(ei)
    with pytest.raises(DotsEngineError) as ei:
        e.set_row_drafts(2, [1])                                      # a free slot
    assert "(-3)" in _code(ei)
    e.slot_release(3)
    for bad in ((3, 0, 4), (3, 5, 4), (3, 2, 65)):
        with pytest.raises(DotsEngineError) as ei:
            e.set_speculation(*bad)
        assert "(-1)" in _code(ei)
    with pytest.raises(ValueError):
        e.set_speculation(16)
    assert e.spec_k == 3 and e.usable_slots == 4                      # the refused calls changed nothing


def test_speculation_switched_off_is_the_plain_engine(ref, spec):
    cfg, _, tokens = ref
    _, e = spec
    _fresh(e, 3)
    e.slots_reset()
    e.set_speculation(0)
    assert e.usable_slots == 16
    got = _plain_run(e, [_prompt(cfg, s, n) for s, n, _ in REQS], [cap for _, _, cap in REQS])
    assert got == [tokens(s, n, cap) for s, n, cap in REQS]
    assert e.spec_stats() == {"steps": 0, "drafted": 0, "accepted": 0}
    assert all(e.spec_stats(b) == {"steps": 0, "drafted": 0, "accepted": 0} for b in range(16))
    p = _prompt(cfg, 3, P_LEN)
    e.slots_prefill([15], p, [len(p)], [4])                           # every slot is usable again
    e.slot_release(15)
