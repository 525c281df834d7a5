"""Speculative decoding of sampled and stop-string rows on the GPU (Engine.set_speculation_rows).  Every comparison is
bitwise equality of token ids (and hit records) against the same model on an engine that never speculates: a sampled row's draft rows are
drawn by the row's own sampler with the counter of the output index they stand for, so for the same seed the speculating engine must
commit exactly the tokens of the sequential one, only in fewer steps.  No tolerance appears anywhere.

`ref` never speculates; its token lists are computed once per request and shared.  The accept path is driven deterministically through
Engine.set_row_drafts (planted drafts); the built-in drafter runs end to end through the ContinuousBatcher.  The token-byte table of the
stop-string tests is synthetic: token i has 1 to 4 bytes over {a, b, c}, a few ids have none."""
import numpy as np
import pytest

from dots_ocr_amd.config import DotsConfig
from dots_ocr_amd.engine import DotsEngineError, LogitRules, NgramRule, SamplingParams
from dots_ocr_amd.stop_strings import first_stop
from dots_ocr_amd.weights import random_state_dict

pytestmark = pytest.mark.gpu

SEQ = 640
V = 1024
K = 3
P_LEN = 61          # rows 0 .. 3 of the first speculating step sit at positions 61 .. 64: they straddle the 64-token page boundary
P_CAP = 24
NO_BYTES = (3, 77, 500, 1001, 1023)


def _token_table():
    g = np.random.default_rng(20)
    toks = [bytes(g.choice(list(b"abc"), int(g.integers(1, 5))).astype(np.uint8)) for _ in range(V)]
    for t in NO_BYTES:
        toks[t] = b""
    return toks


TOKS = _token_table()


def _engine(max_batch=16, kv_cache_dtype=None):
    from dots_ocr_amd.engine import Engine
    cfg = DotsConfig.tiny(layers=3, v_layers=3, vocab=V)
    e = Engine(cfg, max_batch=max_batch, max_seq_len=SEQ, max_patches=4096, max_prefill_tokens=2048, kv_cache_dtype=kv_cache_dtype)
    e.load_state_dict(random_state_dict(cfg, seed=11))
    e.set_token_bytes(TOKS)
    return cfg, e


def _prompt(seed, length):
    return np.random.default_rng(seed).integers(0, V - 8, length).astype(np.int32)


def _plain(e, eos=()):
    e.set_sampling(0.0, 1.0, 0)
    e.slots_reset()
    e.set_eos(list(eos))


def _fresh(e, k=K, sampled=False, stop=False, max_n=0, eos=()):
    e.set_sampling(0.0, 1.0, 0)
    e.slots_reset()
    e.set_speculation(k, 2, max_n)
    e.set_speculation_rows(sampled=sampled, stop=stop)
    e.set_eos(list(eos))


def _setup_row(e, slot, sp=None, stop=None):
    """the row's features, before its prefill.  stop: (strings, min_tokens)"""
    if sp is not None:
        e.set_row_sampling(slot, sp)
    if stop is not None:
        e.set_row_stop(slot, e.create_stop(list(stop[0])), stop[1])


def _finish(e, slots, chunk=16, limit=8):
    for _ in range(limit):
        fin, lens = e.slots_poll()
        if all(fin[s] == 1 for s in slots):
            break
        e.slots_decode(chunk)
    fin, lens = e.slots_poll()
    assert all(fin[s] == 1 for s in slots), (fin[:8], lens[:8])
    return fin, lens


def _seq_run(e, prompt, cap, sp=None, stop=None, eos=(), slot=0):
    """one request on an engine that does not speculate: dict(toks, hit)"""
    _plain(e, eos)
    _setup_row(e, slot, sp, stop)
    e.slots_prefill([slot], prompt, [len(prompt)], [cap])
    _, lens = _finish(e, [slot])
    out = dict(toks=e.slot_read(slot, int(lens[slot])).tolist(), hit=e.row_stop_hit(slot) if stop is not None else None)
    e.slot_release(slot)
    return out


@pytest.fixture(scope="module")
def ref():
    """the unspeculated engine and its token lists, keyed by the whole request"""
    cfg, e = _engine()
    cache = {}

    def tokens(seed, length, cap, sp=None, eos=()):
        key = (seed, length, cap, sp, tuple(eos))
        if key not in cache:
            cache[key] = _seq_run(e, _prompt(seed, length), cap, sp, eos=eos)["toks"]
        return list(cache[key])
    yield e, tokens
    e.close()


@pytest.fixture(scope="module")
def spec():
    _, e = _engine()
    yield e
    e.close()


def _planted_run(e, prompt, T, cap, make_drafts, slot=0, sp=None, stop=None):
    """One row driven step by step with host drafts; after every step out_lens must be what the host's walk of `T` predicts (T: the
    tokens of the sequential run, which ends at the cap, an EOS or a stop string).  -> (tokens, the row's counters, the host's)"""
    _setup_row(e, slot, sp, stop)
    e.slots_prefill([slot], prompt, [len(prompt)], [cap])
    end = len(T)
    L, steps, drafted, accepted = 1, 0, 0, 0
    while L < end:
        drafts = make_drafts(L)
        e.set_row_drafts(slot, drafts)
        e.slots_decode(1)
        # the host's walk: row 0 commits T[L]; while the row is not finished and draft `acc` is the token just committed, the next token
        # of T is committed too.  The cap cuts the drafts that are verified
        live = max(0, min(len(drafts), cap - L - 1))
        n, acc = L + 1, 0
        while acc < live and n < end and drafts[acc] == T[n - 1]:
            acc, n = acc + 1, n + 1
        steps, drafted, accepted = steps + 1, drafted + live, accepted + acc
        L = n
        fin, lens = e.slots_poll()
        assert int(lens[slot]) == L, (steps, int(lens[slot]), L)
        assert int(fin[slot]) == (1 if L >= end else 0)
    e.slots_decode(1)                                                 # a finished row commits nothing more
    fin, lens = e.slots_poll()
    assert int(lens[slot]) == end and int(fin[slot]) == 1
    toks = e.slot_read(slot, SEQ).tolist()
    st = e.spec_stats(slot)
    hit = e.row_stop_hit(slot) if stop is not None else None
    e.slot_release(slot)
    return toks, st, {"steps": steps, "drafted": drafted, "accepted": accepted}, hit


def _wrong(t):
    return (t + 1) % (V - 8)


def _drive(e, slots, truth, k=K, limit=400):
    """decode step by step; before every step each running row of `truth` gets its true continuation planted.  -> {slot: tokens}"""
    for _ in range(limit):
        fin, lens = e.slots_poll()
        if all(fin[s] == 1 for s in slots):
            break
        for s in slots:
            if fin[s] == 0 and truth.get(s) is not None:
                L = int(lens[s])
                e.set_row_drafts(s, truth[s][L:L + k])
        e.slots_decode(1)
    fin, lens = e.slots_poll()
    assert all(fin[s] == 1 for s in slots)
    return {s: e.slot_read(s, int(lens[s])).tolist() for s in slots}


# ---------------------------------------------------------------------------------------------------- 1. planted drafts, sampled

PARAMS = {
    "T0.1": SamplingParams(temperature=0.1, seed=9001),
    "T0.8": SamplingParams(temperature=0.8, seed=9002),
    "T0.8_k5": SamplingParams(temperature=0.8, top_k=5, seed=9003),
    "T1.0_p0.7": SamplingParams(temperature=1.0, top_p=0.7, seed=9004),
    "T0.9_k40_p0.8": SamplingParams(temperature=0.9, top_k=40, top_p=0.8, seed=9005),
    "T0_k3": SamplingParams(temperature=0.0, top_k=3, seed=9006),
}
P_SEED = 3


@pytest.mark.parametrize("case,per_step", [("true", 4), ("second_wrong", 2), ("all_wrong", 1)])
@pytest.mark.parametrize("name", sorted(PARAMS))
def test_planted_drafts_on_a_sampled_row(ref, spec, name, case, per_step):
    _, tokens = ref
    e = spec
    sp, cap = PARAMS[name], P_CAP
    T = tokens(P_SEED, P_LEN, cap, sp)
    assert len(T) == cap
    pad = T + [0] * 4

    def make(L):
        d = pad[L:L + K][:max(0, cap - L)]
        if case == "second_wrong" and len(d) > 1:
            d[1] = _wrong(d[1])
        if case == "all_wrong":
            d = [_wrong(t) for t in d]
        return d
    _fresh(e, sampled=True)
    toks, st, want, _ = _planted_run(e, _prompt(P_SEED, P_LEN), T, cap, make, sp=sp)
    assert toks == T
    assert st == want
    assert want["steps"] == -(-(cap - 1) // per_step) and want["drafted"] > 0
    if case == "true":
        assert want["accepted"] == cap - 1 - want["steps"] and want["drafted"] == want["accepted"]
    if case == "all_wrong":
        assert want["accepted"] == 0
    assert e.spec_stats() == want                                     # the engine's totals: this row is all that ran since set_speculation


def test_the_parameter_sets_differ(ref):
    """the six rows are six different runs: the test above is not one check repeated (a sampler that ignored its parameters would pass it)"""
    _, tokens = ref
    runs = {n: tuple(tokens(P_SEED, P_LEN, P_CAP, sp)) for n, sp in PARAMS.items()}
    assert len(set(runs.values())) >= 4, runs


# ---------------------------------------------------------------------------------------------------- 2. slot and batch invariance

NEIGHBOURS = [(41, 30, None), (42, 64, SamplingParams(temperature=0.1, seed=77)), (43, 17, SamplingParams(temperature=0.9, top_k=40, seed=78))]


@pytest.mark.parametrize("slot,beside", [(0, False), (3, False), (0, True), (3, True)])
def test_slot_and_batch_invariance(ref, spec, slot, beside):
    _, tokens = ref
    e = spec
    sp, cap = PARAMS["T0.9_k40_p0.8"], P_CAP
    T = tokens(P_SEED, P_LEN, cap, sp)
    _fresh(e, sampled=True, stop=True, max_n=4)
    rows = {slot: (P_SEED, P_LEN, sp)}
    if beside:
        for s, nb in zip([x for x in range(4) if x != slot], NEIGHBOURS):
            rows[s] = nb
    slots = sorted(rows)
    for s in slots:
        _setup_row(e, s, rows[s][2])
    prompts = [_prompt(rows[s][0], rows[s][1]) for s in slots]
    e.slots_prefill(slots, np.concatenate(prompts), [len(p) for p in prompts], [cap] * len(slots))
    truth = {s: tokens(rows[s][0], rows[s][1], cap, rows[s][2]) for s in slots}
    got = _drive(e, slots, truth)
    st = e.spec_stats(slot)
    for s in slots:
        e.slot_release(s)
    assert got[slot] == T
    assert got == truth
    assert st["accepted"] > 0 and st["steps"] + st["accepted"] == cap - 1


# ---------------------------------------------------------------------------------------------------- 3. EOS and the cap at draft index 1

def _fresh_at_draft_1(T):
    """the first position p = L + 2 of a step of the all-true run (L = 1, 5, 9, ...) whose token T[p] occurs nowhere before it, or None"""
    return next((q for q in range(3, len(T) - 3, 4) if T[q] not in T[:q]), None)


@pytest.fixture(scope="module")
def eos_case(ref):
    """a T = 0.8 request whose sequential run has a token that is new at draft index 1 of a step of the all-true run"""
    _, tokens = ref
    for seed in range(16):
        sp = SamplingParams(temperature=0.8, seed=500 + seed)
        T = tokens(P_SEED, P_LEN, P_CAP, sp)
        if _fresh_at_draft_1(T) is not None:
            return sp, T
    raise AssertionError("no sampler seed in [500, 516) gives a token that is new at draft index 1: a test error, widen the search")


def test_eos_at_draft_index_1_of_a_sampled_row(ref, spec, eos_case):
    _, tokens = ref
    e = spec
    sp, T = eos_case
    p = _fresh_at_draft_1(T)
    eos = [T[p]]
    Te = tokens(P_SEED, P_LEN, P_CAP, sp, eos)
    assert Te == T[:p + 1]                                            # the draw does not depend on the EOS ids: the sequential run stops there
    _fresh(e, sampled=True, eos=eos)
    total, free = e.kv_pool_info()
    assert free == total
    toks, st, want, _ = _planted_run(e, _prompt(P_SEED, P_LEN), Te, P_CAP, lambda L: (T + [0] * 4)[L:L + K], sp=sp)
    assert toks == Te and st == want
    assert want["steps"] == (p - 3) // 4 + 1 and want["accepted"] == p - want["steps"]
    assert e.kv_pool_info() == (total, total)


def test_cap_at_draft_index_1_of_a_sampled_row(ref, spec, eos_case):
    _, tokens = ref
    e = spec
    sp, long = eos_case
    cap = 8                                                           # the step at L = 5 may commit T[5], T[6], T[7]: draft index 2 is past the cap
    T = tokens(P_SEED, P_LEN, cap, sp)
    assert T == long[:cap]
    _fresh(e, sampled=True)
    total, _ = e.kv_pool_info()
    toks, st, want, _ = _planted_run(e, _prompt(P_SEED, P_LEN), T, cap, lambda L: long[L:L + K], sp=sp)
    assert toks == T and len(toks) == cap
    assert st == want and want == {"steps": 2, "drafted": 3 + 2, "accepted": 3 + 2}
    assert e.kv_pool_info() == (total, total)


# ---------------------------------------------------------------------------------------------------- 4. stop strings

S_CAP = 40


def _pick_stop(chunks, second):
    """A stop string from the row's own bytes whose match completes at token q = 3 (mod 4), q >= 7: draft index 1 of the step of the
    all-true run that starts at L = q - 2 and would otherwise accept 3.  second: the string also matches earlier, at q1 < q, and with
    min_tokens = q1 + 1 the match at q is the first that counts.  -> (strings, min_tokens, hit) or None"""
    data = b"".join(chunks)
    for q in range(7, len(chunks) - 2, 4):
        before = sum(len(c) for c in chunks[:q])
        for used in range(len(chunks[q]), 0, -1):
            end = before + used
            for m in range(2, min(end, 16) + 1):
                s = data[end - m:end].decode()
                h0 = first_stop(chunks, [s])
                if not second:
                    if h0 is not None and h0[0] == q:
                        return [s], 0, h0
                    continue
                if h0 is None or h0[0] >= q:
                    continue
                h1 = first_stop(chunks, [s], h0[0] + 1)
                if h1 is not None and h1[0] == q:
                    return [s], h0[0] + 1, h1
    return None


def _stop_case(tokens, sp, second):
    """(prompt seed, baseline tokens, strings, min_tokens, hit): the first prompt whose baseline offers the wanted stop string"""
    for seed in range(600, 640):
        T = tokens(seed, P_LEN, S_CAP, sp)
        picked = _pick_stop([TOKS[t] for t in T], second)
        if picked is not None:
            return (seed, T) + picked
    raise AssertionError("no prompt seed in [600, 640) offers the stop string the test wants: a test error, widen the search")


@pytest.mark.parametrize("second", [False, True], ids=["first_match", "min_tokens_second_match"])
@pytest.mark.parametrize("kind", ["greedy_mode_stop", "sampled_mode_all"])
def test_stop_string_completes_at_draft_index_1(ref, spec, kind, second):
    plain, tokens = ref
    e = spec
    sp = None if kind == "greedy_mode_stop" else SamplingParams(temperature=0.8, seed=4242)
    seed, T, strings, min_tokens, hit = _stop_case(tokens, sp, second)
    q = hit[0]
    assert q % 4 == 3 and 7 <= q < S_CAP - 2
    if second:
        assert min_tokens >= 1 and first_stop([TOKS[t] for t in T], strings)[0] == min_tokens - 1      # the first match is below min_tokens
    want = _seq_run(plain, _prompt(seed, P_LEN), S_CAP, sp, (strings, min_tokens))
    assert want["toks"] == T[:q + 1] and want["hit"] == hit          # the sequential engine agrees with the rule stated on the host
    _fresh(e, sampled=sp is not None, stop=True)
    toks, st, host, got_hit = _planted_run(e, _prompt(seed, P_LEN), want["toks"], S_CAP, lambda L: (T + [0] * 4)[L:L + K], sp=sp,
                                           stop=(strings, min_tokens))
    assert toks == want["toks"] and len(toks) == q + 1               # nothing committed past the hit
    assert got_hit == want["hit"]
    assert st == host
    # the last step verified three true drafts and accepted two: the match finished the row mid-walk
    assert host["steps"] == (q - 3) // 4 + 1 and host["accepted"] == q - host["steps"] and host["drafted"] == host["accepted"] + 1


# ---------------------------------------------------------------------------------------------------- 5. the built-in drafter, end to end

REQS = [(101, 7, 40, "greedy"), (102, 61, 33, "sampled"), (103, 30, 50, "stop"), (104, 64, 17, "sampled"), (105, 100, 64, "greedy"),
        (106, 15, 25, "stop")]


def _requests(tokens):
    from dots_ocr_amd.scheduler import Request
    reqs = []
    for i, (s, n, cap, kind) in enumerate(REQS):
        kw = {}
        if kind == "sampled":
            kw["sampling"] = SamplingParams(temperature=0.1, seed=3000 + i)
        if kind == "stop":                                            # bytes out of the middle of the row's own unstopped output
            chunks = [TOKS[t] for t in tokens(s, n, cap)]
            text = b"".join(chunks[10:14]).decode()
            assert 2 <= len(text) <= 16
            kw["stop"] = [text]
        reqs.append(Request(_prompt(s, n), max_new_tokens=cap, **kw))
    return reqs


def _batched(e, reqs, chunk):
    from dots_ocr_amd.scheduler import ContinuousBatcher
    cb = ContinuousBatcher(e, eos_ids=[], chunk=chunk)
    outs = cb.run(reqs)
    return [o.tolist() for o in outs], cb


@pytest.fixture(scope="module")
def e2e(ref):
    plain, tokens = ref
    reqs = _requests(tokens)
    _plain(plain)
    want, _ = _batched(plain, reqs, 16)
    stopped = [i for i, r in enumerate(REQS) if r[3] == "stop" and len(want[i]) < r[2]]
    assert stopped, "no stop request of the mix ends before its cap: a test error, choose other bytes"
    return reqs, want


@pytest.mark.parametrize("chunk", [1, 16])
def test_builtin_drafter_end_to_end(spec, e2e, chunk):
    e = spec
    reqs, want = e2e
    _fresh(e, sampled=True, stop=True, max_n=4)
    got, cb = _batched(e, reqs, chunk)
    assert cb.n_slots == 4
    assert got == want
    st = e.spec_stats()
    assert st["steps"] + st["accepted"] == sum(len(t) - 1 for t in want)      # every decode token is row 0 of a step or an accepted draft
    assert 0 <= st["accepted"] <= st["drafted"]
    total, free = e.kv_pool_info()
    assert free == total


def test_builtin_drafter_under_the_partition_plan(spec, e2e):
    e = spec
    reqs, want = e2e
    _fresh(e, sampled=True, stop=True, max_n=4)
    e.set_decode_plan(1)
    try:
        got, _ = _batched(e, reqs, 16)
    finally:
        e.set_decode_plan(0)
    assert got == want


def test_builtin_drafter_with_the_fp8_kv_cache(ref):
    _, tokens = ref
    _, plain = _engine(16, "fp8")
    _, e = _engine(16, "fp8")
    try:
        reqs = _requests(tokens)                                      # the stop bytes come from the bf16 run: any bytes do
        _plain(plain)
        want, _ = _batched(plain, reqs, 16)
        _fresh(e, sampled=True, stop=True, max_n=4)
        got, _ = _batched(e, reqs, 16)
        assert got == want
        st = e.spec_stats()
        assert st["steps"] + st["accepted"] == sum(len(t) - 1 for t in want)
    finally:
        plain.close()
        e.close()


# ---------------------------------------------------------------------------------------------------- 6. who still does not speculate

def _feature_run(e, kind, truth=None, cap=20):
    """one row of `kind` in slot 0 from its prefill to the cap; truth: its sequential tokens, planted before every step.  -> (tokens, counters)"""
    from dots_ocr_amd import guided as G
    if kind == "penalty":
        e.set_row_sampling(0, SamplingParams(temperature=0.8, repetition_penalty=1.1, seed=61))
    elif kind == "rules":
        e.set_row_logit_rules(0, LogitRules(bias={5: 2.0, 9: float("-inf")}, vocab_size=V))
    elif kind == "guide":
        e.set_row_guide(0, e.create_guide(G.compile_regex(r"[a-c]*")))
    elif kind == "ngram":
        e.set_row_ngram(0, NgramRule(2))
    elif kind == "logprobs":
        e.set_row_logprobs(0, 3)
    p = _prompt(70, 33)
    e.slots_prefill([0], p, [len(p)], [cap])
    toks = _drive(e, [0], {0: truth})[0]
    st = e.spec_stats(0)
    e.slot_release(0)
    return toks, st


@pytest.mark.parametrize("kind", ["penalty", "rules", "guide", "ngram", "logprobs"])
def test_rows_that_never_speculate_under_mode_all(ref, spec, kind):
    plain, _ = ref
    e = spec
    _plain(plain)
    want, _ = _feature_run(plain, kind)
    _fresh(e, sampled=True, stop=True, max_n=4)
    got, st = _feature_run(e, kind, truth=want)
    assert got == want
    assert st == {"steps": len(want) - 1, "drafted": 0, "accepted": 0}


def test_nobody_speculates_under_an_engine_wide_temperature(ref, spec):
    plain, _ = ref
    e = spec
    own = SamplingParams(temperature=0.5, seed=88)
    prompts = [_prompt(71, 20), _prompt(72, 40)]

    def run(eng, truth):
        eng.set_sampling(0.8, 1.0, 5)
        try:
            eng.set_row_sampling(1, own)
            eng.slots_prefill([0, 1], np.concatenate(prompts), [20, 40], [20, 20])
            toks = _drive(eng, [0, 1], truth)
            st = [eng.spec_stats(b) for b in (0, 1)]
            eng.slot_release(0)
            eng.slot_release(1)
        finally:
            eng.set_sampling(0.0, 1.0, 0)
        return toks, st
    _plain(plain)
    want, _ = run(plain, {})
    _fresh(e, sampled=True, stop=True, max_n=4)
    got, st = run(e, want)
    assert got == want
    assert all(s == {"steps": 19, "drafted": 0, "accepted": 0} for s in st), st


# ---------------------------------------------------------------------------------------------------- 7. mode 0 is today's engine

def test_without_the_setting_sampled_and_stop_rows_draft_nothing(ref):
    """a new engine, set_speculation(3) alone: the default of dots_set_speculation_rows"""
    _, tokens = ref
    _, e = _engine()
    try:
        e.set_sampling(0.0, 1.0, 0)
        e.slots_reset()
        e.set_speculation(K, 2, 0)
        e.set_eos([])
        sp = PARAMS["T0.8"]
        T0 = tokens(P_SEED, P_LEN, P_CAP, sp)
        T1 = tokens(P_SEED + 1, 30, P_CAP)
        strings = [b"".join(TOKS[t] for t in T1[P_CAP - 3:]).decode() + "abcabcabcabc"]      # held but never matched: the row runs to its cap
        assert first_stop([TOKS[t] for t in T1], strings) is None
        _setup_row(e, 0, sp)
        _setup_row(e, 1, None, (strings, 0))
        prompts = [_prompt(P_SEED, P_LEN), _prompt(P_SEED + 1, 30)]
        e.slots_prefill([0, 1, 2], np.concatenate(prompts + [prompts[1]]), [P_LEN, 30, 30], [P_CAP] * 3)
        got = _drive(e, [0, 1, 2], {0: T0, 1: T1, 2: T1})
        assert got == {0: T0, 1: T1, 2: T1}
        for b in (0, 1):
            assert e.spec_stats(b) == {"steps": P_CAP - 1, "drafted": 0, "accepted": 0}, b
        assert e.spec_stats(2)["accepted"] == P_CAP - 1 - e.spec_stats(2)["steps"] > 0      # the plain greedy row beside them speculates
    finally:
        e.close()


# ---------------------------------------------------------------------------------------------------- 8. fork

def test_fork_of_a_sampled_request(ref, spec):
    plain, _ = ref
    e = spec
    sps = [SamplingParams(temperature=0.8, top_k=20, seed=7000 + b) for b in range(3)]
    p = _prompt(P_SEED, P_LEN)

    def run(eng, truth):
        for b in range(3):
            eng.set_row_sampling(b, sps[b])
        eng.slots_prefill([0], p, [len(p)], [P_CAP])
        eng.slots_fork(0, [1, 2])
        toks = _drive(eng, [0, 1, 2], truth)
        st = [eng.spec_stats(b) for b in range(3)]
        for b in range(3):
            eng.slot_release(b)
        return toks, st
    _plain(plain)
    want, _ = run(plain, {})
    assert len({tuple(t) for t in want.values()}) == 3                # three seeds, three sequences
    _fresh(e, sampled=True)
    total, _ = e.kv_pool_info()
    got, st = run(e, want)
    assert got == want
    for b in range(3):
        assert st[b]["accepted"] > 0 and st[b]["steps"] + st[b]["accepted"] == P_CAP - 1, (b, st[b])
    assert e.kv_pool_info() == (total, total)


# ---------------------------------------------------------------------------------------------------- 9. guards

def test_guards(ref, spec):
    _, tokens = ref
    e = spec
    _fresh(e, sampled=False, stop=False)
    for bad in (4, 8, 7, -1):
        assert e.lib.dots_set_speculation_rows(e.h, bad) == -1        # DOTS_E_INVALID: unknown bits
    p = _prompt(P_SEED, P_LEN)
    e.slots_prefill([0], p, [len(p)], [8])
    assert e.lib.dots_set_speculation_rows(e.h, 1) == -3              # DOTS_E_STATE: a slot is occupied
    with pytest.raises(DotsEngineError) as ei:
        e.set_speculation_rows(sampled=True)
    assert "(-3)" in str(ei.value) and e.spec_rows == 0
    e.slot_release(0)
    # the setting survives speculation being switched off and on again
    e.set_speculation_rows(sampled=True)
    e.set_speculation(0)
    e.set_speculation(K, 2, 0)
    sp = PARAMS["T0.8_k5"]
    T = tokens(P_SEED, P_LEN, P_CAP, sp)
    _setup_row(e, 0, sp)
    e.slots_prefill([0], p, [len(p)], [P_CAP])
    got = _drive(e, [0], {0: T})
    st = e.spec_stats(0)
    e.slot_release(0)
    assert got[0] == T and st["accepted"] == P_CAP - 1 - st["steps"] > 0
    # and the refused calls left it alone; switching it off stops the row from drafting
    e.set_speculation_rows()
    _setup_row(e, 0, sp)
    e.slots_prefill([0], p, [len(p)], [P_CAP])
    got = _drive(e, [0], {0: T})
    st = e.spec_stats(0)
    e.slot_release(0)
    assert got[0] == T and st == {"steps": P_CAP - 1, "drafted": 0, "accepted": 0}
