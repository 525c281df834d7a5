"""Speculative decoding of rows that return logprobs on the GPU (Engine.set_speculation_logprobs).  A row's logprobs are a
function of its raw logits row alone and a draft row's logits are those of the sequential step at its position, so a speculating engine
must leave, at every output position, tok_lp, top_ids and top_lp IDENTICAL IN EVERY BIT to those of an engine that never speculates —
and the same tokens, only in fewer steps.  Every comparison is on raw bits (float32 viewed as uint32, so NaN padding compares too) over
the whole row_logprobs(row, cap) range, together with the token lists.  No tolerance appears anywhere.

The tiny model, the synthetic token bytes over {a, b, c} and the prompt length (61: the first speculating step straddles the 64-token page
boundary) are those of tests/test_spec_sampled_gpu.py.  `ref` never speculates; its runs are computed once per request and shared.  At
V = 1024 a logprob chunk holds 16 values, so top_n = 20 exercises chunk lists with empty entries; 5 and 0 are the other two cases."""
import dataclasses

import numpy as np
import pytest

from dots_ocr_amd import guided as G
from dots_ocr_amd.config import DotsConfig
from dots_ocr_amd.engine import DotsEngineError, LogitRules, NgramRule, SamplingParams
from dots_ocr_amd.stop_strings import first_stop
from dots_ocr_amd.weights import random_state_dict

pytestmark = pytest.mark.gpu

SEQ = 640
V = 1024
K = 3
P_LEN = 61
P_CAP = 24
P_SEED = 3
NO_BYTES = (3, 77, 500, 1001, 1023)
TWO = (210, 640)                             # a greedy row held to two ids repeats itself at once: the built-in drafter has something to find
FILL_BITS = 0xFFFFFFFF                       # a position nobody wrote: the 0xFF fill (a NaN as float32, -1 as int32)


def _nan(bits):
    """which float32 values, given as raw bits, are NaN (the padding a written entry carries behind its top_n, or the fill)"""
    return np.isnan(bits.view(np.float32))


def _token_table():
    g = np.random.default_rng(20)
    toks = [bytes(g.choice(list(b"abc"), int(g.integers(1, 5))).astype(np.uint8)) for _ in range(V)]
    for t in NO_BYTES:
        toks[t] = b""
    return toks


TOKS = _token_table()
GUIDE = G.compile_regex(r"((abc|cab)b?)*")


def _engine(max_batch=16, kv_cache_dtype=None):
    from dots_ocr_amd.engine import Engine
    cfg = DotsConfig.tiny(layers=3, v_layers=3, vocab=V)
    e = Engine(cfg, max_batch=max_batch, max_seq_len=SEQ, max_patches=4096, max_prefill_tokens=2048, kv_cache_dtype=kv_cache_dtype)
    e.load_state_dict(random_state_dict(cfg, seed=11))
    e.set_token_bytes(TOKS)
    e.test_guide = None
    return e


def _prompt(seed, length=P_LEN, vocab=V):
    return np.random.default_rng(seed).integers(0, vocab - 8, length).astype(np.int32)


@dataclasses.dataclass(frozen=True)
class Row:
    """the features of one request (hashable: the key of the reference cache)"""
    lp: int = None                           # top_n, None = logprobs off
    sp: SamplingParams = None
    rules: LogitRules = None
    ngram: NgramRule = None
    guide: bool = False
    stop: tuple = None                       # (strings, min_tokens)


def _setup_row(e, slot, row):
    if row.sp is not None:
        e.set_row_sampling(slot, row.sp)
    if row.rules is not None:
        e.set_row_logit_rules(slot, row.rules)
    if row.ngram is not None:
        e.set_row_ngram(slot, row.ngram)
    if row.guide:
        if e.test_guide is None:
            e.test_guide = e.create_guide(GUIDE)
        e.set_row_guide(slot, e.test_guide)
    if row.stop is not None:
        e.set_row_stop(slot, e.create_stop(list(row.stop[0])), row.stop[1])
    if row.lp is not None:
        e.set_row_logprobs(slot, row.lp)


def _plain(e, eos=()):
    e.set_sampling(0.0, 1.0, 0)
    e.slots_reset()
    e.set_eos(list(eos))


def _fresh(e, lp=True, k=K, sampled=False, stop=False, guided=False, shaped=None, max_n=0, eos=()):
    e.set_sampling(0.0, 1.0, 0)
    e.slots_reset()
    e.set_speculation(k, 2, max_n)
    e.set_speculation_rows(sampled=sampled, stop=stop)
    e.set_speculation_guided(guided)
    e.set_speculation_shaped(**(shaped or {}))
    e.set_speculation_logprobs(lp)
    e.set_eos(list(eos))


def _bits(lp):
    """(tok_lp, top_ids, top_lp) as Engine.row_logprobs returns them -> their raw bits"""
    tok, ids, top = lp
    return tok.view(np.uint32).copy(), ids.copy(), top.view(np.uint32).copy()


def _read_lp(e, slot, n):
    return _bits(e.row_logprobs(slot, n))


def _assert_lp(got, want, n, what=""):
    """the first n positions of `want` are exactly what `got` holds: n positions, every bit"""
    for g, w, name in zip(got, want, ("tok_lp", "top_ids", "top_lp")):
        assert g.shape[0] == n, (what, name, g.shape, n)
        same = g == w[:n]
        assert same.all(), (what, name, "first differing position", int(np.argwhere(~same.reshape(n, -1).all(axis=1))[0, 0]))


def _finish(e, slots, chunk=16, limit=8):
    for _ in range(limit):
        fin, lens = e.slots_poll()
        if all(fin[s] == 1 for s in slots):
            break
        e.slots_decode(chunk)
    fin, lens = e.slots_poll()
    assert all(fin[s] == 1 for s in slots), (fin[:8], lens[:8])
    return fin, lens


def _seq_run(e, prompt, cap, row, eos=(), slot=0):
    """one request on an engine that does not speculate: dict(toks, lp, hit)"""
    _plain(e, eos)
    _setup_row(e, slot, row)
    e.slots_prefill([slot], prompt, [len(prompt)], [cap])
    _, lens = _finish(e, [slot])
    out = dict(toks=e.slot_read(slot, int(lens[slot])).tolist(), lp=_read_lp(e, slot, cap), hit=e.row_stop_hit(slot) if row.stop is not None else None)
    e.slot_release(slot)
    return out


@pytest.fixture(scope="module")
def ref():
    """the unspeculated engine and its runs, keyed by the whole request; a run is computed once and never changed"""
    e = _engine()
    cache = {}

    def run(seed, row=Row(), cap=P_CAP, eos=(), length=P_LEN):
        key = (seed, length, cap, row, tuple(eos))
        if key not in cache:
            cache[key] = _seq_run(e, _prompt(seed, length), cap, row, eos=eos)
        return cache[key]
    yield e, run
    e.close()


@pytest.fixture(scope="module")
def spec():
    e = _engine()
    yield e
    e.close()


def _check_ref_lp(want, row):
    """the reference itself: every position carries a value, the top lists hold top_n entries and -1 / NaN behind them"""
    tok, ids, top = want["lp"]
    n = len(want["toks"])
    assert tok.shape == (n,) and ids.shape == top.shape == (n, 20)
    assert not _nan(tok).any() and not _nan(top[:, :row.lp]).any()
    assert (ids[:, :row.lp] >= 0).all() and (ids[:, row.lp:] == -1).all() and _nan(top[:, row.lp:]).all()


def _planted_run(e, prompt, want, cap, make_drafts, row, slot=0):
    """One row driven step by step with host drafts.  After every step out_lens must be what the host's walk of T (the tokens of the
    sequential run) predicts, and the logprob entries written so far must be the reference's: exactly out_lens positions, every bit.
    -> (tokens, logprob bits, the row's counters, the host's, the hit record)"""
    T = want["toks"]
    _setup_row(e, slot, row)
    e.slots_prefill([slot], prompt, [len(prompt)], [cap])
    end = len(T)
    L, steps, drafted, accepted = 1, 0, 0, 0
    if row.lp is not None:
        _assert_lp(_read_lp(e, slot, cap), want["lp"], 1, "after the prefill")
    while L < end:
        drafts = make_drafts(L)
        e.set_row_drafts(slot, drafts)
        e.slots_decode(1)
        live = max(0, min(len(drafts), cap - L - 1))
        n, acc = L + 1, 0
        while acc < live and n < end and drafts[acc] == T[n - 1]:
            acc, n = acc + 1, n + 1
        steps, drafted, accepted = steps + 1, drafted + live, accepted + acc
        L = n
        fin, lens = e.slots_poll()
        assert int(lens[slot]) == L, (steps, int(lens[slot]), L, e.slot_read(slot, int(lens[slot])).tolist(), T)
        assert int(fin[slot]) == (1 if L >= end else 0)
        if row.lp is not None:
            _assert_lp(_read_lp(e, slot, cap), want["lp"], L, f"after step {steps}")
    e.slots_decode(1)                                                 # a finished row commits nothing more, and writes nothing more
    fin, lens = e.slots_poll()
    assert int(lens[slot]) == end and int(fin[slot]) == 1
    toks = e.slot_read(slot, SEQ).tolist()
    lp = _read_lp(e, slot, cap)
    st = e.spec_stats(slot)
    hit = e.row_stop_hit(slot) if row.stop is not None else None
    e.slot_release(slot)
    return toks, lp, st, {"steps": steps, "drafted": drafted, "accepted": accepted}, hit


def _wrong(t):
    return (t + 1) % (V - 8)


PLANS = ["all_right", "first_wrong", "second_wrong"]


def _plan(T, cap, plan, k=K, wrong=_wrong):
    pad = T + [0] * (k + 1)

    def make(L):
        d = pad[L:L + k][:max(0, cap - L)]
        if plan == "first_wrong" and len(d) > 0:
            d[0] = wrong(d[0])
        if plan == "second_wrong" and len(d) > 1:
            d[1] = wrong(d[1])
        return d
    return make


def _check(e, run, seed, row, plan, cap=P_CAP, eos=(), **fresh):
    """the speculating engine against the reference for one request and one draft plan -> (reference run, host counters)"""
    want = run(seed, row, cap, eos)
    T = want["toks"]
    _check_ref_lp(want, row)
    _fresh(e, eos=eos, **fresh)
    toks, lp, st, host, hit = _planted_run(e, _prompt(seed), want, cap, _plan(T, cap, plan), row)
    assert toks == T
    _assert_lp(lp, want["lp"], len(T), "at the end")
    assert st == host and hit == want["hit"]
    if plan == "all_right" and len(T) > 2:
        assert st["accepted"] > 0
        assert st["steps"] == -(-(len(T) - 1) // (K + 1)) < len(T) - 1           # fewer steps than tokens
        assert st["accepted"] == len(T) - 1 - st["steps"]
    if plan == "first_wrong":
        assert st["accepted"] == 0 and st["steps"] == len(T) - 1 and st["drafted"] > 0
    if plan == "second_wrong":
        assert 0 < st["accepted"] < st["drafted"]
    return want, host


# ---------------------------------------------------------------------------------------------------- 1. planted drafts, step by step

@pytest.mark.parametrize("plan", PLANS)
@pytest.mark.parametrize("top_n", [20, 5, 0])
def test_planted_drafts_on_a_logprob_row(ref, spec, top_n, plan):
    _, run = ref
    want, host = _check(spec, run, P_SEED, Row(lp=top_n), plan)
    assert len(want["toks"]) == P_CAP
    assert want["toks"] == run(P_SEED, Row())["toks"]                  # logprobs move no token
    assert spec.spec_stats() == host                                  # the engine's totals: this row is all that ran since set_speculation


def test_the_top_lists_rank_the_raw_logits(ref):
    """the reference is the log-softmax of the logits: each list is sorted (value descending, index ascending), its first entry is the
    chosen token of a greedy row, and top_n = 5 is the head of top_n = 20 in every bit"""
    _, run = ref
    a, b = run(P_SEED, Row(lp=20)), run(P_SEED, Row(lp=5))
    tok, ids, top = a["lp"]
    vals = top.view(np.float32)
    assert (ids[:, 0] == np.asarray(a["toks"])).all() and (top[:, 0] == tok).all()
    assert (np.diff(vals, axis=1) <= 0).all() and (vals <= 0).all()
    ties = np.diff(vals, axis=1) == 0
    assert (np.diff(ids, axis=1)[ties] > 0).all()
    assert (b["lp"][0] == tok).all() and (b["lp"][1][:, :5] == ids[:, :5]).all() and (b["lp"][2][:, :5] == top[:, :5]).all()


# ---------------------------------------------------------------------------------------------------- 2. finishing mid-walk

def _aligned(T, cap, q):
    """right drafts, as many per step as keep a step starting at L = q - 2: that step verifies three right drafts, and T[q] stands at
    draft index 1 of it"""
    pad = T + [0] * (K + 1)

    def make(L):
        d = pad[L:L + K][:max(0, cap - L)]
        return d if L >= q - 2 else d[:max(0, min(K, q - 2 - L - 1))]
    return make


def _first_new(T):
    """the first position p >= 3 whose token occurs nowhere before it, or None"""
    return next((q for q in range(3, len(T) - 2) if T[q] not in T[:q]), None)


def test_eos_at_draft_index_1(ref, spec):
    _, run = ref
    row = Row(lp=5)
    seed = next((s for s in (P_SEED, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37, 41) if _first_new(run(s, row)["toks"]) is not None), None)
    assert seed is not None, "no prompt gives a token that is new at a position >= 3: a test error, widen the search"
    T = run(seed, row)["toks"]
    p = _first_new(T)
    eos = [T[p]]
    want = run(seed, row, P_CAP, eos)
    assert want["toks"] == T[:p + 1]                                  # the sequential run ends there, EOS included
    _check_ref_lp(want, row)                                          # and the EOS has its entry
    _fresh(spec, eos=eos)
    toks, lp, st, host, _ = _planted_run(spec, _prompt(seed), want, P_CAP, _aligned(T, P_CAP, p), row)
    assert toks == want["toks"] and st == host
    _assert_lp(lp, want["lp"], p + 1, "at the end")                   # the entries end exactly where the reference's end
    # the last step verified three right drafts and accepted two: the EOS finished the row mid-walk
    assert host["accepted"] >= 2 and host["drafted"] == host["accepted"] + 1


def test_the_cap_inside_the_drafts(ref, spec):
    _, run = ref
    row = Row(lp=20)
    long = run(P_SEED, row)["toks"]
    cap = 8                                                           # the step at L = 5 may commit T[5], T[6], T[7]: draft index 2 is past the cap
    want = run(P_SEED, row, cap)
    assert want["toks"] == long[:cap]
    _check_ref_lp(want, row)
    _fresh(spec)
    toks, lp, st, host, _ = _planted_run(spec, _prompt(P_SEED), want, cap, lambda L: long[L:L + K], row)
    assert toks == want["toks"] and len(toks) == cap
    _assert_lp(lp, want["lp"], cap, "at the end")
    assert st == host and host == {"steps": 2, "drafted": 3 + 2, "accepted": 3 + 2}


S_CAP = 40


def _pick_stop(chunks):
    """a stop string from the row's own bytes whose first match completes at a token q >= 3  -> (strings, hit) or None"""
    data = b"".join(chunks)
    for q in range(3, len(chunks) - 2):
        before = sum(len(c) for c in chunks[:q])
        for used in range(len(chunks[q]), 0, -1):
            end = before + used
            for m in range(2, min(end, 16) + 1):
                s = data[end - m:end].decode()
                h = first_stop(chunks, [s])
                if h is not None and h[0] == q:
                    return [s], h
    return None


def test_a_stop_string_completes_at_draft_index_1(ref, spec):
    _, run = ref
    row = Row(lp=5)
    picked = None
    for seed in range(600, 640):
        T = run(seed, row, S_CAP)["toks"]
        picked = _pick_stop([TOKS[t] for t in T])
        if picked is not None:
            break
    assert picked is not None, "no prompt seed in [600, 640) offers the stop string the test wants: a test error, widen the search"
    strings, hit = picked
    q = hit[0]
    srow = dataclasses.replace(row, stop=(tuple(strings), 0))
    want = run(seed, srow, S_CAP)
    assert want["toks"] == T[:q + 1] and want["hit"] == hit           # the sequential engine agrees with the rule stated on the host
    _check_ref_lp(want, srow)
    _fresh(spec, stop=True)
    toks, lp, st, host, got_hit = _planted_run(spec, _prompt(seed), want, S_CAP, _aligned(T, S_CAP, q), srow)
    assert toks == want["toks"] and len(toks) == q + 1 and got_hit == hit
    _assert_lp(lp, want["lp"], q + 1, "at the end")
    # the last step verified three right drafts and accepted two: the match finished the row mid-walk
    assert st == host and host["accepted"] >= 2 and host["drafted"] == host["accepted"] + 1


# ---------------------------------------------------------------------------------------------------- 3. a sampled row

def _off_list(want, n):
    """positions whose drawn token is not among the row's top-n entries"""
    ids = want["lp"][1]
    return [i for i, t in enumerate(want["toks"]) if t not in ids[i, :n].tolist()]


@pytest.mark.parametrize("plan", ["all_right", "second_wrong"])
def test_a_sampled_row(ref, spec, plan):
    _, run = ref
    rows = [Row(lp=5, sp=SamplingParams(temperature=0.8, top_k=40, seed=9003 + i)) for i in range(8)]
    # a draw off the top-5 list at a position the all-right run commits from a draft row (row 0 of its steps commits positions 1, 5, 9, ...)
    row = next((r for r in rows if any(i > 0 and i % 4 != 1 for i in _off_list(run(P_SEED, r), 5))), None)
    assert row is not None, "no sampler seed draws a token off the top-5 list at a draft row: a test error, widen the search"
    want, _ = _check(spec, run, P_SEED, row, plan, sampled=True)
    off = _off_list(want, 5)
    assert not _nan(want["lp"][0][off]).any()                         # a drawn token keeps its own value off the list
    assert want["toks"] != run(P_SEED, Row(lp=5))["toks"]             # and the row is not the greedy one


# ---------------------------------------------------------------------------------------------------- 4. shaped and guided rows

def _bites(run, row, seeds=(P_SEED, 5, 7, 11, 13, 17, 19, 23)):
    """the first prompt seed for which the feature moves the tokens off the plain greedy run, at a position where the raw arg max (the first
    entry of the top list) is therefore NOT the committed token: logprobs taken from the shaped values would show there"""
    for seed in seeds:
        want = run(seed, row)
        if want["toks"] != run(seed, Row(lp=row.lp))["toks"] and (want["lp"][1][:, 0] != np.asarray(want["toks"])).any():
            return seed
    raise AssertionError(f"{row} never bites for the seeds {seeds}: a test error, the case proves nothing")


def _raw_values(run, seed, row):
    """the logprobs of a shaped row are those of the raw logits: while its tokens are the plain greedy run's, so are its entries; and at
    the first position where they part the top lists are still equal (the context is the same), only the chosen token's value differs"""
    want, plain = run(seed, row), run(seed, Row(lp=row.lp))
    d = next(i for i, (a, b) in enumerate(zip(want["toks"], plain["toks"])) if a != b)
    for g, w in zip(want["lp"][1:], plain["lp"][1:]):
        assert (g[:d + 1] == w[:d + 1]).all()
    assert (want["lp"][0][:d] == plain["lp"][0][:d]).all() and want["lp"][0][d] != plain["lp"][0][d]


SHAPED = {
    "ngram": (Row(lp=5, ngram=NgramRule(2), rules=LogitRules(allowed=TWO, vocab_size=V)), dict(shaped=dict(ngram=True, rules=True))),
    "penalty": (Row(lp=5, sp=SamplingParams(temperature=0.0, repetition_penalty=1.5)), dict(sampled=True, shaped=dict(penalties=True))),
    "guide": (Row(lp=5, guide=True), dict(guided=True)),
}


@pytest.mark.parametrize("plan", ["all_right", "second_wrong"])
@pytest.mark.parametrize("kind", sorted(SHAPED))
def test_shaped_and_guided_rows(ref, spec, kind, plan):
    _, run = ref
    row, fresh = SHAPED[kind]
    seed = _bites(run, row)
    _raw_values(run, seed, row)
    want, _ = _check(spec, run, seed, row, plan, **fresh)
    assert len(want["toks"]) == P_CAP


# ---------------------------------------------------------------------------------------------------- 5. the built-in drafter, end to end

REQS = [(101, 7, 40, "two", 5), (102, 61, 33, "sampled", 20), (103, 30, 50, "two", None), (104, 64, 17, "plain", 0), (105, 100, 64, "two", 20),
        (106, 15, 25, "plain", None)]
E2E = dict(sampled=True, shaped=dict(rules=True), max_n=4)


def _requests():
    from dots_ocr_amd.scheduler import Request
    kinds = {
        "two": lambda i: dict(rules=LogitRules(allowed=TWO, vocab_size=V)),
        "sampled": lambda i: dict(sampling=SamplingParams(temperature=0.1, seed=3000 + i)),
        "plain": lambda i: dict(),
    }
    return [Request(_prompt(s, n), max_new_tokens=cap, logprobs=lp, **kinds[kind](i)) for i, (s, n, cap, kind, lp) in enumerate(REQS)]


def _batched(e, chunk):
    """-> (token lists, logprob bits of the requests that asked or None, the batcher)"""
    from dots_ocr_amd.scheduler import ContinuousBatcher
    cb = ContinuousBatcher(e, eos_ids=[], chunk=chunk)
    reqs = _requests()
    outs = cb.run(reqs)
    return [o.tolist() for o in outs], [None if r.logprobs is None else _bits(r.logprobs_out) for r in reqs], cb


def _same_batch(got, want):
    (g_toks, g_lp), (w_toks, w_lp) = got, want
    assert g_toks == w_toks
    for i, (g, w) in enumerate(zip(g_lp, w_lp)):
        assert (g is None) == (w is None) == (REQS[i][4] is None)
        if g is not None:
            _assert_lp(g, w, len(w_toks[i]), f"request {i}")
            assert not _nan(w[0]).any() and (w[1][:, :REQS[i][4]] >= 0).all() and (w[1][:, REQS[i][4]:] == -1).all()


@pytest.fixture(scope="module")
def e2e(ref):
    plain, _ = ref
    _plain(plain)
    toks, lp, _ = _batched(plain, 16)
    assert [len(t) for t in toks] == [r[2] for r in REQS]
    return toks, lp


@pytest.mark.parametrize("chunk", [1, 16])
def test_builtin_drafter_end_to_end(spec, e2e, chunk):
    e = spec
    _fresh(e, **E2E)
    toks, lp, cb = _batched(e, chunk)
    assert cb.n_slots == 4
    _same_batch((toks, lp), e2e)
    st = e.spec_stats()
    assert st["steps"] + st["accepted"] == sum(len(t) - 1 for t in toks)      # every decode token is row 0 of a step or an accepted draft
    assert 0 < st["accepted"] <= st["drafted"]
    total, free = e.kv_pool_info()
    assert free == total


def test_builtin_drafter_with_the_fp8_kv_cache():
    plain, e = _engine(16, "fp8"), _engine(16, "fp8")
    try:
        _plain(plain)
        w_toks, w_lp, _ = _batched(plain, 16)
        _fresh(e, **E2E)
        toks, lp, _ = _batched(e, 16)
        _same_batch((toks, lp), (w_toks, w_lp))
        st = e.spec_stats()
        assert 0 < st["accepted"] <= st["drafted"]
    finally:
        plain.close()
        e.close()


def test_logprobs_switched_on_mid_run(ref, spec):
    """the row starts with logprobs off, speculates, and is switched on between two steps: its class does not move, the positions before
    stay NaN / -1 and the ones after are the reference's — an unspeculated row switched on at the same output length"""
    plain, run = ref
    e = spec
    T = run(P_SEED)["toks"]
    p = _prompt(P_SEED)
    _fresh(e, max_n=4)
    e.slots_prefill([0], p, [len(p)], [P_CAP])
    for _ in range(2):
        L = int(e.slots_poll()[1][0])
        e.set_row_drafts(0, T[L:L + K])
        e.slots_decode(1)
    L0 = int(e.slots_poll()[1][0])
    assert L0 == 1 + 2 * (K + 1)
    e.set_row_logprobs(0, 5)
    while int(e.slots_poll()[0][0]) == 0:
        L = int(e.slots_poll()[1][0])
        e.set_row_drafts(0, T[L:L + K])
        e.slots_decode(1)
    assert e.slot_read(0, SEQ).tolist() == T
    got, st = _read_lp(e, 0, P_CAP), e.spec_stats(0)
    e.slot_release(0)
    assert st["steps"] == -(-(P_CAP - 1) // (K + 1)) and st["accepted"] == P_CAP - 1 - st["steps"]      # it went on speculating

    _plain(plain)
    plain.slots_prefill([0], p, [len(p)], [P_CAP])
    plain.slots_decode(L0 - 1)
    assert int(plain.slots_poll()[1][0]) == L0
    plain.set_row_logprobs(0, 5)
    _finish(plain, [0])
    want = _read_lp(plain, 0, P_CAP)
    plain.slot_release(0)
    _assert_lp(got, want, P_CAP, "switched on mid-run")
    assert (want[0][:L0] == FILL_BITS).all() and (want[1][:L0] == -1).all() and (want[2][:L0] == FILL_BITS).all()
    assert not _nan(want[0][L0:]).any() and (want[1][L0:, :5] >= 0).all()


# ---------------------------------------------------------------------------------------------------- 6. off means off

def _driven(e, run, seed, row, cap=P_CAP):
    """one row with its true continuation planted before every step -> (tokens, logprob bits, counters)"""
    T = run(seed, row, cap)["toks"]
    _setup_row(e, 0, row)
    p = _prompt(seed)
    e.slots_prefill([0], p, [len(p)], [cap])
    for _ in range(4 * cap):
        fin, lens = e.slots_poll()
        if fin[0] == 1:
            break
        L = int(lens[0])
        e.set_row_drafts(0, T[L:L + K])
        e.slots_decode(1)
    toks, lp, st = e.slot_read(0, SEQ).tolist(), _read_lp(e, 0, cap), e.spec_stats(0)
    e.slot_release(0)
    return toks, lp, st


def test_with_the_switch_off_a_logprob_row_drafts_nothing(ref, spec):
    _, run = ref
    row = Row(lp=5)
    want = run(P_SEED, row)
    _fresh(spec, lp=False)
    assert spec.spec_logprobs is False
    toks, lp, st = _driven(spec, run, P_SEED, row)
    assert toks == want["toks"]
    _assert_lp(lp, want["lp"], P_CAP)
    assert st == {"steps": P_CAP - 1, "drafted": 0, "accepted": 0}


def test_a_new_engine_has_the_switch_off(ref):
    """set_speculation alone: the default of dots_set_speculation_logprobs"""
    _, run = ref
    e = _engine()
    try:
        e.set_sampling(0.0, 1.0, 0)
        e.slots_reset()
        e.set_speculation(K, 2, 0)
        e.set_eos([])
        toks, lp, st = _driven(e, run, P_SEED, Row(lp=0))
        assert toks == run(P_SEED, Row(lp=0))["toks"] and st == {"steps": P_CAP - 1, "drafted": 0, "accepted": 0}
        _assert_lp(lp, run(P_SEED, Row(lp=0))["lp"], P_CAP)
    finally:
        e.close()


def test_the_switch_is_refused_while_a_slot_is_occupied_and_survives_set_speculation(ref, spec):
    _, run = ref
    e = spec
    row = Row(lp=20)
    want = run(P_SEED, row)
    _fresh(e, lp=False)
    p = _prompt(P_SEED)
    e.slots_prefill([0], p, [len(p)], [8])
    assert e.lib.dots_set_speculation_logprobs(e.h, 1) == -3          # DOTS_E_STATE: a slot is occupied
    with pytest.raises(DotsEngineError) as ei:
        e.set_speculation_logprobs(True)
    assert "(-3)" in str(ei.value) and e.spec_logprobs is False
    e.slot_release(0)
    toks, lp, st = _driven(e, run, P_SEED, row)                       # the refused calls left it off
    assert toks == want["toks"] and st == {"steps": P_CAP - 1, "drafted": 0, "accepted": 0}
    # the setting survives speculation being switched off and on again
    e.set_speculation_logprobs(True)
    e.set_speculation(0)
    e.set_speculation(K, 2, 0)
    assert e.spec_logprobs is True
    toks, lp, st = _driven(e, run, P_SEED, row)
    assert toks == want["toks"] and st["accepted"] == P_CAP - 1 - st["steps"] > 0
    _assert_lp(lp, want["lp"], P_CAP)
    e.set_speculation_logprobs(False)
    toks, lp, st = _driven(e, run, P_SEED, row)
    assert toks == want["toks"] and st == {"steps": P_CAP - 1, "drafted": 0, "accepted": 0}
    _assert_lp(lp, want["lp"], P_CAP)


def test_the_switch_without_a_logprob_row_changes_nothing_for_plain_rows(ref, spec):
    _, run = ref
    e = spec
    seeds = (P_SEED, 5)
    truth = [run(s)["toks"] for s in seeds]

    def go(lp):
        _fresh(e, lp=lp)
        prompts = [_prompt(s) for s in seeds]
        e.slots_prefill([0, 1], np.concatenate(prompts), [P_LEN, P_LEN], [P_CAP, P_CAP])
        for _ in range(4 * P_CAP):
            fin, lens = e.slots_poll()
            if fin[0] == 1 and fin[1] == 1:
                break
            for b in (0, 1):
                d = truth[b][int(lens[b]):int(lens[b]) + K]
                if b == 1 and len(d) > 1:
                    d[1] = _wrong(d[1])                               # row 1 accepts one draft per step, row 0 all of them
                if fin[b] == 0:
                    e.set_row_drafts(b, d)
            e.slots_decode(1)
        out = [e.slot_read(b, SEQ).tolist() for b in (0, 1)], [e.spec_stats(b) for b in (0, 1)], e.spec_stats()
        e.slot_release(0)
        e.slot_release(1)
        return out
    off, on = go(False), go(True)
    assert on == off and off[0] == truth
    assert off[1][0]["accepted"] > off[1][1]["accepted"] > 0


# ---------------------------------------------------------------------------------------------------- 7. the real vocabulary

def test_the_real_vocabulary():
    """V = 151936: a chunk holds 2376 values and the last one is ragged (151936 - 63 * 2376 = 2248); one slot, top_n = 20, a dozen tokens,
    all drafts right — the draft-row kernels take the float4 path and the tail"""
    from dots_ocr_amd.engine import Engine
    BIG, cap = 151936, 12
    cfg = DotsConfig.tiny(layers=3, v_layers=3, vocab=BIG)
    sd = random_state_dict(cfg, seed=11)
    p = _prompt(P_SEED, P_LEN, BIG)
    engines = []
    try:
        for _ in range(2):
            e = Engine(cfg, max_batch=4, max_seq_len=256, max_patches=4096, max_prefill_tokens=2048)
            engines.append(e)
            e.load_state_dict(sd)
            e.set_sampling(0.0, 1.0, 0)
            e.slots_reset()
            e.set_eos([])
        plain, e = engines
        plain.set_row_logprobs(0, 20)
        plain.slots_prefill([0], p, [len(p)], [cap])
        _finish(plain, [0])
        T, want = plain.slot_read(0, cap).tolist(), _read_lp(plain, 0, cap)
        plain.slot_release(0)
        assert len(T) == cap and not _nan(want[0]).any() and (want[1] >= 0).all() and (want[1] < BIG).all()
        assert (want[1][:, 0] == np.asarray(T)).all()

        e.set_speculation(K, 2, 0)
        e.set_speculation_logprobs(True)
        e.set_row_logprobs(0, 20)
        e.slots_prefill([0], p, [len(p)], [cap])
        steps = 0
        while int(e.slots_poll()[0][0]) == 0:
            L = int(e.slots_poll()[1][0])
            e.set_row_drafts(0, T[L:L + K][:max(0, cap - L)])
            e.slots_decode(1)
            steps += 1
            _assert_lp(_read_lp(e, 0, cap), want, int(e.slots_poll()[1][0]), f"after step {steps}")
        assert e.slot_read(0, cap).tolist() == T
        _assert_lp(_read_lp(e, 0, cap), want, cap, "at the end")
        st = e.spec_stats(0)
        e.slot_release(0)
        assert st["steps"] == steps == 3 and st["accepted"] == cap - 1 - steps
    finally:
        for e in engines:
            e.close()
