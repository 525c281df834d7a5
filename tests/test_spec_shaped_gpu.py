"""Speculative decoding of rows whose logits are shaped — an n-gram rule, logit rules, penalties — on the GPU (DESIGN §6.6,
Engine.set_speculation_shaped).  Every comparison is bitwise equality of token ids (and stop hits, guide states, counters) against the same
model on an engine that never speculates: draft row j is selected under the hypothesis that drafts 1 .. j were committed, and under it the
history the n-gram rule reads, the output counts and the output index are those the sequential engine holds there, so the speculating
engine must commit exactly the tokens of the sequential one, only in fewer steps.  No tolerance appears anywhere.

The tiny model, the synthetic token bytes over {a, b, c} and the prompt length (61: the first speculating step straddles the 64-token page
boundary) are those of tests/test_spec_sampled_gpu.py.  `ref` never speculates; its runs are computed once per request and shared.  The
accept path is driven through Engine.set_row_drafts (planted drafts); the built-in drafter runs end to end through the ContinuousBatcher.

A case in which the feature never bites proves nothing, so every case states that the unspeculated run WITH the feature differs from the
unspeculated run WITHOUT it (_bites).  Where a pigeonhole argument forces that (a greedy row held to two ids must repeat a bigram), one
prompt is used; elsewhere the first prompt seed of a short list for which it holds."""
import dataclasses

import numpy as np
import pytest

from dots_ocr_amd import guided as G
from dots_ocr_amd.config import DotsConfig
from dots_ocr_amd.engine import DotsEngineError, LogitRules, NgramRule, SamplingParams, banned_ngram_ids
from dots_ocr_amd.weights import random_state_dict

pytestmark = pytest.mark.gpu

SEQ = 640
V = 1024
K = 3
P_LEN = 61
P_CAP = 24
P_SEED = 3
NO_BYTES = (3, 77, 500, 1001, 1023)
EOS = 1020
TWO = (210, 640)                             # a greedy row held to two ids repeats a bigram within 6 tokens and a trigram within 11
THREE = (210, 640, 901)


def _token_table():
    g = np.random.default_rng(20)
    toks = [bytes(g.choice(list(b"abc"), int(g.integers(1, 5))).astype(np.uint8)) for _ in range(V)]
    for t in NO_BYTES:
        toks[t] = b""
    return toks


TOKS = _token_table()
GUIDE = G.compile_regex(r"((abc|cab)b?)*")      # tight: a few tokens per state, so a guided run differs from the unguided one at once


def _engine(max_batch=16, kv_cache_dtype=None):
    from dots_ocr_amd.engine import Engine
    cfg = DotsConfig.tiny(layers=3, v_layers=3, vocab=V)
    e = Engine(cfg, max_batch=max_batch, max_seq_len=SEQ, max_patches=4096, max_prefill_tokens=2048, kv_cache_dtype=kv_cache_dtype)
    e.load_state_dict(random_state_dict(cfg, seed=11))
    e.set_token_bytes(TOKS)
    e.test_guide = None
    return e


def _prompt(seed, length=P_LEN):
    return np.random.default_rng(seed).integers(0, V - 8, length).astype(np.int32)


@dataclasses.dataclass(frozen=True)
class Row:
    """the features of one request (hashable: the key of the reference cache)"""
    sp: SamplingParams = None
    rules: LogitRules = None
    ngram: NgramRule = None
    guide: bool = False
    stop: tuple = None                       # (strings, min_tokens)
    lp: int = None

    def without(self, *names):
        return dataclasses.replace(self, **{n: (False if n == "guide" else None) for n in names})


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


ALL = dict(ngram=True, rules=True, penalties=True)


def _fresh(e, k=K, shaped=ALL, sampled=True, stop=True, guided=True, max_n=0, eos=()):
    e.set_sampling(0.0, 1.0, 0)
    e.slots_reset()
    e.set_speculation(k, 2, max_n)
    e.set_speculation_rows(sampled=sampled, stop=stop)
    e.set_speculation_guided(guided)
    e.set_speculation_shaped(**(shaped or {}))
    e.set_eos(list(eos))


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
    """one request on an engine that does not speculate: dict(toks, hit, state)"""
    _plain(e, eos)
    _setup_row(e, slot, row)
    e.slots_prefill([slot], prompt, [len(prompt)], [cap])
    _, lens = _finish(e, [slot])
    out = dict(toks=e.slot_read(slot, int(lens[slot])).tolist(), hit=e.row_stop_hit(slot) if row.stop is not None else None,
               state=e.row_guide_state(slot) if row.guide else None)
    e.slot_release(slot)
    return out


@pytest.fixture(scope="module")
def ref():
    """the unspeculated engine and its runs, keyed by the whole request"""
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


def _bites(run, row, feature, cap=P_CAP, eos=(), seeds=(P_SEED, 5, 7, 11, 13, 17, 19, 23)):
    """the first prompt seed for which the unspeculated run with `feature` (names of Row fields) differs from the run without it"""
    for seed in seeds:
        if run(seed, row, cap, eos)["toks"] != run(seed, row.without(*feature), cap, eos)["toks"]:
            return seed
    raise AssertionError(f"{feature} never bites for the seeds {seeds}: a test error, the case proves nothing")


def _planted_run(e, prompt, T, cap, make_drafts, row, slot=0):
    """One row driven step by step with host drafts; after every step out_lens must be what the host's walk of `T` predicts (T: the
    tokens of the sequential run, which ends at the cap, an EOS / stop id or a stop string).  -> (tokens, the row's counters, the
    host's, the hit record, the guide state)"""
    _setup_row(e, slot, row)
    e.slots_prefill([slot], prompt, [len(prompt)], [cap])
    end = len(T)
    L, steps, drafted, accepted = 1, 0, 0, 0
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
    e.slots_decode(1)                                                 # a finished row commits nothing more
    fin, lens = e.slots_poll()
    assert int(lens[slot]) == end and int(fin[slot]) == 1
    toks = e.slot_read(slot, SEQ).tolist()
    st = e.spec_stats(slot)
    hit = e.row_stop_hit(slot) if row.stop is not None else None
    state = e.row_guide_state(slot) if row.guide else None
    e.slot_release(slot)
    return toks, st, {"steps": steps, "drafted": drafted, "accepted": accepted}, hit, state


def _true(T, cap):
    pad = T + [0] * 4
    return lambda L: pad[L:L + K][:max(0, cap - L)]


def _wrong(t):
    return (t + 1) % (V - 8)


def _cases(T, cap, case):
    pad = T + [0] * 4

    def make(L):
        d = pad[L:L + K][:max(0, cap - L)]
        if case == "half" and len(d) > 1:
            d[1] = _wrong(d[1])
        if case == "none":
            d = [_wrong(t) for t in d]
        return d
    return make


def _check(e, run, seed, row, case, cap=P_CAP, eos=(), make=None, shaped=ALL):
    """the speculating engine against the reference for one request and one way of planting drafts; -> (T, host counters)"""
    want = run(seed, row, cap, eos)
    T = want["toks"]
    _fresh(e, shaped=shaped, eos=eos)
    toks, st, host, hit, state = _planted_run(e, _prompt(seed), T, cap, make or _cases(T, cap, case), row)
    assert toks == T
    assert st == host
    assert hit == want["hit"] and state == want["state"]
    if case == "full" and len(T) > 2:
        assert host["steps"] == -(-(len(T) - 1) // (K + 1)) < len(T) - 1 and host["accepted"] == len(T) - 1 - host["steps"] > 0
    if case == "none":
        assert host["accepted"] == 0 and host["steps"] == len(T) - 1
    return T, host


CASES = ["full", "half", "none"]


# ---------------------------------------------------------------------------------------------------- 1. n-gram rows

def _ngram_row(n, window, allowed=TWO, whitelist=()):
    return Row(rules=LogitRules(allowed=allowed, vocab_size=V), ngram=NgramRule(n, window, whitelist))


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("n,window", [(2, 0), (2, 5), (3, 0), (3, 5)])
def test_ngram_row_held_to_two_ids(ref, spec, n, window, case):
    """the row may only pick two ids, so without the rule it repeats itself at once; with it the run is forced off its greedy path, and —
    n = 2 — into steps in which both ids are banned and the all -inf fallback id 0 is committed"""
    _, run = ref
    row = _ngram_row(n, window)
    seed = _bites(run, row, ["ngram"])
    T, _ = _check(spec, run, seed, row, case)
    assert len(T) == P_CAP
    for L in range(1, len(T)):                                        # the reference obeys the rule as the host states it
        banned = banned_ngram_ids(T[:L], n, window)
        if set(TWO) <= banned:
            assert T[L] == 0                                          # every allowed id banned: the all -inf fallback
        else:
            assert T[L] in TWO and T[L] not in banned
    if n == 2 and window == 0:
        # four bigrams over two ids, six with the fallback's: a run of 23 transitions that repeats none must fall back, also from draft rows
        assert 0 in T and 0 not in TWO
    U = run(seed, row.without("ngram"))["toks"]
    assert set(U) <= set(TWO)


def test_ngram_row_alone_and_with_a_whitelist(ref, spec):
    """the n-gram rule with nothing beside it (the RULES bit is not needed), and a whitelisted id that the rule would ban"""
    _, run = ref
    row = Row(ngram=NgramRule(1))                                     # n = 1: no id twice, which a greedy row of this model wants somewhere
    seed = _bites(run, row, ["ngram"], cap=40)
    T, host = _check(spec, run, seed, row, "full", cap=40, shaped=dict(ngram=True))
    assert len(set(T)) == len(T)
    white = _ngram_row(2, 0, THREE, whitelist=(THREE[0],))
    seed = _bites(run, white, ["ngram"])
    T = run(seed, white)["toks"]
    # nine bigrams over three ids and 23 transitions: some bigram repeats, and only one that ends in the whitelisted id can
    assert any(T[i] in banned_ngram_ids(T[:i], 2) and T[i] == THREE[0] for i in range(1, len(T)))
    assert T != run(seed, _ngram_row(2, 0, THREE))["toks"]
    for case in CASES:
        _check(spec, run, seed, white, case)


@pytest.mark.parametrize("at", [0, 1])
def test_a_planted_draft_that_is_the_banned_id(ref, spec, at):
    """draft index `at` of every step is an id the rule bans at its position (when there is one), true drafts around it: the row that
    would have to select it cannot, so it is rejected with everything behind it"""
    _, run = ref
    row = _ngram_row(2, 0, THREE)
    seed = _bites(run, row, ["ngram"])
    T = run(seed, row)["toks"]
    pad = T + [0] * 4
    planted = []

    def make(L):
        d = pad[L:L + K][:max(0, P_CAP - L)]
        if len(d) > at:
            banned = sorted(banned_ngram_ids(T[:L + at], 2) & set(THREE))
            if banned:
                d[at] = banned[0]
                assert d[at] != T[L + at]
                planted.append(L)
        return d
    _, host = _check(spec, run, seed, row, "planted", make=make)
    assert len(planted) >= 3 and host["drafted"] > host["accepted"]


# ---------------------------------------------------------------------------------------------------- 2. ruled rows

@pytest.mark.parametrize("case", CASES)
def test_bias_and_allowed_ids(ref, spec, case):
    _, run = ref
    ids = (5, 9, 210, 333, 640, 777, 901, 1000)
    row = Row(rules=LogitRules(bias={5: 2.0, 9: float("-inf"), 333: -1.5, 12: 4.0}, allowed=ids, vocab_size=V))
    seed = _bites(run, row, ["rules"])
    T, _ = _check(spec, run, seed, row, case, shaped=dict(rules=True))
    assert set(T) <= set(ids) - {9} and len(T) == P_CAP
    biased = Row(rules=LogitRules(bias={t: 1000.0 for t in THREE}, vocab_size=V))      # a bias alone, no allowed list
    seed = _bites(run, biased, ["rules"])
    T, _ = _check(spec, run, seed, biased, case, shaped=dict(rules=True))
    assert set(T) <= set(THREE)


@pytest.mark.parametrize("m", [3, 4, 6])
def test_min_tokens_is_crossed_inside_a_step(ref, spec, m):
    """the EOS carries a bias that makes it the arg max everywhere, so the run is m tokens and then the EOS: draft row j of the step at
    out_lens = L is below min_tokens iff L + j < m, and the step that holds index m selects the EOS from a draft row (m = 3: j = 2 of the
    first step; m = 4: j = 3; m = 6: j = 1 of the second)"""
    _, run = ref
    row = Row(rules=LogitRules(bias={EOS: 1000.0}, min_tokens=m, vocab_size=V, eos_ids=(EOS,)))
    seed = _bites(run, row, ["rules"], eos=[EOS])
    assert run(seed, Row(rules=LogitRules(bias={EOS: 1000.0}, vocab_size=V)), eos=[EOS])["toks"] == [EOS]      # without min_tokens: at once
    T, host = _check(spec, run, seed, row, "full", eos=[EOS], shaped=dict(rules=True))
    assert len(T) == m + 1 and T[-1] == EOS and EOS not in T[:-1]
    assert (m - 1) % (K + 1) != 0                                     # index m is not row 0 of a step
    for case in ("half", "none"):
        _check(spec, run, seed, row, case, eos=[EOS], shaped=dict(rules=True))


def _first_emitted_on_a_draft_row(run, lo, seeds=(P_SEED, 5, 7, 11, 13, 17, 19, 23)):
    """(seed, U, at): the plain greedy run U of a prompt seed and an index at >= lo, not row 0 of a step of the all-true walk, at which U
    emits an id for the first time"""
    for seed in seeds:
        U = run(seed)["toks"]
        for at in range(lo, len(U) - 4):
            if (at - 1) % (K + 1) != 0 and U[at] not in U[:at]:
                return seed, U, at
    raise AssertionError("no plain run emits a fresh id on a draft row: a test error, widen the search")


@pytest.mark.parametrize("lo", [2, 6])
def test_a_stop_id_as_a_draft(ref, spec, lo):
    """the row's own stop id is planted as a draft with the unruled run's continuation behind it: the walk commits it, finishes the row
    there and commits nothing of what follows"""
    _, run = ref
    seed, U, at = _first_emitted_on_a_draft_row(run, lo)
    row = Row(rules=LogitRules(stop=[U[at]], vocab_size=V))
    T = run(seed, row)["toks"]
    assert T == U[:at + 1] and T != U
    pad = U + [0] * 4
    _, host = _check(spec, run, seed, row, "stop", make=lambda L: pad[L:L + K], shaped=dict(rules=True))
    assert host["accepted"] == at - host["steps"] > 0 and host["drafted"] > host["accepted"]


def test_ignore_eos(ref, spec):
    """an EOS id of the engine that the run emits: without ignore_eos the run ends there, with it the id is committed from a draft row and
    the walk goes on behind it"""
    _, run = ref
    seed, U, at = _first_emitted_on_a_draft_row(run, 2)
    E = U[at]
    row = Row(rules=LogitRules(ignore_eos=True, vocab_size=V))
    assert run(seed, Row(), eos=[E])["toks"] == U[:at + 1]
    T, host = _check(spec, run, seed, row, "full", eos=[E], shaped=dict(rules=True))
    assert T == U and E in T
    # the same engine EOS still finishes a plain row, from the same draft row
    _check(spec, run, seed, Row(), "eos", eos=[E], make=lambda L: (U + [0] * 4)[L:L + K])


# ---------------------------------------------------------------------------------------------------- 3. penalised rows

PEN = dict(repetition_penalty=1.3, frequency_penalty=0.5, presence_penalty=0.4)
PEN_PARAMS = {
    "greedy": SamplingParams(temperature=0.0, **PEN),
    "T0.8": SamplingParams(temperature=0.8, seed=9102, **PEN),
    "T0.9_k40_p0.8": SamplingParams(temperature=0.9, top_k=40, top_p=0.8, seed=9105, **PEN),
}


def _unpenalised(sp):
    return dataclasses.replace(sp, repetition_penalty=1.0, frequency_penalty=0.0, presence_penalty=0.0)


def _pen_bites(run, row, seeds=(P_SEED, 5, 7, 11, 13, 17, 19, 23)):
    for seed in seeds:
        if run(seed, row)["toks"] != run(seed, dataclasses.replace(row, sp=_unpenalised(row.sp)))["toks"]:
            return seed
    raise AssertionError("the penalties never bite: a test error, the case proves nothing")


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("name", sorted(PEN_PARAMS))
def test_penalised_row(ref, spec, name, case):
    _, run = ref
    row = Row(sp=PEN_PARAMS[name])
    seed = _pen_bites(run, row)
    T, _ = _check(spec, run, seed, row, case, shaped=dict(penalties=True))
    assert len(T) == P_CAP


@pytest.mark.parametrize("name", ["greedy", "T0.8"])
def test_drafts_t_t_t_the_adjusted_count_decides(ref, spec, name):
    """the row is held to two ids and penalised by count, and every step's drafts are [t, t, t] with t the token row 0 is about to commit:
    draft 1 is always accepted, and the token behind it is selected with count(t) + 1 — with the count of the head of the step it would
    be selected as if t had not just been emitted.  The second draft is accepted wherever the run really repeats t"""
    _, run = ref
    row = Row(sp=PEN_PARAMS[name], rules=LogitRules(allowed=TWO, vocab_size=V))
    seed = _pen_bites(run, row)
    T = run(seed, row)["toks"]
    assert set(T) <= set(TWO) and len(set(T)) == 2
    _, host = _check(spec, run, seed, row, "ttt", make=lambda L: [T[L]] * min(K, max(0, P_CAP - L)))
    repeats = sum(T[i] == T[i - 1] for i in range(2, len(T)))
    assert host["accepted"] >= host["steps"] - 1 and repeats < len(T) - 2          # the run alternates somewhere: [t, t, t] is not its truth


@pytest.mark.parametrize("name", ["greedy", "T0.8"])
def test_rejected_drafts_leak_no_counts(ref, spec, name):
    """twelve tokens of steps whose three drafts are all the other allowed id — attractive, rejected — then true drafts to the cap: a count
    that a rejected draft row left behind would move the penalised values of every later token"""
    _, run = ref
    row = Row(sp=PEN_PARAMS[name], rules=LogitRules(allowed=TWO, vocab_size=V))
    seed = _pen_bites(run, row)
    cap = 40
    T = run(seed, row, cap)["toks"]
    assert len(T) == cap
    pad = T + [0] * 4

    def make(L):
        if L < 12:
            other = TWO[0] if T[L] == TWO[1] else TWO[1]
            return [other] * K
        return pad[L:L + K][:max(0, cap - L)]
    _, host = _check(spec, run, seed, row, "leak", cap=cap, make=make)
    assert host["steps"] >= 11 + (cap - 12) // (K + 1) and host["accepted"] > 0


# ---------------------------------------------------------------------------------------------------- 4. everything on one row, batches

def _guide_walks(T):
    """every token of T moved the automaton: no all -inf fallback in the run (a draft of the fallback id verifies nothing past it, which the
    host's walk of _planted_run does not model; tests/test_spec_guided_gpu.py covers that case)"""
    state = GUIDE.start
    for t in T:
        state = GUIDE.walk(state, TOKS[t]) if TOKS[t] else G.DEAD
        if state == G.DEAD:
            return False
    return True


def _combined(run, seeds=(P_SEED, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37, 41)):
    """n-gram, guide, sampled, penalty and a stop string taken from the row's own bytes, for the first prompt seed at which every one of
    them bites.  -> (seed, Row)"""
    for ngram in (NgramRule(2), NgramRule(1)):                        # the bigram rule where it bites, else "no id twice"
        base = Row(sp=SamplingParams(temperature=0.5, top_k=8, seed=9201, **PEN), ngram=ngram, guide=True)
        for seed in seeds:
            T = run(seed, base, 40)["toks"]
            text = b"".join(TOKS[t] for t in T[20:23])
            if not text:
                continue
            row = dataclasses.replace(base, stop=((text.decode(),), 4))
            want = run(seed, row, 40)
            if want["hit"] is None or len(want["toks"]) >= 40 or not _guide_walks(want["toks"]):
                continue
            if any(want["toks"] == run(seed, row.without(f), 40)["toks"] for f in ("ngram", "guide", "stop")):
                continue
            if want["toks"] == run(seed, dataclasses.replace(row, sp=_unpenalised(row.sp)), 40)["toks"]:
                continue
            return seed, row
    raise AssertionError("no prompt seed at which the n-gram rule, the guide, the stop string and the penalties all bite: a test error")


@pytest.mark.parametrize("case", CASES)
def test_every_feature_on_one_row(ref, spec, case):
    _, run = ref
    seed, row = _combined(run)
    want = run(seed, row, 40)
    assert want["hit"][0] >= 4 and len(want["toks"]) == want["hit"][0] + 1 < 40      # the stop string ends it, not below min_tokens
    _check(spec, run, seed, row, case, cap=40)


def _batch_rows(run):
    ng = _ngram_row(2, 0, THREE)
    pen = Row(sp=PEN_PARAMS["T0.8"], rules=LogitRules(allowed=THREE, vocab_size=V))
    return {0: (_bites(run, ng, ["ngram"]), ng), 1: (41, Row()), 2: (_pen_bites(run, pen), pen), 3: (43, Row(ngram=NgramRule(2), lp=3))}


def _drive(e, slots, truth, k=K, limit=400, chunk=1):
    """decode; before every call each running row of `truth` gets its true continuation planted.  -> {slot: tokens}"""
    for _ in range(limit):
        fin, lens = e.slots_poll()
        if all(fin[s] == 1 for s in slots):
            break
        for s in slots:
            if fin[s] == 0 and truth.get(s) is not None:
                L = int(lens[s])
                e.set_row_drafts(s, truth[s][L:L + k])
        e.slots_decode(chunk)
    fin, lens = e.slots_poll()
    assert all(fin[s] == 1 for s in slots)
    return {s: e.slot_read(s, int(lens[s])).tolist() for s in slots}


@pytest.mark.parametrize("order", [(0, 1, 2, 3), (3, 1, 0, 2)])
def test_shaped_rows_beside_plain_rows_and_a_logprob_row(ref, spec, order):
    """the four slots of a k = 3 step — an n-gram row, a plain row, a penalised sampled row, a logprob row —: a row index b * (k + 1) + j instead of j * rows + b, or a ban / count row of another slot, shows here"""
    _, run = ref
    e = spec
    rows = dict(zip(order, _batch_rows(run).values()))
    slots = sorted(rows)
    truth = {s: run(rows[s][0], rows[s][1])["toks"] for s in slots}
    _fresh(e)
    for s in slots:
        _setup_row(e, s, rows[s][1])
    prompts = [_prompt(rows[s][0]) for s in slots]
    e.slots_prefill(slots, np.concatenate(prompts), [P_LEN] * len(slots), [P_CAP] * len(slots))
    got = _drive(e, slots, truth)
    st = {s: e.spec_stats(s) for s in slots}
    for s in slots:
        e.slot_release(s)
    assert got == truth
    for s in slots:
        if rows[s][1].lp is not None:                                 # a logprob row never speculates
            assert st[s] == {"steps": P_CAP - 1, "drafted": 0, "accepted": 0}
        else:
            assert st[s]["accepted"] > 0 and st[s]["steps"] + st[s]["accepted"] == P_CAP - 1, (s, st[s])


# ---------------------------------------------------------------------------------------------------- 5. the switch

def _switch_rows(run):
    ng = _ngram_row(2, 0, THREE)
    ru = Row(rules=LogitRules(bias={t: 1000.0 for t in THREE}, vocab_size=V))
    pe = Row(sp=PEN_PARAMS["greedy"])
    return {"ngram": (_bites(run, ng, ["ngram"]), ng, dict(ngram=True, rules=True)), "rules": (_bites(run, ru, ["rules"]), ru, dict(rules=True)),
            "penalties": (_pen_bites(run, pe), pe, dict(penalties=True))}


def _driven(e, run, seed, row):
    T = run(seed, row)["toks"]
    _setup_row(e, 0, row)
    e.slots_prefill([0], _prompt(seed), [P_LEN], [P_CAP])
    got = _drive(e, [0], {0: T})[0]
    st = e.spec_stats(0)
    e.slot_release(0)
    assert got == T
    return T, st


@pytest.mark.parametrize("kind", ["ngram", "rules", "penalties"])
def test_full_acceptance_takes_fewer_steps_than_tokens(ref, spec, kind):
    _, run = ref
    e = spec
    assert callable(getattr(e, "set_speculation_shaped", None))
    seed, row, shaped = _switch_rows(run)[kind]
    _fresh(e, shaped=shaped)
    T, st = _driven(e, run, seed, row)
    assert st["steps"] == -(-(len(T) - 1) // (K + 1)) < len(T) - 1 and st["accepted"] == len(T) - 1 - st["steps"]
    # with the switch at 0 — and with every bit but the row's own — the row drafts nothing
    others = {k: True for k in ALL if k not in shaped}
    for off in ({}, others):
        _fresh(e, shaped=off)
        T, st = _driven(e, run, seed, row)
        assert st == {"steps": len(T) - 1, "drafted": 0, "accepted": 0}, (off, st)


def test_a_logprob_row_never_speculates(ref, spec):
    _, run = ref
    e = spec
    for row in (Row(lp=0), Row(ngram=NgramRule(2), lp=5), Row(sp=PEN_PARAMS["T0.8"], lp=1), Row(rules=LogitRules(allowed=THREE, vocab_size=V), lp=20)):
        _fresh(e, max_n=4)
        T, st = _driven(e, run, P_SEED, row)
        assert st == {"steps": len(T) - 1, "drafted": 0, "accepted": 0}, row


def test_guards(ref, spec):
    _, run = ref
    e = spec
    seed, row, shaped = _switch_rows(run)["ngram"]
    _fresh(e, shaped={})
    assert e.spec_shaped == 0
    for bad in (8, 15, -1, 64):
        assert e.lib.dots_set_speculation_shaped(e.h, bad) == -1      # DOTS_E_INVALID: an unknown bit
    for bad in (4, 8, 16, 32, 63):
        assert e.lib.dots_set_speculation_rows(e.h, bad) == -1        # no bit of the rows setting
    e.slots_prefill([0], _prompt(seed), [P_LEN], [8])
    assert e.lib.dots_set_speculation_shaped(e.h, 1) == -3            # DOTS_E_STATE: a slot is occupied
    with pytest.raises(DotsEngineError) as ei:
        e.set_speculation_shaped(ngram=True)
    assert "(-3)" in str(ei.value) and e.spec_shaped == 0
    e.slot_release(0)
    T, st = _driven(e, run, seed, row)                                # the refused calls left it off
    assert st == {"steps": len(T) - 1, "drafted": 0, "accepted": 0}
    # the setting survives speculation being switched off and on again, and leaves the other two settings alone
    e.set_speculation_shaped(**shaped)
    e.set_speculation(0)
    e.set_speculation(K, 2, 0)
    assert e.spec_shaped == 3 and e.spec_rows == 3 and e.spec_guided is True
    T, st = _driven(e, run, seed, row)
    assert st["accepted"] == len(T) - 1 - st["steps"] > 0
    e.set_speculation_shaped()
    T, st = _driven(e, run, seed, row)
    assert st == {"steps": len(T) - 1, "drafted": 0, "accepted": 0}


# ---------------------------------------------------------------------------------------------------- 6. the built-in drafter, end to end

REQS = [(101, 7, 40, "ngram"), (102, 61, 33, "pen"), (103, 30, 50, "rules"), (104, 64, 17, "plain"), (105, 100, 64, "all"), (106, 15, 25, "ngram_only"),
        (107, 20, 30, "lp")]


def _requests(e):
    from dots_ocr_amd.scheduler import Request
    if e.test_guide is None:
        e.test_guide = e.create_guide(GUIDE)
    kinds = {
        "ngram": dict(ngram=NgramRule(3, 0), rules=LogitRules(allowed=THREE, vocab_size=V)),
        "pen": dict(sampling=SamplingParams(temperature=0.1, seed=3001, **PEN), rules=LogitRules(allowed=tuple(range(200, 216)), vocab_size=V)),
        "rules": dict(rules=LogitRules(bias={EOS: 1000.0, 210: 3.0}, min_tokens=21, allowed=THREE + (EOS,), vocab_size=V)),
        "plain": dict(),
        "all": dict(sampling=SamplingParams(temperature=0.1, top_k=8, seed=3005, **PEN), ngram=NgramRule(4, 16, (640,)), guide=e.test_guide,
                    rules=LogitRules(bias={640: 1.0, 210: -1.0}, vocab_size=V), stop=["cabcabcabcab"]),
        "ngram_only": dict(ngram=NgramRule(1)),
        "lp": dict(ngram=NgramRule(2), logprobs=2),
    }
    return [Request(_prompt(s, n), max_new_tokens=cap, **kinds[kind]) for s, n, cap, kind in REQS]


def _batched(e, chunk):
    from dots_ocr_amd.scheduler import ContinuousBatcher
    cb = ContinuousBatcher(e, eos_ids=[EOS], chunk=chunk)
    outs = cb.run(_requests(e))
    return [o.tolist() for o in outs], cb


@pytest.fixture(scope="module")
def e2e(ref):
    plain, _ = ref
    _plain(plain)
    want, _ = _batched(plain, 16)
    assert want[2][-1] == EOS and len(want[2]) == 22 and set(want[0]) <= set(THREE) | {0}      # min_tokens = 21 held the EOS back
    return want


@pytest.mark.parametrize("chunk", [1, 16])
def test_builtin_drafter_end_to_end(spec, e2e, chunk):
    e = spec
    _fresh(e, max_n=4)
    got, cb = _batched(e, chunk)
    assert cb.n_slots == 4
    assert got == e2e
    st = e.spec_stats()
    assert 0 < st["accepted"] <= st["drafted"]
    total, free = e.kv_pool_info()
    assert free == total


def test_builtin_drafter_with_the_fp8_kv_cache():
    plain, e = _engine(16, "fp8"), _engine(16, "fp8")
    try:
        _plain(plain)
        want, _ = _batched(plain, 16)
        _fresh(e, max_n=4)
        got, _ = _batched(e, 16)
        assert got == want
        st = e.spec_stats()
        assert 0 < st["accepted"] <= st["drafted"]
    finally:
        plain.close()
        e.close()
