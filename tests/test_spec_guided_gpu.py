"""Speculative decoding of guided rows on the GPU (Engine.set_speculation_guided).  Every comparison is bitwise equality of
token ids (and automaton states, hit records, counters) against the same model on an engine that never speculates: draft row j of a guided
slot is selected under the slot's state walked over the bytes of drafts 1 .. j, which is the state the sequential engine holds there if
those drafts are accepted, so the speculating engine must commit exactly the tokens of the sequential one, only in fewer steps.  No
tolerance appears anywhere.

The tiny model, the synthetic token bytes over {a, b, c} and the prompt length (61: the first speculating step straddles the 64-token page
boundary) are those of tests/test_spec_sampled_gpu.py.  `ref` never speculates; its runs are computed once per request and shared.  The
accept path is driven through Engine.set_row_drafts (planted drafts); the built-in drafter runs end to end through the ContinuousBatcher.
The host's statement of the state chain is Guide.draft_states (tests/test_spec_guided_cpu.py checks it by hand)."""
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
EOS = 1020                                   # an id with bytes like any other: as an EOS id a guide allows it iff its state is accepting


def _token_table():
    g = np.random.default_rng(20)
    toks = [bytes(g.choice(list(b"abc"), int(g.integers(1, 5))).astype(np.uint8)) for _ in range(V)]
    for t in NO_BYTES:
        toks[t] = b""
    return toks


TOKS = _token_table()
TB = G.TokenBytes(TOKS)

GUIDES = {
    "any": G.compile_regex(r"[a-c]*"),                               # unbounded, every state accepting
    "struct": G.compile_regex(r"((abc|cab)b?)*"),
    # 16 to 18 bytes in tokens of 1 to 4: 4 to 18 tokens and the EOS, so a run always ends inside the cap of 24
    "choice": G.compile_choice(["abcabcabccabcababc", "cabcabbabccabcaba", "bcabcabcabcaabcc"]),
    "abc3": G.compile_regex(r"(abc){3}"), "abc4": G.compile_regex(r"(abc){4}"), "cab3": G.compile_regex(r"(cab){3}"),
    "abc5": G.compile_regex(r"(abc){5}"), "cab4": G.compile_regex(r"(cab){4}"),
}


def _engine(max_batch=16, kv_cache_dtype=None):
    from dots_ocr_amd.engine import Engine
    cfg = DotsConfig.tiny(layers=3, v_layers=3, vocab=V)
    e = Engine(cfg, max_batch=max_batch, max_seq_len=SEQ, max_patches=4096, max_prefill_tokens=2048, kv_cache_dtype=kv_cache_dtype)
    e.load_state_dict(random_state_dict(cfg, seed=11))
    e.set_token_bytes(TOKS)
    e.test_guides = {}
    return e


def _handle(e, name):
    if name not in e.test_guides:
        e.test_guides[name] = e.create_guide(GUIDES[name])
    return e.test_guides[name]


def _prompt(seed, length):
    return np.random.default_rng(seed).integers(0, V - 8, length).astype(np.int32)


def _plain(e, eos=()):
    e.set_sampling(0.0, 1.0, 0)
    e.slots_reset()
    e.set_eos(list(eos))


def _fresh(e, k=K, guided=True, sampled=False, stop=False, max_n=0, eos=()):
    e.set_sampling(0.0, 1.0, 0)
    e.slots_reset()
    e.set_speculation(k, 2, max_n)
    e.set_speculation_rows(sampled=sampled, stop=stop)
    e.set_speculation_guided(guided)
    e.set_eos(list(eos))


def _setup_row(e, slot, guide=None, sp=None, stop=None):
    """the row's features, before its prefill.  guide: a name of GUIDES; stop: (strings, min_tokens)"""
    if guide is not None:
        e.set_row_guide(slot, _handle(e, guide))
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


def _seq_run(e, prompt, cap, guide=None, sp=None, stop=None, eos=(), slot=0):
    """one request on an engine that does not speculate: dict(toks, hit)"""
    _plain(e, eos)
    _setup_row(e, slot, guide, sp, stop)
    e.slots_prefill([slot], prompt, [len(prompt)], [cap])
    _, lens = _finish(e, [slot])
    out = dict(toks=e.slot_read(slot, int(lens[slot])).tolist(), hit=e.row_stop_hit(slot) if stop is not None else None)
    e.slot_release(slot)
    return out


def _state_after(g, toks, eos=()):
    """the row's automaton after it committed `toks`, as commit_token advances it: an EOS id moves nothing (and finishes the row), a token
    the guide did not allow (the all -inf fallback) moves nothing.  -> (state, tokens that did not move it)"""
    s, stuck = g.start, 0
    for t in toks:
        if t in eos:
            break
        n = g.walk(s, TOKS[t]) if TOKS[t] else G.DEAD
        if n == G.DEAD:
            stuck += 1
        else:
            s = n
    return s, stuck


def _text(toks, eos=()):
    return b"".join(TOKS[t] for t in toks if t not in eos)


@pytest.fixture(scope="module")
def ref():
    """the unspeculated engine and its token lists, keyed by the whole request"""
    e = _engine()
    cache = {}

    def tokens(seed, length, cap, guide=None, sp=None, eos=()):
        key = (seed, length, cap, guide, sp, tuple(eos))
        if key not in cache:
            cache[key] = _seq_run(e, _prompt(seed, length), cap, guide, sp, eos=eos)["toks"]
        return list(cache[key])
    yield e, tokens
    e.close()


@pytest.fixture(scope="module")
def spec():
    e = _engine()
    yield e
    e.close()


def _planted_run(e, prompt, T, cap, make_drafts, guide, slot=0, sp=None, stop=None, eos=()):
    """One guided row driven step by step with host drafts.  After every step out_lens must be what the host's walk of `T` predicts (T:
    the tokens of the sequential run) and the row's automaton must be where Guide.walk puts it after the tokens committed so far.
    -> (tokens, the row's counters, the host's, the hit record)"""
    g = GUIDES[guide]
    _setup_row(e, slot, guide, sp, stop)
    e.slots_prefill([slot], prompt, [len(prompt)], [cap])
    end = len(T)
    L, steps, drafted, accepted = 1, 0, 0, 0
    assert e.row_guide_state(slot) == _state_after(g, T[:1], eos)[0]
    while L < end:
        drafts = make_drafts(L)
        e.set_row_drafts(slot, drafts)
        e.slots_decode(1)
        # the host's walk: row 0 commits T[L]; while the row is not finished, draft `acc` is the token just committed and the chain did not
        # mark its row dead, the next token of T is committed too.  The cap cuts the drafts that are verified
        live = max(0, min(len(drafts), cap - L - 1))
        chain = g.draft_states(_state_after(g, T[:L], eos)[0], drafts, TB, eos)
        n, acc = L + 1, 0
        while acc < live and n < end and drafts[acc] == T[n - 1] and chain[acc] >= 0:
            acc, n = acc + 1, n + 1
        steps, drafted, accepted = steps + 1, drafted + live, accepted + acc
        L = n
        fin, lens = e.slots_poll()
        assert int(lens[slot]) == L, (steps, int(lens[slot]), L)
        assert int(fin[slot]) == (1 if L >= end else 0)
        assert e.row_guide_state(slot) == _state_after(g, T[:L], eos)[0], (steps, L)
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


def _true(T, cap):
    pad = T + [0] * 4
    return lambda L: pad[L:L + K][:max(0, cap - L)]


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


# ---------------------------------------------------------------------------------------------------- 1. planted drafts, greedy guided row

@pytest.mark.parametrize("case,per_step", [("true", 4), ("second_wrong", 2), ("all_wrong", 1)])
@pytest.mark.parametrize("guide", ["any", "struct", "choice"])
def test_planted_drafts_on_a_greedy_guided_row(ref, spec, guide, case, per_step):
    _, tokens = ref
    e = spec
    g, cap = GUIDES[guide], P_CAP
    eos = [EOS] if guide == "choice" else []                         # the finite language ends by its EOS; the others run to the cap
    T = tokens(P_SEED, P_LEN, cap, guide, eos=eos)
    assert 5 <= len(T) <= cap and _state_after(g, T, eos)[1] == 0    # every token moved the automaton: no fallback in this run
    if guide == "choice":
        assert T[-1] == EOS and g.matches(_text(T, eos))
    else:
        assert len(T) == cap and g.walk(g.start, _text(T)) != G.DEAD
    # the same request without the guide leaves the language: the guide is doing something.  ([a-c]* holds every token that has bytes: no
    # run of this vocabulary's byte-carrying tokens can violate it, so there is nothing to show for it)
    if guide != "any":
        U = tokens(P_SEED, P_LEN, cap, eos=eos)
        assert U != T and g.walk(g.start, _text(U, eos)) == G.DEAD
    pad = T + [0] * 4

    def make(L):
        d = pad[L:L + K][:max(0, cap - L)]
        if case == "second_wrong" and len(d) > 1:
            d[1] = _wrong(d[1])
        if case == "all_wrong":
            d = [_wrong(t) for t in d]
        return d
    _fresh(e, eos=eos)
    toks, st, want, _ = _planted_run(e, _prompt(P_SEED, P_LEN), T, cap, make, guide, eos=eos)
    assert toks == T
    assert st == want
    assert want["steps"] == -(-(len(T) - 1) // per_step) and want["drafted"] > 0
    if case == "true":
        assert want["accepted"] == len(T) - 1 - want["steps"] > 0
    if case == "all_wrong":
        assert want["accepted"] == 0
    assert e.spec_stats() == want                                     # the engine's totals: this row is all that ran since set_speculation


# ---------------------------------------------------------------------------------------------------- 2. drafts the guide forbids

def _forbidden(g, state):
    """a token with bytes that the automaton forbids at `state`"""
    m = g.mask(state, TB)
    return next(t for t in range(V - 8) if TOKS[t] and not m[t])


@pytest.mark.parametrize("index", [1, 2])
@pytest.mark.parametrize("kind", ["forbidden", "no_bytes", "eos"])
def test_a_draft_the_guide_forbids(ref, spec, kind, index):
    """the bad draft stands at draft index `index` of every step, true drafts around it: it is rejected, and so is everything behind it"""
    _, tokens = ref
    e = spec
    guide, cap, eos = "struct", P_CAP, [EOS]
    g = GUIDES[guide]
    T = tokens(P_SEED, P_LEN, cap, guide, eos=eos)
    assert len(T) == cap and EOS not in T
    pad = T + [0] * 4

    def make(L):
        d = pad[L:L + K][:max(0, cap - L)]
        if len(d) >= index:
            at = _state_after(g, T[:L + index - 1], eos)[0]            # the state the bad draft would be committed at
            d[index - 1] = {"forbidden": _forbidden(g, at), "no_bytes": NO_BYTES[1], "eos": EOS}[kind]
            assert d[index - 1] != T[L + index - 1] and g.draft_states(_state_after(g, T[:L], eos)[0], d, TB, eos)[index - 1:] == [-1] * (len(d) - index + 1)
        return d
    _fresh(e, eos=eos)
    toks, st, want, _ = _planted_run(e, _prompt(P_SEED, P_LEN), T, cap, make, guide, eos=eos)
    assert toks == T and st == want
    assert want["steps"] == -(-(cap - 1) // index)                   # every step: row 0 and the index - 1 true drafts before the bad one
    assert want["accepted"] == cap - 1 - want["steps"] and want["drafted"] > want["accepted"]


def test_the_fallback_token_verifies_nothing_past_it(ref, spec):
    """§6.3's all -inf fallback: a finite language without an EOS id leaves nothing to select once it is matched; the row commits id 0 and
    its state does not move.  A draft of id 0 then equals the committed token without being a token of the guide: its row is dead"""
    _, tokens = ref
    e = spec
    guide, cap = "abc3", 16
    g = GUIDES[guide]
    T = tokens(P_SEED, P_LEN, cap, guide)
    state, stuck = _state_after(g, T)
    assert len(T) == cap and stuck >= 4 and T[-stuck:] == [0] * stuck and g.accepting[state] and TOKS[0]
    _fresh(e)
    toks, st, want, _ = _planted_run(e, _prompt(P_SEED, P_LEN), T, cap, _true(T, cap), guide)
    assert toks == T and st == want
    assert want["accepted"] == len(T) - stuck - 1 - (want["steps"] - stuck)      # once the language is matched every step commits one token


# ---------------------------------------------------------------------------------------------------- 3. forced EOS in mid-walk, the cap

def test_forced_eos_is_committed_from_a_draft_row(ref, spec):
    """at the final state of a finite language everything but the EOS is -inf: with true drafts the EOS comes out of a draft row, finishes
    the row there, and every page comes back"""
    _, tokens = ref
    e = spec
    eos = [EOS]
    for guide in ("abc3", "abc4", "cab3", "abc5", "cab4"):
        T = tokens(P_SEED, P_LEN, P_CAP, guide, eos=eos)
        if T[-1] == EOS and (len(T) - 2) % (K + 1) != 0:             # the EOS at index len - 1 is row 0 of a step iff (len - 2) % 4 == 0
            break
    else:
        raise AssertionError("no finite language of the list ends on a draft row: a test error, add one")
    g = GUIDES[guide]
    assert g.matches(_text(T, eos)) and len(T) < P_CAP and _state_after(g, T, eos)[1] == 0
    _fresh(e, eos=eos)
    total, free = e.kv_pool_info()
    assert free == total
    toks, st, want, _ = _planted_run(e, _prompt(P_SEED, P_LEN), T, P_CAP, _true(T, P_CAP), guide, eos=eos)
    assert toks == T and st == want
    assert want["steps"] == -(-(len(T) - 1) // (K + 1)) and want["accepted"] == len(T) - 1 - want["steps"]
    assert e.kv_pool_info() == (total, total)


def test_cap_at_draft_index_1_of_a_guided_row(ref, spec):
    _, tokens = ref
    e = spec
    long = tokens(P_SEED, P_LEN, P_CAP, "struct")
    cap = 8                                                           # the step at L = 5 may commit T[5], T[6], T[7]: draft index 2 is past the cap
    T = tokens(P_SEED, P_LEN, cap, "struct")
    assert T == long[:cap]
    _fresh(e)
    total, _ = e.kv_pool_info()
    toks, st, want, _ = _planted_run(e, _prompt(P_SEED, P_LEN), T, cap, lambda L: long[L:L + K], "struct")
    assert toks == T and len(toks) == cap
    assert st == want and want == {"steps": 2, "drafted": 3 + 2, "accepted": 3 + 2}
    assert e.kv_pool_info() == (total, total)


# ---------------------------------------------------------------------------------------------------- 4. sampled guided rows

PARAMS = {
    "T0.1": SamplingParams(temperature=0.1, seed=9001),
    "T0.8": SamplingParams(temperature=0.8, seed=9002),
    "T0.8_k5": SamplingParams(temperature=0.8, top_k=5, seed=9003),
    "T1.0_p0.7": SamplingParams(temperature=1.0, top_p=0.7, seed=9004),
    "T0_k3": SamplingParams(temperature=0.0, top_k=3, seed=9006),
}


@pytest.mark.parametrize("guide", ["any", "struct"])
@pytest.mark.parametrize("name", sorted(PARAMS))
def test_sampled_guided_row(ref, spec, name, guide):
    _, tokens = ref
    e = spec
    sp, cap = PARAMS[name], P_CAP
    T = tokens(P_SEED, P_LEN, cap, guide, sp)
    assert len(T) == cap and _state_after(GUIDES[guide], T)[1] == 0
    _fresh(e, sampled=True)
    toks, st, want, _ = _planted_run(e, _prompt(P_SEED, P_LEN), T, cap, _true(T, cap), guide, sp=sp)
    assert toks == T and st == want
    assert want["accepted"] == cap - 1 - want["steps"] > 0 and want["steps"] == -(-(cap - 1) // (K + 1))
    # the same row without DOTS_SPEC_ROWS_SAMPLED drafts nothing: the guide alone does not let its parameters through
    _fresh(e, sampled=False)
    _setup_row(e, 0, guide, sp)
    p = _prompt(P_SEED, P_LEN)
    e.slots_prefill([0], p, [len(p)], [cap])
    got = _drive(e, [0], {0: T})[0]
    st = e.spec_stats(0)
    e.slot_release(0)
    assert got == T and st == {"steps": cap - 1, "drafted": 0, "accepted": 0}


def test_the_sampled_guided_runs_differ(ref):
    """ten different runs: the test above is not one check repeated"""
    _, tokens = ref
    runs = {(n, g): tuple(tokens(P_SEED, P_LEN, P_CAP, g, sp)) for n, sp in PARAMS.items() for g in ("any", "struct")}
    assert len(set(runs.values())) >= 7, runs


# ---------------------------------------------------------------------------------------------------- 5. a guided row with stop strings

S_CAP = 40


def _pick_stop(chunks):
    """a stop string from the row's own bytes whose first match completes at token q = 3 (mod 4), q >= 7: draft index 2 of the step of the
    all-true run that starts at L = q - 2 and would otherwise accept 3.  -> (strings, hit) or None"""
    data = b"".join(chunks)
    for q in range(7, len(chunks) - 2, 4):
        before = sum(len(c) for c in chunks[:q])
        for used in range(len(chunks[q]), 0, -1):
            end = before + used
            for m in range(2, min(end, 16) + 1):
                s = data[end - m:end].decode()
                h0 = first_stop(chunks, [s])
                if h0 is not None and h0[0] == q:
                    return [s], h0
    return None


def test_guided_row_with_stop_strings(ref, spec):
    plain, tokens = ref
    e = spec
    guide = "struct"
    for seed in range(600, 640):
        T = tokens(seed, P_LEN, S_CAP, guide)
        picked = _pick_stop([TOKS[t] for t in T])
        if picked is not None:
            break
    else:
        raise AssertionError("no prompt seed in [600, 640) offers the stop string the test wants: a test error, widen the search")
    strings, hit = picked
    q = hit[0]
    want = _seq_run(plain, _prompt(seed, P_LEN), S_CAP, guide, stop=(strings, 0))
    assert want["toks"] == T[:q + 1] and want["hit"] == hit          # the sequential engine agrees with the rule stated on the host
    _fresh(e, stop=True)
    toks, st, host, got_hit = _planted_run(e, _prompt(seed, P_LEN), want["toks"], S_CAP, _true(T, S_CAP), guide, stop=(strings, 0))
    assert toks == want["toks"] and len(toks) == q + 1 and got_hit == want["hit"]
    assert st == host
    assert host["steps"] == (q - 3) // 4 + 1 and host["accepted"] == q - host["steps"] and host["drafted"] == host["accepted"] + 1
    # without DOTS_SPEC_ROWS_STOP the row drafts nothing
    _fresh(e, stop=False)
    _setup_row(e, 0, guide, stop=(strings, 0))
    p = _prompt(seed, P_LEN)
    e.slots_prefill([0], p, [len(p)], [S_CAP])
    got = _drive(e, [0], {0: T})[0]
    st = e.spec_stats(0)
    e.slot_release(0)
    assert got == want["toks"] and st == {"steps": q, "drafted": 0, "accepted": 0}


# ---------------------------------------------------------------------------------------------------- 6. row indexing

@pytest.mark.parametrize("slots", [(0, 1, 2), (3, 1, 0)])
def test_three_slots_in_one_step(ref, spec, slots):
    """guide A, a plain greedy row and guide B side by side, each at its own state: a state or a mask written to b * (k + 1) + j instead of
    j * rows + b lands in another slot's row and shows here"""
    _, tokens = ref
    e = spec
    reqs = [(P_SEED, P_LEN, "struct"), (41, 30, None), (43, 47, "choice")]
    eos = [EOS]
    _fresh(e, eos=eos)
    rows = dict(zip(slots, reqs))
    order = sorted(rows)
    for s in order:
        _setup_row(e, s, rows[s][2])
    prompts = [_prompt(rows[s][0], rows[s][1]) for s in order]
    e.slots_prefill(order, np.concatenate(prompts), [len(p) for p in prompts], [P_CAP] * 3)
    truth = {s: tokens(rows[s][0], rows[s][1], P_CAP, rows[s][2], eos=eos) for s in order}
    got = _drive(e, order, truth)
    st = {s: e.spec_stats(s) for s in order}
    for s in order:
        e.slot_release(s)
    assert got == truth
    assert len({tuple(t) for t in truth.values()}) == 3
    for s in order:
        assert st[s]["accepted"] > 0 and st[s]["steps"] + st[s]["accepted"] == len(truth[s]) - 1, (s, st[s])


# ---------------------------------------------------------------------------------------------------- 7. who still does not speculate

def _feature_run(e, kind, truth=None, cap=20):
    """a guided row that carries one more feature, in slot 0 from its prefill to the cap; truth: its sequential tokens, planted before
    every step.  -> (tokens, counters)"""
    e.set_row_guide(0, _handle(e, "any"))
    if kind == "penalty":
        e.set_row_sampling(0, SamplingParams(temperature=0.8, repetition_penalty=1.1, seed=61))
    elif kind == "rules":
        e.set_row_logit_rules(0, LogitRules(bias={5: 2.0, 9: float("-inf")}, vocab_size=V))
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


@pytest.mark.parametrize("kind", ["penalty", "rules", "ngram", "logprobs"])
def test_guided_rows_that_never_speculate(ref, spec, kind):
    plain, _ = ref
    e = spec
    _plain(plain)
    want, _ = _feature_run(plain, kind)
    _fresh(e, sampled=True, stop=True, max_n=4)
    got, st = _feature_run(e, kind, truth=want)
    assert got == want
    assert st == {"steps": len(want) - 1, "drafted": 0, "accepted": 0}


def test_no_guided_row_speculates_under_an_engine_wide_temperature(ref, spec):
    plain, _ = ref
    e = spec
    p = _prompt(71, 20)

    def run(eng, truth):
        eng.set_sampling(0.8, 1.0, 5)
        try:
            eng.set_row_guide(0, _handle(eng, "struct"))
            eng.slots_prefill([0], p, [20], [20])
            toks = _drive(eng, [0], truth)
            st = eng.spec_stats(0)
            eng.slot_release(0)
        finally:
            eng.set_sampling(0.0, 1.0, 0)
        return toks, st
    _plain(plain)
    want, _ = run(plain, {})
    _fresh(e, sampled=True, stop=True, max_n=4)
    got, st = run(e, want)
    assert got == want
    assert st == {"steps": 19, "drafted": 0, "accepted": 0}


def test_a_guided_row_drawn_by_a_kept_engine_wide_entry_does_not_speculate(ref, spec):
    """a guided row without parameters of its own is selected with the engine-wide setting as it stood when the guide was set (§6.1).  Set
    under a temperature, it is drawn by the stage even after the engine went back to greedy: its draft rows would be arg maxima, so it
    verifies nothing"""
    plain, tokens = ref
    e = spec
    p = _prompt(71, 20)

    def run(eng, truth):
        eng.set_sampling(0.8, 1.0, 5)
        eng.set_row_guide(0, _handle(eng, "struct"))
        eng.set_sampling(0.0, 1.0, 0)
        eng.slots_prefill([0], p, [20], [20])
        toks = _drive(eng, [0], truth)
        st = eng.spec_stats(0)
        eng.slot_release(0)
        return toks, st
    _plain(plain)
    want, _ = run(plain, {})
    assert want[0] != tokens(71, 20, 20, "struct")                    # the row is drawn, not the greedy guided run
    _fresh(e, sampled=True, stop=True, max_n=4)
    got, st = run(e, want)
    assert got == want
    assert st == {"steps": 19, "drafted": 0, "accepted": 0}


# ---------------------------------------------------------------------------------------------------- 8. the built-in drafter, end to end

REQS = [(101, 7, 40, "struct", None), (102, 61, 33, "any", 0.1), (103, 30, 50, "choice", None), (104, 64, 17, "struct", 0.1), (105, 100, 64, "any", None),
        (106, 15, 25, "struct", None)]


def _requests(e):
    from dots_ocr_amd.scheduler import Request
    return [Request(_prompt(s, n), max_new_tokens=cap, guide=_handle(e, guide),
                    sampling=None if t is None else SamplingParams(temperature=t, seed=3000 + i))
            for i, (s, n, cap, guide, t) in enumerate(REQS)]


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
    for (_, _, cap, guide, _), t in zip(REQS, want):
        assert GUIDES[guide].walk(GUIDES[guide].start, _text(t, [EOS])) != G.DEAD and 2 <= len(t) <= cap
    return want


@pytest.mark.parametrize("chunk", [1, 16])
def test_builtin_drafter_end_to_end(spec, e2e, chunk):
    e = spec
    _fresh(e, sampled=True, max_n=4)
    got, cb = _batched(e, chunk)
    assert cb.n_slots == 4
    assert got == e2e
    st = e.spec_stats()
    assert st["steps"] + st["accepted"] == sum(len(t) - 1 for t in e2e)       # every decode token is row 0 of a step or an accepted draft
    assert 0 < st["accepted"] <= st["drafted"]
    total, free = e.kv_pool_info()
    assert free == total


def test_builtin_drafter_under_the_partition_plan(spec, e2e):
    e = spec
    _fresh(e, sampled=True, max_n=4)
    e.set_decode_plan(1)
    try:
        got, _ = _batched(e, 16)
    finally:
        e.set_decode_plan(0)
    assert got == e2e
    st = e.spec_stats()
    assert st["steps"] + st["accepted"] == sum(len(t) - 1 for t in e2e)


def test_builtin_drafter_with_the_fp8_kv_cache():
    plain, e = _engine(16, "fp8"), _engine(16, "fp8")
    try:
        _plain(plain)
        want, _ = _batched(plain, 16)
        _fresh(e, sampled=True, max_n=4)
        got, _ = _batched(e, 16)
        assert got == want
        st = e.spec_stats()
        assert st["steps"] + st["accepted"] == sum(len(t) - 1 for t in want)
    finally:
        plain.close()
        e.close()


# ---------------------------------------------------------------------------------------------------- 9. guards

def test_guards(ref, spec):
    _, tokens = ref
    e = spec
    guide, cap = "struct", P_CAP
    T = tokens(P_SEED, P_LEN, cap, guide)
    p = _prompt(P_SEED, P_LEN)

    def run():
        _setup_row(e, 0, guide)
        e.slots_prefill([0], p, [len(p)], [cap])
        got = _drive(e, [0], {0: T})[0]
        st = e.spec_stats(0)
        e.slot_release(0)
        return got, st
    _fresh(e, guided=False)
    assert e.spec_guided is False
    e.slots_prefill([0], p, [len(p)], [8])
    assert e.lib.dots_set_speculation_guided(e.h, 1) == -3            # DOTS_E_STATE: a slot is occupied
    with pytest.raises(DotsEngineError) as ei:
        e.set_speculation_guided(True)
    assert "(-3)" in str(ei.value) and e.spec_guided is False
    e.slot_release(0)
    got, st = run()                                                   # the refused calls left it off
    assert got == T and st == {"steps": cap - 1, "drafted": 0, "accepted": 0}
    # the setting survives speculation being switched off and on again, and leaves dots_set_speculation_rows alone
    e.set_speculation_guided(True)
    e.set_speculation(0)
    e.set_speculation(K, 2, 0)
    assert e.spec_guided is True and e.spec_rows == 0
    for bad in (4, 7, 8):
        assert e.lib.dots_set_speculation_rows(e.h, bad) == -1        # still no bit of the rows setting
    got, st = run()
    assert got == T and st["accepted"] == cap - 1 - st["steps"] > 0
    # switching it off returns the row to drafting nothing
    e.set_speculation_guided(False)
    got, st = run()
    assert got == T and st == {"steps": cap - 1, "drafted": 0, "accepted": 0}


def test_clearing_the_guide_of_a_running_row_takes_effect_at_the_next_step(ref, spec):
    plain, tokens = ref
    e = spec
    guide, cap, cut = "struct", P_CAP, 9
    p = _prompt(P_SEED, P_LEN)
    T = tokens(P_SEED, P_LEN, cap, guide)

    def run(eng, truth, step):
        _setup_row(eng, 0, guide)
        eng.slots_prefill([0], p, [len(p)], [cap])
        while True:
            fin, lens = eng.slots_poll()
            L = int(lens[0])
            if L >= cut:
                break
            if truth is not None:
                eng.set_row_drafts(0, truth[L:L + min(K, cut - L - 1)])      # never past the cut: both engines clear the guide at L == cut
            eng.slots_decode(step)
        assert L == cut and eng.slot_read(0, L).tolist() == T[:cut]
        eng.set_row_guide(0, None)
        assert eng.row_guide_state(0) == -1
        toks = _drive(eng, [0], {0: truth})[0]
        st = eng.spec_stats(0)
        eng.slot_release(0)
        return toks, st
    _plain(plain)
    want, _ = run(plain, None, 1)
    assert want[:cut] == T[:cut] and want != T and GUIDES[guide].walk(GUIDES[guide].start, _text(want)) == G.DEAD
    _fresh(e)
    got, st = run(e, want, 1)
    assert got == want
    assert st["accepted"] > 0 and st["steps"] + st["accepted"] == cap - 1


# ---------------------------------------------------------------------------------------------------- 10. the draft-row mask at the real vocabulary

def test_draft_row_masks_at_the_real_vocabulary():
    """the state chain and the mask of the draft rows alone (dots_op_spec_guide_masks) at V = 151 936 under the layout guide, bit for bit
    against Guide.draft_states / Guide.mask: three slots at three states, one of them unguided, a dead tail, a draft list cut by n_live"""
    from dots_ocr_amd.engine import Engine
    from test_guided_gpu import EOS as BIG_EOS, V as BIG_V, synthetic_tokens
    cfg = DotsConfig.tiny(layers=1, v_layers=1, vocab=BIG_V)
    e = Engine(cfg, max_batch=1, max_seq_len=128, max_patches=256, max_prefill_tokens=128)
    try:
        tb = synthetic_tokens(BIG_V, 5, special=BIG_EOS)
        e.set_token_bytes(tb)
        e.set_eos(BIG_EOS)
        g = G.compile_json_schema(G.layout_schema())
        h = e.create_guide(g)
        ids = {tb.token(t): t for t in range(BIG_V - 1, 255, -1) if tb.token(t)}      # bytes -> the lowest id that holds them

        def tok(b):
            return ids[b] if b in ids else b[0]
        s0 = g.start
        s1 = g.walk(g.start, b'[{"bbox": [1')
        assert s1 != G.DEAD
        k = 4
        drafts = [[tok(b"["), tok(b'{"'), tok(b"bbox"), tok(b'":')],           # all four alive
                  [tok(b"2"), tok(b", "), tok(b"x"), tok(b"3")],               # "x" is no digit: a dead tail of two
                  [tok(b"["), tok(b"["), tok(b"["), tok(b"[")],               # an unguided slot
                  [tok(b"["), 97 * 3, tok(b'{"'), tok(b"bbox")],               # a byte-less id at draft index 2
                  [tok(b"["), tok(b'{"'), BIG_EOS[0], tok(b'"')]]               # an EOS id at draft index 3
        guides, states, n_live = [h, h, None, h, h], [s0, s1, 0, s0, s0], [4, 4, 4, 3, 4]
        rows = len(guides)
        got_s, got_m = e.spec_guide_masks_op(guides, states, drafts, n_live, k)
        alive = 0
        for b in range(rows):
            chain = [-1] * k if guides[b] is None else g.draft_states(states[b], drafts[b][:n_live[b]], tb, BIG_EOS) + [-1] * (k - n_live[b])
            assert got_s[b] == -1                                     # a head row: the chain writes the draft rows only
            for j in range(1, k + 1):
                r = j * rows + b
                assert got_s[r] == chain[j - 1], (b, j)
                want = g.mask(chain[j - 1], tb) if chain[j - 1] >= 0 else np.zeros(BIG_V, bool)
                assert np.array_equal(got_m[r], want), (b, j, int((got_m[r] != want).sum()))
                alive += chain[j - 1] >= 0
        assert alive == 4 + 2 + 0 + 1 + 2
    finally:
        e.close()
