"""No-repeat n-gram blocking on the GPU: a row never completes an n-gram its own output already holds.

The single-stage entry (Engine.select_tokens_ngram) runs at the real vocabulary against engine.banned_ngram_ids plus numpy on planted
logits whose deciding margins are >= 0.5; a mask changes no value, so tokens are compared exactly.  The tiny engine checks the decode
loop.  dots_get_logits serves the static batch only, so the step-by-step replays (every committed token against the host's choice from
the raw logits and the tokens so far) run there, one eager step at a time; the slot-mode runs check the captured chunks against them."""
import numpy as np
import pytest
import torch

from dots_ocr_amd.config import DotsConfig
from dots_ocr_amd.engine import DotsEngineError, LogitRules, NgramRule, SamplingParams, banned_ngram_ids
from dots_ocr_amd.weights import random_state_dict

pytestmark = pytest.mark.gpu

V = 151936


@pytest.fixture(scope="module")
def eng():
    from dots_ocr_amd.engine import Engine
    cfg = DotsConfig.tiny(layers=3, v_layers=3, vocab=1024)
    e = Engine(cfg, max_batch=4, max_seq_len=640, max_patches=4096, max_prefill_tokens=2048)
    e.load_state_dict(random_state_dict(cfg, seed=11))
    yield cfg, e
    e.close()


# ---------------------------------------------------------------------------------------------------- the stage at the real vocabulary

def _select(e, logits, params, rules, ngrams, hists, n_prompt):
    B = len(params)
    stride = max(1, max(len(h) for h in hists))
    H = np.full((B, stride), -1, np.int32)
    for b, h in enumerate(hists):
        H[b, :len(h)] = h
    d_l = torch.from_numpy(np.ascontiguousarray(logits, np.float32)).cuda()
    d_h = torch.from_numpy(H).cuda()
    d_n = torch.tensor([len(h) for h in hists], dtype=torch.int32, device="cuda")
    d_p = torch.tensor(n_prompt, dtype=torch.int32, device="cuda")
    out = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    if ngrams is None:
        e.select_tokens_rules(d_l.data_ptr(), B, V, params, rules, None, d_h.data_ptr(), d_n.data_ptr(), stride, d_p.data_ptr(), out.data_ptr())
    else:
        e.select_tokens_ngram(d_l.data_ptr(), B, V, params, rules, ngrams, d_h.data_ptr(), d_n.data_ptr(), stride, d_p.data_ptr(), out.data_ptr())
    return out.cpu().numpy()


def _shaped(l, rules, ngram, hist, n_prompt, p):
    """numpy fp64 restatement of the order: l + bias, -inf for not allowed and for what the n-gram rule bans, then the penalties"""
    s = l.astype(np.float64).copy()
    if rules is not None:
        for t, v in rules.bias:
            s[t] += v
        if rules.allowed is not None:
            keep = np.zeros(V, bool)
            keep[list(rules.allowed)] = True
            s[~keep] = -np.inf
    if ngram is not None:
        banned = banned_ngram_ids(hist[n_prompt:], ngram.size, ngram.window, ngram.whitelist)
        s[sorted(banned)] = -np.inf
    hist = np.asarray(hist, np.int64)
    c = np.bincount(hist[n_prompt:], minlength=V).astype(np.float64)
    seen = c > 0
    seen[hist[:n_prompt]] = True
    r = p.repetition_penalty
    if r != 1.0:
        s[seen] = np.where(s[seen] > 0, s[seen] / r, s[seen] * r)
    return s - (p.frequency_penalty * c + p.presence_penalty * (c > 0))


def _planted_row(rng, case):
    """(logits, hist, n_prompt, params, rules, ngram) of one greedy row.  Raw: a = 10 > b = 9 > c = 8 > d = 7 over N(0, 1) noise
    (max ~ 4.5).  x, y and the filler f are distinct ids, so the planted n-grams are the only repeats of the generated part."""
    l = rng.normal(0.0, 1.0, V).astype(np.float32)
    ids = [int(t) for t in rng.choice(V - 2000, 48, replace=False)]
    a, b, c, d, x, y = ids[:6]
    f = ids[6:]
    l[a], l[b], l[c], l[d] = 10.0, 9.0, 8.0, 7.0
    # the prompt repeats the planted trigram: the prompt is not part of the history, so that alone bans nothing
    prompt = [int(t) for t in rng.integers(0, V - 2000, 36)] + [x, y, a, x]
    p, rules = SamplingParams(), None
    if case == "ban_max":
        gen, ng = f[:5] + [x, y, a] + f[5:10] + [x, y], NgramRule(3)                       # b = 9 is next
    elif case == "top3_banned":
        gen, ng = [x, y, a, f[0], x, y, b, f[1], x, y, c, f[2], x, y], NgramRule(3)         # three matches ban a, b, c: d = 7 is next
    elif case == "window_out":
        gen = f[:3] + [x, y, a] + f[3:9] + [x, y]                                           # the match starts at i = 3, L = 14
        ng = NgramRule(3, window=len(gen) - 3 - 1)                                          # i = L - W - 1: outside
    elif case == "window_edge":
        gen = f[:3] + [x, y, a] + f[3:9] + [x, y]
        ng = NgramRule(3, window=len(gen) - 3)                                              # i = L - W: the oldest n-gram that counts
    elif case == "last_pos":
        gen, ng = f[:7] + [a, a, a], NgramRule(3)                                           # i = L - n: out[L-3 .. L-1) == out[L-2 .. L)
    elif case == "whitelist":
        gen, ng = f[:5] + [x, y, a] + f[5:10] + [x, y], NgramRule(3, whitelist=[f[20], a])
    elif case == "n1":
        gen, ng = f[:4] + [a] + f[4:8] + [b], NgramRule(1)                                  # every generated id: c = 8 is next
    elif case == "short":
        gen, ng = [a, a], NgramRule(4)                                                      # L = n - 2: no prefix yet
    elif case == "long":
        gen = [int(t) for t in rng.integers(0, V - 2000, 4096)]                             # L = 4096, n = 64
        gen[3000:3063] = gen[-63:]                                                          # i = 3000: far past a thread's first stride
        gen[3063] = a
        ng = NgramRule(64)
    elif case == "with_rules":
        gen, ng = f[:5] + [x, y, a] + f[5:10] + [x, y], NgramRule(3)
        rules = LogitRules(allowed=[a, b, c, f[30], f[31]], bias={b: -3.0})                 # a banned, b = 6: c = 8
    elif case == "with_pen":
        l[a] = 12.0
        gen, ng = f[:3] + [b, x, y, a] + f[3:8] + [b, x, y], NgramRule(3)
        p = SamplingParams(repetition_penalty=1.2, frequency_penalty=0.4, presence_penalty=0.3)
        # without the rule a = 12 / 1.2 - 0.7 = 9.3 wins; with it c = 8 does, the penalties having taken b to 9 / 1.2 - 1.1 = 6.4
    elif case == "none":
        gen, ng = f[:5] + [x, y, a] + f[5:10] + [x, y], None
    return l, prompt + gen, len(prompt), p, rules, ng


CASES = ("ban_max", "top3_banned", "window_out", "window_edge", "last_pos", "whitelist", "n1", "short", "long", "with_rules", "with_pen", "none")
FLIPS = {"ban_max", "top3_banned", "window_edge", "last_pos", "n1", "long", "with_rules", "with_pen"}


def _margin(sh):
    top = np.sort(sh[np.isfinite(sh)])[-2:]
    return top[1] - top[0]


@pytest.mark.parametrize("B", [1, 8, 64])
def test_stage_matches_the_restatement(eng, B):
    _, e = eng
    e.set_eos([])
    rng = np.random.default_rng(300 + B)
    calls = [[k] for k in range(len(CASES))] if B == 1 else [list(range(B))]          # B = 1: every case as a call of one row
    seen = set()
    for call in calls:
        names = [CASES[(k + B) % len(CASES)] for k in call]
        rows = [_planted_row(rng, nm) for nm in names]
        L = np.stack([r[0] for r in rows])
        params, rules, ngrams = [r[3] for r in rows], [r[4] for r in rows], [r[5] for r in rows]
        hists, n_prompt = [r[1] for r in rows], [r[2] for r in rows]
        got = _select(e, L, params, rules, ngrams, hists, n_prompt)
        without = _select(e, L, params, rules, None, hists, n_prompt)                  # the same rows through the entry without n-gram rules
        for b, (l, hist, n_p, p, rl, ng) in enumerate(rows):
            sh, free = _shaped(l, rl, ng, hist, n_p, p), _shaped(l, rl, None, hist, n_p, p)
            assert _margin(sh) >= 0.5 and _margin(free) >= 0.5, names[b]
            assert got[b] == int(np.argmax(sh)), (b, names[b], int(got[b]), int(np.argmax(sh)))
            assert without[b] == int(np.argmax(free)), (b, names[b])
            # a flipping case flips because of the rule, and only those flip
            assert (int(np.argmax(sh)) != int(np.argmax(free))) == (names[b] in FLIPS), names[b]
            if names[b] == "none":
                assert got[b] == int(np.argmax(l))                                       # the plain arg max
            seen.add(names[b])
        # top_k = 1 is greedy at any temperature: the shaped values (the ban included) reach the threshold and draw kernels
        p1 = [SamplingParams(temperature=0.8, top_k=1, seed=b, repetition_penalty=r[3].repetition_penalty,
                             frequency_penalty=r[3].frequency_penalty, presence_penalty=r[3].presence_penalty) for b, r in enumerate(rows)]
        assert np.array_equal(_select(e, L, p1, rules, ngrams, hists, n_prompt), got)
    assert seen == set(CASES) if B != 8 else len(seen) == 8


def test_bad_rules_are_refused_at_the_call(eng):
    cfg, e = eng
    bad = [(0, 0, ()), (65, 0, ()), (3, 2, ()), (3, 641, ()), (3, -1, ()), (2, 0, (cfg.vocab_size,)), (2, 0, (-1,)), (2, 0, (5, 5)),
           (2, 0, tuple(range(17)))]
    from dots_ocr_amd.engine import CDotsNgramRule
    import ctypes
    for n, w, wl in bad:                                    # past the Python checks, straight at the C entry
        c = CDotsNgramRule(n, w, min(len(wl), 17) if len(wl) <= 16 else 17)
        for j, t in enumerate(wl[:16]):
            c.whitelist[j] = t
        assert e.lib.dots_set_row_ngram(e.h, 0, ctypes.byref(c)) == -1, (n, w, wl)
    with pytest.raises(DotsEngineError):
        e.set_row_ngram(4, NgramRule(2))                    # row out of range
    e.set_row_ngram(0, NgramRule(64, 640, tuple(range(16))))     # the limits themselves are fine
    e.set_row_ngram(0, None)
    e.set_row_ngram(1, None)                                # clearing a row that never had one


# ---------------------------------------------------------------------------------------------------- decode loop, tiny engine

CAP = 24


def _prompt(cfg, seed):
    g = np.random.default_rng(seed)
    return g.integers(0, cfg.vocab_size - 8, 6 + seed % 4).astype(np.int32)


def _run(e, prompts, slots=None, ngram=None, rules=None, sampling=None, cap=CAP, chunk=8, switch=None):
    """prefill `prompts` into `slots` and decode to the end in captured chunks: token lists.  switch = (after_steps, slot, rule)"""
    slots = list(range(len(prompts))) if slots is None else slots
    e.set_sampling(0.0, 1.0, 0)
    e.slots_reset()
    e.set_eos([])
    for i, s in enumerate(slots):
        if ngram and ngram[i] is not None:
            e.set_row_ngram(s, ngram[i])
        if rules and rules[i] is not None:
            e.set_row_logit_rules(s, rules[i])
        if sampling and sampling[i] is not None:
            e.set_row_sampling(s, sampling[i])
    e.slots_prefill(slots, np.concatenate(prompts), [len(p) for p in prompts], [cap] * len(prompts))
    steps = 0
    while steps < cap:
        e.slots_decode(chunk)
        steps += chunk
        if switch and steps == switch[0]:
            e.set_row_ngram(switch[1], switch[2])
    fin, lens = e.slots_poll()
    toks = [e.slot_read(s, int(lens[s])).tolist() for s in slots]
    assert all(fin[s] == 1 for s in slots)
    for s in slots:
        e.slot_release(s)
    return toks


def _static(e, prompts, ngram=None, rules=None, steps=CAP - 1, switch=None, lp=None):
    """static prefill + eager decode steps, one at a time: (logits [steps + 1, B, V], tokens [steps + 1, B], logprobs).
    switch = (tokens_held, row, rule): the n-gram rule of that row is set when the rows hold that many tokens"""
    e.set_sampling(0.0, 1.0, 0)
    e.set_eos([])
    rows = range(len(prompts))
    try:
        for b in rows:
            if ngram and ngram[b] is not None:
                e.set_row_ngram(b, ngram[b])
            if rules and rules[b] is not None:
                e.set_row_logit_rules(b, rules[b])
            if lp and lp[b] is not None:
                e.set_row_logprobs(b, lp[b])
        e.prefill(np.concatenate(prompts), np.array([len(p) for p in prompts], np.int32))
        logits, toks = [e.get_logits()], [e.get_last_tokens()]
        for k in range(steps):
            if switch and len(toks) == switch[0]:
                e.set_row_ngram(switch[1], switch[2])
            e.decode_step()
            logits.append(e.get_logits())
            toks.append(e.get_last_tokens())
        lps = [e.row_logprobs(b, steps + 1) if lp and lp[b] is not None else None for b in rows]
    finally:
        for b in rows:
            e.set_row_ngram(b, None)
            e.set_row_logit_rules(b, None)
            e.set_row_logprobs(b, None)
    return np.stack(logits), np.stack(toks), lps


def _host_choice(logits, out, rule, rules=None):
    """what the contract selects for a greedy row: the arg max of raw logit + bias with the banned ids at -inf (lowest index on a tie)"""
    s = logits.astype(np.float64).copy()
    for t, v in (rules.bias if rules is not None else ()):
        s[t] += v
    if rule is not None:
        s[sorted(banned_ngram_ids(out, rule.size, rule.window, rule.whitelist))] = -np.inf
    return int(np.argmax(s))


def _first_violation(toks, n, window=0, whitelist=()):
    """first position whose token completes an n-gram the window before it already holds, or None"""
    for k in range(len(toks)):
        if toks[k] in banned_ngram_ids(toks[:k], n, window, whitelist):
            return k
    return None


A, A2 = 37, 611                                   # the ids a bias of +1e4 confines rows 0 and 1 to: their free runs repeat them for ever
HOLD = [LogitRules(bias={A: 1e4}), LogitRules(bias={A2: 1e4}), None, None]


@pytest.fixture(scope="module")
def replay(eng):
    """Four rows, step by step in the static batch, computed once.  Rows 0 and 1 are held to one id each by a bias, so the run without
    an n-gram rule repeats a trigram from its fourth token on, whatever the model does: a repeat inside the window by construction
    rather than by a lucky prompt.  Row 2 carries no logit rules, row 3 nothing at all.
    free: no n-gram rule anywhere.  ruled: row 0 n = 3, W = 8 and one whitelisted id (the id its first ban falls back to, so that the
    whitelist is exercised), row 1 n = 3, W = 8, row 2 n = 1 (no token twice), row 3 none."""
    cfg, e = eng
    prompts = [_prompt(cfg, 900 + b) for b in range(4)]
    free_logits, free, _ = _static(e, prompts, rules=HOLD)
    first = [NgramRule(3, 8), NgramRule(3, 8), NgramRule(1), None]
    _, t1, _ = _static(e, prompts, rules=HOLD, ngram=first)
    x0 = int(t1[3, 0])                             # out = [A, A, A]: A is banned, the row falls back to the model's own choice
    ngram = [NgramRule(3, 8, [x0]), NgramRule(3, 8), NgramRule(1), None]
    logits, toks, _ = _static(e, prompts, rules=HOLD, ngram=ngram)
    return dict(prompts=prompts, ngram=ngram, x0=x0, logits=logits, toks=toks, free_logits=free_logits, free=free)


def test_every_step_commits_the_hosts_choice(eng, replay):
    """n = 3, W = 8, one whitelisted id, 24 steps, step by step: the committed token is the host's choice from the raw logits and the
    tokens so far, at every step and for every row."""
    r = replay
    logits, toks, free, x0 = r["logits"], r["toks"], r["free"], r["x0"]
    assert free[:, 0].tolist() == [A] * CAP and free[:, 1].tolist() == [A2] * CAP
    for b in (0, 1):                                                            # the run without the rule repeats a trigram inside the window
        assert _first_violation(free[:, b].tolist(), 3, 8) == 3
    for b in range(4):
        out = []
        for k in range(CAP):
            assert int(toks[k, b]) == _host_choice(logits[k, b], out, r["ngram"][b], HOLD[b]), (b, k)
            out.append(int(toks[k, b]))
    for b in (0, 1):
        out = toks[:, b].tolist()
        assert out[:3] == free[:3, b].tolist() and out[3] != free[3, b]          # the first ban, where the free run repeats
        assert _first_violation(out, 3, 8, r["ngram"][b].whitelist) is None
    assert x0 != A and toks[3, 0] == x0
    # the whitelist was exercised: at some step the rule would have banned x0 and did not
    assert any(x0 in banned_ngram_ids(toks[:k, 0].tolist(), 3, 8) for k in range(CAP))
    assert len(set(toks[:, 2].tolist())) == CAP                                 # n = 1: no token twice
    # the row without anything: tokens and raw logits bitwise those of the free run
    assert np.array_equal(toks[:, 3], free[:, 3]) and np.array_equal(logits[:, 3].view(np.uint32), r["free_logits"][:, 3].view(np.uint32))
    assert np.array_equal(logits[0].view(np.uint32), r["free_logits"][0].view(np.uint32))      # the rule never touches the raw logits


def test_captured_chunks_give_the_tokens_of_single_steps(eng, replay):
    _, e = eng
    r = replay
    one = _run(e, r["prompts"], rules=HOLD, ngram=r["ngram"], chunk=1)
    assert all(len(t) == CAP for t in one)
    assert _run(e, r["prompts"], rules=HOLD, ngram=r["ngram"], chunk=8) == one
    assert _run(e, r["prompts"], rules=HOLD, ngram=r["ngram"], chunk=16) == one
    assert one == [r["toks"][:, b].tolist() for b in range(4)]                  # and those of the step-by-step replay
    assert _run(e, r["prompts"], rules=HOLD, chunk=8) == [r["free"][:, b].tolist() for b in range(4)]      # the rows were cleared


def test_pigeonhole_greedy(eng):
    """A bias of +1e4 confines a row to two ids: without the rule a bigram repeats within 6 tokens; with n = 2 no bigram occurs twice,
    so a third id appears by position 5 (5 is the longest sequence over two symbols without a repeated bigram)."""
    cfg, e = eng
    a, b = 17, 901
    rules = LogitRules(bias={a: 1e4, b: 1e4})
    p = [_prompt(cfg, 950)]
    free = _run(e, p, rules=[rules], cap=12, chunk=4)[0]
    assert len(free) == 12 and set(free) <= {a, b}
    big = list(zip(free[:5], free[1:6]))
    assert len(set(big)) < len(big)                                             # some bigram twice within the first 6 tokens
    got = _run(e, p, rules=[rules], ngram=[NgramRule(2)], cap=12, chunk=4)[0]
    assert len(got) == 12
    big = list(zip(got[:-1], got[1:]))
    assert len(set(big)) == len(big), got                                       # no bigram twice anywhere
    assert any(t not in (a, b) for t in got[:6]), got


def test_ruled_request_is_the_same_alone_in_a_batch_and_in_any_slot(eng, replay):
    _, e = eng
    r = replay
    p, ng = r["prompts"], r["ngram"]
    want = [r["toks"][:, b].tolist() for b in range(4)]
    for b in (0, 2):                                                            # a row with logit rules beside the n-gram rule, and one without
        assert _run(e, [p[b]], slots=[0], rules=[HOLD[b]], ngram=[ng[b]])[0] == want[b]
        assert _run(e, [p[b]], slots=[3], rules=[HOLD[b]], ngram=[ng[b]])[0] == want[b]
    # another order in the batch, neighbours without any rule: the ruled rows keep their tokens, the neighbours run free
    plain = _run(e, [p[3], p[1]])
    got = _run(e, [p[3], p[0], p[1], p[2]], rules=[None, HOLD[0], None, None], ngram=[None, ng[0], None, ng[2]])
    assert got[1] == want[0] and got[3] == want[2]
    assert got[0] == plain[0] == r["free"][:, 3].tolist() and got[2] == plain[1]
    # static batch, step by step: a neighbour's tokens and dots_get_logits are bitwise the same whether or not the others carry a rule
    assert np.array_equal(r["toks"][:, 3], r["free"][:, 3])
    assert np.array_equal(r["logits"][:, 3].view(np.uint32), r["free_logits"][:, 3].view(np.uint32))


def test_rule_switched_on_between_chunks_is_exact_from_the_next_step(eng, replay):
    _, e = eng
    p0, rule = replay["prompts"][0], NgramRule(3, 8)
    # step by step: the rule arrives when the row holds 9 tokens (the prefill's and those of one chunk of 8); from then on every token is
    # the host's choice under the rule computed from ALL the tokens so far, those generated before the switch included
    logits, toks, _ = _static(e, [p0], rules=HOLD[:1], switch=(9, 0, rule))
    out = []
    for k in range(CAP):
        assert int(toks[k, 0]) == _host_choice(logits[k, 0], out, rule if k >= 9 else None, HOLD[0]), k
        out.append(int(toks[k, 0]))
    assert out[:9] == [A] * 9 and out[9] != A                                   # exact at once: nine A's are history, the tenth is banned
    assert _run(e, [p0], rules=HOLD[:1], chunk=8, switch=(8, 0, rule))[0] == out             # the same between captured chunks of 8
    # cleared mid-run with None: free again from the next step
    off = _run(e, [p0], rules=HOLD[:1], ngram=[rule], chunk=8, switch=(8, 0, None))[0]
    assert off[:3] == [A] * 3 and off[3] != A and _first_violation(off[:9], 3, 8) is None      # ruled up to the switch ...
    assert off[9:] == [A] * (CAP - 9)                                                          # ... and the free run's id ever after


def test_release_and_reset_clear_the_row(eng, replay):
    """The next occupant of a slot runs free.  It is held to the id A by a bias, so its output is A throughout if and only if no
    NgramRule(1) is left on the row: under that rule A could appear once."""
    _, e = eng
    p0 = replay["prompts"][0]
    ruled = _run(e, [p0], slots=[1], rules=HOLD[:1], ngram=[NgramRule(1)])[0]
    assert ruled[0] == A and len(set(ruled)) == CAP

    def occupant(slot):
        e.set_row_logit_rules(slot, HOLD[0])
        e.slots_prefill([slot], p0, [len(p0)], [CAP])
        e.slots_decode(CAP)
        _, lens = e.slots_poll()
        got = e.slot_read(slot, int(lens[slot])).tolist()
        e.slot_release(slot)
        return got
    assert occupant(1) == [A] * CAP                                             # _run released slot 1, no reset in between
    e.set_row_ngram(2, NgramRule(1))
    e.slots_reset()                                                             # a reset clears every row
    assert occupant(2) == [A] * CAP


def test_sampled_row_repeats_no_bigram_and_is_the_same_in_any_slot(eng):
    cfg, e = eng
    ids = (33, 480, 777)
    rules = LogitRules(bias={t: 1e4 for t in ids})
    sp = SamplingParams(temperature=1.0, seed=12)
    p = [_prompt(cfg, 970)]
    free = _run(e, p, rules=[rules], sampling=[sp])[0]
    assert len(free) == CAP and set(free) <= set(ids)                           # the free run stays inside the three ids ...
    big = list(zip(free[:10], free[1:11]))
    assert len(set(big)) < len(big)                                             # ... so a bigram repeats by token 11 (3 symbols allow 10)
    got = _run(e, p, slots=[0], rules=[rules], sampling=[sp], ngram=[NgramRule(2)])[0]
    big = list(zip(got[:-1], got[1:]))
    assert len(got) == CAP and len(set(big)) == len(big), got
    assert any(t not in ids for t in got)
    assert _run(e, p, slots=[2], rules=[rules], sampling=[sp], ngram=[NgramRule(2)])[0] == got


def test_logprobs_of_an_ngram_row_are_those_of_the_raw_logits(eng, replay):
    _, e = eng
    r = replay
    logits, toks, lps = _static(e, r["prompts"], rules=HOLD, ngram=r["ngram"], lp=[2, None, 2, None])
    assert np.array_equal(toks, r["toks"])                                      # asking for logprobs changes no token
    for b in (0, 2):
        tok_lp, top_ids, top_lp = lps[b]
        for k in range(CAP):
            x = logits[k, b].astype(np.float64)
            ref = x - (x.max() + np.log(np.exp(x - x.max()).sum()))
            order = np.lexsort((np.arange(x.shape[0]), -x))
            # fp32 log-sum-exp against fp64: the bound of tests/test_logprobs_gpu.py.  Raw logits: neither the bias of +1e4 nor a ban shows
            assert abs(float(tok_lp[k]) - ref[int(toks[k, b])]) <= 1e-4 + 1e-5 * abs(ref[int(toks[k, b])]), (b, k)
            assert np.array_equal(top_ids[k, :2], order[:2]), (b, k)
            assert np.all(np.abs(top_lp[k, :2].astype(np.float64) - ref[order[:2]]) <= 1e-4 + 1e-5 * np.abs(ref[order[:2]])), (b, k)


# ---------------------------------------------------------------------------------------------------- modeling.generate

@pytest.mark.parametrize("continuous", [False, True])
def test_generate_routes_the_rule_to_its_rows(continuous):
    from dots_ocr_amd.modeling import DotsOcrHipForCausalLM
    cfg = DotsConfig.tiny(layers=2, v_layers=2)
    model = DotsOcrHipForCausalLM(cfg, random_state_dict(cfg, seed=1), device=0, max_batch=2, max_seq_len=256, max_patches=256)
    g = torch.Generator().manual_seed(4)
    ids = torch.randint(0, cfg.vocab_size - 8, (2, 9), generator=g)
    T, n = ids.shape[1], 16
    a, b = 21, 400
    kw = dict(max_new_tokens=n, eos_token_id=[], continuous=continuous, logit_bias={a: 1e4, b: 1e4})
    free = model.generate(input_ids=ids, **kw)[:, T:].tolist()
    assert all(len(r) == n and set(r) <= {a, b} for r in free)
    got = model.generate(input_ids=ids, no_repeat_ngram_size=2, **kw)[:, T:].tolist()
    for r in got:
        big = list(zip(r[:-1], r[1:]))
        assert len(r) == n and len(set(big)) == len(big), r
    white = model.generate(input_ids=ids, no_repeat_ngram_size=2, no_repeat_ngram_whitelist=[a, b], **kw)[:, T:].tolist()
    assert white == free                                                        # everything the rule could ban is whitelisted
    win = model.generate(input_ids=ids, no_repeat_ngram_size=2, no_repeat_ngram_window=4, **kw)[:, T:].tolist()
    for r in win:
        assert all(r[k] not in banned_ngram_ids(r[:k], 2, 4) for k in range(n)), r
    with pytest.raises(ValueError):
        model.generate(input_ids=ids, no_repeat_ngram_size=3, no_repeat_ngram_window=2, **kw)
    assert model.generate(input_ids=ids, **kw)[:, T:].tolist() == free          # the rows were cleared
    model.engine.close()
