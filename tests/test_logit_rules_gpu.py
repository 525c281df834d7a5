"""Per-request logit rules on the GPU: logit_bias, allowed ids, min_tokens, stop ids, ignore_eos per decode row.

The single-stage entry (Engine.select_tokens_rules) runs at the real vocabulary against a numpy fp64 restatement of the contract on
planted logits whose deciding margins are >= 0.5 (far above fp32 rounding: the chosen token must be equal, not close); the tiny engine
checks the decode loop: per-row stops, min_tokens, ignore_eos, invariance over slot and batch, rules switched between captured chunks.
The engine exposes no count of captured graphs, so the switch test asserts on results only."""
import math

import numpy as np
import pytest
import torch

from dots_ocr_amd.config import DotsConfig
from dots_ocr_amd.engine import DotsEngineError, LogitRules, SamplingParams
from dots_ocr_amd.weights import random_state_dict

pytestmark = pytest.mark.gpu

V = 151936
EOS = [151643, 151673]                     # engine EOS ids of the stage tests (any ids inside the vocabulary)


@pytest.fixture(scope="module")
def eng():
    from dots_ocr_amd.engine import Engine
    cfg = DotsConfig.tiny(layers=3, v_layers=3, vocab=1024)
    e = Engine(cfg, max_batch=4, max_seq_len=640, max_patches=4096, max_prefill_tokens=2048)
    e.load_state_dict(random_state_dict(cfg, seed=11))
    yield cfg, e
    e.close()


# ---------------------------------------------------------------------------------------------------- helpers (after test_sampling_rows_gpu.py)

def _select(e, logits, params, rules, n_gen, hists, n_prompt):
    B = len(params)
    stride = max(1, max(len(h) for h in hists))
    H = np.full((B, stride), -1, np.int32)
    for b, h in enumerate(hists):
        H[b, :len(h)] = h
    d_l = torch.from_numpy(np.ascontiguousarray(logits, np.float32)).cuda()
    d_h = torch.from_numpy(H).cuda()
    d_n = torch.tensor([len(h) for h in hists], dtype=torch.int32, device="cuda")
    d_p = torch.tensor(n_prompt, dtype=torch.int32, device="cuda")
    out = torch.empty(B, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    e.select_tokens_rules(d_l.data_ptr(), B, V, params, rules, n_gen, d_h.data_ptr(), d_n.data_ptr(), stride, d_p.data_ptr(), out.data_ptr())
    return out.cpu().numpy()


def _shaped(l, rules, n, hist, n_prompt, p):
    """numpy fp64 restatement: l + bias, -inf for banned / not allowed / (n < min_tokens) EOS and stop ids, then the penalties"""
    s = l.astype(np.float64).copy()
    if rules is not None:
        for t, v in rules.bias:
            s[t] += v
        if rules.allowed is not None:
            keep = np.zeros(V, bool)
            keep[list(rules.allowed)] = True
            s[~keep] = -np.inf
        if n < rules.min_tokens:
            s[list(EOS) + list(rules.stop)] = -np.inf
    hist = np.asarray(hist, np.int64)
    c = np.bincount(hist[n_prompt:], minlength=V).astype(np.float64)
    seen = c > 0
    seen[hist[:n_prompt]] = True
    r = p.repetition_penalty
    if r != 1.0:
        s[seen] = np.where(s[seen] > 0, s[seen] / r, s[seen] * r)
    return s - (p.frequency_penalty * c + p.presence_penalty * (c > 0))


def _kept(sh, p):
    """tokens the top-k / top-p filters keep (index array sorted by value) and their probabilities; -inf tokens are never kept"""
    t = sh / p.temperature
    order = np.argsort(-t, kind="stable")
    order = order[np.isfinite(t[order])]
    if p.top_k > 0:
        kth = t[order[min(p.top_k, len(order)) - 1]]
        order = order[t[order] >= kth]
    e = np.exp(t[order] - t[order[0]])
    pr = e / e.sum()
    if p.top_p < 1.0:
        n = int(np.searchsorted(np.cumsum(pr), p.top_p)) + 1
        order, pr = order[:n], pr[:n] / pr[:n].sum()
    return order, pr


def _planted_row(rng, case):
    """(logits, hist, n_prompt, params, rules, n) of one greedy row.  Raw: a = 10 > b = 9 > c = 8 over N(0, 1) noise (max ~ 4.5)."""
    l = rng.normal(0.0, 1.0, V).astype(np.float32)
    a, b, c, d1, d2, d3 = (int(x) for x in rng.choice(V - 2000, 6, replace=False))      # clear of the EOS ids
    l[a], l[b], l[c] = 10.0, 9.0, 8.0
    l[EOS] = -3.0
    prompt = [int(x) for x in rng.integers(0, V - 2000, 40)]
    gen = [int(x) for x in rng.integers(0, V - 2000, 6)]
    p, rules, n = SamplingParams(), None, 6
    if case == "bias_flip":
        rules = LogitRules(bias={b: 2.0, d1: -1.0})                    # 9 + 2 > 10
    elif case == "ban_max":
        rules = LogitRules(bias={a: -math.inf})                         # b = 9 is next
    elif case == "allowed":
        l[d1], l[d2], l[d3] = 6.0, 5.0, 4.5
        rules = LogitRules(allowed=[d1, d2, d3])                        # the top three are outside
    elif case == "order":
        prompt.append(a)
        p = SamplingParams(repetition_penalty=2.0)
        rules = LogitRules(bias={a: 6.0})                               # penalise(10 + 6) = 8 < 9; penalise(10) + 6 = 11 would keep a
    elif case == "tie":
        lo, mid, hi = sorted((d1, d2, d3))
        l[lo], l[mid], l[hi] = 2.0, 6.0, 6.0
        rules = LogitRules(allowed=[lo, mid, hi])                       # equal maxima inside the list: the lowest index
    elif case == "min_below":
        l[EOS[1]] = 12.0
        rules, n = LogitRules(min_tokens=7), 6                          # n < min_tokens: the EOS is -inf, a wins
    elif case == "min_at":
        l[EOS[1]] = 12.0
        rules, n = LogitRules(min_tokens=6), 6                          # n == min_tokens: the EOS is free again
    elif case == "stop_min":
        rules, n = LogitRules(stop=[a, d1], min_tokens=3), 2            # a stop id below min_tokens is -inf too
    elif case == "ban_neg":
        l -= 25.0                                                       # every logit negative: the penalty multiplies
        l[a], l[b], l[c] = -1.0, -2.0, -2.4
        gen += [a, b]
        p = SamplingParams(repetition_penalty=1.5)
        rules = LogitRules(bias={a: -math.inf})                         # -inf * r stays -inf, b -> -3.0: c = -2.4 wins
    elif case == "pen_only":
        gen.append(a)
        p = SamplingParams(presence_penalty=1.5)                        # a row without rules beside the ruled ones: 10 - 1.5 < 9
    return l, prompt + gen, len(prompt), p, rules, n


CASES = ("bias_flip", "ban_max", "allowed", "order", "tie", "min_below", "min_at", "stop_min", "ban_neg", "pen_only", "none")
FLIPS = {"bias_flip", "ban_max", "allowed", "order", "tie", "min_below", "stop_min", "ban_neg", "pen_only"}


def _margin(sh):
    top = np.sort(sh[np.isfinite(sh)])[-2:]
    return top[1] - top[0]


@pytest.mark.parametrize("B", [1, 8, 64])
def test_greedy_rules_match_numpy(eng, B):
    _, e = eng
    e.set_eos(EOS)
    rng = np.random.default_rng(100 + B)
    order = [0, 3, 5] if B == 1 else range(B)              # B = 1: three calls of one row each
    want_flips = flips = 0
    calls = [[k] for k in order] if B == 1 else [list(order)]
    for call in calls:
        names = [CASES[(k + B) % len(CASES)] for k in call]
        rows = [_planted_row(rng, nm) for nm in names]
        L = np.stack([r[0] for r in rows])
        args = ([r[3] for r in rows], [r[4] for r in rows], [r[5] for r in rows], [r[1] for r in rows], [r[2] for r in rows])
        got = _select(e, L, *args)
        for b, (l, hist, n_p, p, rules, n) in enumerate(rows):
            sh = _shaped(l, rules, n, hist, n_p, p)
            if names[b] != "tie":
                assert _margin(sh) >= 0.5, names[b]
            assert got[b] == int(np.argmax(sh)), (b, names[b])             # np.argmax: the lowest index on a tie
            flips += int(np.argmax(sh) != np.argmax(l))
            want_flips += int(names[b] in FLIPS)
            if names[b] == "order":                                        # the other order of bias and penalty picks another token
                wrong = _shaped(l, None, n, hist, n_p, p)
                for t, v in rules.bias:
                    wrong[t] += v
                assert int(np.argmax(wrong)) != int(np.argmax(sh))
        # rows without rules give the parent's answer: the same call through the entry without rules
        plain = [b for b, r in enumerate(rows) if r[4] is None]
        if plain:
            stride = max(len(r[1]) for r in rows)
            H = np.full((len(rows), stride), -1, np.int32)
            for b, r in enumerate(rows):
                H[b, :len(r[1])] = r[1]
            d_l, d_h = torch.from_numpy(L).cuda(), torch.from_numpy(H).cuda()
            d_n = torch.tensor([len(r[1]) for r in rows], dtype=torch.int32, device="cuda")
            d_p = torch.tensor([r[2] for r in rows], dtype=torch.int32, device="cuda")
            out = torch.empty(len(rows), dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            e.select_tokens(d_l.data_ptr(), len(rows), V, args[0], d_h.data_ptr(), d_n.data_ptr(), stride, d_p.data_ptr(), out.data_ptr())
            assert np.array_equal(out.cpu().numpy()[plain], got[plain])
        # top_k = 1 is greedy at any temperature: the shaped values reach the threshold and draw kernels
        p1 = [SamplingParams(temperature=0.8, top_k=1, seed=b, repetition_penalty=r[3].repetition_penalty,
                             frequency_penalty=r[3].frequency_penalty, presence_penalty=r[3].presence_penalty) for b, r in enumerate(rows)]
        got1 = _select(e, L, p1, *args[1:])
        keep = [b for b in range(len(rows)) if names[b] != "tie"]           # top_k keeps ties at the k-th value: both maxima stay
        assert np.array_equal(got1[keep], got[keep])
    assert flips == want_flips and flips >= (2 if B == 1 else B // 2), (flips, want_flips)


def _peaked(rng):
    l = rng.normal(0.0, 1.0, V).astype(np.float32)
    ids = rng.choice(V - 2000, 24, replace=False)
    l[ids] = np.linspace(7.0, 4.5, 24, dtype=np.float32)
    return l, [int(x) for x in ids]


def _sampled_setup(kind):
    rng = np.random.default_rng(31)
    l, ids = _peaked(rng)
    hist = ids[:2] + ids[4:5] + ids[4:5]                                   # prompt: 2 ids; output: ids[4] twice
    if kind == "allowed":                                                  # 40 ids: 14 of the peak, 26 of the noise floor
        others = [int(x) for x in rng.choice(V - 2000, 26, replace=False) if int(x) not in ids]
        rules = LogitRules(allowed=ids[:14] + others, bias={ids[1]: -math.inf, ids[3]: 1.0})
        p0 = SamplingParams(temperature=1.3, repetition_penalty=1.2, frequency_penalty=0.2)
    else:                                                                  # a biased top-k / top-p row
        rules = LogitRules(bias={ids[0]: -math.inf, ids[20]: 3.0, ids[21]: 2.0, ids[2]: -1.0}, min_tokens=5, stop=[ids[1]])
        p0 = SamplingParams(temperature=1.1, top_k=12, presence_penalty=0.3)
        kept, prob = _kept(_shaped(l, rules, 2, hist, 2, p0), p0)
        cum = np.cumsum(prob)
        p0 = SamplingParams(temperature=1.1, top_k=12, presence_penalty=0.3, top_p=float((cum[5] + cum[6]) / 2))   # between two tokens
    return l, hist, rules, p0


@pytest.mark.parametrize("kind", ["allowed", "topk_topp"])
def test_sampled_rows_stay_in_the_kept_set_and_follow_its_softmax(eng, kind):
    import dataclasses
    _, e = eng
    e.set_eos(EOS)
    l, hist, rules, p0 = _sampled_setup(kind)
    sh = _shaped(l, rules, 2, hist, 2, p0)
    kept, prob = _kept(sh, p0)
    assert 2 < len(kept) <= 64
    if kind == "allowed":
        assert set(kept.tolist()) <= set(rules.allowed) and len(kept) == len(rules.allowed) - 1       # one allowed id is banned
    else:
        assert len(kept) == 7 and rules.bias[0][0] not in kept.tolist() and rules.stop[0] not in kept.tolist()
    counts, n = {}, 0
    L = np.tile(l, (64, 1))
    for call in range(47):
        params = [dataclasses.replace(p0, seed=7 + 64 * call + b) for b in range(64)]
        for t in _select(e, L, params, [rules] * 64, None, [hist] * 64, [2] * 64).tolist():
            counts[t] = counts.get(t, 0) + 1
            n += 1
    assert n >= 3000 and set(counts) <= set(int(x) for x in kept), sorted(set(counts) - set(kept.tolist()))
    assert len(counts) > 2
    for t, q in zip(kept.tolist(), prob.tolist()):
        exp, got = q * n, counts.get(t, 0)
        assert abs(got - exp) < 5 * (exp * (1 - q)) ** 0.5 + 3, (t, exp, got)


def test_rules_that_can_never_select_are_refused(eng):
    cfg, e = eng
    e.set_eos([7, 9])
    for bad in (LogitRules(allowed=[cfg.vocab_size]), LogitRules(bias={cfg.vocab_size + 3: 1.0}), LogitRules(stop=[cfg.vocab_size]),
                LogitRules(allowed=[7, 9, 11], stop=[11], min_tokens=2), LogitRules(allowed=[7], min_tokens=1)):
        with pytest.raises(DotsEngineError):
            e.set_row_logit_rules(0, bad)
    e.set_row_logit_rules(0, LogitRules(allowed=[7, 9, 11], stop=[11]))     # fine without min_tokens
    e.set_row_logit_rules(0, None)
    with pytest.raises(DotsEngineError):
        e.set_row_logit_rules(4, LogitRules(min_tokens=1))                  # row out of range
    e.set_eos([])


# ---------------------------------------------------------------------------------------------------- decode loop, tiny engine

CAP = 24


def _prompts(cfg, n=4):
    out = []
    for b in range(n):
        g = np.random.default_rng(900 + b)
        out.append(g.integers(0, cfg.vocab_size - 8, 6 + b).astype(np.int32))
    return out


def _run(e, prompts, slots=None, rules=None, sampling=None, lp=None, eos=(), cap=CAP, chunk=8, switch=None):
    """prefill `prompts` into `slots` and decode to the end: token lists (and logprobs where asked).  switch = (after_steps, slot, rules)"""
    slots = list(range(len(prompts))) if slots is None else slots
    e.set_sampling(0.0, 1.0, 0)
    e.slots_reset()
    e.set_eos(list(eos))
    for i, s in enumerate(slots):
        if rules and rules[i] is not None:
            e.set_row_logit_rules(s, rules[i])
        if sampling and sampling[i] is not None:
            e.set_row_sampling(s, sampling[i])
        if lp and lp[i] is not None:
            e.set_row_logprobs(s, lp[i])
    e.slots_prefill(slots, np.concatenate(prompts), [len(p) for p in prompts], [cap] * len(prompts))
    steps = 0
    while steps < cap:
        e.slots_decode(chunk)
        steps += chunk
        if switch and steps == switch[0]:
            e.set_row_logit_rules(switch[1], switch[2])
    fin, lens = e.slots_poll()
    toks = [e.slot_read(s, int(lens[s])).tolist() for s in slots]
    lps = [e.row_logprobs(s, int(lens[s])) if lp and lp[i] is not None else None for i, s in enumerate(slots)]
    assert all(fin[s] == 1 for s in slots)
    for s in slots:
        e.slot_release(s)
    return toks, lps


def _first_fresh(seq, k0):
    """first position >= k0 whose token did not occur before it"""
    for k in range(k0, len(seq) - 2):
        if seq[k] not in seq[:k]:
            return k
    return None


@pytest.fixture(scope="module")
def free(eng):
    cfg, e = eng
    prompts = _prompts(cfg)
    toks, _ = _run(e, prompts)
    assert all(len(t) == CAP for t in toks)
    return prompts, toks


def test_min_tokens_holds_the_eos_back(eng, free):
    _, e = eng
    prompts, toks = free
    b, k = next((b, _first_fresh(t, 3)) for b, t in enumerate(toks) if _first_fresh(t, 3) is not None and _first_fresh(t, 3) <= 8)
    E = toks[b][k]
    short, _ = _run(e, [prompts[b]], eos=[E])
    assert short[0] == toks[b][:k + 1]                                      # the free run stops at its EOS
    m = k + 7
    got, _ = _run(e, [prompts[b]], eos=[E], rules=[LogitRules(min_tokens=m)])
    assert len(got[0]) >= m and E not in got[0][:m] and got[0][:k] == toks[b][:k]
    assert got[0][k] != toks[b][k]


def test_stop_id_finishes_its_row_only(eng, free):
    _, e = eng
    prompts, toks = free
    r, k = next((b, _first_fresh(t, 5)) for b, t in enumerate(toks) if _first_fresh(t, 5) is not None)
    S = toks[r][k]
    rules = [LogitRules(stop=[S]) if b == r else None for b in range(4)]
    got, _ = _run(e, prompts, rules=rules)
    assert got[r] == toks[r][:k + 1] and got[r][-1] == S
    for b in range(4):
        if b != r:
            assert got[b] == toks[b]                                        # even where a neighbour emits the id S itself
    # static batch, step by step: the neighbours' tokens and dots_get_logits are bitwise those of the free run
    packed, lens = np.concatenate(prompts), np.array([len(p) for p in prompts], np.int32)

    def steps(rule):
        e.set_eos([])
        if rule is not None:
            e.set_row_logit_rules(r, rule)
        try:
            e.prefill(packed, lens)
            out = [(e.get_logits().copy(), e.get_last_tokens().copy())]
            for _ in range(k + 3):
                e.decode_step()
                out.append((e.get_logits().copy(), e.get_last_tokens().copy()))
        finally:
            e.set_row_logit_rules(r, None)
        return out
    a, b_ = steps(None), steps(LogitRules(stop=[S], bias={toks[r][0]: 0.0}))
    others = [b for b in range(4) if b != r]
    for (la, ta), (lb, tb) in zip(a, b_):
        assert np.array_equal(la[others].view(np.uint32), lb[others].view(np.uint32)) and np.array_equal(ta[others], tb[others])
    for i in range(k + 1):                                                   # the ruled row itself: raw logits untouched up to its stop
        assert np.array_equal(a[i][0][r].view(np.uint32), b_[i][0][r].view(np.uint32))


def test_ignore_eos_runs_to_the_cap(eng, free):
    _, e = eng
    prompts, toks = free
    b, k = next((b, _first_fresh(t, 3)) for b, t in enumerate(toks) if _first_fresh(t, 3) is not None)
    E = toks[b][k]
    got, _ = _run(e, [prompts[b], prompts[(b + 1) % 4]], eos=[E], rules=[LogitRules(ignore_eos=True), None])
    assert got[0] == toks[b] and len(got[0]) == CAP
    other = toks[(b + 1) % 4]
    assert got[1] == (other[:other.index(E) + 1] if E in other else other)
    got, _ = _run(e, [prompts[b]], eos=[E], rules=[LogitRules(ignore_eos=True, stop=[toks[b][k + 1]])])
    assert got[0] == toks[b][:toks[b].index(toks[b][k + 1]) + 1]            # its own stop ids still end it


def test_ruled_request_is_the_same_alone_in_a_batch_and_in_any_slot(eng, free):
    cfg, e = eng
    prompts, toks = free
    g = np.random.default_rng(5)
    allowed = sorted(int(x) for x in g.choice(cfg.vocab_size - 8, 60, replace=False))
    rules = LogitRules(allowed=allowed, bias={allowed[0]: -math.inf, allowed[1]: 1.5, allowed[2]: -0.7}, min_tokens=4, stop=[allowed[3]])
    sp = SamplingParams(temperature=0.9, top_k=20, top_p=0.9, repetition_penalty=1.1, seed=17)
    alone, lp_a = _run(e, [prompts[1]], slots=[0], rules=[rules], sampling=[sp], lp=[3])
    other, lp_o = _run(e, [prompts[1]], slots=[3], rules=[rules], sampling=[sp], lp=[3])
    full, lp_f = _run(e, [prompts[0], prompts[2], prompts[1], prompts[3]], rules=[None, LogitRules(min_tokens=2), rules, None],
                      sampling=[None, None, sp, SamplingParams(temperature=0.7, seed=3)], lp=[None, None, 3, None])
    assert alone[0] == other[0] == full[2]
    assert set(alone[0]) <= set(allowed) - {allowed[0]} and len(set(alone[0])) > 2
    assert allowed[3] not in alone[0][:4]
    for x, y in ((lp_a[0], lp_o[0]), (lp_a[0], lp_f[2])):
        for u, v in zip(x, y):
            assert np.array_equal(u.view(np.uint32) if u.dtype == np.float32 else u, v.view(np.uint32) if v.dtype == np.float32 else v)
    assert full[0] == toks[0]                                               # a greedy row without rules beside them: the free run


def test_rules_switched_between_captured_chunks(eng, free):
    cfg, e = eng
    prompts, toks = free
    g = np.random.default_rng(6)
    ids = [int(x) for x in g.choice(cfg.vocab_size - 8, 40, replace=False)]
    A, B_ = LogitRules(allowed=ids[:20]), LogitRules(allowed=ids[20:])
    got, _ = _run(e, [prompts[0], prompts[1]], rules=[A, None], switch=(8, 0, B_))
    assert set(got[0][:9]) <= set(ids[:20]) and set(got[0][9:]) <= set(ids[20:]) and len(got[0]) == CAP
    assert got[1] == toks[1]
    same, _ = _run(e, [prompts[0], prompts[1]], rules=[A, None], switch=(8, 0, A))
    assert same[0][:9] == got[0][:9] and set(same[0]) <= set(ids[:20])
    off, _ = _run(e, [prompts[0], prompts[1]], rules=[A, None], switch=(8, 0, None))      # NULL clears mid-run
    assert off[0][:9] == got[0][:9] and not set(off[0][9:]) <= set(ids[:20])


def test_slot_release_clears_the_rules(eng, free):
    cfg, e = eng
    prompts, toks = free
    ruled, _ = _run(e, [prompts[2]], slots=[1], rules=[LogitRules(allowed=[3, 4, 5], ignore_eos=True)])
    assert set(ruled[0]) <= {3, 4, 5}
    # _run released slot 1 (no reset in between): its next occupant carries no rules
    e.slots_prefill([1], prompts[2], [len(prompts[2])], [CAP])
    e.slots_decode(CAP)
    _, lens = e.slots_poll()
    assert e.slot_read(1, int(lens[1])).tolist() == toks[2]
    e.slot_release(1)


@pytest.mark.parametrize("sp", [None, SamplingParams(temperature=0.8, top_k=5, top_p=0.9, repetition_penalty=1.2, seed=3),
                                SamplingParams(temperature=1.2, seed=4)], ids=["greedy", "topk_topp", "plain_draw"])
def test_all_masked_row_commits_the_lowest_index(eng, free, sp):
    """The EOS ids changed after the rules were accepted: every allowed id is -inf below min_tokens.  Memory-safe: id 0 is committed,
    by the arg max and by the sampled path alike (m = -inf, every tempered value NaN: no weight, the fallback is the arg max)."""
    cfg, e = eng
    prompts, _ = free
    e.set_sampling(0.0, 1.0, 0)
    e.slots_reset()
    e.set_eos([])
    e.set_row_logit_rules(0, LogitRules(allowed=[40, 41], min_tokens=3))
    if sp is not None:
        e.set_row_sampling(0, sp)
    e.set_eos([40, 41])
    e.slots_prefill([0], prompts[0], [len(prompts[0])], [8])
    e.slots_decode(8)
    _, lens = e.slots_poll()
    got = e.slot_read(0, int(lens[0])).tolist()
    e.slot_release(0)
    e.set_eos([])
    assert got[:3] == [0, 0, 0] and got[3] in (40, 41) and len(got) == 4


# ---------------------------------------------------------------------------------------------------- modeling.generate

@pytest.mark.parametrize("continuous", [False, True])
def test_generate_routes_the_rules_to_its_rows(continuous):
    from dots_ocr_amd.modeling import DotsOcrHipForCausalLM
    cfg = DotsConfig.tiny(layers=2, v_layers=2)
    model = DotsOcrHipForCausalLM(cfg, random_state_dict(cfg, seed=1), device=0, max_batch=2, max_seq_len=256, max_patches=256)
    g = torch.Generator().manual_seed(4)
    ids = torch.randint(0, cfg.vocab_size - 8, (2, 9), generator=g)
    T, n, pad = ids.shape[1], 12, cfg.pad_token_id
    kw = dict(max_new_tokens=n, eos_token_id=[], continuous=continuous)
    free = model.generate(input_ids=ids, **kw)[:, T:].tolist()
    assert all(len(r) == n for r in free)
    k = next(k for k in range(2, n - 1) if free[0][k] not in free[0][:k] and free[0][k] not in free[1] and free[0][k] != pad)
    S = free[0][k]
    got = model.generate(input_ids=ids, stop_token_ids=[S], **kw)[:, T:].tolist()
    assert got[0][:k + 1] == free[0][:k + 1] and all(t == pad for t in got[0][k + 1:])     # row 0 ends at its stop id, kept as its last token
    assert got[1] == free[1]
    ban = model.generate(input_ids=ids, logit_bias={free[0][0]: -math.inf, free[1][0]: -100.0}, **kw)[:, T:].tolist()
    assert ban[0][0] != free[0][0] and ban[1][0] != free[1][0] and free[0][0] not in ban[0]
    allowed = sorted({3, 4, 5, 6, 7})
    only = model.generate(input_ids=ids, allowed_token_ids=allowed, do_sample=True, temperature=1.0, seed=5, **kw)[:, T:].tolist()
    assert all(set(r) <= set(allowed) for r in only)
    j = next(j for j in range(1, 5) if free[1][j] not in free[1][:j] and free[1][j] != pad)
    E = free[1][j]                                            # an EOS that ends row 1 after j + 1 tokens ...
    kw["eos_token_id"] = [E]
    short = model.generate(input_ids=ids, **kw)[:, T:].tolist()
    assert short[1][:j + 1] == free[1][:j + 1] and all(t == pad for t in short[1][j + 1:])
    held = model.generate(input_ids=ids, min_tokens=j + 5, **kw)[:, T:].tolist()          # ... is held back by min_tokens
    assert E not in held[1][:j + 5] and held[1][:j] == free[1][:j]
    with pytest.raises(Exception):                            # never selectable against THIS call's EOS ids
        model.generate(input_ids=ids, allowed_token_ids=[E], min_tokens=2, **kw)
    again = model.generate(input_ids=ids, max_new_tokens=n, eos_token_id=[], continuous=continuous)[:, T:].tolist()
    assert again == free                                      # the rows were cleared
    model.engine.close()
