"""Guided decoding on the GPU: regex / choice / JSON-schema guides as device automata.

The single-stage entry (Engine.select_tokens_guided) runs at the real vocabulary over a synthetic token table, with rows at assorted
states of several guides, against the numpy restatement of the contract: host mask (Guide.mask) -> the shaping of §6.3 -> arg max, and
Guide.walk for the next state.  The logits are planted with deciding margins >= 0.5, so a tie cannot decide.  The tiny engine checks the
decode loop: a finite language ends by EOS with a matching text, an unbounded one is a live prefix at its cap — and the same request
without its guide violates the pattern, which is what keeps these tests from passing without the feature."""
import math
import re

import numpy as np
import pytest
import torch

from dots_ocr_amd import guided as G
from dots_ocr_amd.config import DotsConfig
from dots_ocr_amd.engine import DotsEngineError, LogitRules, SamplingParams
from dots_ocr_amd.weights import random_state_dict

pytestmark = pytest.mark.gpu

V = 151936
EOS = [151643, 151673]

PIECES = [b"0", b"1", b"7", b"12", b"345", b"9,", b", ", b"[", b"]", b"{", b"}", b'"', b'":', b'{"', b'"bbox"', b"bbox", b'"category"', b"Text",
          b"Title", b"Table", b'"text"', b"yes", b"no", b"may", b"be", b"ye", b"s", b"-", b".", b"e", b" ", b"\n", b"ab", b"abc", b"a", b"b",
          b"c", "é".encode(), "中".encode(), "中".encode()[:2], "中".encode()[2:], "é".encode()[:1], b"\xa9", b"x", b"hello", b": ", b"],"]


def synthetic_tokens(vocab, seed, special=()):
    """ids 0..255: the single bytes; then seeded concatenations of PIECES (whole and partial UTF-8 sequences among them); every 97th entry
    empty; `special` ids without bytes"""
    rng = np.random.default_rng(seed)
    toks = [bytes([i]) for i in range(256)]
    for i in range(256, vocab):
        if i % 97 == 0:
            toks.append(b"")
        elif i < 256 + len(PIECES):
            toks.append(PIECES[i - 256])
        else:
            toks.append(b"".join(PIECES[int(j)] for j in rng.integers(0, len(PIECES), int(rng.integers(1, 4)))))
    return G.TokenBytes(toks, special)


@pytest.fixture(scope="module")
def big():
    """an engine at the real vocabulary for the stage entry (no weights: the stage runs on caller logits)"""
    from dots_ocr_amd.engine import Engine
    cfg = DotsConfig.tiny(layers=1, v_layers=1, vocab=V)
    e = Engine(cfg, max_batch=1, max_seq_len=128, max_patches=256, max_prefill_tokens=128)
    tb = synthetic_tokens(V, 5, special=EOS)
    guides = {"choice": G.compile_choice(["yes", "no", "maybe"]), "number": G.compile_regex(r"-?[0-9]+(\.[0-9]+)?"),
              "layout": G.compile_json_schema(G.layout_schema()), "abc": G.compile_regex(r"(ab|c)+é?[^a-z]{0,3}")}
    with pytest.raises(DotsEngineError):
        h = e.create_guide(guides["choice"])
        try:
            e.set_row_guide(0, h)                               # before the token bytes: DOTS_E_STATE
        finally:
            e.destroy_guide(h)
    e.set_token_bytes(tb)
    e.set_eos(EOS)
    handles = {k: e.create_guide(g) for k, g in guides.items()}
    yield e, tb, guides, handles
    e.close()


def _select(e, logits, params, rules, n_gen, gids, states, hists, n_prompt):
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
    st = e.select_tokens_guided(d_l.data_ptr(), B, V, params, rules, n_gen, gids, states, d_h.data_ptr(), d_n.data_ptr(), stride, d_p.data_ptr(),
                                out.data_ptr())
    return out.cpu().numpy(), st


def _shaped(l, guide, state, tb, rules, n, hist, n_prompt, p):
    """numpy fp64 restatement: l + bias; -inf for banned / not allowed ids, for ids the guide's mask leaves out (EOS and stop ids: allowed
    iff the state is accepting) and for EOS / stop ids below min_tokens; then the penalties"""
    s = l.astype(np.float64).copy()
    stop = list(rules.stop) if rules is not None else []
    if rules is not None:
        for t, v in rules.bias:
            s[t] += v
        if rules.allowed is not None:
            keep = np.zeros(V, bool)
            keep[list(rules.allowed)] = True
            s[~keep] = -np.inf
    if guide is not None:
        m = guide.mask(state, tb)
        m[EOS + stop] = bool(guide.accepting[state])
        s[~m] = -np.inf
    if rules is not None and n < rules.min_tokens:
        s[EOS + stop] = -np.inf
    hist = np.asarray(hist, np.int64)
    c = np.bincount(hist[n_prompt:], minlength=V).astype(np.float64)
    seen = c > 0
    seen[hist[:n_prompt]] = True
    r = p.repetition_penalty
    if r != 1.0:
        s[seen] = np.where(s[seen] > 0, s[seen] / r, s[seen] * r)
    return s - (p.frequency_penalty * c + p.presence_penalty * (c > 0))


def _state_after(g, text):
    s = g.walk(g.start, text)
    assert s != G.DEAD, text
    return s


# (guide, prefix that leads to the row's state, kind of row)
ROWS = [("choice", b"", "plain"), ("choice", b"ye", "plain"), ("choice", b"yes", "end"), ("choice", b"yes", "end_min"),
        ("number", b"", "plain"), ("number", b"12", "acc_eos"), ("number", b"12", "acc_go"), ("number", b"12.", "eos_masked"),
        ("layout", b"", "plain"), ("layout", b'[{"bbox": [1, 2', "plain"), ("layout", b'[{"bbox": [1, 2, 3, 4], "category": "T', "bias"),
        ("layout", b'[{"bbox": [1, 2, 3, 4], "category": "Text", "text": "a', "pen"), ("layout", b"[]", "end"),
        ("abc", b"ab", "acc_go"), ("abc", "abcé".encode(), "min"), (None, b"", "free"), (None, b"", "free_pen")]


def _planted_row(rng, tb, guides, spec):
    """(logits, hist, n_prompt, params, rules, n, guide name, state) of one greedy row.  An id the guide forbids carries the raw maximum
    12; among the allowed ids a = 9 > b = 8; the EOS ids sit at -3 / -4 unless the row is about them."""
    name, prefix, kind = spec
    g = guides[name] if name else None
    state = _state_after(g, prefix) if g else 0
    l = rng.normal(0.0, 1.0, V).astype(np.float32)
    l[EOS[0]], l[EOS[1]] = -3.0, -4.0                                     # apart: where only the EOS ids are left, no tie decides
    prompt = [int(x) for x in rng.integers(0, V - 2000, 30)]
    gen = [int(x) for x in rng.integers(0, V - 2000, 5)]
    p, rules, n = SamplingParams(), None, 5
    if g is not None:
        m = g.mask(state, tb)
        m[EOS] = False
        ok, bad = np.nonzero(m)[0], np.nonzero(~m)[0]
        bad = bad[bad < V - 2000]
        x = int(rng.choice(bad))
        l[x] = 12.0                                                       # the raw arg max is never allowed
        if kind in ("end", "end_min"):
            assert len(ok) == 0 and g.accepting[state]                    # accepting, no live successor: only the EOS ids are left
            if kind == "end_min":
                rules, n = LogitRules(min_tokens=9), 5                    # ... and min_tokens takes them too: all -inf, id 0
        else:
            assert len(ok) >= 2
            a, b = (int(t) for t in rng.choice(ok, 2, replace=False))
            l[a], l[b] = 9.0, 8.0
            if kind == "acc_eos":
                assert g.accepting[state]
                l[EOS[1]] = 11.0                                          # accepting: the EOS is allowed and wins
            elif kind == "acc_go":
                assert g.accepting[state]                                 # accepting with successors, the EOS low: it goes on
            elif kind == "eos_masked":
                assert not g.accepting[state]
                l[EOS[0]] = 11.0                                          # not accepting: the EOS is -inf whatever its logit
            elif kind == "bias":
                rules = LogitRules(bias={b: 2.0, a: -0.2})                # 8 + 2 > 9 - 0.2: the guide composes with the bias
            elif kind == "pen":
                gen.append(a)
                p = SamplingParams(presence_penalty=1.5)                  # 9 - 1.5 < 8
            elif kind == "min":
                assert g.accepting[state]
                l[EOS[0]] = 11.0
                rules, n = LogitRules(min_tokens=6, stop=[a]), 5          # below min_tokens: the EOS and the stop id a are -inf, b wins
    else:
        a, b = (int(t) for t in rng.choice(V - 2000, 2, replace=False))
        l[a], l[b] = 10.0, 9.0
        if kind == "free_pen":
            gen.append(a)
            p = SamplingParams(presence_penalty=1.5)
    return l, prompt + gen, len(prompt), p, rules, n, name, state


@pytest.mark.parametrize("B", [1, 8, 64])
def test_guided_stage_matches_numpy(big, B):
    e, tb, guides, handles = big
    rng = np.random.default_rng(300 + B)
    calls = [[k] for k in (0, 2, 5, 9, 15)] if B == 1 else [[(k * 5 + B) % len(ROWS) for k in range(B)]]
    flips = 0
    for call in calls:
        rows = [_planted_row(rng, tb, guides, ROWS[k]) for k in call]
        L = np.stack([r[0] for r in rows])
        gids = [handles[r[6]] if r[6] else None for r in rows]
        got, st = _select(e, L, [r[3] for r in rows], [r[4] for r in rows], [r[5] for r in rows], gids, [r[7] for r in rows],
                          [r[1] for r in rows], [r[2] for r in rows])
        for b, (l, hist, n_p, p, rules, n, name, state) in enumerate(rows):
            g = guides[name] if name else None
            kind = ROWS[call[b]][2]
            sh = _shaped(l, g, state, tb, rules, n, hist, n_p, p)
            if kind == "end_min":
                assert not np.isfinite(sh).any() and got[b] == 0 and st[b] == state          # §6.3's fallback; the state does not move
                continue
            fin = np.sort(sh[np.isfinite(sh)])
            assert len(fin) == 1 or fin[-1] - fin[-2] >= 0.5, (b, kind)
            want = int(np.argmax(sh))
            assert got[b] == want, (b, name, kind, got[b], want)
            flips += int(want != int(np.argmax(l)))
            if g is None:
                assert st[b] == -1
            elif want in EOS or (rules is not None and want in rules.stop):
                assert st[b] == state and g.accepting[state]
            else:
                nxt = g.walk(state, tb.token(want))
                assert nxt != G.DEAD and st[b] == nxt, (b, name, kind)
        # the rows without a guide are the parent's rows: the same call through the entry without guides gives their tokens
        plain = [b for b, r in enumerate(rows) if r[6] is None]
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
            e.select_tokens(d_l.data_ptr(), len(rows), V, [r[3] for r in rows], d_h.data_ptr(), d_n.data_ptr(), stride, d_p.data_ptr(), out.data_ptr())
            assert np.array_equal(out.cpu().numpy()[plain], got[plain])
        # top_k = 1 is greedy at any temperature: the shaped values of a guided row reach the threshold and draw kernels
        p1 = [SamplingParams(temperature=0.8, top_k=1, seed=b, presence_penalty=r[3].presence_penalty) for b, r in enumerate(rows)]
        got1, st1 = _select(e, L, p1, [r[4] for r in rows], [r[5] for r in rows], gids, [r[7] for r in rows], [r[1] for r in rows],
                            [r[2] for r in rows])
        assert np.array_equal(got1, got) and np.array_equal(st1, st)
    assert flips >= (3 if B == 1 else B // 2), flips                        # the guide decided: the raw arg max was refused


def test_guide_objects(big):
    e, tb, guides, handles = big
    with pytest.raises(DotsEngineError):
        e.set_row_guide(0, 99)                                              # no such guide
    with pytest.raises(DotsEngineError):
        e.set_row_guide(1, handles["choice"])                               # row out of range (max_batch = 1)
    bad = G.Guide(guides["choice"].table.copy(), guides["choice"].accepting, 0, "bad")
    bad.table[0, 65] = bad.n_states                                         # a transition out of the table
    with pytest.raises(DotsEngineError):
        e.create_guide(bad)
    e.set_row_guide(0, handles["number"])
    assert e.row_guide_state(0) == guides["number"].start
    with pytest.raises(DotsEngineError):
        e.destroy_guide(handles["number"])                                  # held by row 0
    e.set_row_guide(0, handles["abc"])                                      # switching releases the old one
    h2 = e.create_guide(guides["number"])
    e.destroy_guide(h2)
    e.set_row_guide(0, None)
    assert e.row_guide_state(0) == -1


# ---------------------------------------------------------------------------------------------------- decode loop, tiny engine

CAP = 24
E_ID = 1020                                                                  # the tiny engine's EOS id: a special entry, no bytes
FINITE = {"choice": ("choice", ["yes", "no", "maybe"]), "bounded": ("regex", r"[0-9]{2,4}-[a-c]{1,3}")}
OPEN = {"words": ("regex", r"([a-c]+ )*"), "layout": ("json", None)}


def _compile(kind, arg):
    if kind == "choice":
        return G.compile_choice(arg), "|".join(re.escape(c) for c in arg)
    if kind == "regex":
        return G.compile_regex(arg), arg
    schema = G.layout_schema()
    return G.compile_json_schema(schema), G.schema_to_regex(schema)


@pytest.fixture(scope="module")
def eng():
    from dots_ocr_amd.engine import Engine
    cfg = DotsConfig.tiny(layers=3, v_layers=3, vocab=1024)
    e = Engine(cfg, max_batch=4, max_seq_len=640, max_patches=4096, max_prefill_tokens=2048)
    e.load_state_dict(random_state_dict(cfg, seed=11))
    tb = synthetic_tokens(cfg.vocab_size, 9, special=range(cfg.vocab_size - 8, cfg.vocab_size))
    e.set_token_bytes(tb)
    yield cfg, e, tb
    e.close()


def _prompts(cfg, n=4):
    return [np.random.default_rng(900 + b).integers(0, cfg.vocab_size - 8, 6 + b).astype(np.int32) for b in range(n)]


def _text(tb, toks):
    return b"".join(tb.token(t) for t in toks if t != E_ID)


def _run(e, prompts, slots=None, guides=None, sampling=None, rules=None, lp=None, cap=CAP, chunk=8, switch=None, release=True):
    """prefill `prompts` into `slots` and decode to the end.  guides: a handle or None per prompt; switch = (after_steps, slot, handle)"""
    slots = list(range(len(prompts))) if slots is None else slots
    e.set_sampling(0.0, 1.0, 0)
    e.slots_reset()
    e.set_eos([E_ID])
    for i, s in enumerate(slots):
        if guides and guides[i] is not None:
            e.set_row_guide(s, guides[i])
        if sampling and sampling[i] is not None:
            e.set_row_sampling(s, sampling[i])
        if rules and rules[i] is not None:
            e.set_row_logit_rules(s, rules[i])
        if lp and lp[i] is not None:
            e.set_row_logprobs(s, lp[i])
    e.slots_prefill(slots, np.concatenate(prompts), [len(p) for p in prompts], [cap] * len(prompts))
    steps = 0
    while steps < cap:
        e.slots_decode(chunk)
        steps += chunk
        if switch and steps == switch[0]:
            e.set_row_guide(switch[1], switch[2])
    fin, lens = e.slots_poll()
    assert all(fin[s] == 1 for s in slots)
    toks = [e.slot_read(s, int(lens[s])).tolist() for s in slots]
    states = [e.row_guide_state(s) for s in slots]
    lps = [e.row_logprobs(s, int(lens[s])) if lp and lp[i] is not None else None for i, s in enumerate(slots)]
    if release:
        for s in slots:
            e.slot_release(s)
    return toks, states, lps


SAMPLED = SamplingParams(temperature=0.9, top_k=30, top_p=0.95, seed=21)


@pytest.mark.parametrize("sp", [None, SAMPLED], ids=["greedy", "sampled"])
@pytest.mark.parametrize("name", sorted(FINITE))
def test_finite_language_ends_by_eos_with_a_match(eng, name, sp):
    cfg, e, tb = eng
    g, pat = _compile(*FINITE[name])
    prompts = _prompts(cfg)
    h = e.create_guide(g)
    try:
        toks, states, _ = _run(e, prompts[:2], guides=[h, h], sampling=[sp, sp])
    finally:
        e.slots_reset()
        e.destroy_guide(h)
    for t in toks:
        assert t[-1] == E_ID and len(t) < CAP, t                            # finished by the EOS id, not by the cap
        text = _text(tb, t).decode()
        assert re.fullmatch(pat, text), text
        assert g.matches(text.encode())
    free, _, _ = _run(e, prompts[:2], sampling=[sp, sp])                     # the same request without its guide violates the pattern
    for t in free:
        assert not g.matches(_text(tb, t)), t


@pytest.mark.parametrize("sp", [None, SAMPLED], ids=["greedy", "sampled"])
@pytest.mark.parametrize("name", sorted(OPEN))
def test_unbounded_language_is_a_live_prefix_at_its_cap(eng, name, sp):
    cfg, e, tb = eng
    g, _ = _compile(*OPEN[name])
    prompts = _prompts(cfg)
    h = e.create_guide(g)
    try:
        # "words" has no state without a successor, so min_tokens can hold the EOS back to the cap; the layout array can close ("]" leaves
        # only the EOS), so it runs without: a row that closes it ends by EOS with a whole match, any other is cut at the cap
        hold = [LogitRules(min_tokens=CAP)] * 2 if name == "words" else None
        toks, states, _ = _run(e, prompts[:2], guides=[h, h], sampling=[sp, sp], rules=hold, release=False)
    finally:
        e.slots_reset()
        e.destroy_guide(h)
    for t, st in zip(toks, states):
        s = g.walk(g.start, _text(tb, t))
        assert s != G.DEAD and st == s                                       # a prefix of a match, and the device's state is the host's
        if t[-1] == E_ID:
            assert name != "words" and g.accepting[s] and E_ID not in t[:-1]
        else:
            assert len(t) == CAP and E_ID not in t                           # the cap cut the row
    free, _, _ = _run(e, prompts[:2], sampling=[sp, sp])
    for t in free:
        assert g.walk(g.start, _text(tb, t)) == G.DEAD, t


def test_guided_request_is_the_same_alone_in_a_batch_and_in_any_slot(eng):
    cfg, e, tb = eng
    g, _ = _compile(*OPEN["layout"])
    g2 = G.compile_regex(r"[a-c ]*")
    prompts = _prompts(cfg)
    h, h2 = e.create_guide(g), e.create_guide(g2)
    sp = SamplingParams(temperature=0.9, top_k=20, top_p=0.9, repetition_penalty=1.1, seed=17)
    try:
        plain, _, _ = _run(e, prompts)
        alone, _, lp_a = _run(e, [prompts[1]], slots=[0], guides=[h], sampling=[sp], lp=[3])
        other, _, lp_o = _run(e, [prompts[1]], slots=[3], guides=[h], sampling=[sp], lp=[3])
        full, _, lp_f = _run(e, [prompts[0], prompts[2], prompts[1], prompts[3]], guides=[None, h2, h, None],
                             sampling=[None, None, sp, SamplingParams(temperature=0.7, seed=3)], lp=[None, None, 3, None])
        assert alone[0] == other[0] == full[2]
        assert g.walk(g.start, _text(tb, alone[0])) != G.DEAD
        for x, y in ((lp_a[0], lp_o[0]), (lp_a[0], lp_f[2])):
            for u, v in zip(x, y):
                assert np.array_equal(u.view(np.uint32) if u.dtype == np.float32 else u, v.view(np.uint32) if v.dtype == np.float32 else v)
        assert full[0] == plain[0]                                           # a greedy row without a guide beside them: the free run
        # static batch, step by step: the unguided neighbours' tokens and logits are bitwise those of the run without a guided row, and
        # the guided row's logprobs are those of its RAW logits (a token the guide forbids keeps its probability)
        packed, lens = np.concatenate(prompts), np.array([len(p) for p in prompts], np.int32)
        r = 1

        def steps(handle):
            e.set_eos([])
            e.set_row_logprobs(r, 2)
            if handle is not None:
                e.set_row_guide(r, handle)
            try:
                e.prefill(packed, lens)
                out = [(e.get_logits().copy(), e.get_last_tokens().copy())]
                for _ in range(10):
                    e.decode_step()
                    out.append((e.get_logits().copy(), e.get_last_tokens().copy()))
                lp = e.row_logprobs(r, 11)
            finally:
                e.set_row_guide(r, None)
                e.set_row_logprobs(r, None)
            return out, lp
        (a, _), (b_, lp_g) = steps(None), steps(h)
        others = [b for b in range(4) if b != r]
        for (la, ta), (lb, tb_) in zip(a, b_):
            assert np.array_equal(la[others].view(np.uint32), lb[others].view(np.uint32)) and np.array_equal(ta[others], tb_[others])
        assert [int(t[r]) for _, t in a] != [int(t[r]) for _, t in b_]          # the guide did change row r
        for i, (lg, tk) in enumerate(b_):
            raw = lg[r].astype(np.float64)
            ref = raw - (np.log(np.exp(raw - raw.max()).sum()) + raw.max())
            assert abs(float(lp_g[0][i]) - ref[int(tk[r])]) < 1e-3
            assert int(lp_g[1][i][0]) == int(np.argmax(raw))                     # the top entry is the raw arg max, allowed or not
    finally:
        e.slots_reset()
        e.destroy_guide(h)
        e.destroy_guide(h2)


def test_guides_switched_and_cleared_between_captured_chunks(eng):
    cfg, e, tb = eng
    gA, gB = G.compile_regex(r"[a-c]*"), G.compile_regex(r"[0-9]*")
    prompts = _prompts(cfg)
    hA, hB = e.create_guide(gA), e.create_guide(gB)
    hold = [LogitRules(min_tokens=CAP), None]
    try:
        plain, _, _ = _run(e, prompts[:2])
        got, _, _ = _run(e, prompts[:2], guides=[hA, None], rules=hold, switch=(8, 0, hB))
        assert re.fullmatch(rb"[a-c]*", _text(tb, got[0][:9])) and re.fullmatch(rb"[0-9]*", _text(tb, got[0][9:])) and len(got[0]) == CAP
        assert len(_text(tb, got[0][:9])) >= 9 and len(_text(tb, got[0][9:])) >= CAP - 9
        assert got[1] == plain[1]
        off, _, _ = _run(e, prompts[:2], guides=[hA, None], rules=hold, switch=(8, 0, None))          # None clears mid-run
        assert off[0][:9] == got[0][:9] and not re.fullmatch(rb"[a-c]*", _text(tb, off[0][9:]))
        # slot_release clears: the slot's next occupant (no reset in between) is the free run; then the guide can be destroyed
        _run(e, [prompts[1]], slots=[1], guides=[hA])
        e.slots_prefill([1], prompts[1], [len(prompts[1])], [CAP])
        e.slots_decode(CAP)
        _, lens = e.slots_poll()
        assert e.slot_read(1, int(lens[1])).tolist() == plain[1]
        e.slot_release(1)
        # the prefill starts the automaton over: a row left in the middle of a match is at the start state after its next prefill
        e.slots_reset()
        e.set_eos([E_ID])
        e.set_row_guide(0, hB)
        e.set_row_logit_rules(0, LogitRules(min_tokens=4))
        e.slots_prefill([0], prompts[0], [len(prompts[0])], [4])
        e.slots_decode(4)
        first = e.slot_read(0, 4).tolist()
        with pytest.raises(DotsEngineError):
            e.destroy_guide(hB)                                              # held
        e.slot_release(0)
        e.destroy_guide(hB)
        hB = e.create_guide(G.compile_choice(["12", "7"]))                   # a finite guide: a state carried over would not fit it
        e.set_row_guide(0, hB)
        e.slots_prefill([0], prompts[0], [len(prompts[0])], [CAP])
        e.slots_decode(8)
        _, lens = e.slots_poll()
        t = e.slot_read(0, int(lens[0])).tolist()
        assert t[-1] == E_ID and _text(tb, t) in (b"12", b"7") and len(first) == 4
        # ... also when the row keeps its guide from one prefill to the next (a static batch, step by step)
        e.set_eos([])
        e.set_row_guide(0, hA)
        e.prefill(prompts[0], np.array([len(prompts[0])], np.int32))
        for _ in range(3):
            e.decode_step()
        e.prefill(prompts[0], np.array([len(prompts[0])], np.int32))
        assert e.row_guide_state(0) == gA.walk(gA.start, tb.token(int(e.get_last_tokens()[0])))
        e.set_row_guide(0, None)
    finally:
        e.slots_reset()
        e.destroy_guide(hA)
        e.destroy_guide(hB)


# ---------------------------------------------------------------------------------------------------- modeling.generate

@pytest.mark.parametrize("continuous", [False, True])
def test_generate_routes_the_guide_to_its_rows(continuous):
    from dots_ocr_amd.modeling import DotsOcrHipForCausalLM
    cfg = DotsConfig.tiny(layers=2, v_layers=2)
    model = DotsOcrHipForCausalLM(cfg, random_state_dict(cfg, seed=1), device=0, max_batch=2, max_seq_len=256, max_patches=256)
    tb = synthetic_tokens(cfg.vocab_size, 9, special=range(cfg.vocab_size - 8, cfg.vocab_size))
    g = torch.Generator().manual_seed(4)
    ids = torch.randint(0, cfg.vocab_size - 8, (3, 9), generator=g)
    T, n, pad = ids.shape[1], 12, cfg.pad_token_id
    kw = dict(max_new_tokens=n, eos_token_id=[E_ID], continuous=continuous)
    with pytest.raises(ValueError):
        model.generate(input_ids=ids, guided_regex="[0-9]+", **kw)          # no token bytes yet
    model.engine.set_token_bytes(tb)
    free = model.generate(input_ids=ids, **kw)[:, T:].tolist()

    def texts(out):
        return [_text(tb, [t for t in row if t != pad]).decode(errors="replace") for row in out[:, T:].tolist()]
    pat = r"[0-9]{1,3}(, [0-9]{1,3})?"                                      # at most 8 bytes: it ends by EOS inside max_new_tokens
    for kwargs, rx in ((dict(guided_regex=pat), pat), (dict(guided_choice=["yes", "no"]), "yes|no"),
                       (dict(guided_json={"type": "array", "items": {"enum": [1, 22, "x"]}, "maxItems": 2}, guided_whitespace_pattern=""),
                        r'\[((1|22|"x")(,(1|22|"x"))?)?\]')):
        got = texts(model.generate(input_ids=ids, **kwargs, **kw))
        assert all(re.fullmatch(rx, t) for t in got), (kwargs, got)
        assert not any(re.fullmatch(rx, t) for t in texts(model.generate(input_ids=ids, **kw)))
    sampled = texts(model.generate(input_ids=ids, guided_regex=pat, do_sample=True, temperature=1.0, seed=5, **kw))
    assert all(re.fullmatch(pat, t) for t in sampled)
    with pytest.raises(ValueError):
        model.generate(input_ids=ids, guided_regex="a", guided_choice=["a"], **kw)
    assert model.generate(input_ids=ids, **kw)[:, T:].tolist() == free      # the rows were cleared
    model.engine.close()
