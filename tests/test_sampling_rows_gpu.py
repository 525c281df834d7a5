"""Per-row token selection on the GPU: penalties, top-k, top-p and seeds per decode row.

The single-kernel entry (Engine.select_tokens) runs at the real vocabulary (151 936: every thread of the stage walks a chunk of
~149 values) against numpy fp64 references on planted logits whose margins are far above fp32 rounding; the tiny engine checks that
the decode loop keeps the same state and that rows without their own parameters are untouched."""
import numpy as np
import pytest
import torch

from dots_ocr_amd.config import DotsConfig
from dots_ocr_amd.engine import SamplingParams
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


def _select(e, logits, params, hists, n_prompt):
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
    e.select_tokens(d_l.data_ptr(), B, V, params, d_h.data_ptr(), d_n.data_ptr(), stride, d_p.data_ptr(), out.data_ptr())
    return out.cpu().numpy()


def _penalised(l, hist, n_prompt, p):
    """numpy fp64 reference of the penalties (repetition first, then frequency / presence on the output counts)"""
    l = l.astype(np.float64).copy()
    hist = np.asarray(hist, np.int64)
    c = np.bincount(hist[n_prompt:], minlength=V).astype(np.float64)
    seen = c > 0
    seen[hist[:n_prompt]] = True
    r = p.repetition_penalty
    if r != 1.0:
        l[seen] = np.where(l[seen] > 0, l[seen] / r, l[seen] * r)
    return l - (p.frequency_penalty * c + p.presence_penalty * (c > 0))


def _kept(pen, p):
    """tokens the top-k / top-p filters keep (numpy, index array sorted by value) and their probabilities"""
    t = pen / p.temperature
    order = np.argsort(-t, kind="stable")
    if p.top_k > 0:
        kth = t[order[p.top_k - 1]]
        order = order[t[order] >= kth]
    e = np.exp(t[order] - t[order[0]])
    pr = e / e.sum()
    if p.top_p < 1.0:
        n = int(np.searchsorted(np.cumsum(pr), p.top_p)) + 1
        order, pr = order[:n], pr[:n] / pr[:n].sum()
    return order, pr


def _planted_row(rng, case):
    """(logits, hist, n_prompt, params) of one greedy row; the penalty flips the choice from token a to token b"""
    l = rng.normal(0.0, 1.0, V).astype(np.float32)
    a, b, c, d = (int(x) for x in rng.choice(V, 4, replace=False))
    l[a], l[b], l[c] = 10.0, 9.0, 8.0
    prompt = [int(x) for x in rng.integers(0, V, 40)]
    gen = [int(x) for x in rng.integers(0, V, 6)]
    p = SamplingParams()
    if case == "rep":
        prompt.append(a)
        p = SamplingParams(repetition_penalty=1.3)                   # 10 / 1.3 < 9
    elif case == "rep_neg":
        l -= 25.0                                                   # every logit negative: the penalty multiplies
        l[a], l[b], l[c] = -1.0, -1.2, -5.0
        gen.append(a)
        p = SamplingParams(repetition_penalty=1.5)                   # -1.5 < -1.2
    elif case == "freq":
        gen += [a, a]
        p = SamplingParams(frequency_penalty=0.8)                    # 10 - 1.6 < 9
    elif case == "pres":
        gen.append(a)
        p = SamplingParams(presence_penalty=1.5)                     # 10 - 1.5 < 9
    elif case == "negative":
        gen += [c, c, c]
        p = SamplingParams(frequency_penalty=-0.8)                   # 8 + 2.4 > 10: a negative penalty promotes c
    elif case == "all":
        prompt.append(b)
        gen += [a, c]
        p = SamplingParams(repetition_penalty=1.2, frequency_penalty=0.5, presence_penalty=0.5)
    elif case == "tie":
        lo, hi = min(a, d), max(a, d)
        l[lo], l[hi] = 11.0, 11.0                                   # equal maxima: the lowest index wins
        gen.append(b)
        p = SamplingParams(presence_penalty=0.25)
    return l, prompt + gen, len(prompt), p


CASES = ("rep", "rep_neg", "freq", "pres", "negative", "all", "tie", "none")


@pytest.mark.parametrize("B", [1, 8, 64])
def test_greedy_penalties_match_numpy(eng, B):
    _, e = eng
    rng = np.random.default_rng(B)
    rows = [_planted_row(rng, CASES[(b + B) % len(CASES)]) for b in range(B)]
    got = _select(e, np.stack([r[0] for r in rows]), [r[3] for r in rows], [r[1] for r in rows], [r[2] for r in rows])
    flips = 0
    for b, (l, hist, n_p, p) in enumerate(rows):
        pen = _penalised(l, hist, n_p, p)
        assert got[b] == int(np.argmax(pen)), (b, CASES[(b + B) % len(CASES)])
        flips += int(np.argmax(pen) != np.argmax(l))
    assert flips >= (1 if B == 1 else B // 2)
    # top_k = 1 is greedy at any temperature
    p1 = [SamplingParams(temperature=0.8, top_k=1, seed=b, repetition_penalty=r[3].repetition_penalty,
                         frequency_penalty=r[3].frequency_penalty, presence_penalty=r[3].presence_penalty) for b, r in enumerate(rows)]
    got1 = _select(e, np.stack([r[0] for r in rows]), p1, [r[1] for r in rows], [r[2] for r in rows])
    plain = [b for b in range(B) if CASES[(b + B) % len(CASES)] != "tie"]      # top_k keeps ties at the k-th value: both maxima stay
    assert np.array_equal(got1[plain], got[plain])


def _peaked(rng):
    l = rng.normal(0.0, 1.0, V).astype(np.float32)
    ids = rng.choice(V, 24, replace=False)
    l[ids] = np.linspace(7.0, 4.5, 24, dtype=np.float32)
    return l, [int(x) for x in ids]


def test_top_k_and_top_p_keep_samples_in_the_nucleus(eng):
    _, e = eng
    rng = np.random.default_rng(5)
    l, ids = _peaked(rng)
    hist = ids[:3] + ids[5:6]
    p0 = SamplingParams(temperature=0.7, top_k=10, top_p=0.8, repetition_penalty=1.1)
    kept, _ = _kept(_penalised(l, hist, 3, p0), p0)
    allowed = set(int(x) for x in kept)
    pen = _penalised(l, hist, 3, p0)
    order = np.argsort(-pen, kind="stable")
    allowed.add(int(order[len(kept)]))                                # +1 for boundary slack
    seen = []
    for call in range(5):
        params = [SamplingParams(temperature=0.7, top_k=10, top_p=0.8, repetition_penalty=1.1, seed=1000 + 64 * call + b) for b in range(64)]
        seen += _select(e, np.tile(l, (64, 1)), params, [hist] * 64, [3] * 64).tolist()
    assert len(seen) >= 300 and set(seen) <= allowed, sorted(set(seen) - allowed)
    assert len(set(seen)) > 2


@pytest.mark.parametrize("top_k", [8, 0])                            # 0: no filter at all (the threshold kernel is skipped)
def test_first_draw_histogram_matches_softmax_of_kept_set(eng, top_k):
    _, e = eng
    rng = np.random.default_rng(9)
    l, ids = _peaked(rng)
    hist = ids[:2] + ids[4:5] + ids[4:5]                              # prompt: 2 ids; output: ids[4] twice
    p0 = SamplingParams(temperature=1.3, top_k=top_k, repetition_penalty=1.2, frequency_penalty=0.2, presence_penalty=0.3)
    kept, prob = _kept(_penalised(l, hist, 2, p0), p0)
    counts = {}
    n = 0
    for call in range(47):
        params = [SamplingParams(temperature=1.3, top_k=top_k, repetition_penalty=1.2, frequency_penalty=0.2, presence_penalty=0.3,
                                 seed=7 + 64 * call + b) for b in range(64)]
        for t in _select(e, np.tile(l, (64, 1)), params, [hist] * 64, [2] * 64).tolist():
            counts[t] = counts.get(t, 0) + 1
            n += 1
    assert n >= 3000 and set(counts) <= set(int(x) for x in kept)
    for t, q in zip(kept.tolist(), prob.tolist()):
        exp, got = q * n, counts.get(t, 0)
        assert abs(got - exp) < 5 * (exp * (1 - q)) ** 0.5 + 3, (t, exp, got)


def test_slot_and_batch_never_enter_the_draw(eng):
    _, e = eng
    rng = np.random.default_rng(21)
    l, ids = _peaked(rng)
    l[ids] = np.linspace(5.0, 4.0, 24, dtype=np.float32)               # flat top: different seeds must give different tokens
    hist = ids[:4] + ids[7:9]
    alone, wide = [], []
    for seed in range(24):
        p = SamplingParams(temperature=1.0, top_p=0.95, top_k=20, presence_penalty=0.4, seed=seed)
        alone.append(int(_select(e, l[None], [p], [hist], [4])[0]))
        others = [_planted_row(rng, "all") for _ in range(64)]
        L = np.stack([o[0] for o in others])
        L[37] = l
        params = [o[3] for o in others]
        params[37] = p
        hists = [o[1] for o in others]
        hists[37] = hist
        nps = [o[2] for o in others]
        nps[37] = 4
        wide.append(int(_select(e, L, params, hists, nps)[37]))
    assert alone == wide
    assert len(set(alone)) > 4


def _req_inputs(cfg, seed, n_text):
    g = torch.Generator().manual_seed(seed)
    grid = np.array([[1, 4, 4]], np.int64)
    pv = torch.randn(16, cfg.vision.patch_dim, generator=g).numpy()
    ids = torch.cat([torch.randint(0, cfg.vocab_size - 8, (3,), generator=g), torch.full((4,), cfg.image_token_id),
                     torch.randint(0, cfg.vocab_size - 8, (n_text,), generator=g)]).numpy().astype(np.int32)
    return ids, pv, grid


def test_continuous_batching_with_mixed_parameters_equals_each_request_alone(eng):
    from dots_ocr_amd.scheduler import ContinuousBatcher, Request
    cfg, e = eng
    e.set_sampling(0.0, 1.0, 0)
    mix = [None, SamplingParams(),
           SamplingParams(repetition_penalty=1.3),
           SamplingParams(temperature=0.9, top_p=0.9, seed=11),
           SamplingParams(temperature=0.5, top_k=20, frequency_penalty=0.3, seed=12),
           SamplingParams(temperature=1.4, top_p=0.7, top_k=50, presence_penalty=0.5, repetition_penalty=1.1, seed=13)]
    caps = [12, 20, 16, 24, 9, 18]
    reqs = [(_req_inputs(cfg, 300 + i, 4 + i), caps[i], mix[i]) for i in range(6)]
    alone = []
    for (ids, pv, grid), cap, sp in reqs:
        alone.append(ContinuousBatcher(e, chunk=4).run([Request(ids, pv, grid, cap, sampling=sp)])[0].tolist())
    got = ContinuousBatcher(e, chunk=4).run([Request(ids, pv, grid, cap, sampling=sp) for (ids, pv, grid), cap, sp in reqs])
    assert [g.tolist() for g in got] == alone


def test_repetition_penalty_end_to_end_against_numpy(eng):
    cfg, e = eng
    e.set_sampling(0.0, 1.0, 0)
    p = SamplingParams(repetition_penalty=1.3)
    checked = flips = 0
    try:
        for k in range(3):
            g = np.random.default_rng(40 + k)
            ids = g.integers(0, cfg.vocab_size - 8, 12).astype(np.int32)
            e.set_row_sampling(0, p)
            e.prefill(ids, np.array([len(ids)], np.int32))
            hist = ids.tolist()
            for step in range(40):
                if step:
                    e.decode_step()
                raw = e.get_logits()[0].astype(np.float64)
                tok = int(e.get_last_tokens()[0])
                Vt = cfg.vocab_size
                seen = np.zeros(Vt, bool)
                seen[hist] = True
                pen = raw.copy()
                pen[seen] = np.where(pen[seen] > 0, pen[seen] / 1.3, pen[seen] * 1.3)
                top2 = np.sort(pen)[-2:]
                if top2[1] - top2[0] >= 1e-4:
                    assert tok == int(np.argmax(pen)), (k, step)
                    checked += 1
                    flips += int(np.argmax(pen) != np.argmax(raw))
                hist.append(tok)
    finally:
        e.set_row_sampling(0, None)
    assert checked >= 16 and flips >= 1, (checked, flips)


def test_rows_without_own_parameters_are_unchanged(eng):
    cfg, e = eng
    prompts = [_req_inputs(cfg, 500 + b, 5 + b)[0] for b in range(4)]
    prompts = [p[p != cfg.image_token_id] for p in prompts]
    packed, lens = np.concatenate(prompts), np.array([len(p) for p in prompts], np.int32)
    e.set_sampling(0.7, 1.0, 5)
    a, la = e.generate(packed, lens, max_new_tokens=24)
    e.prefill(packed, lens)
    logits0 = e.get_logits()
    try:
        e.set_row_sampling(3, SamplingParams(temperature=0.5, top_k=30, repetition_penalty=1.2, seed=9))
        b, lb = e.generate(packed, lens, max_new_tokens=24)
        e.prefill(packed, lens)
        logits1 = e.get_logits()
    finally:
        e.set_row_sampling(3, None)
        e.set_sampling(0.0, 1.0, 0)
    for r in range(3):
        assert la[r] == lb[r] and np.array_equal(a[r, :la[r]], b[r, :lb[r]])
    assert np.array_equal(logits0, logits1)


def test_parameters_changed_mid_run_apply_from_the_next_token(eng):
    cfg, e = eng
    ids = _req_inputs(cfg, 77, 6)[0]
    ids = ids[ids != cfg.image_token_id]
    e.set_sampling(0.0, 1.0, 0)
    e.slots_reset()
    e.set_eos([])
    e.slots_prefill([0], ids, [len(ids)], [40])
    e.slots_decode(11)
    greedy = e.slot_read(0, 64).tolist()
    e.slot_release(0)
    e.set_row_sampling(0, SamplingParams())                        # the per-row stage from the first token on, greedy
    e.slots_prefill([0], ids, [len(ids)], [40])
    e.slots_decode(5)
    e.set_row_sampling(0, SamplingParams(temperature=2.0, seed=3))   # same graph: only the table entry changes
    e.slots_decode(6)
    got = e.slot_read(0, 64).tolist()
    e.slot_release(0)
    assert len(got) == len(greedy) == 12
    assert got[:6] == greedy[:6] and got[6:] != greedy[6:]
