"""The per-row selection stage held to its definition: on the cases of tests/sampling_reference.py EVERY token that
select_thresh_kernel / select_rows_kernel draw must be one the numpy / Python-int model accepts for that seed and counter — the kept set is
exact in the keys, the draw is within DELTA = 2^-16 of the mass (the device exp).  test_sampling_exact_cpu.py shows without a GPU that the
cases decide and that a kept set wrong by one key group would fail here.  Then the decode loop on the tiny engine (which counter n and
which slot the real step feeds the draw) and the engine-wide sampler (sample_step_kernel, top_p = 1, STEP_DELTA = 2^-12).

Every test prints the largest distance by which a drawn token's u lay outside the token's own interval of the reference CDF, as a
fraction of the tolerance, and the smallest distance between a u and the nearer edge of the interval it was drawn in: measured, not
asserted (DESIGN §6.1 *Tests* records both)."""
import numpy as np
import pytest
import torch

import sampling_reference as sr
from dots_ocr_amd.config import DotsConfig
from dots_ocr_amd.engine import SamplingParams
from dots_ocr_amd.weights import random_state_dict

pytestmark = pytest.mark.gpu

CASES = {c.name: c for c in sr.cases()}
STEPS = 16


@pytest.fixture(scope="module")
def eng():
    from dots_ocr_amd.engine import Engine
    cfg = DotsConfig.tiny(layers=3, v_layers=3, vocab=1024)
    e = Engine(cfg, max_batch=4, max_seq_len=640, max_patches=4096, max_prefill_tokens=2048)
    e.load_state_dict(random_state_dict(cfg, seed=11))
    e.set_eos([])
    yield cfg, e
    e.close()


def _select(e, row, params, hists, n_prompt):
    """one call of the stage: the same logits in every row"""
    B, V = len(params), len(row)
    stride = max(1, max(len(h) for h in hists))
    H = np.full((B, stride), -1, np.int32)
    for b, h in enumerate(hists):
        H[b, :len(h)] = h
    d_l = torch.from_numpy(np.ascontiguousarray(np.tile(row, (B, 1)), np.float32)).cuda()
    d_h = torch.from_numpy(H).cuda()
    d_n = torch.tensor([len(h) for h in hists], dtype=torch.int32, device="cuda")
    d_p = torch.tensor(n_prompt, dtype=torch.int32, device="cuda")
    out = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    e.select_tokens(d_l.data_ptr(), B, V, params, d_h.data_ptr(), d_n.data_ptr(), stride, d_p.data_ptr(), out.data_ptr())
    return out.cpu().numpy()


def _report(what, worst, near, delta):
    print(f"\nsampling-exact {what}: worst distance outside the token's interval {worst:.3e} = {worst / delta:.3f} of the tolerance; "
          f"nearest edge inside it {near:.3e}")


@pytest.mark.parametrize("name", list(CASES))
def test_every_draw_of_the_stage_is_accepted_by_the_definition(eng, name):
    _, e = eng
    c = CASES[name]
    K = c.kept()
    cdf = sr.cdf_of(K.w, K.mask())
    draws = sr.draws()
    prompt = list(c.prompt)
    got = []
    for call in range(4):
        part = draws[64 * call:64 * call + 64]
        params = [SamplingParams(temperature=c.T, top_k=c.top_k, top_p=c.top_p, repetition_penalty=c.repetition_penalty, seed=s) for s, _ in part]
        got += _select(e, c.row, params, [prompt + [c.fill] * n for _, n in part], [len(prompt)] * 64).tolist()
    assert len(got) == sr.DRAWS
    bad, worst, near = [], 0.0, 1.0
    for i, ((seed, n), tok) in enumerate(zip(draws, got)):
        u = sr.row_u(seed, n)
        if tok not in cdf.accepted(u, sr.DELTA).tolist():
            bad.append((i, seed, n, tok, cdf.exact(u), cdf.distance(u, tok)))
        else:
            worst, near = max(worst, cdf.distance(u, tok)), min(near, cdf.margin(u, tok))
    _report(name, worst, near, sr.DELTA)
    assert not bad, (len(bad), bad[:8])
    if len(cdf.idx) >= 2:
        assert len(set(got)) >= 2


def _prompts(cfg, k, n):
    g = np.random.default_rng(900 + k)
    return [g.integers(0, cfg.vocab_size - 8, 9 + 2 * b).astype(np.int32) for b in range(n)]


def _loop(e, prompts, check):
    """prefill, then STEPS - 1 decode steps; check(step, logits [B, V], tokens [B]) at every selected token (the prefill's is step 0)"""
    e.prefill(np.concatenate(prompts), np.array([len(p) for p in prompts], np.int32))
    for step in range(STEPS):
        if step:
            e.decode_step()
        check(step, e.get_logits(), e.get_last_tokens())


@pytest.mark.parametrize("params", [dict(temperature=0.8, top_k=5), dict(temperature=1.3)], ids=["T0.8_k5", "T1.3_unfiltered"])
@pytest.mark.parametrize("rows,row", [(1, 0), (4, 3)], ids=["alone", "slot3_of_4"])
def test_decode_loop_draws_token_n_with_counter_n(eng, params, rows, row):
    cfg, e = eng
    seed = 2 ** 63 + 12345
    p = SamplingParams(seed=seed, **params)
    worst, near, tokens = [0.0], [1.0], []

    def check(step, logits, toks):
        K = sr.kept_set(logits[row], p.temperature, p.top_k, p.top_p)
        cdf = sr.cdf_of(K.w, K.mask())
        u, tok = sr.row_u(seed, step), int(toks[row])
        assert tok in cdf.accepted(u, sr.DELTA).tolist(), (step, tok, cdf.exact(u), cdf.distance(u, tok))
        if p.top_k:
            assert int(K.mask().sum()) >= p.top_k
        worst[0], near[0] = max(worst[0], cdf.distance(u, tok)), min(near[0], cdf.margin(u, tok))
        tokens.append(tok)

    e.set_sampling(0.0, 1.0, 0)
    e.set_row_sampling(row, p)
    try:
        _loop(e, _prompts(cfg, 1, rows), check)
    finally:
        e.set_row_sampling(row, None)
    _report(f"decode loop {params} row {row} of {rows}", worst[0], near[0], sr.DELTA)
    assert len(tokens) == STEPS and len(set(tokens)) >= 2


def test_engine_wide_sampler_draws_from_slot_and_position(eng):
    cfg, e = eng
    T, seed = 0.9, 2 ** 64 - 3
    worst, near, tokens = [0.0], [1.0], []

    def check(step, logits, toks):
        for b in range(2):
            cdf = sr.step_cdf(logits[b], T)
            u, tok = sr.step_u(seed, b, step), int(toks[b])
            assert tok in cdf.accepted(u, sr.STEP_DELTA).tolist(), (b, step, tok, cdf.exact(u), cdf.distance(u, tok))
            worst[0], near[0] = max(worst[0], cdf.distance(u, tok)), min(near[0], cdf.margin(u, tok))
            tokens.append(tok)

    e.set_sampling(T, 1.0, seed)
    try:
        _loop(e, _prompts(cfg, 2, 2), check)
    finally:
        e.set_sampling(0.0, 1.0, 0)
    _report("engine-wide sampler", worst[0], near[0], sr.STEP_DELTA)
    assert len(tokens) == 2 * STEPS and len(set(tokens)) >= 4
