"""The matmul probes (matmul_probes.py) without a GPU.  For every probe configuration test_matmul_probes_gpu.py runs:
  (a) the exactness bounds and the shares of outputs that exercise the rounding hold;
  (b) the oracle's own emulated path (om.linear + om._r, om.rms_norm, om.quantize_rows_fp8) reproduces the expected BITS: the expectation is
      pinned to the reference, not to a kernel;
  (c) every applicable mutant (the reference with one defect) breaks the rule in EVERY block of 16 rows x 16 columns — or, where that
      cannot hold (a swapped pair of rows, the `eps` mutants on rows without a visible eps), in every block that is named.
The probes' rows are independent draws, so (c) is judged on a 49-row prefix (three row blocks and a ragged tail; blocks(): the last row
block is aligned to the end) of the widest M / B the GPU test runs, (a) on all of it.  Run with -s for the tables.

test_the_gap_...: the four precision-path defects pass test_kernels_gpu.py::test_gemm's own inputs and close() — the reason for this file.
"""
import math

import numpy as np
import pytest
import torch

import matmul_probes as mp
from oracle import model as om

MUT_ROWS = 49


def _dq(w):
    q, s = om.quantize_rows_fp8(w)
    return q * s[:, None]


def _table(title, rows):
    print(f"\n{title}")
    for name, seen, looked, n_bad in rows:
        print(f"  {name:58s} blocks {seen:5d} / {looked:5d}   elements {n_bad}")


def _mutant_rows(p, configs, M):
    rows = []
    for epi, bias, inplace in configs:
        want = mp.evaluate(p, epi, M=M, bias=bias, inplace=inplace)
        for name, (d, r, c) in mp.dense_mutants(p, epi, M, bias=bias, inplace=inplace).items():
            bad = mp.wrong(mp.evaluate(p, epi, M=M, bias=bias, inplace=inplace, d=d), want)
            seen, looked = mp.blocks(bad, r, c)
            rows.append((f"{epi}{'+bias' if bias else ''}{' in place' if inplace else ''}: {name}", seen, looked, int(bad.sum())))
    return rows


def _assert_all_seen(rows, what):
    missed = [r for r in rows if r[1] != r[2] or r[2] == 0]
    assert not missed, f"{what}: mutants not seen in every (named) block: {missed}"


def _shares(v):
    return float(mp.not_bf16(v).double().mean()), float((mp.is_tie(v) & (v.abs() < 256)).double().mean())


# ------------------------------------------------------------------------------------------------ bf16 GEMM
@pytest.mark.parametrize("K", mp.GEMM_K)
@pytest.mark.parametrize("N", mp.GEMM_N)
def test_gemm_probe(N, K):
    M = max(mp.GEMM_M)
    p = mp.dense(M, N, K)
    assert p.bound < mp.LIMIT
    for epi in ("none", "residual"):
        v = mp.pre_rounding(p, epi)
        nb, tie = _shares(v)
        assert nb >= 0.01 and tie >= 0.001, (epi, nb, tie)                  # the rounding is exercised, ties (n + 1/2 at ulp 1) included
        print(f"\ngemm {M}x{N}x{K} {epi}: r {p.r}, sum|a||w| {p.bound:.0f}, max |v| {float(v.abs().max())}, not bf16 {nb:.3f}, ties at ulp 1 {tie:.4f}", end="")
    # (b) the oracle's emulated path gives the expected bits
    y = om.linear(p.A.float(), p.W.float(), p.bias_bf.float())
    assert torch.equal(mp.bits(om._r(y, True).bfloat16()), mp.bits(mp.evaluate(p, "none", check=True)))
    assert torch.equal(mp.bits(om._r(y + p.R_bf.float(), True).bfloat16()), mp.bits(mp.evaluate(p, "residual", check=True)))
    assert torch.equal(mp.bits(om.linear(p.A.float(), p.W.float())), mp.bits(mp.evaluate(p, "f32", bias=False)))
    # (c)
    rows = _mutant_rows(p, [("none", True, False), ("residual", True, True), ("residual", False, False), ("f32", False, False), ("swiglu", True, False)], MUT_ROWS)
    _table(f"gemm N={N} K={K}", rows)
    _assert_all_seen(rows, f"gemm N={N} K={K}")


@pytest.mark.parametrize("N,K", mp.GEMM_COLSCALE_NK)
def test_gemm_colscale_probe(N, K):
    p = mp.dense(max(mp.GEMM_M), N, K, w8=True)
    q, s = om.quantize_rows_fp8(p.W)                                         # lossless: the scale is the power of two the row was built with
    assert torch.equal(q.double(), p.Wi) and torch.equal(s.double(), p.sw)
    y = om.linear(p.A.float(), _dq(p.W), p.bias_bf.float())
    assert torch.equal(mp.bits(om._r(y + p.R_bf.float(), True).bfloat16()), mp.bits(mp.evaluate(p, "residual", check=True)))
    rows = _mutant_rows(p, [("none", True, False), ("residual", True, False), ("swiglu", True, False)], MUT_ROWS)
    _table(f"gemm + colscale N={N} K={K}", rows)
    _assert_all_seen(rows, "colscale")


@pytest.mark.parametrize("M,N,K", mp.GEMM_FP8)
def test_gemm_fp8_probe(M, N, K):
    p = mp.dense(M, N, K, w8=True, a8=True)
    qa, sa = om.quantize_rows_fp8(p.A)
    assert torch.equal(qa.double(), p.Ai) and torch.equal(sa.double(), p.sa) and float(p.sa[3]) == 1.0 and not p.Ai[3].any()       # the all-zero token: scale 1
    assert (p.Ai.abs().argmax(1)[:3] % 2 == 0).all() and (p.Wi.abs().argmax(1) % 2 == 1).all()                                       # the 448s sit in different k columns
    y = om.linear(p.A.float(), _dq(p.W), p.bias_bf.float(), a8=True)
    assert torch.equal(mp.bits(om._r(y, True).bfloat16()), mp.bits(mp.evaluate(p, "none", check=True)))
    assert torch.equal(mp.bits(om._r(y + p.R_bf.float(), True).bfloat16()), mp.bits(mp.evaluate(p, "residual", check=True)))
    nb, _ = _shares(mp.pre_rounding(p, "none"))
    assert nb >= 0.01
    rows = _mutant_rows(p, [("none", True, False), ("residual", True, False), ("swiglu", True, False)], MUT_ROWS)
    _table(f"fp8 gemm {M}x{N}x{K}", rows)
    zero = [r for r in rows if "row scale" in r[0]]
    assert zero and all(r[1] == r[2] for r in zero)
    _assert_all_seen(rows, "fp8 gemm")


def test_activation_probe_covers_the_range_and_the_rules_hold_for_the_exact_function():
    ap = mp.act_probe()
    x = ap.swiglu.x
    for v in list(range(-30, 31)) + [-100, -88]:
        assert (x == v).any()
    # the exact functions evaluated in fp32 (torch) obey the rules the kernels are held to
    g32, a32 = x.float(), ap.A.float()
    u32 = a32[:, ap.I:]
    assert not mp.wrong(torch.nn.functional.silu(g32) * u32, ap.swiglu).any()
    assert not mp.wrong(torch.nn.functional.gelu(a32), ap.gelu).any()
    # and a silu without the gate (the up value alone), or the tanh form of GELU, does not
    assert mp.wrong(u32, ap.swiglu).any()
    assert mp.wrong(torch.nn.functional.gelu(a32, approximate="tanh"), ap.gelu).any()


# ------------------------------------------------------------------------------------------------ norms
@pytest.mark.parametrize("eps", [mp.EPS_LM, mp.EPS_TOWER])
def test_norm_rows_are_exact_under_the_oracle_and_eps_is_visible(eps):
    c = mp.eps_c(eps)
    ratio = c / math.sqrt(c * c + eps)
    assert mp.boundary_margin(ratio) >= 2.0 ** -12
    if eps == mp.EPS_LM:
        assert c == 2.0 ** -10 and round(ratio * 256) == 179
    for dim in mp.NORM_DIMS:
        nr = mp.norm_rows(max(mp.NORM_ROWS), dim, eps=eps)
        assert min(mp.norm_margins(nr)) >= 2.0 ** -12
        X = mp.norm_image(nr)
        got = om.rms_norm(nr.h.float(), nr.ln_w.float(), eps, True)
        assert torch.equal(got.double(), X), "the oracle's emulated rmsnorm is not the exact image"
        rows = []
        for name, defect in mp.NORM_DEFECTS.items():
            bad = mp.norm_image(nr, defect) != X
            named = None if defect == "neighbour_rstd" else torch.nonzero(nr.is_eps).flatten().tolist()
            assert bad.any(1)[named if named is not None else slice(None)].all(), f"{name}: not visible on every named row"
            seen, looked = mp.blocks(bad, named)
            rows.append((name, seen, looked, int(bad.sum())))
        _table(f"rmsnorm dim={dim} eps={eps}", rows)
        _assert_all_seen(rows, "rmsnorm")


@pytest.mark.parametrize("dim", mp.NORM_DIMS)
def test_layernorm_probe_stays_below_the_cap_of_boundary_elements(dim):
    lp = mp.layernorm_probe(max(mp.NORM_ROWS), dim, 1e-6)
    assert float(lp.nr.h.double().sum(1).abs().max()) == 0.0                   # balanced rows: mean exactly 0
    share = float(lp.near.double().mean())
    assert share < mp.LN_MAX_NEAR, share
    assert float(lp.ref.abs().min()) > 0.25                                    # no cancellation beyond a factor 6 (layernorm_probe)
    got = om.layer_norm(lp.nr.h.float(), lp.w.float(), lp.b.float(), 1e-6, True).bfloat16()
    assert not mp.layernorm_wrong(got, lp).any()
    no_eps = mp.rne_bf16(lp.nr.h.double() / lp.nr.c[:, None] * lp.w.double() + lp.b.double())
    assert mp.layernorm_wrong(no_eps, lp)[lp.nr.is_eps].any(1).all()
    print(f"\nlayernorm dim={dim}: {share:.5f} of the elements within 2^-19 of a rounding boundary")


# ------------------------------------------------------------------------------------------------ decode kernels
@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("N,K", mp.DEC_PROJ_NK)
def test_dec_proj_probe(N, K, fp8):
    B = max(mp.DEC_B)
    p = mp.dense(B, N, K, seed=1, w8=fp8)
    assert p.bound < mp.LIMIT
    v = mp.pre_rounding(p, "residual", bias=False)
    nb, tie = float(mp.not_bf16(v).double().mean()), float(mp.is_tie(v).double().mean())      # no bias, so no n + 1/2: the ties are odd integers above 256
    assert nb >= 0.01 and tie >= 0.001
    w = _dq(p.W) if fp8 else p.W.float()
    ref = om._r(p.R_bf.float() + p.A.float() @ w.t(), True)
    assert torch.equal(mp.bits(ref.bfloat16()), mp.bits(mp.evaluate(p, "residual", bias=False, check=True)))
    rows = _mutant_rows(p, [("residual", False, True)], MUT_ROWS)
    _table(f"dec_proj N={N} K={K} fp8={fp8}", rows)
    _assert_all_seen(rows, "dec_proj")


def _fused_mutants(fp, want_of, rule):
    rows = []
    for name, defect in mp.NORM_DEFECTS.items():
        if defect == "neighbour_rstd" and fp.B < 2:
            continue
        bad = rule(want_of(defect))
        named = None if defect == "neighbour_rstd" else torch.nonzero(fp.nr.is_eps).flatten().tolist()
        seen, looked = mp.blocks(bad, named)
        rows.append((name, seen, looked, int(bad.sum())))
    return rows


@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("H", mp.DEC_LMHEAD_H)
def test_dec_lmhead_probe(H, fp8):
    B, V = max(mp.DEC_B), max(mp.DEC_LMHEAD_V)
    fp = mp.fused_probe(B, H, V, fp8)
    y = mp.fused_output(fp)
    w = _dq(fp.w.W) if fp8 else fp.w.W.float()
    ref = om.linear(om.rms_norm(fp.nr.h.float(), fp.nr.ln_w.float(), mp.EPS_LM, True), w)
    assert torch.equal(mp.bits(ref), mp.bits(y.float())), "the oracle's logits are not the exact values"
    rows = _fused_mutants(fp, lambda d: mp.fused_output(fp, d).float(), lambda m: mp.bits(m) != mp.bits(y.float()))
    bad = mp.bits(mp.rne_bf16(y).float()) != mp.bits(y.float())
    rows.append(("logits rounded to bf16", *mp.blocks(bad), int(bad.sum())))
    _table(f"dec_lmhead H={H} fp8={fp8}", rows)
    _assert_all_seen(rows, "lm_head")


@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("H,Hq,Hkv", mp.DEC_QKV)
def test_dec_qkv_probe(H, Hq, Hkv, fp8):
    B, N = max(mp.DEC_QKV_B), (Hq + 2 * Hkv) * 128
    fp = mp.fused_probe(B, H, N, fp8, with_bias=True)
    y = mp.fused_output(fp)
    nb, _ = _shares(y)
    assert nb >= 0.01
    w = _dq(fp.w.W) if fp8 else fp.w.W.float()
    ref = om._r(om.linear(om.rms_norm(fp.nr.h.float(), fp.nr.ln_w.float(), mp.EPS_LM, True), w, fp.bias_bf.float()), True)
    assert torch.equal(mp.bits(ref.bfloat16()), mp.bits(mp.rne_bf16(y)))
    # position 0: cos = 1 and sin = 0 exactly in the oracle's table too
    cos, sin = om.lm_rope_cos_sin(torch.zeros(1, dtype=torch.int64), 128, 1e6)
    assert bool((cos == 1).all()) and bool((sin == 0).all())
    rows = _fused_mutants(fp, lambda d: mp.rne_bf16(mp.fused_output(fp, d)), lambda m: mp.bits(m) != mp.bits(mp.rne_bf16(y)))
    _table(f"dec_qkv H={H} fp8={fp8}", rows)
    _assert_all_seen(rows, "dec_qkv")


@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("H,I", mp.DEC_GATEUP_HI)
def test_dec_gateup_probe(H, I, fp8):
    B = max(mp.DEC_B)
    gp, up = mp.gateup_reference(B, H, I, fp8)
    want = mp.swiglu_of(mp.fused_output(gp), mp.fused_output(up))
    x = om.rms_norm(gp.nr.h.float(), gp.nr.ln_w.float(), mp.EPS_LM, True)
    wg, wu = (_dq(gp.w.W), _dq(up.w.W)) if fp8 else (gp.w.W.float(), up.w.W.float())
    g32, u32 = x @ wg.t(), x @ wu.t()
    assert torch.equal(g32.double(), want.x) and torch.equal(u32.double(), mp.fused_output(up))
    assert not mp.wrong(om._r(torch.nn.functional.silu(g32) * u32, True).bfloat16(), want).any()
    rows = _fused_mutants(gp, lambda d: mp.rne_bf16(mp.swiglu_of(mp.fused_output(gp, d), mp.fused_output(up, d)).ref), lambda m: mp.wrong(m, want))
    _table(f"dec_gateup H={H} I={I} fp8={fp8}", rows)
    _assert_all_seen(rows, "gate|up")


# ------------------------------------------------------------------------------------------------ rope
@pytest.mark.parametrize("two_d", [False, True])
def test_rope_tolerance_holds_the_oracle_and_sees_the_mutants(two_d):
    rp = mp.rope_probe(two_d)
    T, Hq = rp.T, rp.Hq
    if not two_d:
        assert set(mp.ROPE_POS_1D) <= set(rp.pos.tolist())
    else:
        assert rp.pos.max() == 238 and [238, 238] in rp.pos.tolist()
    x = rp.qkv[:, :Hq * 128].view(T, Hq, 128)
    ref, tol = mp.rope_reference(x, rp.pos, rp.base, two_d)
    # the oracle's table (torch fp32 cos / sin of the fp32 product), emulated roundings
    pos = torch.from_numpy(rp.pos.astype(np.int64))
    if two_d:
        inv = 1.0 / (rp.base ** (torch.arange(0, 64, 2, dtype=torch.float) / 64))
        fr = (pos.float().unsqueeze(-1) * inv).flatten(1)
        emb = torch.cat([fr, fr], -1)
        cos, sin = emb.cos(), emb.sin()
    else:
        cos, sin = om.lm_rope_cos_sin(pos, 128, rp.base)
    xf = x.float()
    got = om._r(xf * cos.unsqueeze(1) + om.rotate_half(xf) * sin.unsqueeze(1), True).double()
    worst = float(((got - mp.rne_bf16(ref).double()).abs() / tol).max())
    print(f"\nrope two_d={two_d}: the emulated oracle at {worst:.3f} of the tolerance")
    assert worst <= 1.0
    for name, d in mp.ROPE_MUTANTS.items():
        if name == "2-D h and w swapped" and not two_d:
            continue
        if name == "position truncated to 16 bits" and two_d:
            continue
        mut, _ = mp.rope_reference(x, rp.pos, rp.base, two_d, d)
        out = ((mp.rne_bf16(mut).double() - mp.rne_bf16(ref).double()).abs() > tol).flatten(1).any(1).numpy()
        rows = mp.mutant_rows(rp, name)
        assert len(rows) and out[rows].all(), f"{name}: inside the tolerance on rows {rows[~out[rows]]}"
        print(f"  {name:40s} outside the tolerance on {int(out.sum())} of {T} rows (required on {len(rows)})")


def test_qkv_proj_probe_positions_zero():
    for lens, Hq, Hkv, K in mp.QKV_PROJ:
        T, N = sum(lens), (Hq + 2 * Hkv) * 128
        p = mp.dense(T, N, K, seed=2)
        want = mp.evaluate(p, "none", check=True)
        assert torch.equal(mp.bits(om._r(om.linear(p.A.float(), p.W.float(), p.bias_bf.float()), True).bfloat16()), mp.bits(want))
        v = want[:, (Hq + Hkv) * 128:].view(T, Hkv, 128)
        vt = mp.vt_reference(v, list(lens))
        assert vt.shape == (Hkv, 128, sum((n + 63) // 64 * 64 for n in lens))


# ------------------------------------------------------------------------------------------------ the gap this file closes
def _close_bad(got, ref, rel=2 ** -7, abs_=1e-3):
    got, ref = got.float(), ref.float()
    return (got - ref).abs() > rel * ref.abs() + abs_ * max(1.0, float(ref.abs().max()))


@pytest.mark.parametrize("M,N,K", [(300, 256, 128), (129, 1536, 1536), (40, 1536, 8960)])
def test_the_gap_precision_path_defects_pass_the_randn_tolerance_check(M, N, K):
    """test_kernels_gpu.py::test_gemm / test_decode_kernels_gpu.py::test_dec_proj_residual on their own randn inputs: the reference with ONE
    precision-path defect stays inside close() (2^-7 |ref| + 1e-3 max|ref|) although up to half of its output bits are wrong."""
    g = torch.Generator().manual_seed(M * 7 + N + 1)
    A = torch.randn(M, K, generator=g).bfloat16().double()
    W = (torch.randn(N, K, generator=g) / math.sqrt(K)).bfloat16().double()
    bias = torch.randn(N, generator=g).bfloat16().double()
    R = torch.randn(M, N, generator=g).bfloat16().double()
    acc = A @ W.t()
    ref = mp.rne_bf16(acc + bias + R)
    q = K // 4
    mutants = {
        "fp32 -> bf16 by truncation": mp.trunc_bf16(acc + bias + R),
        "K-quarter partial sums stored as bf16": mp.rne_bf16(sum(mp.rne_bf16(A[:, i * q:(i + 1) * q] @ W[:, i * q:(i + 1) * q].t()).double() for i in range(4)) + bias + R),
        "accumulator rounded to bf16 before bias / residual": mp.rne_bf16(mp.rne_bf16(acc).double() + bias + R),
        "bias added, rounded, then residual": mp.rne_bf16(mp.rne_bf16(acc + bias).double() + R),
    }
    print(f"\n{M}x{N}x{K}: defect, elements outside close(), share of elements with wrong bits")
    for name, out in mutants.items():
        outside, flipped = int(_close_bad(out, ref).sum()), float((mp.bits(out) != mp.bits(ref)).double().mean())
        print(f"  {name:52s} {outside:6d} of {ref.numel()}   {flipped:.3f}")
        assert outside <= 1e-4 * ref.numel() and flipped > 0.05, (name, outside, flipped)
    dropped = mp.rne_bf16(acc - A[:, :32] @ W[:, :32].t() + bias + R)
    assert float(_close_bad(dropped, ref).double().mean()) > 0.3                # a dropped k-step IS caught by the old check
