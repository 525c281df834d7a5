"""Exact-integer probes on the GPU (needs an MI355X): every GEMM and decode projection kernel is handed inputs whose right answer is known
exactly (matmul_probes.py) and must return its BITS — RNE_bf16(exact), or the exact fp32 value for EPI_F32 and the lm_head.  No tolerance and
no excluded element, except where the module's docstring of matmul_probes.py derives one: SwiGLU / GELU (one bf16 ulp of the fp64 reference),
rope at positions other than 0, layernorm elements within 2^-19 of a rounding boundary.  test_matmul_probes_cpu.py shows without a GPU that
the expectations are the oracle's and that a table of mutants (truncating conversion, double rounding, bf16 split-K partials, a dropped K
tile, a scale from the neighbouring row, a missing eps, ...) fails these checks in every 16 x 16 output block.

Every output lives in the middle of a larger allocation filled with a sentinel (0x7F7F bf16 / an fp32 NaN pattern), GUARD_ROWS rows of ldc
elements before and after, and the guards must come back untouched: a store past a ragged row tail (M % 256, B % 16, an odd V / 16) would land
there.

Out of scope: the kernels selected by switches that are read once per process (DOTS_OCR_GEMM_LOCKSTEP, DOTS_OCR_GEMM_128, DOTS_OCR_PROJ_REG,
DOTS_OCR_QK_FUSE and the like) cannot be flipped inside one pytest process; the probes reach what the default switches and the two per-call
ones (DOTS_OCR_DEC_WIDE_CUS, DOTS_OCR_DEC_KSPLIT) and dots_set_gemm_plan select.
"""
import functools

import numpy as np
import pytest
import torch

import matmul_probes as mp

pytestmark = pytest.mark.gpu

EPS, THETA = mp.EPS_LM, 1e6


@pytest.fixture(scope="module")
def eng():
    from dots_ocr_amd.config import DotsConfig
    from dots_ocr_amd.engine import Engine
    e = Engine(DotsConfig.tiny(), max_batch=2, max_seq_len=256, max_patches=256, max_prefill_tokens=256)
    yield e
    e.set_gemm_plan(1)                                # the process-wide default
    e.close()


def dev(x):
    return x.cuda().contiguous()


class Guarded:
    """rows x ld outputs in the middle of a sentinel-filled allocation"""

    def __init__(self, rows, ld, f32=False, fill=None, spare=0):
        self.f32, self.rows, self.spare = f32, rows, spare
        self.sent = mp.SENTINEL_F32 if f32 else mp.SENTINEL_BF16
        self.buf = torch.full((rows + spare + 2 * mp.GUARD_ROWS, ld), self.sent, dtype=torch.int32 if f32 else torch.int16, device="cuda")
        self.mid = self.buf[mp.GUARD_ROWS:mp.GUARD_ROWS + rows]
        if fill is not None:
            self.mid.copy_(mp.bits(fill).cuda())
        self.ptr = self.mid.data_ptr()

    def result(self, what=""):
        torch.cuda.synchronize()
        b = self.buf.cpu()
        lo, hi = b[:mp.GUARD_ROWS], b[mp.GUARD_ROWS + self.rows + self.spare:]
        assert bool((lo == self.sent).all()), f"{what}: {int((lo != self.sent).sum())} elements written BEFORE the output"
        assert bool((hi == self.sent).all()), f"{what}: {int((hi != self.sent).sum())} elements written AFTER the output"
        return b[mp.GUARD_ROWS:mp.GUARD_ROWS + self.rows].contiguous().view(torch.float32 if self.f32 else torch.bfloat16)


def check(got, want, what):
    bad = mp.wrong(got, want)
    if bad.any():
        i = torch.nonzero(bad)[0].tolist()
        w = mp.rne_bf16(want.ref) if isinstance(want, mp.NS) else want
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements wrong, {mp.blocks(bad)[0]} of {mp.blocks(bad)[1]} 16 x 16 blocks; "
                             f"first at {i}: got {float(got[tuple(i)])!r}, expected {float(w[tuple(i)])!r}")


@functools.lru_cache(maxsize=2)
def _dense(M, N, K, seed=0, w8=False, a8=False):
    return mp.dense(M, N, K, seed=seed, w8=w8, a8=a8)


def _epi(name):
    from dots_ocr_amd import engine as E
    return {"none": E.EPI_NONE, "residual": E.EPI_RESIDUAL, "swiglu": E.EPI_SWIGLU, "gelu": E.EPI_GELU, "f32": E.EPI_F32}[name]


def _gemm_case(eng, fn, p, A, W, bias, R, M, epi, with_bias, inplace, what, colscale=None):
    ldc = p.N // 2 if epi == "swiglu" else p.N
    out = Guarded(M, ldc, f32=epi == "f32", fill=p.R_bf[:M] if inplace else None)
    r_ptr = out.ptr if inplace else (R.data_ptr() if epi == "residual" else None)
    args = (A.data_ptr(), W.data_ptr(), bias.data_ptr() if with_bias else None, r_ptr, out.ptr, M, p.N, p.K, _epi(epi))
    torch.cuda.synchronize()
    fn(*args, colscale.data_ptr()) if colscale is not None else fn(*args)
    eng.synchronize()
    try:
        check(out.result(what), mp.evaluate(p, epi, M=M, bias=with_bias, inplace=inplace), what)
    except AssertionError as e:                              # every configuration of the loop is run; the failures are reported together
        return [str(e)]
    return []


def _report(failures):
    assert not failures, f"{len(failures)} configurations failed:\n" + "\n".join(failures[:12])


GEMM_CONFIGS = (("none", True, False), ("none", False, False), ("residual", True, False), ("residual", False, True), ("f32", False, False),
                ("f32", True, False), ("swiglu", True, False), ("swiglu", False, False), ("gelu", True, False))


# ------------------------------------------------------------------------------------------------ bf16 GEMM
@pytest.mark.parametrize("plan", [0, 1])
@pytest.mark.parametrize("K", mp.GEMM_K)
@pytest.mark.parametrize("N", mp.GEMM_N)
def test_gemm_returns_the_exact_bits(eng, N, K, plan):
    p = _dense(max(mp.GEMM_M), N, K)
    A, W, bias, R = dev(p.A), dev(p.W), dev(p.bias_bf), dev(p.R_bf)
    eng.set_gemm_plan(plan)
    failures = []
    for M in mp.GEMM_M:
        for epi, with_bias, inplace in GEMM_CONFIGS:
            failures += _gemm_case(eng, eng.op_gemm, p, A, W, bias, R, M, epi, with_bias, inplace, f"gemm plan {plan} {M}x{N}x{K} {epi} bias={with_bias} in place={inplace}")
    _report(failures)


@pytest.mark.parametrize("plan", [0, 1])
@pytest.mark.parametrize("N,K", mp.GEMM_COLSCALE_NK)
def test_gemm_colscale_epilogue_returns_the_exact_bits(eng, N, K, plan):
    """power-of-two scales per weight row (what the e4m3 quantiser gives these rows): a scale from the wrong column is off by a power of two"""
    p = _dense(max(mp.GEMM_M), N, K, 0, True)
    A, W, bias, R, sc = dev(p.A), dev(p.Wq), dev(p.bias_bf), dev(p.R_bf), dev(p.sw.float())
    eng.set_gemm_plan(plan)
    failures = []
    for M in mp.GEMM_M:
        for epi, with_bias in (("none", True), ("residual", True), ("residual", False), ("swiglu", True), ("swiglu", False)):
            failures += _gemm_case(eng, eng.op_gemm, p, A, W, bias, R, M, epi, with_bias, False, f"gemm + colscale plan {plan} {M}x{N}x{K} {epi} bias={with_bias}", colscale=sc)
    _report(failures)


@pytest.mark.parametrize("M,N,K", mp.GEMM_FP8)
def test_gemm_fp8_returns_the_exact_bits(eng, M, N, K):
    """W8A8: per-token and per-channel scales are powers of two and the quantisation lossless; one all-zero token (scale 1)"""
    p = _dense(M, N, K, 0, True, True)
    A, W, bias, R = dev(p.A), dev(p.W), dev(p.bias_bf), dev(p.R_bf)
    failures = []
    for m in sorted({M, 1, 5}):
        for epi, with_bias, inplace in (("none", True, False), ("none", False, False), ("residual", True, False), ("residual", False, True),
                                        ("swiglu", True, False), ("gelu", True, False)):
            failures += _gemm_case(eng, eng.op_gemm_fp8, p, A, W, bias, R, m, epi, with_bias, inplace, f"fp8 gemm {m}x{N}x{K} {epi} bias={with_bias} in place={inplace}")
    _report(failures)


@pytest.mark.parametrize("plan", [0, 1])
def test_swiglu_and_gelu_epilogues_on_exact_integers(eng, plan):
    ap = mp.act_probe()
    eng.set_gemm_plan(plan)
    A, W13, Weye = dev(ap.A), dev(ap.W13), dev(ap.Weye)
    for M in (ap.M, 33):
        out = Guarded(M, ap.I)
        eng.op_gemm(A.data_ptr(), W13.data_ptr(), None, None, out.ptr, M, 2 * ap.I, ap.K, _epi("swiglu"))
        eng.synchronize()
        check(out.result("swiglu"), mp.NS(ref=ap.swiglu.ref[:M], x=ap.swiglu.x[:M], u=ap.swiglu.u[:M], kind="swiglu"), f"swiglu on integers, plan {plan}")
        out = Guarded(M, 2 * ap.I)
        eng.op_gemm(A.data_ptr(), Weye.data_ptr(), None, None, out.ptr, M, 2 * ap.I, ap.K, _epi("gelu"))
        eng.synchronize()
        check(out.result("gelu"), mp.NS(ref=ap.gelu.ref[:M], x=ap.gelu.x[:M], kind="gelu"), f"gelu on integers, plan {plan}")


# ------------------------------------------------------------------------------------------------ qkv + rope epilogue
def _qkv_rope(eng, x, w, b, lens, pos, K, Hq, Hkv, two_d, base, fused):
    """-> q [Hq, T, 128], k [Hkv, T, 128], vt [Hkv, 128, Tpad] (bf16, cpu), all guards checked"""
    T, N = sum(lens), (Hq + 2 * Hkv) * 128
    Tpad = sum((n + 63) // 64 * 64 for n in lens)
    cu = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    ws, q, vt = Guarded(T, N), Guarded(Hq * T, 128), Guarded(Hkv * 128, Tpad)
    k = Guarded(Hkv * T, 128, spare=64)                             # the 64 spare K rows the flash kernel may read belong to the buffer
    torch.cuda.synchronize()
    if x is None:
        eng.op_qkv_rope_split(w.data_ptr(), q.ptr, k.ptr, vt.ptr, cu, pos, Hq, Hkv, two_d, base)
    else:
        eng.op_qkv_proj_rope(x.data_ptr(), w.data_ptr(), b.data_ptr() if b is not None else 0, ws.ptr, q.ptr, k.ptr, vt.ptr, cu, pos, K, Hq, Hkv, two_d, base, fused)
    eng.synchronize()
    ws.result("qkv workspace")
    return q.result("q").view(Hq, T, 128), k.result("k").view(Hkv, T, 128), vt.result("v^T").view(Hkv, 128, Tpad)


@pytest.mark.parametrize("fused", [0, 1])
@pytest.mark.parametrize("lens,Hq,Hkv,K", mp.QKV_PROJ)
def test_qkv_proj_rope_at_position_zero_returns_the_exact_projection(eng, lens, Hq, Hkv, K, fused):
    """cos = 1 and sin = 0 exactly at position 0: the head-major q / k must be the bits of the exact projection, V^T at every position"""
    eng.set_gemm_plan(1)
    T, N = sum(lens), (Hq + 2 * Hkv) * 128
    p = _dense(T, N, K, 2)
    want = mp.evaluate(p, "none")
    x, w, b = dev(p.A), dev(p.W), dev(p.bias_bf)
    for two_d in (False, True):
        pos = np.zeros((T, 2) if two_d else (T,), np.int32)
        q, k, vt = _qkv_rope(eng, x, w, b, list(lens), pos, K, Hq, Hkv, two_d, 10000.0 if two_d else THETA, fused)
        check(q.permute(1, 0, 2).reshape(T, Hq * 128), want[:, :Hq * 128].contiguous(), f"q fused={fused} 2-D={two_d}")
        check(k.permute(1, 0, 2).reshape(T, Hkv * 128), want[:, Hq * 128:(Hq + Hkv) * 128].contiguous(), f"k fused={fused} 2-D={two_d}")
        vref = mp.vt_reference(want[:, (Hq + Hkv) * 128:].reshape(T, Hkv, 128), list(lens))
        assert torch.equal(mp.bits(vt), mp.bits(vref)), f"V^T fused={fused}"


@pytest.mark.parametrize("two_d", [False, True])
def test_prefill_rope_at_the_positions_the_engine_reaches(eng, two_d):
    """1-D positions up to 32766, 2-D up to (238, 238), against the fp64 reference with the derived tolerance (matmul_probes.py: Rope); the split
    kernel on its own, and the GEMM with the rope epilogue (and its unfused twin) behind an identity projection that hands it the same integers"""
    eng.set_gemm_plan(1)
    rp = mp.rope_probe(two_d)
    T, Hq, Hkv = rp.T, rp.Hq, rp.Hkv
    N = (Hq + 2 * Hkv) * 128
    x3 = rp.qkv.view(T, Hq + 2 * Hkv, 128)
    qref, qtol = mp.rope_reference(x3[:, :Hq], rp.pos, rp.base, two_d)
    kref, ktol = mp.rope_reference(x3[:, Hq:Hq + Hkv], rp.pos, rp.base, two_d)
    vref = mp.vt_reference(x3[:, Hq + Hkv:].bfloat16(), rp.lens)
    qkv, eye = dev(rp.qkv.bfloat16()), dev(torch.eye(N).bfloat16())
    for name, args in (("split", (None, qkv, None, 0)), ("gemm + split", (qkv, eye, None, 0)), ("fused", (qkv, eye, None, 1))):
        q, k, vt = _qkv_rope(eng, args[0], args[1], args[2], rp.lens, rp.pos, N, Hq, Hkv, two_d, rp.base, args[3])
        for what, got, ref, tol in (("q", q, qref, qtol), ("k", k, kref, ktol)):
            err = (got.permute(1, 0, 2).double() - mp.rne_bf16(ref).double()).abs()
            worst = float((err / tol).max())
            print(f"rope 2-D={two_d} {name} {what}: {worst:.3f} of the tolerance")
            assert worst <= 1.0, f"{name} {what}: {worst:.2f} x the tolerance at row {int((err / tol).flatten(1).max(1).values.argmax())} (position {rp.pos[int((err / tol).flatten(1).max(1).values.argmax())]})"
        assert torch.equal(mp.bits(vt), mp.bits(vref)), f"{name}: V^T"


# ------------------------------------------------------------------------------------------------ norms
@pytest.mark.parametrize("rows", mp.NORM_ROWS)
@pytest.mark.parametrize("dim", mp.NORM_DIMS)
def test_rmsnorm_returns_the_exact_bits_and_eps_is_in_the_right_place(eng, dim, rows):
    for eps in (mp.EPS_LM, mp.EPS_TOWER):
        nr = mp.norm_rows(rows, dim, eps=eps)
        x, w, y = dev(nr.h), dev(nr.ln_w), Guarded(rows, dim)
        torch.cuda.synchronize()
        eng.op_rmsnorm(x.data_ptr(), w.data_ptr(), y.ptr, rows, dim, eps)
        eng.synchronize()
        check(y.result("rmsnorm"), mp.rne_bf16(mp.norm_image(nr)), f"rmsnorm {rows}x{dim} eps={eps}")


@pytest.mark.parametrize("rows", mp.NORM_ROWS)
@pytest.mark.parametrize("dim", mp.NORM_DIMS)
def test_layernorm_equals_the_rounded_fp64_reference(eng, dim, rows):
    for eps in (1e-6, mp.EPS_TOWER):
        lp = mp.layernorm_probe(rows, dim, eps)
        assert float(lp.near.double().mean()) < mp.LN_MAX_NEAR
        x, w, b, y = dev(lp.nr.h), dev(lp.w), dev(lp.b), Guarded(rows, dim)
        torch.cuda.synchronize()
        eng.op_layernorm(x.data_ptr(), w.data_ptr(), b.data_ptr(), y.ptr, rows, dim, eps)
        eng.synchronize()
        bad = mp.layernorm_wrong(y.result("layernorm"), lp)
        assert not bad.any(), f"layernorm {rows}x{dim} eps={eps}: {int(bad.sum())} of {bad.numel()} elements are not RNE_bf16 of the fp64 reference"


# ------------------------------------------------------------------------------------------------ decode projections
def _env_variants(B, monkeypatch, ksplit=False):
    """the launch shapes the per-call switches select for this batch size"""
    wide = (None, "64") if B > 16 else (None,)
    split = ("0", "2") if (ksplit and B > 32) else (None,)
    for w in wide:
        for s in split:
            for name, v in (("DOTS_OCR_DEC_WIDE_CUS", w), ("DOTS_OCR_DEC_KSPLIT", s)):
                if v is None:
                    monkeypatch.delenv(name, raising=False)
                else:
                    monkeypatch.setenv(name, v)
            yield f"wide_cus={w} ksplit={s}"
    monkeypatch.delenv("DOTS_OCR_DEC_WIDE_CUS", raising=False)
    monkeypatch.delenv("DOTS_OCR_DEC_KSPLIT", raising=False)


@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("N,K", mp.DEC_PROJ_NK)
def test_dec_proj_returns_the_exact_bits(eng, N, K, fp8, monkeypatch):
    p = _dense(max(mp.DEC_B), N, K, 1, fp8)
    x, W = dev(p.A), dev(p.W)
    for B in mp.DEC_B:
        xb = x[:B].contiguous()
        for env in _env_variants(B, monkeypatch, ksplit=True):
            h = Guarded(B, N, fill=p.R_bf[:B])
            torch.cuda.synchronize()
            eng.op_dec_proj(xb.data_ptr(), W.data_ptr(), h.ptr, B, N, K, fp8=fp8)
            eng.synchronize()
            check(h.result("dec_proj"), mp.evaluate(p, "residual", M=B, bias=False, inplace=True), f"dec_proj B={B} N={N} K={K} fp8={fp8} {env}")


@functools.lru_cache(maxsize=1)
def _gateup(H, I, fp8):
    gp, up = mp.gateup_reference(max(mp.DEC_B), H, I, fp8)
    return gp, up, mp.fused_output(gp), mp.fused_output(up)


@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("H,I", mp.DEC_GATEUP_HI)
def test_dec_gateup_is_within_one_ulp_on_the_exact_image(eng, H, I, fp8, monkeypatch):
    gp, up, g, u = _gateup(H, I, fp8)
    h, ln, Wg, Wu = dev(gp.nr.h), dev(gp.nr.ln_w), dev(gp.w.W), dev(up.w.W)
    for B in mp.DEC_B:
        hb = h[:B].contiguous()
        for env in _env_variants(B, monkeypatch):
            out = Guarded(B, I)
            torch.cuda.synchronize()
            eng.op_dec_gateup(hb.data_ptr(), ln.data_ptr(), Wg.data_ptr(), Wu.data_ptr(), out.ptr, B, H, I, EPS, fp8=fp8)
            eng.synchronize()
            check(out.result("gate|up"), mp.swiglu_of(g[:B], u[:B]), f"dec_gateup B={B} H={H} I={I} fp8={fp8} {env}")


@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("V", mp.DEC_LMHEAD_V)
@pytest.mark.parametrize("H", mp.DEC_LMHEAD_H)
def test_dec_lmhead_returns_the_exact_fp32_logits(eng, H, V, fp8, monkeypatch):
    fp = mp.fused_probe(max(mp.DEC_B), H, V, fp8)
    y = mp.fused_output(fp).float()
    h, ln, W = dev(fp.nr.h), dev(fp.nr.ln_w), dev(fp.w.W)
    for B in mp.DEC_B:
        hb = h[:B].contiguous()
        for env in _env_variants(B, monkeypatch):
            out = Guarded(B, V, f32=True)
            torch.cuda.synchronize()
            eng.op_dec_lmhead(hb.data_ptr(), ln.data_ptr(), W.data_ptr(), out.ptr, B, H, V, EPS, fp8=fp8)
            eng.synchronize()
            check(out.result("logits"), y[:B].contiguous(), f"dec_lmhead B={B} H={H} V={V} fp8={fp8} {env}")


def _close(got, ref, what, rel=2 ** -7, abs_=2e-3):
    """test_dec_qkv_norm_proj_bias_rope_and_page_append's tolerance"""
    got, ref = got.float(), ref.float()
    err = (got - ref).abs()
    bad = err > rel * ref.abs() + abs_ * max(1.0, float(ref.abs().max()))
    assert torch.isfinite(got).all() and not bad.any(), f"{what}: max err {err.max():.5f}, {int(bad.sum())} / {bad.numel()} out of tolerance"


@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("H,Hq,Hkv", mp.DEC_QKV)
def test_dec_qkv_exact_projection_page_append_and_rope(eng, H, Hq, Hkv, fp8, monkeypatch):
    """rmsnorm (eps rows included) -> qkv + bias -> rope -> page append.  Rows at position 0: q and the appended K are the bits of the exact
    projection; V bitwise at every position; q / K at the other positions (first and last slot of a page, 32766) to the existing tolerance.
    The pool is sentinel-filled and the page table is not the identity.  Rows that also go through the PREFILL path (the same exact X image, the
    same positions) must give K within one bf16 ulp: both kernels compute sincosf((float) pos * inv_freq), only the fma contraction may differ."""
    Bmax, N = max(mp.DEC_QKV_B), (Hq + 2 * Hkv) * 128
    fp = mp.fused_probe(Bmax, H, N, fp8, with_bias=True)
    y = mp.rne_bf16(mp.fused_output(fp))
    h, ln, W, bias = dev(fp.nr.h), dev(fp.nr.ln_w), dev(fp.w.W), dev(fp.bias_bf)
    max_pages = 512
    for B in mp.DEC_QKV_B:
        positions = mp.dec_positions(B)
        pos = np.asarray(positions, np.int32)
        y3 = y[:B].view(B, Hq + 2 * Hkv, 128)
        qref, _ = mp.rope_reference(y3[:, :Hq].double(), pos, THETA, False)
        kref, _ = mp.rope_reference(y3[:, Hq:Hq + Hkv].double(), pos, THETA, False)
        perm = torch.randperm(B + 3, generator=torch.Generator().manual_seed(B))[:B]                # a page table that is not the identity
        table = torch.zeros((B, max_pages), dtype=torch.int32)
        for b in range(B):
            table[b, positions[b] >> 6] = int(perm[b])
        hb, ctx_d, tab_d = h[:B].contiguous(), dev(torch.from_numpy(pos)), dev(table)
        for env in _env_variants(B, monkeypatch):
            what = f"dec_qkv B={B} H={H} fp8={fp8} {env}"
            pool_d = dev(torch.full((B + 3, Hkv, 2, 8192), mp.SENTINEL_BF16, dtype=torch.int16))
            q_out = Guarded(B, Hq * 128)
            torch.cuda.synchronize()
            eng.op_dec_qkv(hb.data_ptr(), ln.data_ptr(), W.data_ptr(), bias.data_ptr(), ctx_d.data_ptr(), tab_d.data_ptr(), max_pages, pool_d.data_ptr(), q_out.ptr,
                           B, H, Hq, Hkv, EPS, THETA, fp8=fp8)
            eng.synchronize()
            q = q_out.result(what).view(B, Hq, 128)
            got = pool_d.cpu()
            touched = torch.zeros_like(got, dtype=torch.bool)
            k_dec = torch.empty(B, Hkv, 128, dtype=torch.bfloat16)
            for b in range(B):
                pg, key = int(table[b, positions[b] >> 6]), positions[b] & 63
                for hk in range(Hkv):
                    k_dec[b, hk] = got[pg, hk, 0][mp.K_IDX[key]].view(torch.bfloat16)
                    vv = got[pg, hk, 1][mp.V_IDX[key]].view(torch.bfloat16)
                    assert torch.equal(mp.bits(vv), mp.bits(y3[b, Hq + Hkv + hk])), f"{what}: V of row {b} (position {positions[b]})"
                    touched[pg, hk, 0][mp.K_IDX[key]] = True
                    touched[pg, hk, 1][mp.V_IDX[key]] = True
            assert (got[~touched] == mp.SENTINEL_BF16).all(), f"{what}: the append wrote outside the new token's slots"
            zero = [b for b in range(B) if positions[b] == 0]
            check(q[zero].reshape(len(zero), -1), y3[zero, :Hq].reshape(len(zero), -1), f"{what}: q at position 0")
            check(k_dec[zero].reshape(len(zero), -1), y3[zero, Hq:Hq + Hkv].reshape(len(zero), -1), f"{what}: K at position 0")
            _close(q, mp.rne_bf16(qref), f"{what}: q")
            _close(k_dec, mp.rne_bf16(kref), f"{what}: K")
        if B == Bmax and not fp8:
            # the prefill path on the same exact image (the projection alone: x = the X image), same positions
            eng.set_gemm_plan(1)
            xd = dev(mp.rne_bf16(fp.X))
            _, k_pre, _ = _qkv_rope(eng, xd, W, bias, [B], pos, H, Hq, Hkv, False, THETA, 1)
            k_pre = k_pre.permute(1, 0, 2)
            _, ktol = mp.rope_reference(y3[:, Hq:Hq + Hkv].double(), pos, THETA, False)
            ulp = mp.bf16_ulp(mp.rne_bf16(kref).double())
            d_pd = float(((k_pre.double() - k_dec.double()).abs() / ulp).max())
            # against the fp64 reference in units of the derived rope tolerance (one bf16 ulp + the fp32 angle's share): in bf16 ulps of an element
            # the figure means little, x cos + rotate_half(x) sin cancels to a small value under an angle error of theta 2^-22
            d_p, d_d = (float(((k.double() - mp.rne_bf16(kref).double()).abs() / ktol).max()) for k in (k_pre, k_dec))
            print(f"K at the same position, H={H}: prefill vs decode {d_pd:.2f} bf16 ulp; against RNE_bf16(fp64 reference): prefill {d_p:.3f}, decode {d_d:.3f} of the rope tolerance")
            assert d_pd <= 1.0, f"prefill and decode K differ by {d_pd:.2f} bf16 ulps at the same position"
