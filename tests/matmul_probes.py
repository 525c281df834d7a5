"""Exact-integer probes for the GEMM and decode projection kernels: inputs for which the right answer is known EXACTLY, an fp64
reference, and a table of mutants (the reference with one defect applied).  Plain torch / numpy on the CPU; the GPU tests
(test_matmul_probes_gpu.py) feed the same inputs to the kernels and compare BITS, test_matmul_probes_cpu.py shows without a GPU that
the expectation is pinned to the oracle and that every mutant is seen.

The contract under test (gemm.hip, decode_dev.h, quant.hip): operands multiplied exactly, accumulated in fp32, then * scale, + bias,
+ residual in fp32, and ONE round-to-nearest-even to bf16.

Why the answer is exact.  All MFMA operands are integers (or lie on a grid 2^-g Z) and sum_k |a| |w| < 2^22 grid units for every
output, so every partial sum is an integer below 2^22 in ANY accumulation order: tiling, split-K, wave order and MFMA shape cannot
change the fp32 accumulator (the bound leaves two bits spare for an adder that aligns to its largest addend).  Scales are powers of
two, bias lies in Z / 2 and the residual is an integer, so the value before the rounding is exact as well (the builders assert that
every intermediate is an fp32 number).  The output then has ONE legal bit pattern, RNE_bf16(exact) — or the exact fp32 value for
EPI_F32 and the lm_head — and the check is torch.equal on bits: no tolerance, no element excluded.

Operand ranges.  An entry range [-r, r] gives an accumulator of standard deviation ~ sqrt(K) r (r + 1) / 3; r is widened for short K
(dense_range) until that is >= 500, so that outputs pass 256 (where bf16 stops holding every integer) and K-quarter / 16-slice partial
sums do too: the rounding mutants then show in every 16 x 16 output block.

Norm-fused decode kernels.  A row of h has every entry +-c with pseudo-random signs, c = 2^j (j = -3 .. 3, mixed inside a 16-row
tile): mean(x^2) = c^2 exactly, bf16(x rstd) = +-1 whatever the last ulp of rsqrtf (eps / c^2 <= 6.4e-5 is far inside a bf16
rounding), and with ln_w in {+-1, +-2, 1/2} the X image bf16(bf16(x rstd) w) is exact.  `eps` rows use c = 2^-10 with eps = 1e-6:
c / sqrt(c^2 + eps) = 0.69868 -> 179 / 256 in bf16 (0.36 of a rounding step from the boundary); without eps the value is 1.

fp8.  A weight row holds e4m3-exact integers times 2^i plus one entry 448 2^i: amax / 448 = 2^i exactly, quantisation is lossless
and the scale a power of two, different per row (a scale taken from the wrong row is off by a power of two).  Per-token fp8
activations (W8A8) are built the same way, with one all-zero token.

SwiGLU / GELU are not exact (exp / erf): gate, up and the GELU input are exact integers, the reference is fp64, the rule one bf16 ulp
from RNE_bf16(reference) (the project's rule for the SwiGLU epilogue, with its allowance for the clamped exponent below x = -80 stated
for any x and u: |x u| e^-80), plus |x| 2^-23 absolute for GELU (the cancellation of fp32 1 + erf on the negative tail).

Rope.  theta = float32(pos) * float32(inv_freq) as ONE fp32 product, inv_freq = 1.0f / powf(base, 2 i / d) in numpy float32, then
x cos + rotate_half(x) sin in fp64.  Tolerance, derived: one bf16 ulp of the reference plus (|x| + |x_partner|) theta 2^-22 (one fp32
ulp of inv_freq from libm differences between the host's powf and numpy, plus one fp32 ulp of the product).
"""
import math
from types import SimpleNamespace as NS

import numpy as np
import torch

LIMIT = 2.0 ** 22
SENTINEL_BF16 = 0x7F7F                      # a bf16 NaN pattern nobody writes
SENTINEL_F32 = 0x7FC12345                   # an fp32 NaN pattern nobody writes
GUARD_ROWS = 256
EPS_LM = 1e-6
LN_W_VALUES = (1.0, -1.0, 2.0, -2.0, 0.5)


# ------------------------------------------------------------------------------------------------ number formats
def is_f32(x):
    return bool((x.float().double() == x).all())


def rne_bf16(x):
    """fp64 (an fp32 number, or rounded to one first) -> bf16, round to nearest even"""
    return x.float().bfloat16()


def trunc_bf16(x):
    b = x.float().view(torch.int32) & -65536
    return b.view(torch.float32).bfloat16()


def away_bf16(x):
    """round half away from zero: add half an ulp to the magnitude bits, truncate"""
    b = (x.float().view(torch.int32) + 0x8000) & -65536
    return b.view(torch.float32).bfloat16()


CONVERSIONS = {"rne": rne_bf16, "trunc": trunc_bf16, "away": away_bf16}


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def bf16_ulp(ref):
    """one bf16 ulp at the magnitude of ref (fp64 tensor holding bf16 values)"""
    _, e = torch.frexp(ref.abs().clamp_min(2.0 ** -126))
    return torch.ldexp(torch.ones_like(ref), e - 8)


def not_bf16(v):
    return rne_bf16(v).double() != v


def is_tie(v):
    """exactly half way between two bf16 neighbours (at ulp 1, magnitudes 128 .. 256, these are the values n + 1/2)"""
    lo = trunc_bf16(v).double()                              # the neighbour towards zero: same binade as v
    return (v != lo) & ((v.abs() - lo.abs()) * 2 == bf16_ulp(lo))


# ------------------------------------------------------------------------------------------------ deterministic integers
def _gen(*key):
    seed = 0x9E3779B1
    for k in key:
        seed = (seed * 1000003 + int(k) + 0x7F4A7C15) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def ints(g, shape, r, nonzero=False):
    x = torch.randint(-r, r + 1, shape, generator=g, dtype=torch.int64)
    if nonzero:
        x = torch.where(x == 0, torch.full_like(x, r), x)
    return x.double()


def dense_range(K):
    r = 2
    while math.sqrt(K) * r * (r + 1) / 3 < 500:
        r += 1
    return r


def fp8_range(K):
    return 16 if K <= 384 else 4


def _fp8_rows(g, rows, K, r, col_of_row, zero_row=None):
    """integers q (|q| <= r, q != 0, one entry 448 per row) and per-row scales 2^i, i in -2 .. 2"""
    q = ints(g, (rows, K), r, nonzero=True)
    idx = torch.arange(rows)
    q[idx, col_of_row(idx)] = 448.0 * (1 - 2 * (idx % 2)).double()
    s = torch.ldexp(torch.ones(rows, dtype=torch.float64), ((idx * 3 + idx // 5) % 5 - 2).int())
    if zero_row is not None and rows > zero_row:
        q[zero_row] = 0
        s[zero_row] = 1.0
    return q, s


# ------------------------------------------------------------------------------------------------ dense probe
def dense(M, N, K, seed=0, w8=False, a8=False):
    """C = A W^T (* row scale * column scale) + bias + R.  Ai / Wi are the integer operands, sa / sw the power-of-two scales (1 without
    fp8), A = Ai sa and W = Wi sw what a kernel that quantises internally is given (Wq = Wi with colscale = sw for the bf16 GEMM's
    colscale epilogue)."""
    g = _gen(M, N, K, seed, w8, a8)
    r = dense_range(K)
    if a8:
        Ai, sa = _fp8_rows(g, M, K, fp8_range(K), lambda m: 2 * ((m * 7) % (K // 2)), zero_row=3)
    else:
        Ai, sa = ints(g, (M, K), r), torch.ones(M, dtype=torch.float64)
    if w8:
        Wi, sw = _fp8_rows(g, N, K, fp8_range(K), lambda n: 2 * ((n * 5) % (K // 2)) + 1)        # odd columns: never A's 448 column
    else:
        Wi, sw = ints(g, (N, K), r), torch.ones(N, dtype=torch.float64)
    bias = ints(g, (N,), 16) / 2
    R = ints(g, (M, N), 200)
    bound = float((Ai.abs() @ Wi.abs().t()).max())
    assert bound < LIMIT, f"sum |a||w| = {bound} >= 2^22"
    p = NS(M=M, N=N, K=K, Ai=Ai, Wi=Wi, sa=sa, sw=sw, bias=bias, R=R, w8=w8, a8=a8, bound=bound, r=r,
           A=(Ai * sa[:, None]).bfloat16(), W=(Wi * sw[:, None]).bfloat16(), Wq=Wi.bfloat16(), bias_bf=bias.bfloat16(), R_bf=R.bfloat16())
    assert torch.equal(p.A.double(), Ai * sa[:, None]) and torch.equal(p.W.double(), Wi * sw[:, None]) and torch.equal(p.R_bf.double(), R)
    assert len(torch.unique(p.A, dim=0)) == M and len(torch.unique(p.W, dim=0)) == N, "rows / columns must be pairwise different"
    return p


def _swap(x, i, j, dim):
    idx = torch.arange(x.shape[dim])
    idx[i], idx[j] = j, i
    return x.index_select(dim, idx)


def _accumulate(A, W, d):
    """the integer accumulator with the K defects of d applied"""
    K = A.shape[1]
    keep = torch.ones(K, dtype=torch.float64)
    if "drop_k32" in d:
        keep[32 * d["drop_k32"]:32 * d["drop_k32"] + 32] = 0
    if "drop_tile" in d:
        keep[64 * d["drop_tile"]:64 * d["drop_tile"] + 64] = 0
    if "dup_tile" in d:
        keep[64 * d["dup_tile"]:64 * d["dup_tile"] + 64] = 2
    if "drop_k" in d:
        keep[d["drop_k"]] = 0
    if "split" in d:                                        # partial sums stored as bf16 before the combine
        step = (K // d["split"] + 31) // 32 * 32
        acc = torch.zeros(A.shape[0], W.shape[0], dtype=torch.float64)
        for k0 in range(0, K, step):
            acc += rne_bf16((A[:, k0:k0 + step] * keep[k0:k0 + step]) @ W[:, k0:k0 + step].t()).double()
        return acc
    return (A * keep) @ W.t()


def evaluate(p, epi="none", M=None, bias=True, inplace=False, d=None, check=False):
    """The output a kernel must produce (d = None) or a mutant's (d = the defects).  epi: none | residual | f32 | swiglu | gelu.
    -> bf16 / fp32 tensor for none, residual, f32; for swiglu / gelu a namespace (ref fp64, x fp64) for the one-ulp rule — a mutant of
    those returns the bf16 rounding of ITS reference."""
    d = d or {}
    M = p.M if M is None else M
    if any(k in d for k in ("drop_k32", "drop_tile", "dup_tile", "drop_k", "split")):
        acc = _accumulate(p.Ai[:M], p.Wi, d)
    else:
        if getattr(p, "acc", None) is None:
            p.acc = p.Ai @ p.Wi.t()                         # computed once, shared by every M and epilogue of the probe
        acc = p.acc[:M]
    sa, sw, b = p.sa[:M], p.sw, (p.bias if bias else torch.zeros_like(p.bias))
    if "rowscale_shift" in d:
        sa = torch.roll(sa, d["rowscale_shift"])
    if "colscale_shift" in d:
        sw = torch.roll(sw, d["colscale_shift"])
    if "bias_shift" in d:
        b = torch.roll(b, d["bias_shift"])
    if d.get("unpacked_index") and epi == "swiglu":         # scale / bias indexed as if gate rows were [0, I) and up rows [I, 2 I)
        I = p.N // 2
        j = torch.arange(p.N)
        un = torch.where((j % 64) < 32, (j // 64) * 32 + j % 32, I + (j // 64) * 32 + j % 32)
        sw, b = sw[un], b[un]
    v = acc * sa[:, None] * sw[None, :]
    if check:
        assert is_f32(v)
    if d.get("acc_bf16"):
        v = rne_bf16(v).double()
    v = v + b
    if check:
        assert is_f32(v)
    if d.get("bias_round"):
        v = rne_bf16(v).double()
    conv = CONVERSIONS[d.get("conv", "rne")]
    if epi == "residual":
        R = p.R[:M]
        if d.get("residual_after_write"):
            R = conv(v + R).double()
        v = v + R
        if check:
            assert is_f32(v)
    if epi == "swiglu":
        y = v.view(M, p.N // 64, 2, 32)
        gate, up = y[:, :, 0].reshape(M, p.N // 2), y[:, :, 1].reshape(M, p.N // 2)
        ref = gate / (1.0 + torch.exp(-gate)) * up
        out = NS(ref=ref, x=gate, u=up, kind="swiglu")
    elif epi == "gelu":
        out = NS(ref=0.5 * v * (1.0 + torch.erf(v / math.sqrt(2.0))), x=v, kind="gelu")
    elif epi == "f32":
        out = v.float()
    else:
        out = conv(v)
    if d is not None and ("swap_rows" in d or "swap_cols" in d):
        for key, dim in (("swap_rows", 0), ("swap_cols", 1)):
            if key in d:
                i, j = d[key]
                if isinstance(out, NS):
                    out = NS(**{k: (v if k == "kind" else _swap(v, i, j, dim)) for k, v in vars(out).items()})
                else:
                    out = _swap(out, i, j, dim)
    if isinstance(out, NS) and d:
        return rne_bf16(out.ref)
    return out


def pre_rounding(p, epi="none", M=None, bias=True):
    """the exact value before the one rounding (fp64)"""
    M = p.M if M is None else M
    v = (p.Ai[:M] @ p.Wi.t()) * p.sa[:M, None] * p.sw[None, :] + (p.bias if bias else 0)
    return v + p.R[:M] if epi == "residual" else v


def wrong(got, want):
    """-> bool tensor of the elements of a kernel's (or mutant's) output that break the rule for `want` (evaluate's result)"""
    if isinstance(want, NS):
        ref = rne_bf16(want.ref).double()
        g = got.double()
        tol = bf16_ulp(ref)
        if want.kind == "swiglu":
            # gemm.hip silu() clamps the exponent at 80 so that 1 + e^-x stays finite: below x = -80 it returns x e^-80 (a tiny negative) where the
            # exact quotient underflows further; times u, and rounded to bf16.  (1e-30 in test_kernels_gpu.py, for |x| <= 120 and |u| <= 8.)
            tol = tol + (want.x * want.u).abs() * (math.exp(-80.0) * 1.01)
        if want.kind == "gelu":
            tol = tol + want.x.abs() * 2.0 ** -23
        return ~((g - ref).abs() <= tol)                    # NaN counts as wrong
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    return bits(got) != bits(want)


def blocks(bad, rows=None, cols=None):
    """-> (blocks of 16 rows x 16 columns that hold a wrong element, blocks looked at).  The last row block is aligned to the END (rows M - 16 ..
    M - 1), so with a ragged M every row still lies in a full block.  rows / cols: only the blocks that hold one of these rows / columns."""
    M, N = bad.shape
    h = min(16, M)
    starts = sorted(set(list(range(0, M - h + 1, 16)) + [M - h]))
    seen = looked = 0
    for r0 in starts:
        if rows is not None and not any(r0 <= r < r0 + h for r in rows):
            continue
        hit = bad[r0:r0 + h].reshape(h, N // 16, 16).any(2).any(0)
        if cols is not None:
            hit = hit[sorted({c // 16 for c in cols})]
        seen += int(hit.sum())
        looked += hit.numel()
    return seen, looked


# ------------------------------------------------------------------------------------------------ mutants of the dense probe
def dense_mutants(p, epi, M, bias=True, inplace=False):
    """name -> (defects, rows, cols): the mutants that apply to this configuration; rows / cols name the blocks where the mutant must show
    (None: every block)."""
    T = p.K // 64
    out = {}
    bitwise = epi in ("none", "residual")
    if bitwise:
        out["truncating conversion"] = ({"conv": "trunc"}, None, None)
        out["round half away"] = ({"conv": "away"}, None, None)
        if bias or epi == "residual":
            out["accumulator rounded to bf16 before bias / residual"] = ({"acc_bf16": True}, None, None)
        if bias and epi == "residual":
            out["bias added, rounded, then residual"] = ({"bias_round": True}, None, None)
    if epi in ("none", "residual", "f32"):
        if p.K >= 256:
            out["K-quarter partials rounded to bf16"] = ({"split": 4}, None, None)
        if p.K >= 1024:
            out["16-slice partials rounded to bf16"] = ({"split": 16}, None, None)
    out["one k-step of 32 dropped"] = ({"drop_k32": (p.K // 32) // 2}, None, None)
    out["one k element dropped"] = ({"drop_k": p.K - 1}, None, None)
    for name, t in {"first": 0, "last": T - 1, **{f"ring phase {ph}": min(T - 1, 5 + ph) for ph in range(5) if T > 5 + ph}}.items():
        out[f"K tile dropped ({name})"] = ({"drop_tile": t}, None, None)
        out[f"K tile doubled ({name})"] = ({"dup_tile": t}, None, None)
    if M >= 2:
        a = M - 1
        out["two rows swapped inside a tile"] = ({"swap_rows": (a, a - 1)}, [a], None)
    if M >= 40:
        out["two rows swapped across tiles"] = ({"swap_rows": (3, 35)}, [3, 35], None)
    ldc = p.N // 2 if epi == "swiglu" else p.N
    out["two columns swapped"] = ({"swap_cols": (5, ldc - 3)}, None, [5, ldc - 3])
    if bias:
        out["bias from column n + 1"] = ({"bias_shift": -1}, None, None)
        out["bias from column n - 1"] = ({"bias_shift": 1}, None, None)
    if p.w8:
        out["scale from column n + 1"] = ({"colscale_shift": -1}, None, None)
        out["scale from column n - 1"] = ({"colscale_shift": 1}, None, None)
    if epi == "swiglu" and (p.w8 or bias):
        out["scale / bias from the unpacked index"] = ({"unpacked_index": True}, None, None)
    if p.a8 and M >= 2:
        out["row scale from row m + 1"] = ({"rowscale_shift": -1}, None, None)
        out["row scale from row m - 1"] = ({"rowscale_shift": 1}, None, None)
    if inplace:
        out["residual read after the write"] = ({"residual_after_write": True}, None, None)
    return out


# ------------------------------------------------------------------------------------------------ activation probe (identity weights)
def act_probe():
    """SwiGLU / GELU on exact integers: A = [x | u] against packed identity blocks, so the epilogue is handed x and u themselves.  x covers
    -30 .. 30 densely plus -100 and -88 (where e^-x overflows fp32)."""
    I = 128
    vals = torch.tensor(list(range(-30, 31)) + [-100, -88], dtype=torch.float64)
    M = 64
    n = torch.arange(M * I)
    x = vals[n % len(vals)].view(M, I)
    u = (((n * 7 + n // 63) % 17) - 8).double().view(M, I)
    A = torch.cat([x, u], 1)
    eye, zero = torch.eye(I, dtype=torch.float64), torch.zeros(I, I, dtype=torch.float64)
    gate, up = torch.cat([eye, zero], 1), torch.cat([zero, eye], 1)
    W13 = torch.stack([gate.view(I // 32, 32, 2 * I), up.view(I // 32, 32, 2 * I)], dim=1).reshape(2 * I, 2 * I)
    plain = torch.eye(2 * I, dtype=torch.float64)
    return NS(M=M, I=I, K=2 * I, A=A.bfloat16(), W13=W13.bfloat16(), Weye=plain.bfloat16(),
              swiglu=NS(ref=x / (1.0 + torch.exp(-x)) * u, x=x, u=u, kind="swiglu"),
              gelu=NS(ref=0.5 * A * (1.0 + torch.erf(A / math.sqrt(2.0))), x=A, kind="gelu"))


# ------------------------------------------------------------------------------------------------ normalised rows
def eps_c(eps):
    """c = 2^-j for an `eps` row: c / sqrt(c^2 + eps) lies in (0.5, 0.8) — eps moves the normalised value by a third — and at least 2^-12
    (relative) from a bf16 rounding boundary, far above what a 1-ulp rsqrtf and two fp32 roundings can move.  eps = 1e-6 -> 2^-10."""
    for j in range(1, 20):
        c = 2.0 ** -j
        ratio = c / math.sqrt(c * c + eps)
        if 0.5 < ratio < 0.8 and boundary_margin(ratio) >= 2.0 ** -12:
            return c
    raise AssertionError(eps)


def boundary_margin(x):
    """relative distance of x > 0 from the nearest bf16 rounding boundary (the midpoint of two neighbouring bf16 values)"""
    m, e = math.frexp(x)                      # x = m 2^e, m in [0.5, 1): bf16 ulp = 2^(e - 8)
    steps = x / 2.0 ** (e - 8)
    return abs(steps - math.floor(steps) - 0.5) * 2.0 ** (e - 8) / x


def norm_rows(B, H, eps=EPS_LM, seed=0, eps_every=4, balanced=False, j_of_row=lambda b: (5 * b) % 7 - 3):
    """h [B, H] bf16 with entries +-c, ln_w [H] in {+-1, +-2, 1/2}.  Row b is an `eps` row (c = eps_c(eps)) when b % eps_every == 0, else
    c = 2^j with j = j_of_row(b) = (5 b) % 7 - 3.  balanced: exactly H / 2 entries of either sign (mean exactly 0, for layernorm)."""
    g = _gen(B, H, seed, 77)
    if balanced:
        sign = torch.stack([torch.where(torch.randperm(H, generator=g) < H // 2, 1.0, -1.0) for _ in range(B)]).double()
    else:
        sign = (torch.randint(0, 2, (B, H), generator=g) * 2 - 1).double()
    b = torch.arange(B)
    is_eps = (b % eps_every) == 0
    c = torch.where(is_eps, torch.full((B,), eps_c(eps), dtype=torch.float64), torch.ldexp(torch.ones(B, dtype=torch.float64), j_of_row(b).int()))
    w = torch.tensor(LN_W_VALUES, dtype=torch.float64)[torch.randint(0, len(LN_W_VALUES), (H,), generator=g)]
    h = sign * c[:, None]
    assert torch.equal(h.bfloat16().double(), h)
    return NS(B=B, H=H, eps=eps, sign=sign, c=c, is_eps=is_eps, w=w, h=h.bfloat16(), ln_w=w.bfloat16())


def norm_image(nr, defect=None):
    """the exact X image bf16(bf16(x rstd) w) as fp64 [B, H].  defect: no_eps | eps_after_sqrt | neighbour_rstd"""
    c, eps = nr.c, nr.eps
    if defect == "no_eps":
        rstd = 1.0 / c
    elif defect == "eps_after_sqrt":
        rstd = 1.0 / (c + eps)
    else:
        rstd = 1.0 / torch.sqrt(c * c + eps)
    if defect == "neighbour_rstd":
        rstd = rstd[torch.arange(nr.B) ^ 1 if nr.B % 2 == 0 else torch.roll(torch.arange(nr.B), 1)]
    xh = rne_bf16(nr.sign * (c * rstd)[:, None]).double()
    return rne_bf16(xh * nr.w).double()


NORM_DEFECTS = {"eps omitted": "no_eps", "eps added after the square root": "eps_after_sqrt", "rstd of the neighbouring row": "neighbour_rstd"}


def norm_margins(nr):
    """relative distance of every row's c / sqrt(c^2 + eps) from a bf16 rounding boundary"""
    return [boundary_margin(float(c / math.sqrt(c * c + nr.eps))) for c in nr.c.tolist()]


# ------------------------------------------------------------------------------------------------ decode probes
def dec_weights(N, K, seed, fp8, r=None):
    g = _gen(N, K, seed, fp8, 5)
    if fp8:
        Wi, sw = _fp8_rows(g, N, K, fp8_range(K), lambda n: 2 * ((n * 5) % (K // 2)) + 1)
    else:
        Wi, sw = ints(g, (N, K), r or dense_range(K)), torch.ones(N, dtype=torch.float64)
    W = Wi * sw[:, None]
    assert torch.equal(W.bfloat16().double(), W)
    return NS(Wi=Wi, sw=sw, W=W.bfloat16())


def fused_probe(B, H, N, fp8=False, seed=0, with_bias=False, nr=None):
    """rmsnorm -> projection: nr (the rows), w (the weights), X (exact image), y = X W^T (+ bias), exact in fp32"""
    nr = nr or norm_rows(B, H, seed=seed)
    # the image lies on 2^-9 Z on the eps rows (179 / 256 * 1/2): the integer bound in units of that grid
    w = dec_weights(N, H, seed, fp8, r=3 if H > 768 else 4)
    X = norm_image(nr)
    bound = float((X.abs() @ w.Wi.abs().t()).max()) * 2.0 ** 9
    assert bound < LIMIT, f"sum |x||w| = {bound} grid units >= 2^22"
    g = _gen(B, N, seed, 9)
    bias = ints(g, (N,), 16) / 2 if with_bias else torch.zeros(N, dtype=torch.float64)
    return NS(B=B, H=H, N=N, nr=nr, w=w, X=X, bias=bias, bias_bf=bias.bfloat16(), bound=bound)


def fused_output(fp, defect=None):
    X = norm_image(fp.nr, defect)
    y = (X @ fp.w.Wi.t()) * fp.w.sw[None, :] + fp.bias
    assert defect is not None or is_f32(y)
    return y


def gateup_reference(B, H, I, fp8, seed=0):
    gp = fused_probe(B, H, I, fp8, seed=seed)
    return gp, fused_probe(B, H, I, fp8, seed=seed + 1, nr=gp.nr)


def swiglu_of(g, u):
    return NS(ref=g / (1.0 + torch.exp(-g)) * u, x=g, u=u, kind="swiglu")


# ---- KV page layout (csrc/decode.hip header), as in tests/test_decode_kernels_gpu.py
_key, _d = torch.arange(64).view(64, 1), torch.arange(128).view(1, 128)
K_IDX = (((_key >> 4) * 4 + (_d >> 5)) * 64 + ((_d >> 3) & 3) * 16 + (_key & 15)) * 8 + (_d & 7)
V_IDX = (((_key >> 5) * 8 + (_d >> 4)) * 64 + (((_key & 31) >> 2) & 3) * 16 + (_d & 15)) * 8 + 4 * ((_key & 31) >> 4) + (_key & 3)

DEC_POSITIONS = (0, 64, 127, 32766, 0, 4095, 8191, 20000)        # first / last slot of a page, the last position of the default capacity


def dec_positions(B):
    return [DEC_POSITIONS[b % len(DEC_POSITIONS)] for b in range(B)]


def vt_reference(v, lens):
    """v [T, H, 128] -> V^T [H, 128, Tpad] with the split kernel's padding and 16-key group order"""
    H = v.shape[1]
    perm = torch.tensor([0, 1, 2, 3, 8, 9, 10, 11, 4, 5, 6, 7, 12, 13, 14, 15])
    outs, t0 = [], 0
    for n in lens:
        npad = (n + 63) // 64 * 64
        vp = torch.zeros(npad, H, 128, dtype=v.dtype)
        vp[:n] = v[t0:t0 + n]
        idx = (torch.arange(npad) // 16 * 16).view(-1, 16)[:, 0:1] + perm.view(1, 16)
        outs.append(vp[idx.reshape(-1)])
        t0 += n
    return torch.cat(outs, 0).permute(1, 2, 0).contiguous()


# ------------------------------------------------------------------------------------------------ rope
def inv_freq_f32(base, two_d):
    """ops.hip: 1.0f / powf(theta, 2 i / d) — numpy float32 throughout"""
    n, d = (32, 64.0) if two_d else (64, 128.0)
    e = (2 * np.arange(n)).astype(np.float32) / np.float32(d)
    return (np.float32(1.0) / np.power(np.float32(base), e, dtype=np.float32)).astype(np.float32)


def rope_angles(pos, base, two_d, d=None):
    """pos [T] or [T, 2] int -> theta [T, 128] fp64, each ONE fp32 product float32(pos) * float32(inv_freq).
    d (mutants): pos16 | freq_shift | swap_hw.  pos16: no position the engine reaches (<= 32766) changes when it is cut to a 16-bit INTEGER, so the
    mutant holds the position in the widest 16-bit float (fp16, 11 significant bits): odd positions above 2048 move."""
    d = d or {}
    pos = np.asarray(pos, dtype=np.int64)
    if d.get("pos16"):
        pos = pos.astype(np.float16).astype(np.int64)                             # the position held in a 16-bit float
    f = inv_freq_f32(base, two_d)
    if d.get("freq_shift"):
        f = np.roll(f, -1)
    if two_d:
        if d.get("swap_hw"):
            pos = pos[:, ::-1]
        ang = np.concatenate([pos[:, 0:1].astype(np.float32) * f[None, :], pos[:, 1:2].astype(np.float32) * f[None, :]], 1)
    else:
        ang = pos[:, None].astype(np.float32) * f[None, :]
    assert ang.dtype == np.float32
    ang = torch.from_numpy(ang.astype(np.float64))
    return torch.cat([ang, ang], 1)


def rotate_half(x):
    x1, x2 = x[..., :64], x[..., 64:]
    return torch.cat((-x2, x1), dim=-1)


def rope_reference(x, pos, base, two_d, d=None):
    """x [T, heads, 128] fp64 -> (rotated fp64, tolerance fp64): one bf16 ulp of the reference + (|x| + |x_partner|) theta 2^-22"""
    d = d or {}
    th = rope_angles(pos, base, two_d, d).unsqueeze(1)
    cos, sin = (torch.sin(th), torch.cos(th)) if d.get("swap_sincos") else (torch.cos(th), torch.sin(th))
    ref = x * cos + rotate_half(x) * sin
    tol = bf16_ulp(rne_bf16(ref).double()) + (x.abs() + rotate_half(x).abs()) * th * 2.0 ** -22
    return ref, tol


ROPE_MUTANTS = {"position truncated to 16 bits": {"pos16": True}, "sin and cos swapped": {"swap_sincos": True},
                "inv_freq index off by one": {"freq_shift": True}, "2-D h and w swapped": {"swap_hw": True}}

ROPE_POS_1D = (0, 1, 63, 64, 4095, 8191, 20000, 32766)


def rope_probe(two_d, Hq=2, Hkv=2, seed=0):
    """A few short sequences whose rows sit at the positions the engine reaches; q / k / v inputs are exact small integers.
    -> lens, pos (int32 [T] or [T, 2]), qkv [T, (Hq + 2 Hkv) 128] fp64 integers"""
    g = _gen(two_d, Hq, Hkv, seed, 31)
    lens = [70, 1, 65]
    T = sum(lens)
    if two_d:
        pos = torch.stack([torch.randint(0, 239, (T,), generator=g), torch.randint(0, 239, (T,), generator=g)], -1)
        pos[0], pos[1], pos[2], pos[T - 1] = torch.tensor([238, 238]), torch.tensor([0, 238]), torch.tensor([238, 0]), torch.tensor([0, 0])
        pos[3] = torch.tensor([237, 1])
    else:
        pos = torch.tensor([ROPE_POS_1D[(t * 3 + t // 8) % len(ROPE_POS_1D)] for t in range(T)])
    qkv = ints(g, (T, (Hq + 2 * Hkv) * 128), 64)
    return NS(lens=lens, T=T, pos=pos.numpy().astype(np.int32), qkv=qkv, Hq=Hq, Hkv=Hkv, two_d=two_d, base=10000.0 if two_d else 1e6)


def mutant_rows(rp, name):
    """the large-position rows on which a rope mutant must leave the tolerance"""
    if rp.two_d:
        return np.nonzero((np.abs(rp.pos[:, 0] - rp.pos[:, 1]) >= 8) if name == "2-D h and w swapped" else (rp.pos.max(1) >= 100))[0]
    if name == "position truncated to 16 bits":
        return np.nonzero((rp.pos >= 4095) & (rp.pos % 2 == 1) | (rp.pos == 32766))[0]
    return np.nonzero(rp.pos >= 4095)[0]


# ------------------------------------------------------------------------------------------------ the probe configurations (CPU and GPU tests run the same)
GEMM_N = (128, 384, 256, 768)                 # 128-wide kernel (N % 256 != 0) / 256-wide kernels
GEMM_K = (64, 192, 320, 384, 1536)            # 1, 3, 5, 6, 24 K tiles: below the plan-1 threshold, ring not wrapped, the ring size, first wrap, the model's K
GEMM_M = (1, 255, 257, 513)
GEMM_COLSCALE_NK = ((256, 64), (128, 192), (768, 384), (384, 1536), (256, 1536))        # the colscale epilogue on both kernel widths
GEMM_FP8 = ((257, 256, 64), (300, 512, 192), (513, 256, 1536))
QKV_PROJ = (((64,), 2, 2, 192), ((257, 1), 12, 2, 1536), ((300, 212), 12, 12, 256))
DEC_B = (1, 8, 9, 16, 17, 32, 33, 64)
DEC_PROJ_NK = ((768, 768), (768, 1536), (1536, 1536), (1536, 8960))
DEC_GATEUP_HI = ((768, 1536), (1536, 8960))
DEC_LMHEAD_H = (768, 1536)
DEC_LMHEAD_V = (1184, 1200)                   # 74 / 75 vocabulary tiles: the streaming kernel pairs tiles, 75 leaves a half-empty pair
DEC_QKV_B = (1, 9, 16, 35, 64)
DEC_QKV = ((768, 6, 1), (1536, 12, 2))
NORM_DIMS = (256, 512, 1536, 4096)
NORM_ROWS = (1, 5, 130)
EPS_TOWER = 1e-5
LN_BOUNDARY = 2.0 ** -19                      # layernorm: 16 fp32 ulps (rsqrtf + four fp32 operations) from a bf16 rounding boundary
LN_MAX_NEAR = 0.01


def layernorm_probe(rows, dim, eps, seed=0):
    """balanced +-c rows (mean exactly 0, variance exactly c^2), weights and bias any bf16 values.  -> the rows, ref fp64 (x - mean) rstd w + b,
    near: the elements whose reference lies within LN_BOUNDARY (relative) of a bf16 rounding boundary (they may differ by one ulp)"""
    # c = 2^j with j = -3 .. -6 off the eps rows: 1 / sqrt(1 + eps / c^2) is then 3e-5 .. 2e-3 below 1, which keeps w + b (a sum of two bf16
    # values, often an exact tie) away from the rounding boundaries; with larger c a third of the row would sit on one
    nr = norm_rows(rows, dim, eps=eps, seed=seed, eps_every=2, balanced=True, j_of_row=lambda b: -3 - (b // 2) % 4)
    g = _gen(rows, dim, seed, 13)
    # |w| in [0.75, 1.5], |b| <= 0.25: |result| >= 0.69 * 0.75 - 0.25, so the sum cancels at most a factor 6 and the kernel's fp32 error (a 1-ulp
    # rsqrtf, two products, one sum) stays below LN_BOUNDARY relative to the RESULT
    w = ((0.75 + 0.75 * torch.rand(dim, generator=g)) * (torch.randint(0, 2, (dim,), generator=g) * 2 - 1)).bfloat16()
    b = (0.5 * torch.rand(dim, generator=g) - 0.25).bfloat16()
    ref = nr.h.double() / torch.sqrt(nr.c * nr.c + eps)[:, None] * w.double() + b.double()
    a = ref.abs().clamp_min(2.0 ** -120)
    _, e = torch.frexp(a)
    steps = a / torch.ldexp(torch.ones_like(a), e - 8)
    near = ((steps - torch.floor(steps) - 0.5).abs() * torch.ldexp(torch.ones_like(a), e - 8) / a) < LN_BOUNDARY
    return NS(nr=nr, w=w, b=b, ref=ref, near=near)


def layernorm_wrong(got, lp):
    want = rne_bf16(lp.ref)
    diff = (got.double() - want.double()).abs()
    return torch.where(lp.near, diff > bf16_ulp(want.double()), bits(got) != bits(want))
