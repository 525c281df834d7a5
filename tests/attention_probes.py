"""Attention probes: inputs in which EVERY key's contribution is visible in the output, an fp64 reference, and a table of mutants
(the reference with one defect applied).  Plain torch on the CPU; the GPU tests (test_attention_probes_gpu.py) feed the same inputs to
the flash and decode-attention kernels, test_attention_probes_cpu.py shows without a GPU that the tolerance is pinned to the reference
and that every mutant lies outside it.

Why: with q, k, v ~ randn the output of an N-key softmax shrinks like 1 / sqrt(N) while an absolute tolerance does not, so at the
benchmark's sizes (5 201 / 19 824 keys) a kernel that never reads its ragged last tile stays inside 4e-3 + 2^-6 max|ref|.

Indicator V.  v[j] = one_hot(class(j)), classes < 128: non-negative, exact in bf16 and (unit scale) in e4m3.  Output element d IS the
softmax mass of class d, the error bound sum p |v| is the output itself, so a purely RELATIVE tolerance is principled.  Codes:
  tile   class = (j // 64) % 128 from 128 tiles up; with fewer tiles the classes the tiles leave free are filled with the position inside
         the tile ((j // 64) % C + C * sub-tile, C = the largest power of two <= tiles), so that every class has a key from 128 keys up
  lane   class = j % 64 + 64 * ((j // 64) % 2)
kv head h shifts the classes by 37 h (heads must not be interchangeable).

Planted keys.  k[j] = alpha * q[r] for chosen (row r, key j): key j then carries a graded share (roughly 5-30 %) of row r's mass.
Planted at the first and last key, both sides of the ragged tile's start, of 64-key tile / page boundaries, of query-block, split, wave
and page-round boundaries; for causal rows at the diagonal key r and its masked neighbour r + 1.

Poison.  What lies behind a sequence (`tail_k`): the 64 spare K rows / the unused slots of the last page hold 0x7F00 (1.7e38), in a packed
batch the next sequence's live keys (one of them planted for this sequence's last row).  V^T padding is zero (the layout contract), the
unused V slots of a KV page are poison.

Tolerance (the rule: relative per element; the largest emulated-oracle-vs-fp64 relative deviation over all probes, times 3).
  measured (test_attention_probes_cpu.py, all probes, both codes): max |oracle_emulated - fp64| / fp64 = 0.00737 (causal, 4 999
  tokens; 0.0042-0.0057 on the long bidirectional probes, 0.0047-0.0072 on the decode probes, bf16 and fp8 pools alike).  The largest
  values come from classes that hold ONE visible key (short and causal rows): one bf16 rounding of P plus one of the output, 2^-8 each.
  REL_TOL = 3 * 0.0074 = 0.0222, plus OUT_ROUND = 2^-8 relative (half a bf16 ulp) for the rounding of the bf16 output.
The emulated oracle rounds P to bf16 and keeps the row sum in fp32, as the kernels do; the margin of 3 covers what the kernels do
differently from it — accumulation in tile order, v_exp_f32, the deferred rescale's P <= 64 — none of which changes the relative size of
a bf16 rounding.  Elements whose reference mass is EXACTLY zero (a class without a visible key: short and causal rows) are not excluded:
they must come back below FLOOR in absolute value.  Elements with 0 < mass < FLOOR are excluded from the relative check; their share is
counted and capped at MAX_EXCLUDED per probe.
"""
import math

import torch

SCALE = 1 / math.sqrt(128)
POISON_BITS = 0x7F00                  # bf16 1.7e38
POISON = 1.7014118346046923e38
REL_TOL = 0.0222
OUT_ROUND = 2.0 ** -8
FLOOR = 1e-6
MAX_EXCLUDED = 0.05
MUTANT_FACTOR = 4.0
DECODE_WAVES = 4                      # csrc/decode.hip decode_attn_waves(): pages in flight per workgroup
ROWS_PER_BLOCK = 256                  # csrc/attn_prefill.hip flash_rows_per_block() (128 with DOTS_OCR_ATTN_ROWS128: its edges are covered too)
CODES = ("tile", "lane")
E4M3_MAX = 448.0


def decode_attn_splits(max_seq_len):
    """csrc/decode.hip decode_attn_splits, restated"""
    pages = (max_seq_len + 63) // 64
    return max(1, min((pages + DECODE_WAVES - 1) // DECODE_WAVES, 64))


# ------------------------------------------------------------------------------------------------ codes
def classes(code, n):
    j = torch.arange(n)
    if code == "lane":
        return j % 64 + 64 * ((j // 64) % 2)
    assert code == "tile", code
    tiles, c = (n + 63) // 64, 1
    while c * 2 <= min(128, tiles):
        c *= 2
    sub = min(128 // c, 64)
    return (j // 64) % c + c * ((j % 64) // (64 // sub))


def quant8(x, s):
    return x.float().div(s).clamp(-E4M3_MAX, E4M3_MAX).to(torch.float8_e4m3fn)


# ------------------------------------------------------------------------------------------------ one sequence
class Seq:
    """One key sequence and its probed query rows.  q [nq, Hq, 128] bf16 (query row r sits at key position r + n - nq), k [n, Hkv, 128]
    bf16, rows: the checked query rows, tail_k [m, Hkv, 128]: what the memory behind key n - 1 holds (tail_v: the V value there).
    scales [Hkv, 2] (K, V): the sequence lives in an fp8 pool and the reference reads the DEQUANTISED K / V."""

    def __init__(self, q, k, rows, causal=False, tail_k=None, tail_v=0.0, n_splits=None, scales=None, name=""):
        self.q, self.k, self.rows, self.causal, self.name = q, k, list(rows), causal, name
        self.n, self.nq, self.Hq, self.Hkv = k.shape[0], q.shape[0], q.shape[1], k.shape[1]
        self.tail_k, self.tail_v, self.n_splits, self.scales = tail_k, tail_v, n_splits, scales
        self.limits = torch.tensor([r + 1 + self.n - self.nq if causal else self.n for r in self.rows])
        self.k8 = None
        if scales is not None:
            self.k8 = quant8(k, scales[:, 0].view(1, -1, 1))
            self.k_ref = self.k8.float() * scales[:, 0].view(1, -1, 1)
        else:
            self.k_ref = k.float()
        self._S = None

    @property
    def tiles(self):
        return (self.n + 63) // 64

    @property
    def ragged(self):
        return self.n % 64

    def v_kernel(self, code):
        """what the kernel is given: bf16 [n, Hkv, 128], or e4m3 in an fp8 pool"""
        cls = classes(code, self.n)
        v = torch.zeros(self.n, self.Hkv, 128)
        for h in range(self.Hkv):
            v[torch.arange(self.n), h, (cls + 37 * h) % 128] = 1.0
        if self.scales is not None:
            return quant8(v, self.scales[:, 1].view(1, -1, 1))
        return v.bfloat16()

    def v_ref(self, code):
        v = self.v_kernel(code).float()
        return v * self.scales[:, 1].view(1, -1, 1) if self.scales is not None else v

    def _scores(self):
        if self._S is None:
            R, G = len(self.rows), self.Hq // self.Hkv
            kk = self.k_ref.double()
            if self.tail_k is not None and len(self.tail_k):
                kk = torch.cat([kk, self.tail_k.double()])
            qs = self.q[self.rows].double().view(R, self.Hkv, G, 128)
            self._S = (torch.einsum("rkgd,nkd->kgrn", qs, kk) * SCALE).reshape(self.Hq, R, kk.shape[0])
        return self._S

    def attend(self, v, mult=None, vsrc=None, tail=False, limit_shift=0):
        """softmax(q k^T scale) v in float64 for the checked rows -> [R, Hq, 128].  The keyword arguments are the mutants' handles:
        mult [R or 1, n] multiplies key weights (0 drops a key, 2 counts it twice), vsrc [n] takes v[vsrc[j]] for key j, tail reads the
        keys behind the sequence unmasked, limit_shift moves the causal limit."""
        n, R, G = self.n, len(self.rows), self.Hq // self.Hkv
        m = len(self.tail_k) if tail else 0
        S = self._scores()[..., :n + m]
        M = (torch.arange(n + m).view(1, -1) < (self.limits + limit_shift).view(-1, 1)).double()
        if tail:
            M[:, n:] = 1.0
        if mult is not None:
            M[:, :n] *= mult
        Sm = S.masked_fill(M == 0, float("-inf"))
        P = torch.exp(Sm - Sm.max(-1, keepdim=True).values) * M
        P = P / P.sum(-1, keepdim=True)
        vv = v.double()
        if vsrc is not None:
            vv = vv[vsrc]
        if tail:
            vv = torch.cat([vv, torch.full((m, self.Hkv, 128), self.tail_v, dtype=torch.float64)])
        out = torch.stack([P[h] @ vv[:, h // G] for h in range(self.Hq)])          # [Hq, R, 128]
        return out.transpose(0, 1).contiguous()

    def reference(self, code):
        return self.attend(self.v_ref(code))


def plant(seq_q, k, r, j, head, kv_head, weight, n_visible):
    """k[j, kv_head] = alpha q[r, head], alpha such that the key weighs `weight` times the ~ 1.65 n_visible of the random keys"""
    qv = seq_q[r, head].float()
    logit = max(math.log(weight * 1.65 * n_visible), 1.0)
    k[j, kv_head] = (qv * (logit / (float(qv.pow(2).sum()) * SCALE))).bfloat16()


def boundary_keys(n, extra=()):
    full, mid = n // 64 * 64, 64 * ((n + 63) // 64 // 2)
    cand = [0, n - 1, full - 1, full, 63, 64, mid - 1, mid, *extra]
    out = []
    for p in cand:
        if 0 <= p < n and p not in out:
            out.append(p)
    return out


# ------------------------------------------------------------------------------------------------ builders
def prefill_rows(n):
    """two rows on each side of every 32-row (wave) and query-block boundary of the first, a middle and the last block; the ends"""
    blocks = (n + ROWS_PER_BLOCK - 1) // ROWS_PER_BLOCK
    rows = {0, 1, n - 2, n - 1}
    for b in {0, blocks // 2, blocks - 1}:
        for e in range(b * ROWS_PER_BLOCK, (b + 1) * ROWS_PER_BLOCK + 1, 32):
            rows |= {e - 2, e - 1, e, e + 1}
    return sorted(r for r in rows if 0 <= r < n)


def poison_rows(m, Hkv):
    return torch.full((m, Hkv, 128), POISON_BITS, dtype=torch.int16).view(torch.bfloat16)


def prefill_probe(lens, H=2, seed=0):
    """A packed bidirectional batch (the ViT's attention): one Seq per sequence."""
    g = torch.Generator().manual_seed(1000 + seed)
    qs = [torch.randn(n, H, 128, generator=g).bfloat16() for n in lens]
    ks = [torch.randn(n, H, 128, generator=g).bfloat16() for n in lens]
    rows = [prefill_rows(n) for n in lens]
    weights = (0.25, 0.5, 1.0)
    for i, n in enumerate(lens):
        blocks = (n + 255) // 256
        edges = [255, 256, 256 * (blocks // 2) - 1, 256 * (blocks // 2), 256 * (blocks - 1) - 1, 256 * (blocks - 1)]
        prow = rows[i][3::max(1, len(rows[i]) // 6)][:6]                           # the planted rows, spread over the checked ones
        for a, j in enumerate(boundary_keys(n, edges)):
            for h in range(H):
                plant(qs[i], ks[i], prow[a % len(prow)], j, h, h, weights[a % 3], n)
    for i, n in enumerate(lens[:-1]):                                              # live data behind a ragged tile: the next sequence's key 1
        if n % 64 and n % 64 < 63:
            for h in range(H):
                kq = torch.empty(2, H, 128, dtype=torch.bfloat16)
                plant(qs[i], kq, n - 1, 1, h, h, 1.0, n)
                ks[i + 1][1, h] = kq[1, h]
    seqs = []
    for i, n in enumerate(lens):
        m = (-n) % 64
        if i + 1 < len(lens):
            tail = torch.cat([ks[i + 1][:m], poison_rows(max(0, m - lens[i + 1]), H)])
        else:                                                                      # k is head-major over the packed tokens: behind a head's last key
            tail = poison_rows(m, H)                                               # lies the next head's first key; the spare rows follow the last head
            tail[:, :H - 1] = ks[0][:m, 1:]
        seqs.append(Seq(qs[i], ks[i], rows[i], tail_k=tail, tail_v=0.0, name=f"seq{i}[{n}]"))
    return seqs


def causal_probe(T, Hq=12, Hkv=2, seed=0):
    """LM prefill, causal GQA: diagonal neighbours planted at every wave boundary of a 256-row block, in the first, a middle and the last block.
    kv head 0 plants for query e - 1 (keys e - 1 and e), kv head 1 for query e (keys e and e + 1): a key serves one query only."""
    g = torch.Generator().manual_seed(2000 + seed)
    q = torch.randn(T, Hq, 128, generator=g).bfloat16()
    k = torch.randn(T, Hkv, 128, generator=g).bfloat16()
    G, blocks = Hq // Hkv, (T + 255) // 256
    rows = {0, 1, 2, T - 2, T - 1}
    for a, b in enumerate(sorted({0, blocks // 2, blocks - 1})):
        for e in range(b * 256 + 64, min((b + 1) * 256, T - 2) + 1, 64):
            rows |= {e - 2, e - 1, e, e + 1}
            for kv, r in ((0, e - 1), (1, e)):
                head = kv * G + (e // 64 + a) % G
                plant(q, k, r, r, head, kv, 1.0, r + 1)
                plant(q, k, r, r + 1, head, kv, 1.0, r + 1)
    plant(q, k, T - 1, 0, 0, 0, 0.5, T)                                             # the first key, for the last row
    plant(q, k, T - 1, T - 1, 0, 0, 0.5, T)
    return [Seq(q, k, sorted(r for r in rows if 0 <= r < T), causal=True, name=f"causal[{T}]")]


def decode_probe(ctxs, max_seq_len, seed=0, scales=None):
    """One decode step: row b attends over ctxs[b] + 1 keys of its pages.  One Seq per row (a single query row at the last key)."""
    g = torch.Generator().manual_seed(3000 + seed + sum(ctxs))
    Hq, Hkv, G = 12, 2, 6
    ns = decode_attn_splits(max_seq_len)
    weights = (0.25, 0.5, 1.0)
    seqs = []
    for b, c in enumerate(ctxs):
        n = c + 1
        q = torch.randn(1, Hq, 128, generator=g).bfloat16()
        k = torch.randn(n, Hkv, 128, generator=g).bfloat16()
        used = min(ns, (n + 255) // 256)
        s = max(1, used // 2)
        rnd = 64 * DECODE_WAVES * ns                                                # second page round of a wave
        edges = [256 * s - 1, 256 * s, 256 * s + 63, 256 * s + 64, 255, 256, rnd - 1, rnd, 256 * (used - 1) - 1, 256 * (used - 1)]
        for a, j in enumerate(boundary_keys(n, edges)):
            kv = a % Hkv
            plant(q, k, 0, j, kv * G + (a // Hkv + b) % G, kv, weights[a % 3], n)
        m = (-n) % 64
        seqs.append(Seq(q, k, [0], tail_k=poison_rows(m, Hkv), tail_v=POISON, n_splits=ns, scales=scales, name=f"row{b}[ctx {c}]"))
    return seqs


# ------------------------------------------------------------------------------------------------ mutants
def _row_mult(seq, lo, hi, f):
    m = torch.ones(1, seq.n, dtype=torch.float64)
    m[:, lo:hi] = f
    return m


def _m_ragged(seq):
    return dict(mult=_row_mult(seq, seq.n // 64 * 64, seq.n, 0.0)) if seq.ragged and seq.tiles > 1 else None


def _m_interior(seq):
    t = seq.tiles // 2
    return dict(mult=_row_mult(seq, 64 * t, 64 * t + 64, 0.0)) if seq.tiles >= 3 else None


def _m_twice(seq):
    t = seq.tiles // 2
    return dict(mult=_row_mult(seq, 64 * t, 64 * t + 64, 2.0)) if seq.tiles >= 3 else None


def _m_last(seq):
    return dict(mult=_row_mult(seq, seq.n - 1, seq.n, 0.0))


def _m_first(seq):
    return dict(mult=_row_mult(seq, 0, 1, 0.0))


def _m_causal_plus(seq):
    return dict(limit_shift=1) if seq.causal else None


def _m_causal_minus(seq):
    return dict(limit_shift=-1) if seq.causal else None


def _m_group_order(seq):
    if seq.n < 16:
        return None
    j = torch.arange(seq.n)
    perm = torch.tensor([0, 1, 2, 3, 8, 9, 10, 11, 4, 5, 6, 7, 12, 13, 14, 15])
    src = j // 16 * 16 + perm[j % 16]
    return dict(vsrc=torch.where(src < seq.n, src, j))


def _m_page_exchange(seq):
    """the ragged last page's table entry exchanged with page 0's: of what now sits last only the first n % 64 keys are inside ctx
    (modelled by that mask effect alone; the poison read in page 0's place only moves the result further)"""
    if seq.n_splits is None or not seq.ragged or seq.tiles < 2:
        return None
    return dict(mult=_row_mult(seq, seq.ragged, 64, 0.0))


def _m_split_missing(seq):
    if seq.n_splits is None:
        return None
    used = min(seq.n_splits, (seq.tiles + DECODE_WAVES - 1) // DECODE_WAVES)
    if used < 2:
        return None
    page = torch.arange(seq.n) // 64
    gone = (page // DECODE_WAVES) % seq.n_splits == used // 2
    return dict(mult=(~gone).double().view(1, -1))


def _m_unmasked(seq):
    return dict(tail=True) if not seq.causal and seq.tail_k is not None and len(seq.tail_k) else None


MUTANTS = {
    "ragged last tile / page dropped": _m_ragged,
    "one interior tile / page dropped": _m_interior,
    "one tile / page counted twice": _m_twice,
    "last key dropped": _m_last,
    "first key dropped": _m_first,
    "causal mask shifted +1": _m_causal_plus,
    "causal mask shifted -1": _m_causal_minus,
    "16-group order not applied": _m_group_order,
    "two page-table entries exchanged": _m_page_exchange,
    "one split left out of the combine": _m_split_missing,
    "keys past ctx not masked": _m_unmasked,
}


# ------------------------------------------------------------------------------------------------ the check
def deviation(got, ref):
    """-> (worst |got - ref| / tolerance over the checked elements, share of elements excluded as 0 < ref < FLOOR, worst relative error)"""
    got, ref = got.double(), ref.double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    zero, low = ref == 0, (ref > 0) & (ref < FLOOR)
    tol = torch.where(zero, torch.full_like(ref, FLOOR), (REL_TOL + OUT_ROUND) * ref)
    err = (got - ref).abs()
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
    ratio = torch.where(low, torch.zeros_like(err), err / tol)
    live = ref >= FLOOR
    rel = float((err[live] / ref[live]).max()) if live.any() else 0.0
    return float(ratio.max()), float(low.sum()) / ref.numel(), rel


def assert_close(got, ref, what):
    worst, excluded, rel = deviation(got, ref)
    assert excluded <= MAX_EXCLUDED, f"{what}: {excluded:.3f} of the elements below the floor"
    assert worst <= 1.0, f"{what}: {worst:.2f} x the tolerance (worst relative error {rel:.4f}, allowed {REL_TOL + OUT_ROUND:.4f})"
    return worst


# ------------------------------------------------------------------------------------------------ the probe configurations (CPU and GPU tests run the same)
MIXED64_LENS = [39648, 19824, 19520, 9216, 5032, 1680]
PREFILL_PROBES = {"a4_19824": [19824], "a3_39648": [39648], "max_56644": [56644], "mixed64_packed": MIXED64_LENS}
CAUSAL_PROBES = {"lm_5200": 5200, "lm_4999": 4999}
DECODE_PROBES = {                                                   # test_decode_attention_matches_oracle's sets + the 64-row x 25-split step
    "one_key": ([0], 64),
    "page_edges": ([1, 63, 64, 65, 0, 127, 128, 255], 640),
    "bench_8x5200": ([5200] * 8, 6224),
    "ragged": ([1, 63, 64, 65, 5200, 6223, 5199, 300], 6224),
    "b9": ([5200 + 100 * i for i in range(9)], 6224),
    "b16_full": ([6223] * 16, 6224),
    "two_rounds_32766": ([32766, 5200, 64], 32768),
    "b21": ([(613 * i) % 1500 + 1 for i in range(21)], 1600),
    "b64_25_splits": ([5150 + (37 * i) % 1000 for i in range(64)], 6288),
}
KV8_SCALES = {"unit": torch.ones(2, 2), "per_head": torch.tensor([[0.015, 0.011], [0.02, 0.03]])}


def build(kind, name, scales=None):
    if kind == "prefill":
        return prefill_probe(PREFILL_PROBES[name], seed=len(name))
    if kind == "causal":
        return causal_probe(CAUSAL_PROBES[name])
    ctxs, max_seq_len = DECODE_PROBES[name]
    return decode_probe(ctxs, max_seq_len, scales=None if scales is None else KV8_SCALES[scales])
