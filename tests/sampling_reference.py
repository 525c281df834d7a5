"""The per-row selection stage restated in numpy and Python ints, the inputs that make it decide, and two mutants of it.

test_sampling_exact_gpu.py feeds the cases below to select_thresh_kernel / select_rows_kernel (Engine.select_tokens) and to the decode
loop and requires EVERY drawn token to be one the definition allows; test_sampling_exact_cpu.py shows without a GPU that on these inputs
the definition is decisive and that a kept set wrong by one key group would be seen.

Definition.  t = (l - max l) * (1 / T), two fp32 operations after an fp32 division (the build has no fast-math: all three are correctly
rounded, and there is no product-sum for the compiler to contract).  In range: t >= -27.  key = bits(0 - t) as uint32 (a smaller key is a
larger t), bin = min(uint32(-t * (2048 / 27)), 2047) in fp32.  Weight w = floor(exp(t) 2^40), here in fp64.
  top-k    with at least top_k tokens in range: keep the keys <= the top_k-th smallest key (ties kept); else keep all in range
  nucleus  z = the kept weight, target = max(1, floor(fp64(fp32(top_p)) * fp64(z))): keep the keys <= the smallest key whose cumulative
           weight over whole key groups, in key order, reaches target
  draw     h = splitmix64(seed ^ splitmix64(n)), u = h / 2^64; the kept token j, in index order, with C_{j-1} <= u Z < C_j
Keys are exact, so the kept set carries no tolerance.  The weights do: the device's __expf(t) is the hardware exp2 (1 ulp) of
t * log2(e) rounded to fp32, and with |t log2 e| <= 39 that rounding is at most 39 * 2^-24 absolute in the exponent, 1.6e-6 relative in
w.  C / Z carries it above and below the bar: 3.3e-6.  DELTA = 2^-16 = 1.5e-5 is more than four times that; the reference accepts every
kept token j with C_{j-1} / Z - DELTA <= u < C_j / Z + DELTA.

The engine-wide sampler (sample_step_kernel, top_p = 1) is restated too: h = splitmix64(seed ^ splitmix64(slot << 32 | pos)),
u = (h >> 40) / 2^24, over e = exp(t) of every token.  Its sums are fp32: at most 149 + 1024 sequential additions and the 16-wave
reduce give about 7e-5 relative in a partial sum; STEP_DELTA = 2^-12 = 2.4e-4 is three times that.

Mutants (of the kept set, in key groups): "drop" loses the last kept key group (exists with >= 2 kept groups), "add" takes the next key
group in range (exists when there is one).  An off-by-one in a radix select, `<` for `<=` at the threshold, a dropped digit pass or a
wrong `before` of a crossing all produce one of the two.

The four conditions on a case's inputs (asserted by test_sampling_exact_cpu.py for every case):
  decisive   the mass fraction before the nucleus boundary group and the fraction including it both differ from top_p by >= 1e-3, far
             above the 3.3e-6 above.  A boundary group with nothing before it is decisive on that side whatever top_p: it is kept as
             soon as target >= 1, which max(1, .) guarantees.
  sensitive  each mutant that exists sends >= 8 of the case's 256 draws outside the accepted sets
  path       the boundary bins hold <= 8192 in-range elements (gathered into LDS) or more (four digit passes over memory), as named
  sharp      the accepted sets hold <= 4 tokens on average
"""
from dataclasses import dataclass, field
from typing import Optional

import numpy as np

V_FULL = 151936
M64 = 2 ** 64 - 1
NONE = 0xFFFFFFFF
TCUT = 27.0
BINS = 2048
CAP = 8192
DELTA = 2.0 ** -16
STEP_DELTA = 2.0 ** -12
DECISIVE = 1e-3
MIN_CAUGHT = 8
MAX_MEAN_ACCEPTED = 4.0
DRAWS = 256
COUNTERS = (0, 1, 2, 3, 37)


def splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def row_u(seed, n):
    """u of the per-row stage: the n-th token of a row with this seed"""
    return splitmix64((seed & M64) ^ splitmix64(n)) / 2.0 ** 64


def step_u(seed, slot, pos):
    """u of the engine-wide sampler"""
    return (splitmix64((seed & M64) ^ splitmix64((slot << 32) | pos)) >> 40) / 2.0 ** 24


def tempered(row, T):
    row = np.asarray(row, np.float32)
    inv = np.float32(1.0) / np.float32(T)
    with np.errstate(invalid="ignore"):
        return ((row - row.max()) * inv).astype(np.float32)


def keys_of(t):
    return (np.float32(0.0) - t).view(np.uint32)


def bins_of(t):
    """bins of in-range values only"""
    scale = np.float32(BINS) / np.float32(TCUT)
    return np.minimum((-t * scale).astype(np.float32).astype(np.uint32), BINS - 1)


def weights_of(t):
    """int64 weights; 0 out of range"""
    inr = t >= -TCUT
    w = np.zeros(t.shape, np.int64)
    w[inr] = np.floor(np.exp(t[inr].astype(np.float64)) * 2.0 ** 40).astype(np.int64)
    return w


def penalised(row, prompt_ids, r):
    """the repetition penalty on ids of the prompt, in fp32 as penalise() (select_dev.h) does it"""
    l = np.asarray(row, np.float32).copy()
    ids = np.unique(np.asarray(prompt_ids, np.int64))
    r = np.float32(r)
    l[ids] = np.where(l[ids] > 0, l[ids] / r, l[ids] * r).astype(np.float32)
    return l


@dataclass
class Kept:
    t: np.ndarray                 # fp32 tempered values
    w: np.ndarray                 # int64 weights, 0 out of range
    keys: np.ndarray
    ukeys: np.ndarray             # distinct in-range keys, ascending
    gcount: np.ndarray            # tokens per key group
    gmass: np.ndarray             # weight per key group (int64)
    n_groups: int                 # key groups kept
    k_groups: Optional[int]       # groups top-k keeps (None: top-k keeps all in range)
    frac_before: Optional[float] = None      # nucleus: mass fraction before / including the boundary group
    frac_incl: Optional[float] = None
    path: str = "none"            # "unfiltered" | "none" (no boundary bin) | "gathered" | "memory"
    info: dict = field(default_factory=dict)

    def mask(self, n_groups=None):
        n = self.n_groups if n_groups is None else n_groups
        return (self.t >= -TCUT) & (self.keys <= self.ukeys[n - 1])

    def mutants(self):
        out = {}
        if self.n_groups >= 2:
            out["drop"] = self.mask(self.n_groups - 1)
        if self.n_groups < len(self.ukeys):
            out["add"] = self.mask(self.n_groups + 1)
        return out


def _first_reaching(cum, target):
    """index of the first entry of the inclusive prefix sums that reaches target, or None"""
    i = int(np.searchsorted(cum, target, side="left"))
    return i if i < len(cum) else None


def kept_set(row, T, top_k=0, top_p=1.0):
    """the kept set of a row (already penalised) and the code path the stage takes to it"""
    t = tempered(row, T)
    inr = t >= -TCUT
    keys, w = keys_of(t), weights_of(t)
    order = np.argsort(keys[inr], kind="stable")
    ks, ws = keys[inr][order], w[inr][order]
    ukeys, start, gcount = np.unique(ks, return_index=True, return_counts=True)
    gmass = np.add.reduceat(ws, start)
    use_k, use_p = top_k > 0, np.float32(top_p) < np.float32(1.0)
    K = Kept(t, w, keys, ukeys, gcount, gmass, len(ukeys), None)
    if not use_k and not use_p:
        K.path = "unfiltered"
        return K
    # ---- the kept set, by the definition
    if use_k and len(ks) >= top_k:
        K.k_groups = int(np.searchsorted(ukeys, ks[top_k - 1])) + 1
        K.n_groups = K.k_groups
    if use_p:
        cum = np.cumsum(gmass[:K.n_groups])
        z = int(cum[-1])
        target = max(1, int(np.float64(np.float32(top_p)) * np.float64(z)))
        g = _first_reaching(cum, target)
        if g is not None:
            K.n_groups = g + 1
            K.frac_before = float(cum[g] - gmass[g]) / z
            K.frac_incl = float(cum[g]) / z
    # ---- the path, as sel_threshold picks it from its histogram
    b = bins_of(t[inr])
    hc = np.bincount(b, minlength=BINS).astype(np.int64)
    hm = np.bincount(b, weights=w[inr].astype(np.float64), minlength=BINS)          # fp64 masses: only bins are read off them
    kb = _first_reaching(np.cumsum(hc), top_k) if use_k else None
    pb = None
    if use_p:
        zlo = hm.sum() if kb is None else hm[:kb].sum()
        pb = _first_reaching(np.cumsum(hm), max(1.0, np.floor(np.float64(np.float32(top_p)) * zlo)))
        if pb is None:
            pb = kb
    g_lo = g_hi = kb
    if pb is not None:
        g_lo = pb if g_lo is None else min(g_lo, pb)
        g_hi = pb if g_hi is None else g_hi
    K.info = dict(kb=kb, pb_lo=pb, g_lo=g_lo, g_hi=g_hi, count_kb=None if kb is None else int(hc[kb]),
                  count_pb=None if pb is None else int(hc[pb]))
    if g_lo is not None:
        n = int(hc[g_lo:g_hi + 1].sum())
        K.info["n_boundary"] = n
        K.path = "gathered" if n <= CAP else "memory"
        # the bin the nucleus ends in, after top-k cut bin kb down to its kept part
        if use_p:
            last = ukeys[K.n_groups - 1]
            K.info["p_bin"] = int(bins_of(-(np.array([last], np.uint32).view(np.float32)))[0])
    return K


@dataclass
class Cdf:
    idx: np.ndarray               # kept tokens in index order
    lo: np.ndarray                # C_{j-1} / Z
    hi: np.ndarray                # C_j / Z

    def accepted(self, u, delta):
        a = int(np.searchsorted(self.hi, u - delta, side="right"))               # first j with hi_j + delta > u
        b = int(np.searchsorted(self.lo, u + delta, side="right"))               # one past the last j with lo_j - delta <= u
        return self.idx[a:b]

    def exact(self, u):
        return int(self.idx[min(int(np.searchsorted(self.hi, u, side="right")), len(self.idx) - 1)])

    def distance(self, u, tok):
        """how far outside token tok's own interval u lies (0 inside); None when tok is not kept"""
        j = int(np.searchsorted(self.idx, tok))
        if j >= len(self.idx) or self.idx[j] != tok:
            return None
        return max(self.lo[j] - u, u - self.hi[j], 0.0)

    def margin(self, u, tok):
        """how far inside token tok's own interval u lies: the distance to the nearer edge (<= 0 outside)"""
        j = int(np.searchsorted(self.idx, tok))
        return min(u - self.lo[j], self.hi[j] - u)


def cdf_of(w, mask=None):
    """the inverse-CDF table of integer (or fp64) weights w over the tokens of mask with weight"""
    wk = np.where(mask, w, 0) if mask is not None else w
    idx = np.flatnonzero(wk > 0)
    c = np.cumsum(wk[idx])
    z = float(c[-1])
    return Cdf(idx, (c - wk[idx]) / z, c / z)


def step_cdf(row, T):
    """the engine-wide sampler at top_p = 1: every token, weight exp(t) (t below -27 included: this sampler has no cut)"""
    t = tempered(row, T).astype(np.float64)
    return cdf_of(np.exp(t))


# ------------------------------------------------------------------------------------------------ cases
@dataclass
class Case:
    name: str
    row: np.ndarray               # fp32 logits [V]
    T: float
    top_k: int = 0
    top_p: float = 1.0
    path: str = "gathered"        # what Kept.path must be
    keeps: Optional[int] = None   # tokens the kept set must hold, where the table of the issue names it
    prompt: tuple = (0,)          # ids of the prompt part of the history
    fill: int = 0                 # the id generated tokens are made of
    repetition_penalty: float = 1.0
    expect: dict = field(default_factory=dict)       # further facts of Kept.info the case is about

    @property
    def V(self):
        return len(self.row)

    def shaped(self):
        return penalised(self.row, self.prompt, self.repetition_penalty) if self.repetition_penalty != 1.0 else self.row

    def kept(self):
        return kept_set(self.shaped(), self.T, self.top_k, self.top_p)


def seeds():
    """256 seeds: the corners of uint64 and a spread of the rest"""
    rng = np.random.default_rng(2024)
    s = [0, 2 ** 63, 2 ** 64 - 1, 1, 2 ** 32, 2 ** 32 - 1]
    s += [int(x) for x in rng.integers(0, 2 ** 64, DRAWS - len(s), dtype=np.uint64)]
    return s


def draws():
    """(seed, n) of a case's 256 draws: row r of call c has seed number 64 c + r and counter COUNTERS[(64 c + r) % 5]"""
    return [(s, COUNTERS[i % len(COUNTERS)]) for i, s in enumerate(seeds())]


def _tail(rng, V=V_FULL, sd=1.0):
    return rng.normal(0.0, sd, V).astype(np.float32)


TIE_VALUES = (9, 8.5, 8.25, 8, 8, 8, 8, 7.5, 7.5, 7.25, 7, 6.5)


def _tie_row():
    rng = np.random.default_rng(101)
    l = _tail(rng)
    ids = rng.choice(V_FULL, len(TIE_VALUES), replace=False)
    l[ids] = np.array(TIE_VALUES, np.float32)
    return l, [int(i) for i in ids]


def _cap_row(n_bin):
    """a head of 3 ids, one bin of exactly n_bin elements in 4 tied groups, the rest 14-26 below the maximum"""
    rng = np.random.default_rng(105)
    l = np.clip(rng.normal(-18.0, 1.5, V_FULL), -26.0, -14.0).astype(np.float32)
    ids = rng.permutation(V_FULL)
    l[ids[:3]] = np.array([0.0, -1.0, -2.0], np.float32)
    sizes = [2048, 2048, 2048, n_bin - 3 * 2048]
    vals = [-4.998, -5.001, -5.004, -5.007]                # all in bin 379 = (-5.0098, -4.9966]: the CPU test counts the bin
    at = 3
    for s, v in zip(sizes, vals):
        l[ids[at:at + s]] = np.float32(v)
        at += s
    return l


def _ragged_row(V):
    rng = np.random.default_rng(1000 + V)
    l = rng.choice(np.array([-0.5, 0.0, 0.5, 1.0], np.float32), V).astype(np.float32)
    l[0] = l[V - 1] = 2.0
    return l


def cases():
    out = []
    # top-k tie: ties at the k-th key, by-count select over a gathered bin
    l, ids = _tie_row()
    out.append(Case("tie_k5", l, 1.0, top_k=5, keeps=7))
    out.append(Case("tie_k8", l, 1.0, top_k=8, keeps=9))
    # shaped row: the repetition penalty takes two of the four 8s to 8 / 1.1 = 7.27, between 7.5 and 7.25; the generated ids are the
    # filler of the prompt, so the shaped values are the same for every counter
    tie8 = [i for i, v in zip(ids, TIE_VALUES) if v == 8]
    filler = int(np.argmin(l))
    pr = (tie8[1], tie8[3], filler)
    out.append(Case("shaped_k5", l, 1.0, top_k=5, keeps=5, prompt=pr, fill=filler, repetition_penalty=1.1))
    out.append(Case("shaped_k8", l, 1.0, top_k=8, keeps=9, prompt=pr, fill=filler, repetition_penalty=1.1))
    # nucleus in the top-k bin: 8 ids inside bin 0, uneven steps so that 3 of 6 is 0.5013 of the mass, not 0.5
    rng = np.random.default_rng(102)
    l = _tail(rng)
    ids = rng.choice(V_FULL, 8, replace=False)
    l[ids] = np.float32(8.0) - np.array([0, 0.0005, 0.001, 0.005, 0.0055, 0.006, 0.0065, 0.007], np.float32)
    out.append(Case("kbin_p50", l, 1.0, top_k=6, top_p=0.5, keeps=3, expect=dict(p_bin_is_kb=True)))
    out.append(Case("kbin_p99", l, 1.0, top_k=6, top_p=0.99, keeps=6, expect=dict(p_bin_is_kb=True)))
    # nucleus only: 6 heavy ids, everything else below -27 T
    rng = np.random.default_rng(103)
    l = (-10.0 - np.abs(rng.normal(0.0, 1.0, V_FULL))).astype(np.float32)
    ids = rng.choice(V_FULL, 6, replace=False)
    l[ids] = np.array([10.0, 9.8, 9.5, 9.0, 8.6, 8.0], np.float32)
    out.append(Case("nucleus_only", l, 0.5, top_p=0.6, keeps=2, expect=dict(kb=None, far_bin=True)))
    # hot row: tied groups, every boundary bin above the LDS cap (clipped to +-4 so that the bin edges, which hang on the maximum, are
    # the same for any generator: at T 100 a bin is 1.32 wide in the logits)
    rng = np.random.default_rng(104)
    l = np.clip(np.round(rng.normal(0.0, 1.0, V_FULL) * 4) / 4, -4.0, 4.0).astype(np.float32)
    out.append(Case("hot_k", l, 100.0, top_k=20000, path="memory", expect=dict(boundary_bins_over_cap=True)))
    out.append(Case("hot_p", l, 100.0, top_p=0.5, path="memory", expect=dict(kb=None, boundary_bins_over_cap=True)))
    out.append(Case("hot_kp", l, 100.0, top_k=50000, top_p=0.7, path="memory", expect=dict(pb_below_kb=True, boundary_bins_over_cap=True)))
    # LDS cap edge: n <= SEL_CAP on both sides; k ends in the second tied group
    out.append(Case("cap_8192", _cap_row(8192), 1.0, top_k=3 + 2048 + 100, path="gathered", keeps=3 + 4096, expect=dict(n_boundary=8192)))
    out.append(Case("cap_8193", _cap_row(8193), 1.0, top_k=3 + 2048 + 100, path="memory", keeps=3 + 4096, expect=dict(n_boundary=8193)))
    # k beyond the range: N(0, 3) at T 0.05 leaves what lies within 1.35 of the maximum.  Three ids are planted on top (0.02 apart:
    # t = 0, -0.4, -0.8) so that the last kept group carries weight and the "drop" mutant is visible; the tail stays out of range.
    rng = np.random.default_rng(106)
    l = _tail(rng, sd=3.0)
    ids = rng.choice(V_FULL, 3, replace=False)
    l[ids] = np.float32(l.max()) + np.array([2.0, 1.98, 1.96], np.float32)
    out.append(Case("k_is_V", l, 0.05, top_k=V_FULL, path="none", keeps=3, expect=dict(kb=None)))
    out.append(Case("k_is_max", l, 0.05, top_k=2 ** 31 - 1, path="none", keeps=3, expect=dict(kb=None)))
    # tiny top_p: exactly the tied maxima; a heavy runner-up makes the "add" mutant visible
    rng = np.random.default_rng(107)
    l = _tail(rng)
    ids = rng.choice(V_FULL, 3, replace=False)
    l[ids] = np.array([12.0, 12.0, 11.5], np.float32)
    out.append(Case("tiny_p", l, 0.7, top_p=1e-6, keeps=2))
    # -inf rows
    rng = np.random.default_rng(108)
    l = np.full(V_FULL, -np.inf, np.float32)
    ids = rng.choice(V_FULL, 3, replace=False)
    l[ids] = np.array([1.0, 0.5, 0.0], np.float32)
    out.append(Case("inf_unfiltered", l, 1.0, path="unfiltered", keeps=3))
    out.append(Case("inf_k2", l, 1.0, top_k=2, keeps=2))
    # small and ragged V: index 0 and V - 1 heavy
    for V in (1, 2, 63, 64, 65, 1000, 1025, 1087):
        l = _ragged_row(V)
        out.append(Case(f"ragged_{V}_kp", l, 0.9, top_k=3, top_p=0.8, path="gathered"))
        out.append(Case(f"ragged_{V}_all", l, 0.9, path="unfiltered", keeps=V))
    return out
