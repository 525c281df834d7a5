// Device arithmetic of a sampled row of the per-row selection stage: the kept set (steps 1-2, sel_threshold) and the draw
// (step 3, sel_draw).  ONE definition: select_thresh_kernel / select_rows_kernel (decode.hip) run it on the rows of a step, the draft-row
// kernels of a speculating step (spec.hip) run it on the draft rows of sampled slots with the counter of the output index the
// row stands for, so a draft row's candidate is the token the sequential step would have drawn there, bit for bit.
//   tempered values t_i = (l_i - m) / T, integer weights w_i = floor(exp(t_i) 2^40) (t_i >= -27; below that w_i = 0), keys
//   k_i = bits(-t_i) (monotone: a smaller key is a larger t); every sum is an integer sum, so no result depends on the order of the atomics.
// Before them, what the stage and the draft-row kernels share about a row whatever its temperature: which features it carries in a launch
// (row_ruled .. row_penalised), the value a token is selected from (shape_logit) and the commit of a selected token (commit_row).
// Every function from sel_key on is called by all SEL_THREADS threads of a workgroup with uniform arguments.
#pragma once
#include "common.h"
#include "kernels.h"
#include "step_dev.h"

constexpr int SEL_THREADS = 1024, SEL_BINS = 2048, SEL_CAP = 8192, SEL_DIG = 256;
constexpr float SEL_TCUT = 27.0f;
constexpr float SEL_BIN_SCALE = (float)SEL_BINS / SEL_TCUT;
constexpr uint32_t SEL_NONE = 0xffffffffu;

DEVI uint64_t splitmix64(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

DEVI bool row_has_pen(const RowParams& p) { return p.repetition_penalty != 1.0f || p.frequency_penalty != 0.0f || p.presence_penalty != 0.0f; }

// does row b carry logit rules in this launch (uniform per workgroup)
DEVI bool row_ruled(const RowSel& rs, int b) { return rs.rules && (rs.rules[b].flags & RULE_ON); }
// does row b hold a guide in this launch (uniform per workgroup)
DEVI bool row_guided(const RowSel& rs, int b) { return rs.guide.rows && rs.guide.rows[b].table; }
// does row b carry an n-gram rule in this launch (uniform per workgroup)
DEVI bool row_ngram(const RowSel& rs, int b) { return rs.ngram.rows && rs.ngram.rows[b].n > 0; }

// does row b hold a loop rule in this launch (uniform per workgroup)
DEVI bool row_looped(const RowSel& rs, int b) { return rs.loop.rows && rs.loop.rows[b].max_period > 0; }

// is row b penalised in this launch (uniform per workgroup): the counts exist, the stage owns the row (the entry of a row it does not own
// is not parameters) and its parameters carry a penalty
DEVI bool row_penalised(const RowSel& rs, int b) { return rs.cnt && rs.own[b] != 0 && row_has_pen(rs.params[b]); }

// HF / vLLM repetition penalty on every token seen in the prompt or the output, then OpenAI frequency / presence on the output counts
DEVI float penalise(float l, int c, bool seen_prompt, const RowParams& p) {
    if ((seen_prompt || c > 0) && p.repetition_penalty != 1.0f) l = l > 0.f ? l / p.repetition_penalty : l * p.repetition_penalty;
    if (c > 0) l = l - (p.frequency_penalty * (float)c + p.presence_penalty);
    return l;
}

// The value token i of a row is selected from, from its logit l.  ONE definition: select_partial_kernel
// (decode.hip) shapes the rows of a step with it, spec_shape_select_kernel (spec.hip) the draft rows of a speculating step.
// In vLLM's order: l + the rule image (-inf: banned / not allowed); -inf for an EOS / stop id of the kill list (below min_tokens, or on a
// guided row whose state is not accepting: the guide's bit does not speak for such an id), else -inf where the guide's bit is clear; -inf
// where the n-gram bit is set; then the penalties on that value (-inf stays -inf: r > 0 and the subtrahend is finite).
// RowShape: what the row carries, uniform per workgroup; a null pointer = the row has no such feature.  drafts: the tokens a draft row
// takes as committed before it, counted on top of cnt (a row of a plain step has none).
struct RowShape {
    const float* img;          // its row of the rule image
    const uint32_t* gbits;     // its allowed bits (a guide)
    const uint32_t* nbits;     // its banned bits (an n-gram rule)
    const int32_t* cnt;        // its output counts: != nullptr = the row is penalised
    const uint32_t* seen;      // its prompt-presence bits (with cnt)
    const int* kill;           // LDS: the EOS / stop ids that fall into the workgroup's chunk
    int n_kill;
    bool kill_on;              // what such an id gets: true = -inf
    const int32_t* drafts;     // LDS
    int n_drafts;
};
DEVI float shape_logit(float l, int i, const RowShape& s, const RowParams& p) {
    if (s.img) l += s.img[i];
    bool term = false;
    for (int k = 0; k < s.n_kill; ++k) term = term || s.kill[k] == i;
    if (term ? s.kill_on : (s.gbits && !((s.gbits[i >> 5] >> (i & 31)) & 1u))) l = -INFINITY;
    if (s.nbits && ((s.nbits[i >> 5] >> (i & 31)) & 1u)) l = -INFINITY;
    if (s.cnt) {
        int c = s.cnt[i];
        for (int k = 0; k < s.n_drafts; ++k) c += s.drafts[k] == i;
        l = penalise(l, c, (s.seen[i >> 5] >> (i & 31)) & 1u, p);
    }
    return l;
}

// The commit of a row the per-row stage owns: the output count of an unfinished penalised row (pen: the row's parameters carry a penalty and
// the counts exist), then commit_token with the row's rules, the guides and the stop automata of the launch.  ONE definition:
// select_rows_kernel commits the rows of a step with it, spec_accept_kernel (spec.hip) every token of its walk.
// Returns commit_token's answer (step_dev.h COMMIT_*).
DEVI int commit_row(const StepState& st, const RowSel& rs, int b, int V, bool pen, int tok) {
    if (pen && !st.finished[b] && tok >= 0 && tok < V) rs.cnt[(size_t)b * V + tok] += 1;     // output counts of the rows with penalties
    return commit_token(st, b, tok, row_ruled(rs, b) ? rs.rules + b : nullptr, rs.guide.rows ? &rs.guide : nullptr, rs.stop.rows ? &rs.stop : nullptr);
}

DEVI uint32_t sel_key(float t) { return __float_as_uint(0.f - t); }              // 0 - (+-0) = +0: the maximum has key 0
DEVI float sel_t(uint32_t key) { return -__uint_as_float(key); }
DEVI bool sel_in(float t) { return t >= -SEL_TCUT; }
DEVI uint32_t sel_bin(float t) { return min((uint32_t)(-t * SEL_BIN_SCALE), (uint32_t)(SEL_BINS - 1)); }
DEVI uint64_t sel_w(float t) { return (uint64_t)(__expf(t) * 1099511627776.0f); }      // 2^40; t in [-27, 0]

// Wave 0 scans h[0, 64 * PER) and finds the first entry whose inclusive prefix sum reaches target: .bin (SEL_NONE when the total stays
// below it) and .before = the sum of the entries before it (the total when none).  Every thread must call; the result is in registers.
struct Cross { uint32_t bin; uint64_t before; };
template <int PER, typename T>
DEVI Cross find_cross(const T* h, uint64_t target, Cross* xch) {
    if (threadIdx.x < 64) {
        const int lane = threadIdx.x;
        uint64_t s = 0;
        for (int j = 0; j < PER; ++j) s += h[lane * PER + j];
        uint64_t incl = s;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint64_t v = __shfl_up(incl, o, 64);
            if (lane >= o) incl += v;
        }
        const uint64_t hit = __ballot(incl >= target);
        if (hit == 0) {
            if (lane == 63) { xch->bin = SEL_NONE; xch->before = incl; }
        } else if (lane == __ffsll((unsigned long long)hit) - 1) {
            uint64_t acc = incl - s;
            int j = 0;
            for (; j < PER - 1; ++j) {
                if (acc + h[lane * PER + j] >= target) break;
                acc += h[lane * PER + j];
            }
            xch->bin = lane * PER + j;
            xch->before = acc;
        }
    }
    __syncthreads();
    const Cross r = *xch;
    __syncthreads();                                                     // xch may be reused at once
    return r;
}

// sum of h[0, n) (every thread must call)
template <int PER, typename T>
DEVI uint64_t sum_below(const T* h, uint32_t n, uint64_t* xch) {
    if (threadIdx.x < 64) {
        uint64_t s = 0;
        for (int j = 0; j < PER; ++j) s += (uint32_t)(threadIdx.x * PER + j) < n ? (uint64_t)h[threadIdx.x * PER + j] : 0;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        if (threadIdx.x == 0) *xch = s;
    }
    __syncthreads();
    const uint64_t r = *xch;
    __syncthreads();
    return r;
}

struct SelLds {
    uint32_t h0_cnt[SEL_BINS];
    uint64_t h0_mass[SEL_BINS];
    uint32_t d_cnt[SEL_DIG];
    uint64_t d_mass[SEL_DIG];
    uint32_t cand[SEL_CAP];
    uint32_t n_cand;
    Cross cr;
    uint64_t tmp, cnt_le, mass_le;
    float best;
    int bi, tok;
};

// Exact radix select over the elements that each() visits (key, weight): the smallest key K whose cumulative count (by_mass = 0) or
// weight (1) over the keys <= K reaches target (>= 1, <= the total).  Returns K; L.cnt_le / L.mass_le = count / weight of the keys <= K.
template <typename Each>
DEVI uint32_t radix_select(Each each, uint64_t target, bool by_mass, SelLds& L) {
    uint32_t prefix = 0;
    uint64_t cnt_before = 0, mass_before = 0;
    for (int shift = 24; shift >= 0; shift -= 8) {
        for (int j = threadIdx.x; j < SEL_DIG; j += SEL_THREADS) { L.d_cnt[j] = 0; L.d_mass[j] = 0; }
        __syncthreads();
        const uint64_t hi_mask = shift == 24 ? 0 : ~0ull << (shift + 8);
        each([&](uint32_t key, uint64_t w) {
            if (((uint64_t)key & hi_mask) != ((uint64_t)prefix & hi_mask)) return;
            const uint32_t d = (key >> shift) & (SEL_DIG - 1);
            atomicAdd(&L.d_cnt[d], 1u);
            if (w) atomicAdd((unsigned long long*)&L.d_mass[d], (unsigned long long)w);
        });
        __syncthreads();
        const Cross c = by_mass ? find_cross<SEL_DIG / 64>(L.d_mass, target, &L.cr) : find_cross<SEL_DIG / 64>(L.d_cnt, target, &L.cr);
        const uint32_t d = c.bin;
        const uint64_t bef = c.before;
        const uint64_t other = by_mass ? sum_below<SEL_DIG / 64>(L.d_cnt, d, &L.tmp) : sum_below<SEL_DIG / 64>(L.d_mass, d, &L.tmp);
        if (by_mass) { mass_before += bef; cnt_before += other; } else { cnt_before += bef; mass_before += other; }
        target -= bef;
        prefix |= d << shift;
        if (shift == 0) { L.cnt_le = cnt_before + L.d_cnt[d]; L.mass_le = mass_before + L.d_mass[d]; }
        __syncthreads();
    }
    return prefix;
}

// the merged arg max partials of row b -> *o_best / *o_bi (every thread must call)
DEVI void merge_partials(const float* __restrict__ pval, const int32_t* __restrict__ pidx, int b, float* o_best, int* o_bi) {
    if (threadIdx.x < 64) {
        float best = pval[b * ARGMAX_CHUNKS + threadIdx.x];
        int bi = pidx[b * ARGMAX_CHUNKS + threadIdx.x];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) argmax_merge(best, bi, __shfl_xor(best, o, 64), __shfl_xor(bi, o, 64));
        if (threadIdx.x == 0) { *o_best = best; *o_bi = bi; }
    }
    __syncthreads();
}

// no top-k and no top-p: every token with weight is kept (the threshold is SEL_NONE, no read of the row)
DEVI bool sel_unfiltered(const RowParams& p) { return p.top_k <= 0 && !(p.top_p < 1.0f); }

// Steps 1-2 of a sampled row with a filter (temperature > 0, !sel_unfiltered(p)): *thr = the largest key the row keeps.
//   row  V values: the logits, or the shaped values of a row with penalties / rules / a guide / an n-gram rule
//   m    their maximum (the merged arg-max partials)
DEVI void sel_threshold(const float* __restrict__ row, int V, const RowParams& p, float m, uint32_t* thr, SelLds& L) {
    const int tid = threadIdx.x;
    const float inv_t = 1.0f / p.temperature;

    // ---- 1. histogram of the tempered values
    for (int j = tid; j < SEL_BINS; j += SEL_THREADS) { L.h0_cnt[j] = 0; L.h0_mass[j] = 0; }
    if (tid == 0) L.n_cand = 0;
    __syncthreads();
    for (int i = tid; i < V; i += SEL_THREADS) {          // coalesced: order does not matter here
        const float t = (row[i] - m) * inv_t;
        if (!sel_in(t)) continue;
        const uint32_t bn = sel_bin(t);
        atomicAdd(&L.h0_cnt[bn], 1u);
        atomicAdd((unsigned long long*)&L.h0_mass[bn], (unsigned long long)sel_w(t));
    }
    __syncthreads();

    const bool use_k = p.top_k > 0, use_p = p.top_p < 1.0f;
    uint32_t kb = SEL_NONE;                                              // bin of the k-th largest value (SEL_NONE: top-k keeps all)
    uint64_t k_before = 0;
    if (use_k) {
        const Cross c = find_cross<SEL_BINS / 64>(L.h0_cnt, (uint64_t)p.top_k, &L.cr);
        kb = c.bin;
        k_before = c.before;
    }
    const uint64_t z_all = sum_below<SEL_BINS / 64>(L.h0_mass, SEL_BINS, &L.tmp);
    const uint64_t m_below_kb = kb == SEL_NONE ? z_all : sum_below<SEL_BINS / 64>(L.h0_mass, kb, &L.tmp);
    // bins that can hold the nucleus boundary: the kept mass lies in [m_below_kb, m_below_kb + mass(kb)]
    uint32_t pb_lo = SEL_NONE;
    if (use_p) {
        const uint64_t zlo = kb == SEL_NONE ? z_all : m_below_kb;
        const Cross c = find_cross<SEL_BINS / 64>(L.h0_mass, max((uint64_t)1, (uint64_t)((double)p.top_p * (double)zlo)), &L.cr);
        pb_lo = c.bin == SEL_NONE ? kb : c.bin;
    }
    // ---- 2. gather the candidate bins [g_lo, g_hi] into LDS when they fit
    uint32_t g_lo = SEL_NONE, g_hi = SEL_NONE;
    if (kb != SEL_NONE) { g_lo = kb; g_hi = kb; }
    if (use_p && pb_lo != SEL_NONE) { g_lo = min(g_lo, pb_lo); g_hi = g_hi == SEL_NONE ? pb_lo : g_hi; }
    bool gathered = false;
    if (g_lo != SEL_NONE) {
        const uint64_t n = sum_below<SEL_BINS / 64>(L.h0_cnt, g_hi + 1, &L.tmp) - sum_below<SEL_BINS / 64>(L.h0_cnt, g_lo, &L.tmp);
        if (n <= SEL_CAP) {
            for (int i = tid; i < V; i += SEL_THREADS) {          // coalesced: order does not matter here
                const float t = (row[i] - m) * inv_t;
                if (!sel_in(t)) continue;
                const uint32_t bn = sel_bin(t);
                if (bn < g_lo || bn > g_hi) continue;
                const uint32_t j = atomicAdd(&L.n_cand, 1u);
                if (j < SEL_CAP) L.cand[j] = sel_key(t);         // the histogram counted exactly these: j < SEL_CAP
            }
            __syncthreads();
            gathered = true;
        }
    }
    // visit every element of bin bn with key <= kmax: from LDS when gathered, else from memory
    auto in_bin = [&](uint32_t bn, uint32_t kmax) {
        const bool lds = gathered && bn >= g_lo && bn <= g_hi;
        return [&, bn, kmax, lds](auto fn) {
            if (lds) {
                const int n = (int)min(L.n_cand, (uint32_t)SEL_CAP);
                for (int j = tid; j < n; j += SEL_THREADS) {
                    const uint32_t key = L.cand[j];
                    const float t = sel_t(key);
                    if (sel_bin(t) == bn && key <= kmax) fn(key, sel_w(t));
                }
            } else {
                for (int i = tid; i < V; i += SEL_THREADS) {          // coalesced: order does not matter here
                    const float t = (row[i] - m) * inv_t;
                    if (!sel_in(t) || sel_bin(t) != bn) continue;
                    const uint32_t key = sel_key(t);
                    if (key <= kmax) fn(key, sel_w(t));
                }
            }
        };
    };
    uint32_t kmax = SEL_NONE;                                            // keep the keys <= kmax
    uint64_t z = z_all;                                                  // their total weight
    if (kb != SEL_NONE) {
        kmax = radix_select(in_bin(kb, SEL_NONE), (uint64_t)p.top_k - k_before, false, L);
        z = m_below_kb + L.mass_le;
    }
    if (use_p) {
        const uint64_t target = max((uint64_t)1, (uint64_t)((double)p.top_p * (double)z));
        if (kb != SEL_NONE) {                                            // the kept part of bin kb only
            if (tid == 0) L.h0_mass[kb] = z - m_below_kb;
            for (int j = kb + 1 + tid; j < SEL_BINS; j += SEL_THREADS) L.h0_mass[j] = 0;
            __syncthreads();
        }
        const Cross c = find_cross<SEL_BINS / 64>(L.h0_mass, target, &L.cr);
        if (c.bin != SEL_NONE) kmax = radix_select(in_bin(c.bin, c.bin == kb ? kmax : SEL_NONE), target - c.before, true, L);
    }
    if (tid == 0) *thr = kmax;
}

// Step 3 of a sampled row (temperature > 0): inverse CDF in index order over the kept weights (keys <= kmax),
// x = floor(h 2^-64 * total), h = splitmix64(seed ^ splitmix64(n)), n = the output index the token is drawn for.  Returns the token to every
// thread, or -1 when nothing carries weight (a numerical corner: the caller takes the arg max).
// Wave w owns the contiguous segment [w seg, (w + 1) seg) and walks it 64 consecutive elements at a time (coalesced loads); the segment
// sums locate the wave holding x, which walks its segment once more with a wave-wide inclusive scan per 64 elements.
struct DrawLds {
    uint64_t part[SEL_THREADS / 64], before;
    int tok, wave;
};
DEVI int sel_draw(const float* __restrict__ row, int V, const RowParams& p, float m, uint32_t kmax, uint32_t n, DrawLds& D) {
    constexpr int NWV = SEL_THREADS / 64;
    const int tid = threadIdx.x;
    const float inv_t = 1.0f / p.temperature;
    const int wave = tid >> 6, lane = tid & 63;
    const int seg = (V + NWV - 1) / NWV;
    const int lo = min(V, wave * seg), hi = min(V, lo + seg);
    auto weight = [&](int i) -> uint64_t {
        if (i >= hi) return 0;
        const float t = (row[i] - m) * inv_t;
        return sel_in(t) && sel_key(t) <= kmax ? sel_w(t) : 0;
    };
    uint64_t s = 0;
    for (int i = lo + lane; i < hi; i += 64) s += weight(i);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0) D.part[wave] = s;
    __syncthreads();
    const uint64_t h = splitmix64(p.seed ^ splitmix64((uint64_t)n));
    if (tid == 0) {
        uint64_t total = 0;
        for (int w = 0; w < NWV; ++w) total += D.part[w];
        const uint64_t x = __umul64hi(h, total);                         // floor(h 2^-64 total) < total
        uint64_t acc = 0;
        int w = 0;
        for (; w < NWV - 1; ++w) {
            if (acc + D.part[w] > x) break;
            acc += D.part[w];
        }
        D.wave = w;
        D.before = acc;
        D.tok = -1;
    }
    __syncthreads();
    if (wave == D.wave) {
        uint64_t total = 0;
        for (int w = 0; w < NWV; ++w) total += D.part[w];
        const uint64_t x = __umul64hi(h, total);
        uint64_t acc = D.before;
        for (int base = lo; base < hi; base += 64) {
            const uint64_t w = weight(base + lane);
            uint64_t incl = w;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const uint64_t v = __shfl_up(incl, o, 64);
                if (lane >= o) incl += v;
            }
            const uint64_t hit = __ballot(w > 0 && acc + incl > x);
            if (hit) {
                if (lane == __ffsll((unsigned long long)hit) - 1) D.tok = base + lane;
                break;
            }
            acc += __shfl(incl, 63, 64);
        }
    }
    __syncthreads();
    return D.tok;
}
