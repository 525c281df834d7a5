// Device pieces of the logprobs stage shared by logprobs.hip and beam.hip: the ranking rule of the top
// lists, the one pass over a vocabulary chunk that leaves its partials (lp_partial_chunk: logprob_partial_kernel for the rows of a step,
// spec_logprob_partial_kernel for the draft rows of a speculating one) and the fixed-order final reduction over a row's LP_CHUNKS
// per-chunk partials.  The final kernels run theirs with ONE wave whose lane c owns chunk c, so a row's log-sum-exp and sorted top-n are
// the same bits wherever they are taken.
#pragma once
#include "common.h"
#include "kernels.h"

constexpr int LP_NONE = 0x7fffffff;                             // index of "no candidate"

// (va, ia) ranks before (vb, ib): larger value, then lower index (the arg max tie rule).  NaN never ranks before anything.
DEVI bool lp_before(float va, int ia, float vb, int ib) { return va > vb || (va == vb && ia < ib); }

DEVI void lp_wave_best(float& v, int& i) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(v, o, 64);
        const int oi = __shfl_xor(i, o, 64);
        if (lp_before(ov, oi, v, i)) { v = ov; i = oi; }
    }
}

constexpr int LP_THREADS = 256;
constexpr int LP_VEC = LP_MAX_CHUNK / (4 * LP_THREADS);         // float4 loads per thread (4)
constexpr int LP_REG = 4 * LP_VEC;                              // values per thread held in registers (16)
static_assert(LP_REG <= 32, "one availability bit per register value");
DEVI int lp_chunk_len(int V) { return (((V + LP_CHUNKS - 1) / LP_CHUNKS) + 3) & ~3; }

// What one chunk's pass stages in LDS: the waves' terms of the maximum and of the sum, and their top lists
struct LpPartialLds {
    float red[LP_THREADS / 64];
    float wv[LP_THREADS / 64][DOTS_MAX_TOP_LOGPROBS];
    int wi[LP_THREADS / 64][DOTS_MAX_TOP_LOGPROBS];
};

// Chunk c of logits row `row` (V values; the row is row b of a matrix whose base is `base` with leading dimension ld: alignment decides
// float4 loads) -> (m_c, s_c = sum exp(l - m_c)) and the chunk's top-n (value, index) pairs in row b of part_ms / part_v / part_i.  The
// LP_THREADS threads of a workgroup call it together (it holds workgroup barriers); b, c and n are uniform.
DEVI void lp_partial_chunk(LpPartialLds& L, const float* __restrict__ base, int V, int ld, int b, int c, int n, float* __restrict__ part_ms,
                           float* __restrict__ part_v, int32_t* __restrict__ part_i) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int per = lp_chunk_len(V);
    const int lo = c * per, hi = min(V, lo + per);
    const float* row = base + (size_t)b * ld;
    const bool vec = (ld & 3) == 0 && (reinterpret_cast<uintptr_t>(base) & 15) == 0;
    float v[LP_REG];
    uint32_t avail = 0;
#pragma unroll
    for (int k = 0; k < LP_VEC; ++k) {
        const int i0 = lo + (k * LP_THREADS + tid) * 4;
        if (vec && i0 + 3 < hi) {
            const float4 f = *reinterpret_cast<const float4*>(row + i0);
            v[4 * k] = f.x; v[4 * k + 1] = f.y; v[4 * k + 2] = f.z; v[4 * k + 3] = f.w;
            avail |= 0xfu << (4 * k);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool ok = i0 + j < hi;
                v[4 * k + j] = ok ? row[i0 + j] : -INFINITY;
                avail |= (ok ? 1u : 0u) << (4 * k + j);
            }
        }
    }
    // ---- (m_c, s_c): block max, then the sum of exp(l - m_c) in a fixed order (registers, wave butterfly, waves 0..3)
    float m = -INFINITY;
#pragma unroll
    for (int r = 0; r < LP_REG; ++r) m = fmaxf(m, v[r]);
    m = wave_max(m);
    if (lane == 0) L.red[w] = m;
    __syncthreads();
    m = fmaxf(fmaxf(L.red[0], L.red[1]), fmaxf(L.red[2], L.red[3]));
    __syncthreads();
    float s = 0.f;
#pragma unroll
    for (int r = 0; r < LP_REG; ++r) s += ((avail >> r) & 1u) ? expf(v[r] - m) : 0.f;
    s = wave_sum(s);
    if (lane == 0) L.red[w] = s;
    __syncthreads();
    if (tid == 0) {
        part_ms[((size_t)b * LP_CHUNKS + c) * 2] = m;
        part_ms[((size_t)b * LP_CHUNKS + c) * 2 + 1] = ((L.red[0] + L.red[1]) + L.red[2]) + L.red[3];
    }
    if (n == 0) return;
    // ---- top-n of the chunk: n rounds of wave arg max per wave (the winner's register leaves the race), then the 4 lists merged
    auto local_best = [&](float& bv, int& bi, int& bs) {
        bv = -INFINITY; bi = LP_NONE; bs = 0;
#pragma unroll
        for (int r = 0; r < LP_REG; ++r) {
            const int idx = lo + ((r >> 2) * LP_THREADS + tid) * 4 + (r & 3);
            if (((avail >> r) & 1u) && lp_before(v[r], idx, bv, bi)) { bv = v[r]; bi = idx; bs = r; }
        }
    };
    float bv;
    int bi, bs;
    local_best(bv, bi, bs);
    for (int r = 0; r < n; ++r) {
        float gv = bv;
        int gi = bi;
        lp_wave_best(gv, gi);
        if (lane == 0) { L.wv[w][r] = gv; L.wi[w][r] = gi; }
        if (gi != LP_NONE && gi == bi) {
            avail &= ~(1u << bs);
            local_best(bv, bi, bs);
        }
    }
    __syncthreads();
    if (tid == 0) {
        int h[LP_THREADS / 64] = {0, 0, 0, 0};
        float* ov = part_v + ((size_t)b * LP_CHUNKS + c) * DOTS_MAX_TOP_LOGPROBS;
        int32_t* oi = part_i + ((size_t)b * LP_CHUNKS + c) * DOTS_MAX_TOP_LOGPROBS;
        for (int r = 0; r < n; ++r) {
            float cv = -INFINITY;
            int ci = LP_NONE, cw = 0;
            for (int q = 0; q < LP_THREADS / 64; ++q)
                if (h[q] < n && L.wi[q][h[q]] != LP_NONE && lp_before(L.wv[q][h[q]], L.wi[q][h[q]], cv, ci)) { cv = L.wv[q][h[q]]; ci = L.wi[q][h[q]]; cw = q; }
            if (ci != LP_NONE) h[cw] += 1;
            ov[r] = cv;
            oi[r] = ci;
        }
    }
}

// What one row's final reduction stages in LDS: the chunk lists, the chunks' terms of the sum and the result
struct LpFinalLds {
    float cv[LP_CHUNKS][DOTS_MAX_TOP_LOGPROBS];
    int ci[LP_CHUNKS][DOTS_MAX_TOP_LOGPROBS];
    float terms[LP_CHUNKS];
    float lse;
};

// Lane c of the one wave: row b's chunk-c partials into LDS, then lse = M + log sum_c s_c exp(m_c - M) summed in chunk order by lane 0.
// Holds two workgroup barriers: every lane of the workgroup calls it.  Returns the row's lse on every lane.
DEVI float lp_final_load(LpFinalLds& l, const float* __restrict__ part_ms, const float* __restrict__ part_v, const int32_t* __restrict__ part_i,
                         int b, int c, int n) {
    const float mc = part_ms[((size_t)b * LP_CHUNKS + c) * 2], sc = part_ms[((size_t)b * LP_CHUNKS + c) * 2 + 1];
    const float M = wave_max(mc);
    l.terms[c] = sc > 0.f ? sc * expf(mc - M) : 0.f;
    for (int r = 0; r < n; ++r) {
        l.cv[c][r] = part_v[((size_t)b * LP_CHUNKS + c) * DOTS_MAX_TOP_LOGPROBS + r];
        l.ci[c][r] = part_i[((size_t)b * LP_CHUNKS + c) * DOTS_MAX_TOP_LOGPROBS + r];
    }
    __syncthreads();
    if (c == 0) {
        float S = 0.f;
        for (int k = 0; k < LP_CHUNKS; ++k) S += l.terms[k];          // chunk order
        l.lse = M + logf(S);
    }
    __syncthreads();
    return l.lse;
}

// One round of the merge of the LP_CHUNKS sorted chunk lists: the best head over the wave (gv, gi; gi == LP_NONE: the lists are
// exhausted); the lane whose head won moves on (h: this lane's head, 0 before the first round)
DEVI void lp_final_next(const LpFinalLds& l, int c, int n, int& h, float& gv, int& gi) {
    gv = h < n ? l.cv[c][h] : -INFINITY;
    gi = h < n ? l.ci[c][h] : LP_NONE;
    lp_wave_best(gv, gi);
    if (gi != LP_NONE && h < n && l.ci[c][h] == gi) h += 1;
}

// One output entry, by the one wave of a final kernel (lane c): the partials of scratch row r — which is also the row of `logits` the
// values came from — reduced to lse and the sorted top-n, written with the value of the committed token `tok` at output entry o (an index
// into tok_lp; entries >= n of the top lists become -1 / NaN).  Holds lp_final_load's barriers: every lane calls it.  tops = false (with
// n == 0): st has no top lists and only tok_lp is written (score.hip, before any call asked for a top list).
DEVI void lp_final_entry(LpFinalLds& l, const float* __restrict__ logits, int V, int ld, const LogprobState& st, int r, int c, int n, size_t o, int tok,
                         bool tops = true) {
    const float lse = lp_final_load(l, st.part_ms, st.part_v, st.part_i, r, c, n);
    int h = 0;
    for (int q = 0; q < n; ++q) {
        float gv;
        int gi;
        lp_final_next(l, c, n, h, gv, gi);
        if (c == 0) {
            st.top_ids[o * DOTS_MAX_TOP_LOGPROBS + q] = gi == LP_NONE ? -1 : gi;
            st.top_lp[o * DOTS_MAX_TOP_LOGPROBS + q] = gi == LP_NONE ? __builtin_nanf("") : gv - lse;
        }
    }
    if (tops && c >= n && c < DOTS_MAX_TOP_LOGPROBS) {
        st.top_ids[o * DOTS_MAX_TOP_LOGPROBS + c] = -1;
        st.top_lp[o * DOTS_MAX_TOP_LOGPROBS + c] = __builtin_nanf("");
    }
    if (c == 0) st.tok_lp[o] = (tok >= 0 && tok < V) ? logits[(size_t)r * ld + tok] - lse : __builtin_nanf("");
}
