// Device pieces of the logprobs stage shared by logprobs.hip and beam.hip: the ranking rule of the top
// lists and the fixed-order final reduction over a row's LP_CHUNKS per-chunk partials (logprob_partial_kernel's output).  Both kernels
// run these with ONE wave whose lane c owns chunk c, so a row's log-sum-exp and sorted top-n are the same bits wherever they are taken.
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
