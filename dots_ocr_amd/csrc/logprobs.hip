// Per-token log-probabilities of the raw logits: log-sum-exp and the top-N (value desc, index asc) of every selected row.
//
//   logprob_partial_kernel  grid (LP_CHUNKS, rows), 256 threads: one pass over a vocabulary chunk (float4 loads) -> the chunk's
//                           (m_c, s_c = sum exp(l - m_c)) and its top-n (value, index) pairs; block (0, b) also snapshots where row b's
//                           token of this step lands (out_lens[b], or -1 for a row that was already finished) — selection has not run yet.
//   logprob_final_kernel    grid rows, one wave: lse = M + log sum_c s_c exp(m_c - M) summed in chunk order, the 64 chunk lists merged
//                           into the row's top-n, the chosen token's value read from the logits; written at the snapshotted position.
//
// Every reduction has a fixed shape and order and no atomics are used, so a row's values depend on its logits only: not on its slot,
// the batch, or the other rows.  Nothing here reads or writes the selection state other than the snapshot (finished / out_lens before
// the step's commit) and the token selection chose (cur_tokens after it).
#include <cstdint>

#include "common.h"
#include "kernels.h"
#include "logprobs_dev.h"

namespace {

constexpr int LP_THREADS = 256;
constexpr int LP_VEC = LP_MAX_CHUNK / (4 * LP_THREADS);         // float4 loads per thread (4)
constexpr int LP_REG = 4 * LP_VEC;                              // values per thread held in registers (16)
static_assert(LP_REG <= 32, "one availability bit per register value");
DEVI int lp_chunk_len(int V) { return (((V + LP_CHUNKS - 1) / LP_CHUNKS) + 3) & ~3; }

__global__ __launch_bounds__(LP_THREADS) void logprob_partial_kernel(const float* __restrict__ logits, int V, int ld, LogprobState st) {
    __shared__ float red[LP_THREADS / 64];
    __shared__ float wv[LP_THREADS / 64][DOTS_MAX_TOP_LOGPROBS];
    __shared__ int wi[LP_THREADS / 64][DOTS_MAX_TOP_LOGPROBS];
    const int c = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    if (st.sel && !st.sel[b]) return;
    const int n = st.top_n[b];
    if (n < 0) return;
    if (c == 0 && tid == 0) st.pos[b] = (st.finished && st.finished[b]) ? -1 : (st.out_lens ? st.out_lens[b] : 0);
    const int per = lp_chunk_len(V);
    const int lo = c * per, hi = min(V, lo + per);
    const float* row = logits + (size_t)b * ld;
    const bool vec = (ld & 3) == 0 && (reinterpret_cast<uintptr_t>(logits) & 15) == 0;
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
    if (lane == 0) red[w] = m;
    __syncthreads();
    m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    __syncthreads();
    float s = 0.f;
#pragma unroll
    for (int r = 0; r < LP_REG; ++r) s += ((avail >> r) & 1u) ? expf(v[r] - m) : 0.f;
    s = wave_sum(s);
    if (lane == 0) red[w] = s;
    __syncthreads();
    if (tid == 0) {
        st.part_ms[((size_t)b * LP_CHUNKS + c) * 2] = m;
        st.part_ms[((size_t)b * LP_CHUNKS + c) * 2 + 1] = ((red[0] + red[1]) + red[2]) + red[3];
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
        if (lane == 0) { wv[w][r] = gv; wi[w][r] = gi; }
        if (gi != LP_NONE && gi == bi) {
            avail &= ~(1u << bs);
            local_best(bv, bi, bs);
        }
    }
    __syncthreads();
    if (tid == 0) {
        int h[LP_THREADS / 64] = {0, 0, 0, 0};
        float* ov = st.part_v + ((size_t)b * LP_CHUNKS + c) * DOTS_MAX_TOP_LOGPROBS;
        int32_t* oi = st.part_i + ((size_t)b * LP_CHUNKS + c) * DOTS_MAX_TOP_LOGPROBS;
        for (int r = 0; r < n; ++r) {
            float cv = -INFINITY;
            int ci = LP_NONE, cw = 0;
            for (int q = 0; q < LP_THREADS / 64; ++q)
                if (h[q] < n && wi[q][h[q]] != LP_NONE && lp_before(wv[q][h[q]], wi[q][h[q]], cv, ci)) { cv = wv[q][h[q]]; ci = wi[q][h[q]]; cw = q; }
            if (ci != LP_NONE) h[cw] += 1;
            ov[r] = cv;
            oi[r] = ci;
        }
    }
}

__global__ __launch_bounds__(64) void logprob_final_kernel(const float* __restrict__ logits, int V, int ld, LogprobState st) {
    __shared__ LpFinalLds l;
    const int b = blockIdx.x, c = threadIdx.x;
    if (st.sel && !st.sel[b]) return;
    const int n = st.top_n[b];
    if (n < 0) return;
    const int pos = st.pos[b];
    if (pos < 0 || pos >= st.stride) return;                   // the row was finished before this step: its token is not appended
    const float lse = lp_final_load(l, st.part_ms, st.part_v, st.part_i, b, c, n);
    const size_t o = (size_t)b * st.stride + pos;
    int h = 0;
    for (int r = 0; r < n; ++r) {
        float gv;
        int gi;
        lp_final_next(l, c, n, h, gv, gi);
        if (c == 0) {
            st.top_ids[o * DOTS_MAX_TOP_LOGPROBS + r] = gi == LP_NONE ? -1 : gi;
            st.top_lp[o * DOTS_MAX_TOP_LOGPROBS + r] = gi == LP_NONE ? __builtin_nanf("") : gv - lse;
        }
    }
    if (c >= n && c < DOTS_MAX_TOP_LOGPROBS) {
        st.top_ids[o * DOTS_MAX_TOP_LOGPROBS + c] = -1;
        st.top_lp[o * DOTS_MAX_TOP_LOGPROBS + c] = __builtin_nanf("");
    }
    if (c == 0) {
        const int tok = st.chosen[b];
        st.tok_lp[o] = (tok >= 0 && tok < V) ? logits[(size_t)b * ld + tok] - lse : __builtin_nanf("");
    }
}

__global__ void set_row_lp_kernel(int32_t* table, int row, int top_n) { table[row] = top_n; }

}  // namespace

hipError_t launch_logprob_partial(hipStream_t s, const float* logits, int V, int ld, int B, const LogprobState& st) {
    if (V < 1 || V > LP_MAX_V || ld < V || B < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(logprob_partial_kernel, dim3(LP_CHUNKS, B), dim3(LP_THREADS), 0, s, logits, V, ld, st);
    return hipGetLastError();
}

hipError_t launch_logprob_final(hipStream_t s, const float* logits, int V, int ld, int B, const LogprobState& st) {
    if (V < 1 || V > LP_MAX_V || ld < V || B < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(logprob_final_kernel, dim3(B), dim3(64), 0, s, logits, V, ld, st);
    return hipGetLastError();
}

hipError_t launch_set_row_lp(hipStream_t s, int32_t* table, int row, int top_n) {
    hipLaunchKernelGGL(set_row_lp_kernel, dim3(1), dim3(1), 0, s, table, row, top_n);
    return hipGetLastError();
}
