// Per-token log-probabilities of the raw logits: log-sum-exp and the top-N (value desc, index asc) of every selected row.
//
//   logprob_partial_kernel  grid (LP_CHUNKS, rows), 256 threads: one pass over a vocabulary chunk (float4 loads) -> the chunk's
//                           (m_c, s_c = sum exp(l - m_c)) and its top-n (value, index) pairs; block (0, b) also snapshots where row b's
//                           token of this step lands (out_lens[b], or -1 for a row that was already finished) — selection has not run yet.
//   logprob_final_kernel    grid rows, one wave: lse = M + log sum_c s_c exp(m_c - M) summed in chunk order, the 64 chunk lists merged
//                           into the row's top-n, the chosen token's value read from the logits; written at the snapshotted position.
//   spec_logprob_partial_kernel, spec_logprob_final_kernel   the same two passes over the draft rows of a speculating step (DESIGN §6.6,
//                           dots_set_speculation_logprobs): the partials of the live draft rows of slots with logprobs on, before the
//                           selection stage; the entries of the candidates the accept walk committed, after it.
//
// Every reduction has a fixed shape and order and no atomics are used, so a row's values depend on its logits only: not on its slot,
// the batch, or the other rows.  Nothing here reads or writes the selection state other than the snapshot (finished / out_lens before
// the step's commit) and the token selection chose (cur_tokens after it).
#include <cstdint>

#include "common.h"
#include "kernels.h"
#include "logprobs_dev.h"

namespace {

__global__ __launch_bounds__(LP_THREADS) void logprob_partial_kernel(const float* __restrict__ logits, int V, int ld, LogprobState st) {
    __shared__ LpPartialLds L;
    const int c = blockIdx.x, b = blockIdx.y;
    if (st.sel && !st.sel[b]) return;
    const int n = st.top_n[b];
    if (n < 0) return;
    if (c == 0 && threadIdx.x == 0) st.pos[b] = (st.finished && st.finished[b]) ? -1 : (st.out_lens ? st.out_lens[b] : 0);
    lp_partial_chunk(L, logits, V, ld, b, c, n, st.part_ms, st.part_v, st.part_i);
}

__global__ __launch_bounds__(64) void logprob_final_kernel(const float* __restrict__ logits, int V, int ld, LogprobState st) {
    __shared__ LpFinalLds l;
    const int b = blockIdx.x, c = threadIdx.x;
    if (st.sel && !st.sel[b]) return;
    const int n = st.top_n[b];
    if (n < 0) return;
    const int pos = st.pos[b];
    if (pos < 0 || pos >= st.stride) return;                   // the row was finished before this step: its token is not appended
    lp_final_entry(l, logits, V, ld, st, b, c, n, (size_t)b * st.stride + pos, st.chosen[b]);
}

// The draft rows of a speculating step.  grid (LP_CHUNKS, rows * k): workgroup (c, x) serves draft row r = rows + x =
// j * rows + b and exits at once unless slot b has logprobs on and the row is live (j <= n_live[b], as spec_argmax_kernel): the chunk's
// pass over logits row r with the slot's top_n, into row r of the scratch — the stage's own launch uses rows [0, rows).  No snapshot: the
// slot's position is the one logprob_partial_kernel takes for row b.
__global__ __launch_bounds__(LP_THREADS) void spec_logprob_partial_kernel(const float* __restrict__ logits, int V, int ld, int rows,
                                                                          const int32_t* __restrict__ n_live, LogprobState st) {
    __shared__ LpPartialLds L;
    const int c = blockIdx.x, r = rows + blockIdx.y, j = r / rows, b = r - j * rows;
    const int n = st.top_n[b];
    if (n < 0 || j > n_live[b]) return;                         // uniform per workgroup
    lp_partial_chunk(L, logits, V, ld, r, c, n, st.part_ms, st.part_v, st.part_i);
}

// grid (rows, k), one wave, after spec_accept_kernel: workgroup (b, a) writes the entry of the a-th candidate the walk of slot b committed
// (acc_n[b] of them, ids acc_tok[b][.]), from the partials and the logits of draft row (a + 1) * rows + b, at the position that commit
// appended at: pos[b] + 1 + a, pos[b] being row 0's.  A slot the stage skipped, one with logprobs off or one that was finished before the
// step (pos < 0; its n_live is -1 and acc_n 0) writes nothing, and neither does a candidate that was not committed.
__global__ __launch_bounds__(64) void spec_logprob_final_kernel(const float* __restrict__ logits, int V, int ld, int rows,
                                                                const int32_t* __restrict__ acc_n, const int32_t* __restrict__ acc_tok,
                                                                LogprobState st) {
    __shared__ LpFinalLds l;
    const int b = blockIdx.x, a = blockIdx.y, c = threadIdx.x;
    if (st.sel && !st.sel[b]) return;
    const int n = st.top_n[b];
    if (n < 0 || a >= acc_n[b]) return;
    const int pos0 = st.pos[b];
    if (pos0 < 0 || pos0 + 1 + a >= st.stride) return;
    lp_final_entry(l, logits, V, ld, st, (a + 1) * rows + b, c, n, (size_t)b * st.stride + pos0 + 1 + a, acc_tok[b * DOTS_MAX_SPEC_DRAFTS + a]);
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

namespace {
bool spec_lp_ok(const float* logits, int V, int ld, int rows, int k, const LogprobState& st) {
    return logits && V >= 1 && V <= LP_MAX_V && ld >= V && rows >= 1 && k >= 1 && k <= DOTS_MAX_SPEC_DRAFTS && rows * (k + 1) <= DOTS_MAX_BATCH && st.top_n &&
           st.part_ms && st.part_v && st.part_i;
}
}  // namespace

hipError_t launch_spec_logprob_partial(hipStream_t s, const float* logits, int V, int ld, int rows, int k, const int32_t* n_live, const LogprobState& st) {
    if (!spec_lp_ok(logits, V, ld, rows, k, st) || !n_live) return hipErrorInvalidValue;
    hipLaunchKernelGGL(spec_logprob_partial_kernel, dim3(LP_CHUNKS, rows * k), dim3(LP_THREADS), 0, s, logits, V, ld, rows, n_live, st);
    return hipGetLastError();
}

hipError_t launch_spec_logprob_final(hipStream_t s, const float* logits, int V, int ld, int rows, int k, const int32_t* acc_n, const int32_t* acc_tok,
                                     const LogprobState& st) {
    if (!spec_lp_ok(logits, V, ld, rows, k, st) || !acc_n || !acc_tok || !st.pos || !st.tok_lp || !st.top_ids || !st.top_lp || st.stride < 1)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(spec_logprob_final_kernel, dim3(rows, k), dim3(64), 0, s, logits, V, ld, rows, acc_n, acc_tok, st);
    return hipGetLastError();
}

hipError_t launch_set_row_lp(hipStream_t s, int32_t* table, int row, int top_n) {
    hipLaunchKernelGGL(set_row_lp_kernel, dim3(1), dim3(1), 0, s, table, row, top_n);
    return hipGetLastError();
}
