// Scoring given tokens on a live sequence (dots_slots_score): the logprob stage of an extend's chunk.
//
// A score is an extend (extend.hip) whose every fed row goes through the lm_head, into a logits scratch of the call's own, and whose rows
// record what the logprob stage (logprobs.hip) would have written had the row selected the NEXT fed token: the same two passes over the
// same device functions (logprobs_dev.h), so an entry is, bit for bit, the one a sequential step forced to that token leaves.
//
//   score_logprob_partial_kernel  grid (LP_CHUNKS, rows of the chunk), 256 threads: lp_partial_chunk over logits row r into scratch row r;
//                                 a row that records nothing (its slot's last fed row) returns at once
//   score_logprob_final_kernel    grid rows of the chunk, one wave: lp_final_entry with the row's target as the token and the slot's
//                                 entry index as the output position
//
// Which row records which entry, and with which target, is the host's plan (score_plan.h); nothing here looks at a neighbouring row.
#include <cstdint>

#include "common.h"
#include "kernels.h"
#include "logprobs_dev.h"

namespace {

__global__ __launch_bounds__(LP_THREADS) void score_logprob_partial_kernel(const float* __restrict__ logits, int V, int ld, ScoreRows sr, int r0,
                                                                           LogprobState st) {
    __shared__ LpPartialLds L;
    const int c = blockIdx.x, r = blockIdx.y;
    if (sr.entry[r0 + r] < 0) return;                          // uniform per workgroup
    lp_partial_chunk(L, logits, V, ld, r, c, sr.top_n[r0 + r], st.part_ms, st.part_v, st.part_i);
}

__global__ __launch_bounds__(64) void score_logprob_final_kernel(const float* __restrict__ logits, int V, int ld, ScoreRows sr, int r0, LogprobState st) {
    __shared__ LpFinalLds l;
    const int r = blockIdx.x, c = threadIdx.x;
    const int o = sr.entry[r0 + r];
    if (o < 0 || o >= st.stride) return;
    const bool tops = st.top_ids != nullptr;
    lp_final_entry(l, logits, V, ld, st, r, c, tops ? sr.top_n[r0 + r] : 0, (size_t)sr.slot[r0 + r] * st.stride + o, sr.target[r0 + r], tops);
}

bool score_ok(const float* logits, int V, int ld, const ScoreRows& sr, int r0, int rows, const LogprobState& st) {
    return logits && V >= 1 && V <= LP_MAX_V && ld >= V && sr.slot && sr.entry && sr.target && sr.top_n && r0 >= 0 && rows >= 1 && rows <= DOTS_MAX_BATCH &&
           st.part_ms && st.part_v && st.part_i;
}

}  // namespace

hipError_t launch_score_logprob_partial(hipStream_t s, const float* logits, int V, int ld, const ScoreRows& sr, int r0, int rows, const LogprobState& st) {
    if (!score_ok(logits, V, ld, sr, r0, rows, st)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(score_logprob_partial_kernel, dim3(LP_CHUNKS, rows), dim3(LP_THREADS), 0, s, logits, V, ld, sr, r0, st);
    return hipGetLastError();
}

hipError_t launch_score_logprob_final(hipStream_t s, const float* logits, int V, int ld, const ScoreRows& sr, int r0, int rows, const LogprobState& st) {
    if (!score_ok(logits, V, ld, sr, r0, rows, st) || !st.tok_lp || (st.top_ids == nullptr) != (st.top_lp == nullptr) || st.stride < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(score_logprob_final_kernel, dim3(rows), dim3(64), 0, s, logits, V, ld, sr, r0, st);
    return hipGetLastError();
}
