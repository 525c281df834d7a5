// Stop strings: the stream-ordered writers of the row table.
//
// A row's stop strings are one Aho-Corasick automaton with its failure links folded into a dense byte DFA (kernels.h RowStop: table
// [n_states][256] uint16 with every transition defined, match_len / match_id per state).  The host compiles it (dots_ocr_amd/stop_strings.py)
// and dots_stop_create uploads it; any number of rows may hold one.  The walk is no kernel of its own: commit_token (step_dev.h) advances
// the row's state over the bytes of the token it just appended — at most a handful of dependent 2-byte reads by the one thread that commits
// the row — and finishes the row at the byte where a listed string ends.  So a step with stop rows launches what a step with any other
// per-row rule launches, the stop is exact inside a captured chunk and in the static batch, and a stopped row writes no further KV.
//
// What is left for this file is the row table's bookkeeping between steps: each writer is a tiny kernel so that it takes its place in the
// stream behind the steps already queued (a hipMemcpy from a stack variable would not).
#include "kernels.h"

namespace {

__device__ inline void stop_to_root(RowStop& r) {
    r.state = 0;
    r.hit_tok = -1; r.hit_bytes = 0; r.hit_len = 0; r.hit_id = -1;
}

__global__ void set_row_stop_kernel(RowStop* table, int row, RowStop r) {
    stop_to_root(r);
    table[row] = r;
}

__global__ void stop_reset_rows_kernel(RowStop* table, const int32_t* __restrict__ dst, int n) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= n) return;
    const int row = dst ? dst[b] : b;
    if (row < 0 || row >= DOTS_MAX_BATCH) return;
    if (table[row].table) stop_to_root(table[row]);
}

__global__ void stop_fork_rows_kernel(RowStop* table, int src, const int32_t* __restrict__ dst, int n) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= n) return;
    const int row = dst[b];
    if (row < 0 || row >= DOTS_MAX_BATCH || row == src) return;
    RowStop r = table[src];
    stop_to_root(r);
    table[row] = r;
}

}  // namespace

hipError_t launch_set_row_stop(hipStream_t s, RowStop* table, int row, const RowStop& r) {
    if (!table || row < 0 || row >= DOTS_MAX_BATCH) return hipErrorInvalidValue;
    if (r.table && (!r.match_len || !r.match_id || r.n_states < 1 || r.n_states > STOP_MAX_STATES || r.min_tokens < 0)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(set_row_stop_kernel, dim3(1), dim3(1), 0, s, table, row, r);
    return hipGetLastError();
}

hipError_t launch_stop_reset_rows(hipStream_t s, RowStop* table, const int32_t* dst, int n) {
    if (!table || n < 1 || n > DOTS_MAX_BATCH) return hipErrorInvalidValue;
    hipLaunchKernelGGL(stop_reset_rows_kernel, dim3(1), dim3(64), 0, s, table, dst, n);
    return hipGetLastError();
}

hipError_t launch_stop_fork_rows(hipStream_t s, RowStop* table, int src, const int32_t* dst, int n) {
    if (!table || !dst || src < 0 || src >= DOTS_MAX_BATCH || n < 1 || n > DOTS_MAX_BATCH) return hipErrorInvalidValue;
    hipLaunchKernelGGL(stop_fork_rows_kernel, dim3(1), dim3(64), 0, s, table, src, dst, n);
    return hipGetLastError();
}
