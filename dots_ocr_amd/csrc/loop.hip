// The loop guard: the stream-ordered writers of the row table and the run counters, and the probe.
//
// A row that holds a rule ends at the first token after which its output has repeated with some period p for L(p) tokens.  The check is
// no kernel of its own: select_rows_kernel (decode.hip) runs loop_after_commit (loop_dev.h) behind the commit of such a row, one thread
// per period, one counter per period in run[row][p - 1].  So a step with loop rows launches what a step with any other per-row rule
// launches, the end is exact inside a captured chunk and in the static batch, and an ended row writes no further KV.
//
// What is left for this file is the bookkeeping between steps — each writer is a small kernel so that it takes its place in the stream
// behind the steps already queued — and loop_probe_kernel, which drives the same loop_step over explicit histories for the tests.
#include "kernels.h"
#include "loop_dev.h"

namespace {

__device__ inline void loop_no_hit(RowLoop& r) { r.hit_tok = -1; r.period = 0; r.span = 0; r._pad = 0; }

// one workgroup of LOOP_THREADS: thread t zeroes the counter of period t + 1
__global__ __launch_bounds__(LOOP_THREADS) void set_row_loop_kernel(RowLoop* table, int32_t* run, int row, RowLoop r) {
    run[(size_t)row * DOTS_MAX_LOOP_PERIOD + threadIdx.x] = 0;
    if (threadIdx.x == 0) { loop_no_hit(r); table[row] = r; }
}

// workgroup i serves row dst[i]
__global__ __launch_bounds__(LOOP_THREADS) void loop_reset_rows_kernel(RowLoop* table, int32_t* run, const int32_t* __restrict__ dst) {
    const int row = dst ? dst[blockIdx.x] : (int)blockIdx.x;
    if (row < 0 || row >= DOTS_MAX_BATCH || table[row].max_period <= 0) return;          // uniform per workgroup
    run[(size_t)row * DOTS_MAX_LOOP_PERIOD + threadIdx.x] = 0;
    if (threadIdx.x == 0) loop_no_hit(table[row]);
}

__global__ __launch_bounds__(LOOP_THREADS) void loop_fork_rows_kernel(RowLoop* table, int32_t* run, int src, const int32_t* __restrict__ dst) {
    const int row = dst[blockIdx.x];
    if (row < 0 || row >= DOTS_MAX_BATCH || row == src) return;                          // uniform per workgroup
    run[(size_t)row * DOTS_MAX_LOOP_PERIOD + threadIdx.x] = 0;
    if (threadIdx.x == 0) { RowLoop r = table[src]; loop_no_hit(r); table[row] = r; }
}

__global__ __launch_bounds__(LOOP_THREADS) void loop_probe_kernel(const int32_t* __restrict__ ids, const int32_t* __restrict__ lens, int stride, RowLoop r,
                                                                  int32_t* __restrict__ hits) {
    __shared__ LoopLds L;
    const int c = blockIdx.x;
    const int32_t* out = ids + (size_t)c * stride;
    const int len = min(max(lens[c], 0), stride);
    int32_t run = 0;
    int hit_n = -1, hit_p = 0;
    for (int n = 0; n < len; ++n) {                                                      // uniform: every thread gets loop_step's answer
        const int p = loop_step(r, run, out, n, out[n], L);
        if (p != LOOP_NONE) { hit_n = n; hit_p = p; break; }
    }
    if (threadIdx.x == 0) {
        hits[c * 3 + 0] = hit_n;
        hits[c * 3 + 1] = hit_p;
        hits[c * 3 + 2] = hit_n >= 0 ? loop_span(r, hit_p) : 0;
    }
}

bool rule_ok(const RowLoop& r) {
    return r.max_period == 0 || (r.min_period >= 1 && r.min_period <= r.max_period && r.max_period <= DOTS_MAX_LOOP_PERIOD && r.repeats >= 2 &&
                                 r.repeats <= 64 && r.min_span >= 0 && r.min_span <= 65535);
}

}  // namespace

hipError_t launch_set_row_loop(hipStream_t s, RowLoop* table, int32_t* run, int row, const RowLoop& r) {
    if (!table || !run || row < 0 || row >= DOTS_MAX_BATCH || !rule_ok(r)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(set_row_loop_kernel, dim3(1), dim3(LOOP_THREADS), 0, s, table, run, row, r);
    return hipGetLastError();
}

hipError_t launch_loop_reset_rows(hipStream_t s, RowLoop* table, int32_t* run, const int32_t* dst, int n) {
    if (!table || !run || n < 1 || n > DOTS_MAX_BATCH) return hipErrorInvalidValue;
    hipLaunchKernelGGL(loop_reset_rows_kernel, dim3(n), dim3(LOOP_THREADS), 0, s, table, run, dst);
    return hipGetLastError();
}

hipError_t launch_loop_fork_rows(hipStream_t s, RowLoop* table, int32_t* run, int src, const int32_t* dst, int n) {
    if (!table || !run || !dst || src < 0 || src >= DOTS_MAX_BATCH || n < 1 || n > DOTS_MAX_BATCH) return hipErrorInvalidValue;
    hipLaunchKernelGGL(loop_fork_rows_kernel, dim3(n), dim3(LOOP_THREADS), 0, s, table, run, src, dst);
    return hipGetLastError();
}

hipError_t launch_loop_probe(hipStream_t s, const int32_t* ids, const int32_t* lens, int cases, int stride, const RowLoop& r, int32_t* hits) {
    if (!ids || !lens || !hits || cases < 1 || stride < 1 || r.max_period == 0 || !rule_ok(r)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(loop_probe_kernel, dim3(cases), dim3(LOOP_THREADS), 0, s, ids, lens, stride, r, hits);
    return hipGetLastError();
}
