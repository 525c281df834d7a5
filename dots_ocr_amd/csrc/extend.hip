// Extending a live sequence (dots_slots_extend): the two kernels the call adds around the unchanged layer loop of a decode
// step.
//
// The call teacher-forces more prompt tokens behind the KV cache of occupied slots.  Its packed rows — row i carries token off[i] of the
// tokens fed to slot slot[i] — are cut into chunks of at most max_batch rows, and a chunk is one pass of the layer loop over step-private
// token / context / block-table arrays, as a speculating step is (spec.hip): row (slot, j) sits at context c_slot + j on the slot's own KV
// pages.  dec_qkv appends the K/V of every row of a launch before the attention launch, so a row attends over what the rows before it
// appended — in this chunk or an earlier one — and, every decode kernel being row-independent and batch-invariant bit for bit, its hidden
// row is that of the sequential step at that position.
//
//   extend_expand_kernel   head of a chunk: tokens, contexts and block-table rows of its rows from the slots' state, which nothing moves
//                          before the last chunk has run
//   extend_commit_kernel   after the last chunk: the per-slot state of a slot prefilled with the longer prompt
#include "kernels.h"

namespace {

// grid (rows), 64 threads
__global__ __launch_bounds__(64) void extend_expand_kernel(ExtendRows ex, int r0, int n_live, const int32_t* __restrict__ cur_tokens,
                                                           const int32_t* __restrict__ ctx_len, const int32_t* __restrict__ finished,
                                                           const int32_t* __restrict__ out_ids, const int32_t* __restrict__ out_lens, int out_stride,
                                                           const int32_t* __restrict__ block_table, int max_pages, int scratch_page) {
    const int r = blockIdx.x;
    const bool live = r < n_live;
    const int b = live ? ex.slot[r0 + r] : 0;
    const int32_t* __restrict__ src = block_table + (size_t)b * max_pages;
    int32_t* __restrict__ dst = ex.block_table + (size_t)r * max_pages;
    for (int p = threadIdx.x; p < max_pages; p += 64) dst[p] = live ? src[p] : scratch_page;
    if (threadIdx.x == 0) {
        int tok = 0;
        if (live) {
            tok = ex.token[r0 + r];
            if (tok < 0) {
                // the pending token.  A finished row keeps stepping and its cur_tokens entry keeps moving (commit_token); its last output
                // token is the pending one
                const int n = out_lens[b];
                tok = finished[b] && n > 0 ? out_ids[(size_t)b * out_stride + n - 1] : cur_tokens[b];
            }
        }
        ex.tokens[r] = tok;
        ex.ctx_len[r] = live ? ctx_len[b] + ex.off[r0 + r] : 0;
    }
}

// one thread per extended slot
__global__ void extend_commit_kernel(const int32_t* __restrict__ slots, const int32_t* __restrict__ fed, const int32_t* __restrict__ max_new, int n,
                                     int32_t* __restrict__ ctx_len, int32_t* __restrict__ out_lens, int32_t* __restrict__ finished,
                                     int32_t* __restrict__ max_len) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int b = slots[i];
    ctx_len[b] += fed[i];
    out_lens[b] = 0;
    finished[b] = 0;
    max_len[b] = max_new[i];
}

}  // namespace

hipError_t launch_extend_expand(hipStream_t s, const ExtendRows& ex, int r0, int n_live, int rows, const int32_t* cur_tokens, const int32_t* ctx_len,
                                const int32_t* finished, const int32_t* out_ids, const int32_t* out_lens, int out_stride, const int32_t* block_table,
                                int max_pages, int scratch_page) {
    if (!ex.slot || !ex.off || !ex.token || !ex.tokens || !ex.ctx_len || !ex.block_table || !cur_tokens || !ctx_len || !finished || !out_ids || !out_lens ||
        !block_table || r0 < 0 || n_live < 1 || rows < n_live || rows > DOTS_MAX_BATCH || out_stride < 1 || max_pages < 1 || scratch_page < 0)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(extend_expand_kernel, dim3(rows), dim3(64), 0, s, ex, r0, n_live, cur_tokens, ctx_len, finished, out_ids, out_lens, out_stride,
                       block_table, max_pages, scratch_page);
    return hipGetLastError();
}

hipError_t launch_extend_commit(hipStream_t s, const int32_t* slots, const int32_t* fed, const int32_t* max_new, int n, int32_t* ctx_len,
                                int32_t* out_lens, int32_t* finished, int32_t* max_len) {
    if (!slots || !fed || !max_new || n < 1 || n > DOTS_MAX_BATCH || !ctx_len || !out_lens || !finished || !max_len) return hipErrorInvalidValue;
    hipLaunchKernelGGL(extend_commit_kernel, dim3(1), dim3(DOTS_MAX_BATCH), 0, s, slots, fed, max_new, n, ctx_len, out_lens, finished, max_len);
    return hipGetLastError();
}
