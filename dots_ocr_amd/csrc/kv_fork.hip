// Tail-page copy of a fork (dots_slots_fork).  The children of a forked sequence name the source's FULL prompt pages in their
// block-table rows; the one partially filled page (prompt length L, L % 64 != 0) cannot be shared, because every row appends its own keys
// to it, so each child gets a copy of it in every layer.
//
// A page is copied whole — [Hkv][K | V][8192] elements, bf16 or e4m3 — so the kernel knows nothing of the in-page order of K and V^T
// (decode.hip): it moves page_vec 16-byte vectors per (layer, page).  Each vector of the source page is loaded once and stored to all n
// children; the children's page indices come from a small device array (uniform over the workgroup: scalar loads).
//   grid (ceil(page_vec / 256), layers), 256 threads
#include "common.h"
#include "kernels.h"

namespace {

__global__ __launch_bounds__(256) void kv_fork_kernel(u32x4* __restrict__ pool, size_t layer_vec, int page_vec, int src_page,
                                                      const int32_t* __restrict__ dst_pages, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= page_vec) return;
    u32x4* base = pool + (size_t)blockIdx.y * layer_vec;
    const u32x4 v = base[(size_t)src_page * page_vec + i];
    for (int c = 0; c < n; ++c) base[(size_t)dst_pages[c] * page_vec + i] = v;
}

}  // namespace

hipError_t launch_kv_fork_pages(hipStream_t s, void* pool, size_t layer_bytes, size_t page_bytes, int layers, int src_page, const int32_t* dst_pages,
                                int n) {
    if (n < 1 || n >= DOTS_MAX_BATCH || layers < 1 || src_page < 0 || page_bytes == 0 || (page_bytes & 15) || (layer_bytes & 15) ||
        page_bytes / 16 > (size_t)INT32_MAX)
        return hipErrorInvalidValue;
    const int page_vec = (int)(page_bytes / 16);
    hipLaunchKernelGGL(kv_fork_kernel, dim3((page_vec + 255) / 256, layers), dim3(256), 0, s, reinterpret_cast<u32x4*>(pool), layer_bytes / 16, page_vec,
                       src_page, dst_pages, n);
    return hipGetLastError();
}
