// Page gather / scatter of dots_slot_suspend and dots_slot_resume.  A sequence's KV is layers x pages chunks of one page
// each, scattered over the pool [layers][n_pool_pages + 1][page]; the host link wants few large copies.  kv_gather_kernel packs the n listed
// pages of every layer into a contiguous staging buffer [page j][layer][page bytes] (one hipMemcpyAsync then moves the chunk to pinned host
// memory); kv_scatter_kernel does the reverse, into a list of possibly different pages.
//
// As in kv_fork.hip a page is copied whole — [Hkv][K | V][8192] elements, bf16 or e4m3 — so neither kernel knows the in-page order of K and
// V^T, and one body serves both pools.  The page index of a workgroup comes from a small device array (uniform over the workgroup: a scalar
// load).  Unlike the fork's tail page, a chunk is tens of MB, so every thread keeps SW_VECS 16-byte loads in flight before its first store:
// 256 threads x 8 x 16 B = 32 KiB per workgroup, which is what a CU needs outstanding to stream from HBM, and a chunk of 32 pages x 28
// layers x 64 KiB gives every CU several such workgroups.  Plain vector loads and stores only.
//   grid (ceil(page_vec / (256 * SW_VECS)), layers, n), 256 threads
#include "common.h"
#include "kernels.h"

namespace {

constexpr int SW_THREADS = 256, SW_VECS = 8, SW_TILE = SW_THREADS * SW_VECS;

// TO_STAGE: pool -> staging (gather), else staging -> pool (scatter)
template <bool TO_STAGE>
DEVI void swap_body(u32x4* __restrict__ pool, size_t layer_vec, int page_vec, u32x4* __restrict__ stage, const int32_t* __restrict__ pages) {
    const int layer = blockIdx.y, j = blockIdx.z, layers = gridDim.y;
    u32x4* in_pool = pool + (size_t)layer * layer_vec + (size_t)pages[j] * page_vec;
    u32x4* in_stage = stage + ((size_t)j * layers + layer) * page_vec;
    const u32x4* src = TO_STAGE ? in_pool : in_stage;
    u32x4* dst = TO_STAGE ? in_stage : in_pool;
    const int i0 = blockIdx.x * SW_TILE + threadIdx.x;
    if (blockIdx.x * SW_TILE + SW_TILE <= page_vec) {                 // a whole tile (uniform per workgroup): every load before the first store
        u32x4 v[SW_VECS];
#pragma unroll
        for (int k = 0; k < SW_VECS; ++k) v[k] = src[i0 + k * SW_THREADS];
#pragma unroll
        for (int k = 0; k < SW_VECS; ++k) dst[i0 + k * SW_THREADS] = v[k];
    } else {                                                          // the page's last, partial tile (pages below 32 KiB only)
        for (int i = i0; i < page_vec; i += SW_THREADS) dst[i] = src[i];
    }
}

__global__ __launch_bounds__(SW_THREADS) void kv_gather_kernel(const u32x4* __restrict__ pool, size_t layer_vec, int page_vec, u32x4* __restrict__ stage,
                                                               const int32_t* __restrict__ pages) {
    swap_body<true>(const_cast<u32x4*>(pool), layer_vec, page_vec, stage, pages);
}
__global__ __launch_bounds__(SW_THREADS) void kv_scatter_kernel(u32x4* __restrict__ pool, size_t layer_vec, int page_vec, const u32x4* __restrict__ stage,
                                                                const int32_t* __restrict__ pages) {
    swap_body<false>(pool, layer_vec, page_vec, const_cast<u32x4*>(stage), pages);
}

hipError_t launch(bool to_stage, hipStream_t s, void* pool, size_t layer_bytes, size_t page_bytes, int layers, void* stage, const int32_t* pages, int n) {
    if (n < 1 || n > KV_SWAP_CHUNK_PAGES || layers < 1 || layers > 65535 || !pool || !stage || !pages || page_bytes == 0 || (page_bytes & 15) ||
        (layer_bytes & 15) || page_bytes / 16 > (size_t)INT32_MAX)
        return hipErrorInvalidValue;
    const int page_vec = (int)(page_bytes / 16);
    const dim3 grid((page_vec + SW_TILE - 1) / SW_TILE, layers, n);
    if (to_stage)
        hipLaunchKernelGGL(kv_gather_kernel, grid, dim3(SW_THREADS), 0, s, reinterpret_cast<const u32x4*>(pool), layer_bytes / 16, page_vec,
                           reinterpret_cast<u32x4*>(stage), pages);
    else
        hipLaunchKernelGGL(kv_scatter_kernel, grid, dim3(SW_THREADS), 0, s, reinterpret_cast<u32x4*>(pool), layer_bytes / 16, page_vec,
                           reinterpret_cast<const u32x4*>(stage), pages);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_kv_gather_pages(hipStream_t s, const void* pool, size_t layer_bytes, size_t page_bytes, int layers, void* stage, const int32_t* pages,
                                  int n) {
    return launch(true, s, const_cast<void*>(pool), layer_bytes, page_bytes, layers, stage, pages, n);
}

hipError_t launch_kv_scatter_pages(hipStream_t s, void* pool, size_t layer_bytes, size_t page_bytes, int layers, const void* stage, const int32_t* pages,
                                   int n) {
    return launch(false, s, pool, layer_bytes, page_bytes, layers, const_cast<void*>(stage), pages, n);
}
