// What every kernel launcher needs from the device, keyed by the kernel itself and cached per device: handles of different GPUs may live in
// one process.  Private, like engine.h; included by the kernel sources.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <mutex>
#include <type_traits>

#include "common.h"
#include "switches.h"

// Dynamic LDS above 64 KiB is opted into per kernel and device.  What is remembered is the largest size so far, not that it happened: a size that
// follows a run-time dimension (16 * K of dec_proj_lds_kernel, 32 * H of the two-tile gate|up) opts in again when a later launch asks for more.
// Per launch: hipGetDevice, one atomic load, one compare.
template <auto Kern>
hipError_t ensure_dyn_lds(size_t bytes) {
    if (bytes <= 64 * 1024) return hipSuccess;
    static size_t opted[32] = {};
    static std::mutex raise;
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    const int d = dev & 31;
    if (__atomic_load_n(&opted[d], __ATOMIC_ACQUIRE) >= bytes) return hipSuccess;
    std::lock_guard<std::mutex> lock(raise);              // raising only: two threads must not leave the smaller size behind the larger record
    if (opted[d] >= bytes) return hipSuccess;
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(Kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e != hipSuccess) return e;
    __atomic_store_n(&opted[d], bytes, __ATOMIC_RELEASE);
    return hipSuccess;
}

template <auto Kern, class... A>
hipError_t launch_dyn_lds(dim3 grid, dim3 block, size_t lds, hipStream_t s, A... args) {
    const hipError_t e = ensure_dyn_lds<Kern>(lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(Kern, grid, block, lds, s, args...);
    return hipGetLastError();
}

// CUs of the current device (256 when the query fails)
inline int device_cus() {
    static int cus[32] = {};
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); return 256; }
    int* slot = &cus[dev & 31];
    if ((v = __atomic_load_n(slot, __ATOMIC_RELAXED)) > 0) return v;
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v < 1) { (void)hipGetLastError(); v = 256; }
    __atomic_store_n(slot, v, __ATOMIC_RELAXED);
    return v;
}

// CUs a decode stream may use: the per-call override (tests, A/B runs), else the partition it is masked to, else the device
inline int wide_cus(int part_cus) {
    if (const int v = sw::parse_dec_wide_cus(sw::read_now(sw::DEC_WIDE_CUS))) return v;
    return part_cus > 0 ? part_cus : device_cus();
}

// workgroups of Kern a CU holds at once (1 when the query fails); the first launch's threads and LDS size stand for the kernel
template <auto Kern>
int resident_blocks_per_cu(int threads, size_t lds) {
    static int blocks[32] = {};
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess) (void)hipGetLastError();
    int* slot = &blocks[dev & 31];
    if ((n = __atomic_load_n(slot, __ATOMIC_RELAXED)) > 0) return n;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, reinterpret_cast<const void*>(Kern), threads, lds) != hipSuccess || n < 1) { (void)hipGetLastError(); n = 1; }
    __atomic_store_n(slot, n, __ATOMIC_RELAXED);
    return n;
}

// Dispatch helpers of the launchers.  by_weight_type: a decode weight image is e4m3 fragments (u32x2, with per-row scales) or bf16 fragments
// (bf16x8); f gets the typed pointer and names the kernel's weight type weight_t<decltype(wd)>.  int_c: a run-time choice handed on as a type.
template <class F>
hipError_t by_weight_type(const void* Wd, bool fp8, F f) { return fp8 ? f(static_cast<const u32x2*>(Wd)) : f(static_cast<const bf16x8*>(Wd)); }
template <class P> using weight_t = std::remove_const_t<std::remove_pointer_t<P>>;
template <int V> using int_c = std::integral_constant<int, V>;
