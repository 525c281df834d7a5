// Shared layout helpers of the decode kernels (decode.hip, decode_fused.hip); see decode.hip's header comment.
#pragma once
#include "common.h"

constexpr int PAGE = 64;
constexpr int PAGE_ELEMS = PAGE * 128;     // per (kv head, K|V)

// Operand layouts of the skinny (B <= 16 rows) GEMMs of the decode step, both in MFMA fragment order
// (v_mfma_f32_16x16x32_bf16: lane = g*16 + i holds 8 consecutive k of row i, k-step = 32 k):
//   weights  Wd[(n_tile*(K/32) + kstep)*64 + lane][8],  lane = g*16 + i  <->  W[16*n_tile + i][32*kstep + 8g .. +7]
//            one contiguous 1 KiB chunk per (tile, k-step); the two 8-row halves of a chunk are four whole 128-B lines each
//   inputs   X[(k/8)*XR + m][8]  <->  X[m][8*(k/8) .. +7],   XR = 8 (B <= 8) or 16 rows
//            lane (g, m) of k-step ks reads slot (4*ks + g)*XR + (m & (XR-1)): with XR = 8 lanes m and m+8 read the same 16 B,
//            so an 8-row batch costs half the L2 traffic and half the LDS of the 16-row image.
// fp8 weights (quant.hip): the chunk of a (tile, k-step) is 512 B, lane (g, i)'s 8 bytes sit at 8-byte slot [i >> 3][g][i & 7]: each 8-row half
// of the tile is 256 contiguous bytes (two whole lines).
DEVI int fp8_lane_slot(int g, int i) { return ((i >> 3) * 4 + g) * 8 + (i & 7); }
DEVI int xr_of(int B) { return B <= 8 ? 8 : 16; }
//            Batches above 16 rows are split into 16-ROW TILES (one MFMA column tile each): tile t = rows 16t .. 16t+15 is a complete
//            XR = 16 image of its own at element offset t * 16 * K, and every dense decode kernel runs one workgroup set per tile
//            (blockIdx.y), i.e. sees a batch of <= 16 rows.
DEVI size_t xfrag_off(int m, int k, int XR) { return ((size_t)(k >> 3) * XR + m) * 8 + (k & 7); }       // inside one tile: m < 16
DEVI size_t ximage_off(int m, int k, int XR, int K) { return (size_t)(m >> 4) * 16 * K + xfrag_off(m & 15, k, XR); }   // any row of the batch
constexpr int MAX_DECODE_ROWS = 64;        // sequences per decode step (4 tiles)

// 4 features (m, k..k+3), k % 4 == 0 -> X image (8-byte store)
DEVI void store_frag4(bf16_t* __restrict__ xf, int m, int k, int XR, float a, float b, float c, float d) {
    u32x2 pk = {pack_bf2(a, b), pack_bf2(c, d)};
    *reinterpret_cast<u32x2*>(xf + xfrag_off(m, k, XR)) = pk;
}

// KV page element offsets (layout in decode.hip's header); host-callable too (engine.hip: dots_debug_read_kv)
#define KV_HD __host__ __device__ __forceinline__
KV_HD int k_chunk(int key, int d) { return ((key >> 4) * 4 + (d >> 5)) * 64 + ((d >> 3) & 3) * 16 + (key & 15); }
KV_HD int v_off(int key, int d) {
    const int kk = key & 31;
    return (((key >> 5) * 8 + (d >> 4)) * 64 + ((kk >> 2) & 3) * 16 + (d & 15)) * 8 + 4 * (kk >> 4) + (kk & 3);
}

// fp8 (e4m3fn) KV pages (DotsConfig.kv_cache_dtype = 1; layout in decode.hip's header): the same fragment order, one byte per element, CHUNK
// PAIRS interleaved so that lane l's 16-byte load at byte (c2 * 64 + l) * 16 holds its 8 bytes of chunk 2 c2, then its 8 bytes of chunk 2 c2 + 1.
// kv8_byte maps an element offset of the bf16 page (chunk * 512 + lane * 8 + j) to its byte offset in the fp8 page.
constexpr int PAGE_BYTES8 = PAGE_ELEMS;    // per (kv head, K|V)
KV_HD int kv8_byte(int e) { return (e & ~1023) | (((e >> 3) & 63) << 4) | (((e >> 9) & 1) << 3) | (e & 7); }
KV_HD int k8_off(int key, int d) { return kv8_byte(k_chunk(key, d) * 8 + (d & 7)); }
KV_HD int v8_off(int key, int d) { return kv8_byte(v_off(key, d)); }
// Quantiser of every fp8-KV writer: e4m3fn(clamp(x / s, -448, 448)), fp32 division, round to nearest even (v_cvt_pk_fp8_f32);
// the clamp makes saturation explicit (an out-of-range value stores as +-448, never NaN).  Two values -> the low 16 bits (a first).
DEVI float kv8_sat(float x, float s) { return fminf(fmaxf(x / s, -448.0f), 448.0f); }
DEVI uint32_t kv8_pack2(float a, float b, float s) { return (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(kv8_sat(a, s), kv8_sat(b, s), 0, false) & 0xffffu; }
// 8 bf16 (one 16-byte fragment row of the bf16 page) -> 8 e4m3 bytes, element order kept
DEVI u32x2 kv8_pack8(u32x4 v, float s) {
    u32x2 o;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        int p = __builtin_amdgcn_cvt_pk_fp8_f32(kv8_sat(lo_bf(v[2 * h]), s), kv8_sat(hi_bf(v[2 * h]), s), 0, false);
        p = __builtin_amdgcn_cvt_pk_fp8_f32(kv8_sat(lo_bf(v[2 * h + 1]), s), kv8_sat(hi_bf(v[2 * h + 1]), s), p, true);
        o[h] = (uint32_t)p;
    }
    return o;
}
// half `hi` of a lane's 16-byte load of an fp8 page -> the bf16x8 MFMA operand the bf16 page holds for that chunk (exact: every e4m3 value is a bf16)
DEVI bf16x8 kv8_frag(u32x4 r, int hi) {
    const uint32_t a = r[2 * hi], b = r[2 * hi + 1];
    const u32x4 o = {__builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(a, 1.0f, false)),
                     __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(a, 1.0f, true)),
                     __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(b, 1.0f, false)),
                     __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(b, 1.0f, true))};
    return __builtin_bit_cast(bf16x8, o);
}
