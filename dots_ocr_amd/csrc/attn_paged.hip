// Causal flash attention of a BLOCK OF QUERY ROWS over a sequence's own KV pages (chunked prefill).
//
// The pages are stored in the fragment order of v_mfma_f32_16x16x32_bf16 (decode.hip's header, decode_layout.h), so a page is an MFMA
// operand as it lies: K is the A operand of S^T = K.Q^T, V the A operand of O^T = V^T.P^T, and P^T leaves the S^T MFMAs in exactly the key
// order the V chunks hold.  This is the arithmetic of decode_attn_kernel's page_step with one difference: the 16 columns of a tile are 16
// query ROWS of one head (each with its own causal limit) instead of the <= 16 query heads of one row.
//
// Work item (PagedQBlock) = one 64-position query block of one sequence: positions [q0, q0 + n), q0 % 64 == 0, 1 <= n <= 64, whose q
// rows are rows tok0 .. tok0 + n - 1 of the pass's head-major workspace q [Hq][T][128] (rope applied).  Its keys are pages 0 .. q0 / 64
// of block-table row `seq` — the page the pass has just written included (launch_kv_to_pages runs first on the same stream).
// grid (items, Hq / G), 4 waves: wave w holds query rows 16 w .. 16 w + 15 of the block for G query heads of ONE kv head, so a page a
// wave has loaded (32 KiB of registers' worth of K and V fragments) serves G heads (3 for the model's group of 6).  A wave whose rows
// lie past n exits at once; the columns past n of the last live wave repeat row n - 1 and are not stored.
//
// ROW INDEPENDENCE, bit for bit (what the exactness of a chunked fill rests on).  A column of the MFMA result depends on its own column
// of the B operand only; the running maximum, the row sum and the rescale factor are per column; the key walk is pages 0, 1, .., q0 / 64
// in ascending order, 64 keys per step — a function of the row's position alone; nothing is decided per tile (no skipped rescale, no
// early exit on a tile's maximum).  The only wave-uniform branches are "first page" (p == 0: O is still zero, the rescale is skipped —
// 0 * alpha = 0 exactly) and "diagonal page" (p == q0 / 64: the causal select; on every earlier page each key is visible to each row).
// So a row's output is a function of its q, its position and keys 0 .. position — not of the rows that share its block or its launch,
// of G, or of where earlier passes were cut.
//
// Masking: on the diagonal page key j is visible to the row at position p iff j <= p.  The select REPLACES the score, so whatever the
// masked slots hold (the unused slots of a ragged last page, NaN or infinite products of poison) never reaches the softmax; their P is
// exactly 0.  V slots behind them must be finite (the engine writes zeros: kv_to_pages_kernel fills the whole page).
//
// fp8 pool (KV8): the e4m3 bytes are converted to the bf16 fragments of the bf16 pool in registers once per page (kv8_frag, exact), s_K
// is folded into the score scale and s_V multiplied into the output, as decode attention's kv8 form does.
//
// Bounds: every index the kernel forms comes from the work list (tok0 + row < T, q0 / 64 < max_pages, seq) and the block table;
// launch_flash_attn_paged checks the host copy of the list before it launches.
#include <cstdlib>
#include <type_traits>

#include "common.h"
#include "decode_layout.h"
#include "kernels.h"
#include "switches.h"

namespace {

template <bool KV8, int G>
__global__ __launch_bounds__(256) void flash_attn_paged_kernel(const bf16_t* __restrict__ q, const void* __restrict__ pool_v,
                                                                const int32_t* __restrict__ block_table, int max_pages,
                                                                const PagedQBlock* __restrict__ items, bf16_t* __restrict__ out, int64_t T,
                                                                int Hq, int Hkv, float scale_log2e, const float* __restrict__ kv_scales) {
    using KVT = typename std::conditional<KV8, uint8_t, bf16_t>::type;
    const KVT* pool = reinterpret_cast<const KVT*>(pool_v);
    const PagedQBlock it = items[blockIdx.x];
    const int l = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), i = l & 15, g = l >> 4;
    if (16 * w >= it.n) return;
    const int h0 = blockIdx.y * G, hkv = h0 / (Hq / Hkv);
    const int row = min(16 * w + i, it.n - 1);             // columns past n repeat the last row (never stored)
    const int pos = it.q0 + row;
    float s_v = 1.0f;
    if constexpr (KV8) {
        scale_log2e *= kv_scales[hkv * 2];
        s_v = kv_scales[hkv * 2 + 1];
    }
    // lane (i, g) of head j reads Q[h0 + j][tok0 + row][32 kk + 8 g .. +7] (the B operand of S^T)
    const bf16_t* qrow = q + ((size_t)h0 * T + it.tok0 + row) * 128 + g * 8;
    const int32_t* tab = block_table + (size_t)it.seq * max_pages;
    const int last = it.q0 >> 6;

    f32x4 o[G][8];
    float m_run[G], l_run[G];
#pragma unroll
    for (int j = 0; j < G; ++j) {
        m_run[j] = -1e30f;
        l_run[j] = 0.f;
#pragma unroll
        for (int dg = 0; dg < 8; ++dg) o[j][dg] = f32x4{0, 0, 0, 0};
    }

    for (int p = 0; p <= last; ++p) {
        const int pg = tab[p];
        const KVT* kp = pool + ((size_t)(pg * Hkv + hkv) * 2) * PAGE_ELEMS;
        const KVT* vp = kp + PAGE_ELEMS;
        bf16x8 kf[16], vf[16];
        if constexpr (KV8) {
            u32x4 k8[8], v8[8];
#pragma unroll
            for (int c2 = 0; c2 < 8; ++c2) k8[c2] = *reinterpret_cast<const u32x4*>(kp + (size_t)(c2 * 64 + l) * 16);
#pragma unroll
            for (int c2 = 0; c2 < 8; ++c2) v8[c2] = *reinterpret_cast<const u32x4*>(vp + (size_t)(c2 * 64 + l) * 16);
#pragma unroll
            for (int c = 0; c < 16; ++c) kf[c] = kv8_frag(k8[c >> 1], c & 1);
#pragma unroll
            for (int c = 0; c < 16; ++c) vf[c] = kv8_frag(v8[c >> 1], c & 1);
        } else {
#pragma unroll
            for (int c = 0; c < 16; ++c) kf[c] = *reinterpret_cast<const bf16x8*>(kp + (size_t)(c * 64 + l) * 8);
#pragma unroll
            for (int c = 0; c < 16; ++c) vf[c] = *reinterpret_cast<const bf16x8*>(vp + (size_t)(c * 64 + l) * 8);
        }
        const bool first = p == 0, diag = p == last;
        const int key0 = p * PAGE;
#pragma unroll
        for (int j = 0; j < G; ++j) {
            bf16x8 qf[4];
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) qf[kk] = *reinterpret_cast<const bf16x8*>(qrow + (size_t)j * T * 128 + kk * 32);
            // S^T[kg]: rows = keys key0 + 16 kg + 4 g + r, column = query row i
            f32x4 s[4];
#pragma unroll
            for (int kg = 0; kg < 4; ++kg) {
                s[kg] = f32x4{0, 0, 0, 0};
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) s[kg] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[kg * 4 + kk], qf[kk], s[kg], 0, 0, 0);
            }
            float mx = -INFINITY;
#pragma unroll
            for (int kg = 0; kg < 4; ++kg)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    if (diag) s[kg][r] = key0 + kg * 16 + 4 * g + r <= pos ? s[kg][r] : -INFINITY;
                    mx = fmaxf(mx, s[kg][r]);
                }
            mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
            mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
            const float m_new = fmaxf(m_run[j], mx * scale_log2e);
            const float alpha = __builtin_amdgcn_exp2f(m_run[j] - m_new);
            m_run[j] = m_new;
            float psum = 0.f;
            bf16x8 pf[2];
#pragma unroll
            for (int slab = 0; slab < 2; ++slab) {
                u32x4 pk;
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    float pv[4];
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        pv[r] = __builtin_amdgcn_exp2f(fmaf(s[slab * 2 + t][r], scale_log2e, -m_new));
                        psum += pv[r];
                    }
                    pk[t * 2] = pack_bf2(pv[0], pv[1]);
                    pk[t * 2 + 1] = pack_bf2(pv[2], pv[3]);
                }
                pf[slab] = __builtin_bit_cast(bf16x8, pk);
            }
            l_run[j] = l_run[j] * alpha + psum;
            if (!first) {
#pragma unroll
                for (int dg = 0; dg < 8; ++dg)
#pragma unroll
                    for (int r = 0; r < 4; ++r) o[j][dg][r] *= alpha;
            }
#pragma unroll
            for (int dg = 0; dg < 8; ++dg) o[j][dg] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf[dg], pf[0], o[j][dg], 0, 0, 0);
#pragma unroll
            for (int dg = 0; dg < 8; ++dg) o[j][dg] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf[8 + dg], pf[1], o[j][dg], 0, 0, 0);
        }
    }
    // O^T[d = 16 dg + 4 g + r][query row i] / l -> out [T][Hq * 128]
    const bool live = 16 * w + i < it.n;
    bf16_t* orow = out + (size_t)(it.tok0 + row) * Hq * 128 + (size_t)h0 * 128 + 4 * g;
#pragma unroll
    for (int j = 0; j < G; ++j) {
        float ls = l_run[j];
        ls += __shfl_xor(ls, 16, 64);
        ls += __shfl_xor(ls, 32, 64);
        const float inv = s_v / ls;
        if (live) {
#pragma unroll
            for (int dg = 0; dg < 8; ++dg) {
                const u32x2 pk = {pack_bf2(o[j][dg][0] * inv, o[j][dg][1] * inv), pack_bf2(o[j][dg][2] * inv, o[j][dg][3] * inv)};
                *reinterpret_cast<u32x2*>(orow + j * 128 + dg * 16) = pk;
            }
        }
    }
}

}  // namespace

hipError_t launch_flash_attn_paged(hipStream_t s, const bf16_t* q, const void* pool_layer, const int32_t* block_table, int max_pages, int table_rows,
                                   const PagedQBlock* items_host, const PagedQBlock* items_dev, int n_items, bf16_t* out, int64_t T, int Hq, int Hkv,
                                   float scale, const float* kv_scales) {
    if (!q || !pool_layer || !block_table || !items_host || !items_dev || !out || n_items < 1 || Hkv < 1 || Hq % Hkv != 0 || max_pages < 1) return hipErrorInvalidValue;
    for (int k = 0; k < n_items; ++k) {
        const PagedQBlock& b = items_host[k];
        // a prefix that is not a multiple of 64 positions has no kernel here: the key walk is whole pages below the block's own
        if (b.q0 < 0 || b.q0 % PAGE != 0 || b.n < 1 || b.n > PAGE || b.q0 / PAGE >= max_pages || b.seq < 0 || b.seq >= table_rows || b.tok0 < 0 ||
            (int64_t)b.tok0 + b.n > T)
            return hipErrorInvalidValue;
    }
    const float sl = scale * 1.44269504088896340736f;
    const int group = Hq / Hkv;
    // G query heads of a kv head per wave: a page a wave has loaded serves G heads.  3 (half of the model's group of 6) is the most the
    // register file holds without spilling (K and V fragments 128 registers, O 32 per head; 6 heads spilled 180 registers).  One head per
    // wave — three times the workgroups, two waves per SIMD — was measured for launches with few work items and lost everywhere (one A4
    // prompt 0.36 against 0.27 ms, a 1 024-position pass of the full-size model 18.4 against 13.7 ms: profiles/chunked_prefill.txt).
    // DOTS_OCR_PAGED_ATTN_HEADS=1 still selects it (read per call): the choice changes no bit (header), which tests/test_paged_prefill_attn_gpu.py checks.
    int g_heads = group % 3 == 0 ? 3 : (group % 2 == 0 ? 2 : 1);
    if (sw::parse_paged_attn_one_head(sw::read_now(sw::PAGED_ATTN_HEADS))) g_heads = 1;
#define PAGED_GO(GV)                                                                                                                       \
    do {                                                                                                                                   \
        const dim3 grid(n_items, Hq / GV);                                                                                                 \
        if (kv_scales)                                                                                                                     \
            hipLaunchKernelGGL((flash_attn_paged_kernel<true, GV>), grid, dim3(256), 0, s, q, pool_layer, block_table, max_pages, items_dev, \
                               out, T, Hq, Hkv, sl, kv_scales);                                                                            \
        else                                                                                                                               \
            hipLaunchKernelGGL((flash_attn_paged_kernel<false, GV>), grid, dim3(256), 0, s, q, pool_layer, block_table, max_pages,          \
                               items_dev, out, T, Hq, Hkv, sl, nullptr);                                                                   \
    } while (0)
    if (g_heads == 3) PAGED_GO(3);
    else if (g_heads == 2) PAGED_GO(2);
    else PAGED_GO(1);
#undef PAGED_GO
    return hipGetLastError();
}
