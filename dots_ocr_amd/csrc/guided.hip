// Guided decoding: the allowed-token bits of the guided rows of a step, and the stream-ordered writers of the row table.
//
// A guide is a byte DFA (kernels.h RowGuide: table [n_states][256] uint16, GUIDE_DEAD = no transition).  The host compiler trims it, so every
// state that is not dead can still reach an accepting one: a token is allowed at state s iff it has bytes and walking them from s never
// meets GUIDE_DEAD.  guide_mask_kernel evaluates that for the whole vocabulary of every guided row, before the per-row selection stage
// reads the logits (select_partial_kernel takes the bit beside the rule image); commit_token (decode.hip) then advances the row's state by
// the bytes of the token it commits.
//
// Cost model at V = 151 936: one thread per token, 8 tokens per thread.  The first byte decides for most of the vocabulary (a JSON guide
// that expects a digit rejects every token that does not start with one), and the 512-byte row of the CURRENT state is the only part of
// the table all those rejects need — it is staged in LDS once per workgroup.  Tokens that survive their first byte go on through the table
// in global memory: at most 4096 states x 512 B = 2 MB, read-only for the whole launch, so it stays in L2.  Offsets are read coalesced
// (thread i reads tok_off[i] and tok_off[i + 1]); the bytes of a token are read one by one, which only the surviving lanes pay for.
// The 64 verdicts of a wave leave as one ballot and one 8-byte vector store by lane 0: no atomics, no read-modify-write of the mask.
#include "common.h"
#include "kernels.h"

namespace {

constexpr int GM_THREADS = 256;
constexpr int GM_TOKENS = 2048;           // tokens per workgroup: 8 per thread, 64 consecutive ones per wave and pass

// The allowed bits of the GM_TOKENS tokens of workgroup blockIdx.x at `state` of `table` into `out` (one row of the mask).  Called by all
// GM_THREADS threads with uniform arguments; s_row: 256 entries of LDS
DEVI void guide_mask_row(const GuideSel& g, const uint16_t* __restrict__ table, int state, uint32_t* __restrict__ out, uint16_t* s_row) {
    s_row[threadIdx.x] = table[(size_t)state * 256 + threadIdx.x];
    __syncthreads();
    const int32_t* __restrict__ off = g.tok_off;
    const uint8_t* __restrict__ bytes = g.tok_bytes;
    const int base = blockIdx.x * GM_TOKENS;
#pragma unroll 1
    for (int k = 0; k < GM_TOKENS / GM_THREADS; ++k) {
        const int i0 = base + k * GM_THREADS + (int)(threadIdx.x & ~63u);      // first token of this wave's pass: a multiple of 64
        if (i0 >= g.V) break;                                                  // uniform per wave
        const int i = i0 + (int)(threadIdx.x & 63u);
        bool ok = false;
        if (i < g.V) {
            int j = off[i];
            const int end = off[i + 1];
            if (j < end) {
                uint32_t s = s_row[bytes[j]];
                for (++j; j < end && s != GUIDE_DEAD; ++j) s = table[(size_t)s * 256 + bytes[j]];
                ok = s != GUIDE_DEAD;
            }
        }
        const unsigned long long bits = __ballot(ok);
        // words is even and i0 a multiple of 64: word i0 / 32 of a 256-byte aligned buffer is 8-byte aligned, and i0 / 32 + 1 < words
        if ((threadIdx.x & 63u) == 0) *reinterpret_cast<uint2*>(out + (i0 >> 5)) = make_uint2((uint32_t)bits, (uint32_t)(bits >> 32));
    }
}

// grid (ceil(V / GM_TOKENS), rows)
__global__ __launch_bounds__(GM_THREADS) void guide_mask_kernel(GuideSel g, const int32_t* __restrict__ sel) {
    __shared__ uint16_t s_row[256];
    const int b = blockIdx.y;
    if (sel && !sel[b]) return;                                       // uniform per workgroup
    const RowGuide rg = g.rows[b];
    if (!rg.table) return;
    guide_mask_row(g, rg.table, rg.state, g.mask + (size_t)b * g.words, s_row);
}

// The draft rows of a speculating step.  grid (ceil(V / GM_TOKENS), rows * k): workgroup y serves step row r = rows + y =
// j * rows + b with the table of slot b at the state the chain kernel (spec.hip) left for r; a dead, idle or unguided row (gstate < 0:
// its slot then may hold no table) exits at once
__global__ __launch_bounds__(GM_THREADS) void guide_mask_drafts_kernel(GuideSel g, int rows, const int32_t* __restrict__ gstate) {
    __shared__ uint16_t s_row[256];
    const int r = rows + blockIdx.y, b = r % rows;
    const int state = gstate[r];
    if (state < 0) return;                                            // uniform per workgroup
    const RowGuide rg = g.rows[b];
    if (!rg.table || state >= rg.n_states) return;                    // never: the chain walked this table
    guide_mask_row(g, rg.table, state, g.mask + (size_t)r * g.words, s_row);
}

__global__ void set_row_guide_kernel(RowGuide* table, int row, RowGuide g) {
    g.state = g.start;
    table[row] = g;
}

__global__ void guide_reset_rows_kernel(RowGuide* table, const int32_t* __restrict__ dst, int n) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= n) return;
    const int row = dst ? dst[b] : b;
    if (row < 0 || row >= DOTS_MAX_BATCH) return;
    if (table[row].table) table[row].state = table[row].start;
}

__global__ void guide_set_states_kernel(RowGuide* table, const int32_t* __restrict__ states, int n) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= n) return;
    if (table[b].table && states[b] >= 0 && states[b] < table[b].n_states) table[b].state = states[b];
}

}  // namespace

hipError_t launch_guide_mask(hipStream_t s, const GuideSel& g, int B, const int32_t* sel) {
    if (!g.rows || !g.mask || !g.tok_off || !g.tok_bytes || B < 1 || B > DOTS_MAX_BATCH || g.V < 1 || g.words != guide_mask_words(g.V)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(guide_mask_kernel, dim3((g.V + GM_TOKENS - 1) / GM_TOKENS, B), dim3(GM_THREADS), 0, s, g, sel);
    return hipGetLastError();
}

hipError_t launch_guide_mask_drafts(hipStream_t s, const GuideSel& g, int rows, int k, const int32_t* gstate) {
    if (!g.rows || !g.mask || !g.tok_off || !g.tok_bytes || !gstate || rows < 1 || k < 1 || k > DOTS_MAX_SPEC_DRAFTS || rows * (k + 1) > DOTS_MAX_BATCH ||
        g.V < 1 || g.words != guide_mask_words(g.V))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(guide_mask_drafts_kernel, dim3((g.V + GM_TOKENS - 1) / GM_TOKENS, rows * k), dim3(GM_THREADS), 0, s, g, rows, gstate);
    return hipGetLastError();
}

hipError_t launch_set_row_guide(hipStream_t s, RowGuide* table, int row, const RowGuide& g) {
    if (!table || row < 0 || row >= DOTS_MAX_BATCH) return hipErrorInvalidValue;
    if (g.table && (!g.accepting || g.n_states < 1 || g.start < 0 || g.start >= g.n_states)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(set_row_guide_kernel, dim3(1), dim3(1), 0, s, table, row, g);
    return hipGetLastError();
}

hipError_t launch_guide_reset_rows(hipStream_t s, RowGuide* table, const int32_t* dst, int n) {
    if (!table || n < 1 || n > DOTS_MAX_BATCH) return hipErrorInvalidValue;
    hipLaunchKernelGGL(guide_reset_rows_kernel, dim3(1), dim3(64), 0, s, table, dst, n);
    return hipGetLastError();
}

hipError_t launch_guide_set_states(hipStream_t s, RowGuide* table, const int32_t* states, int n) {
    if (!table || !states || n < 1 || n > DOTS_MAX_BATCH) return hipErrorInvalidValue;
    hipLaunchKernelGGL(guide_set_states_kernel, dim3(1), dim3(64), 0, s, table, states, n);
    return hipGetLastError();
}
