// No-repeat n-gram blocking: the banned-token bits of the rows of a step that carry an n-gram rule, and the stream-ordered
// writer of the row table.
//
// A row's rule is {n, window W, whitelist} (kernels.h RowNgram).  With out[0 .. L) the tokens the row has generated (StepState's out_ids /
// out_lens: the history is always on the device) and P = out[L - n + 1 .. L) its last n - 1 tokens, every earlier position i in
// [max(0, L - W), L - n] with out[i .. i + n - 1) == P bans the id that followed it, out[i + n - 1], unless that id is whitelisted.
// ngram_ban_kernel evaluates that for every such row before the per-row selection stage reads the logits; select_partial_kernel takes the
// bit beside the guide's bit and the rule image (decode.hip).
//
// One workgroup per row.  The result is a set, so it is built as a bitmask: the row's ceil(V / 32) words (19 KB at V = 151 936) live in
// LDS, a hit is an LDS atomicOr (integer, order-free: thread order cannot enter the result), and the whole row leaves in one coalesced
// pass of plain stores — no clearing pass over global memory, no global atomics, and a row without a single hit still overwrites the
// bits of its previous step.  A list of banned ids would be shorter to write but has no useful bound: with W = 0 every one of the
// L - n + 1 candidates may ban a different id.
// Threads stride over the candidates; each compares its n - 1 tokens against P (staged in LDS once) and leaves at the first mismatch, so
// ordinary text costs about one coalesced 4-byte read per candidate.  A row that really loops (the case the rule exists for) matches long
// prefixes: the worst case is (n - 1) reads per candidate, all of them L2 hits on a history of at most max_seq_len x 4 bytes.
#include "common.h"
#include "kernels.h"

namespace {

constexpr int NG_THREADS = 256;

// The banned bits of one row from a history of L tokens that `out(i)` reads, built in s_bits and stored to dst [g.words].  Called by every
// thread of the workgroup with uniform arguments; s_p / s_white are the caller's LDS.  ngram_ban_kernel reads the row's own output,
// ngram_ban_drafts_kernel the output followed by the drafts a draft row takes as committed: one rule, two histories.
template <typename Hist>
DEVI void ngram_ban_row(const NgramSel& g, const RowNgram& rule, int n, int L, Hist out, uint32_t* __restrict__ dst, uint32_t* s_bits, int32_t* s_p,
                        int32_t* s_white) {
    const int tid = threadIdx.x;
    const int window = rule.window, n_white = min(max(rule.n_white, 0), DOTS_MAX_NGRAM_WHITELIST);
    const int m = n - 1;
    for (int w = tid; w < g.words; w += NG_THREADS) s_bits[w] = 0;
    if (tid < m && L >= m) s_p[tid] = out(L - m + tid);
    if (tid < n_white) s_white[tid] = rule.white[tid];
    __syncthreads();
    // candidates i in [lo, L - n]: the n-gram out[i .. i + n) lies inside the history (and inside the last `window` tokens)
    const int lo = window > 0 ? max(0, L - window) : 0;
    for (int i = lo + tid; i <= L - n; i += NG_THREADS) {
        bool hit = true;
        for (int j = 0; j < m; ++j)
            if (out(i + j) != s_p[j]) { hit = false; break; }
        if (!hit) continue;
        const int id = out(i + m);
        if (id < 0 || id >= g.V) continue;                            // an id from memory indexes the bits only inside [0, V)
        bool white = false;
        for (int k = 0; k < n_white; ++k) white = white || s_white[k] == id;
        if (!white) atomicOr(&s_bits[id >> 5], 1u << (id & 31));
    }
    __syncthreads();
    for (int w = tid; w < g.words; w += NG_THREADS) dst[w] = s_bits[w];
}

// grid (rows); dynamic LDS: g.words x 4 bytes
__global__ __launch_bounds__(NG_THREADS) void ngram_ban_kernel(NgramSel g, const int32_t* __restrict__ out_ids, const int32_t* __restrict__ out_lens,
                                                               int out_stride, const int32_t* __restrict__ finished, const int32_t* __restrict__ sel) {
    extern __shared__ uint32_t s_bits[];
    __shared__ int32_t s_p[DOTS_MAX_NGRAM_SIZE];
    __shared__ int32_t s_white[DOTS_MAX_NGRAM_WHITELIST];
    const int b = blockIdx.x;
    if (sel && !sel[b]) return;                                       // uniform per workgroup, as the two below
    const int n = g.rows[b].n;
    if (n < 1 || n > DOTS_MAX_NGRAM_SIZE) return;
    if (finished && finished[b]) return;
    const int L = min(max(out_lens[b], 0), out_stride);
    const int32_t* __restrict__ out = out_ids + (size_t)b * out_stride;
    ngram_ban_row(g, g.rows[b], n, L, [out](int i) { return out[i]; }, g.mask + (size_t)b * g.words, s_bits, s_p, s_white);
}

// The banned bits of the live draft rows of a speculating step.  grid (rows * k): workgroup x serves step row r = rows + x =
// j * rows + b and exits at once unless the row is live (j <= n_live[b]: the slot is selected, unfinished and speculates) and the slot
// carries a rule.  Draft row (b, j) selects the token at output index L + j under the hypothesis that drafts 1 .. j were committed, so its
// history is out[0 .. L) ++ drafts[b][0 .. j) — values known at the head of the step, L = out_lens[b] before anything commits.  The rule
// is ngram_ban_row's; the bits go to row r of g.mask, which holds rows * (k + 1) rows: the stage keeps the rows below `rows`.
// dynamic LDS: g.words x 4 bytes
__global__ __launch_bounds__(NG_THREADS) void ngram_ban_drafts_kernel(NgramSel g, const int32_t* __restrict__ out_ids, const int32_t* __restrict__ out_lens,
                                                                      int out_stride, const int32_t* __restrict__ drafts, const int32_t* __restrict__ n_live,
                                                                      int rows) {
    extern __shared__ uint32_t s_bits[];
    __shared__ int32_t s_p[DOTS_MAX_NGRAM_SIZE];
    __shared__ int32_t s_white[DOTS_MAX_NGRAM_WHITELIST];
    __shared__ int32_t s_d[DOTS_MAX_SPEC_DRAFTS];
    const int r = rows + blockIdx.x, j = r / rows, b = r - j * rows;
    if (j > n_live[b]) return;                                        // uniform per workgroup, as the one below
    const int n = g.rows[b].n;
    if (n < 1 || n > DOTS_MAX_NGRAM_SIZE) return;
    const int L = min(max(out_lens[b], 0), out_stride);
    const int32_t* __restrict__ out = out_ids + (size_t)b * out_stride;
    if ((int)threadIdx.x < j) s_d[threadIdx.x] = drafts[b * DOTS_MAX_SPEC_DRAFTS + threadIdx.x];      // j <= n_live[b] <= k <= DOTS_MAX_SPEC_DRAFTS
    __syncthreads();
    const int32_t* d = s_d;
    ngram_ban_row(g, g.rows[b], n, L + j, [out, d, L](int i) { return i < L ? out[i] : d[i - L]; }, g.mask + (size_t)r * g.words, s_bits, s_p, s_white);
}

__global__ void set_row_ngram_kernel(RowNgram* table, int row, RowNgram r) { table[row] = r; }

// grid (rows)
__global__ __launch_bounds__(256) void ngram_history_kernel(const int32_t* __restrict__ hist, const int32_t* __restrict__ hist_lens, int stride,
                                                            const int32_t* __restrict__ n_prompt, int32_t* __restrict__ out_ids, int out_stride) {
    const int b = blockIdx.x;
    const int n = min(max(hist_lens[b], 0), stride), np = min(max(n_prompt[b], 0), n);
    for (int j = threadIdx.x; j < n - np; j += 256) out_ids[(size_t)b * out_stride + j] = hist[(size_t)b * stride + np + j];
}

}  // namespace

hipError_t launch_ngram_ban(hipStream_t s, const NgramSel& g, int B, const int32_t* out_ids, const int32_t* out_lens, int out_stride,
                            const int32_t* finished, const int32_t* sel) {
    if (!g.rows || !g.mask || !out_ids || !out_lens || out_stride < 1 || B < 1 || B > DOTS_MAX_BATCH || g.V < 1 || g.V > NGRAM_MAX_V ||
        g.words != ngram_mask_words(g.V))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(ngram_ban_kernel, dim3(B), dim3(NG_THREADS), (size_t)g.words * 4, s, g, out_ids, out_lens, out_stride, finished, sel);
    return hipGetLastError();
}

hipError_t launch_ngram_ban_drafts(hipStream_t s, const NgramSel& g, int rows, int k, const int32_t* out_ids, const int32_t* out_lens, int out_stride,
                                   const int32_t* drafts, const int32_t* n_live) {
    if (!g.rows || !g.mask || !out_ids || !out_lens || !drafts || !n_live || out_stride < 1 || rows < 1 || k < 1 || k > DOTS_MAX_SPEC_DRAFTS ||
        rows * (k + 1) > DOTS_MAX_BATCH || g.V < 1 || g.V > NGRAM_MAX_V || g.words != ngram_mask_words(g.V))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(ngram_ban_drafts_kernel, dim3(rows * k), dim3(NG_THREADS), (size_t)g.words * 4, s, g, out_ids, out_lens, out_stride, drafts, n_live,
                       rows);
    return hipGetLastError();
}

hipError_t launch_set_row_ngram(hipStream_t s, RowNgram* table, int row, const RowNgram& r) {
    if (!table || row < 0 || row >= DOTS_MAX_BATCH || r.n < 0 || r.n > DOTS_MAX_NGRAM_SIZE || r.window < 0 || r.n_white < 0 ||
        r.n_white > DOTS_MAX_NGRAM_WHITELIST)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(set_row_ngram_kernel, dim3(1), dim3(1), 0, s, table, row, r);
    return hipGetLastError();
}

hipError_t launch_ngram_history(hipStream_t s, const int32_t* hist, const int32_t* hist_lens, int stride, const int32_t* n_prompt, int B,
                                int32_t* out_ids, int out_stride) {
    if (!hist || !hist_lens || !n_prompt || !out_ids || B < 1 || B > DOTS_MAX_BATCH || stride < 1 || out_stride < stride) return hipErrorInvalidValue;
    hipLaunchKernelGGL(ngram_history_kernel, dim3(B), dim3(256), 0, s, hist, hist_lens, stride, n_prompt, out_ids, out_stride);
    return hipGetLastError();
}
