// Predicted outputs: a second drafter for the speculating step (spec.hip), which proposes a caller-supplied text instead of
// the row's own output, and the stream-ordered writers of a slot's prediction.  Nothing after the drafter knows where a draft came from:
// expand, the layer loop, the selection, the accept walk verify a predicted draft exactly as they verify an n-gram one, so a row commits
// the tokens of the unspeculated engine whatever the prediction holds.
//
//   predict_draft_kernel   end of the step, after ngram_draft_kernel and only while some slot holds a prediction: overwrites the drafts of
//                          the slots whose grown output it can align with their prediction
//
// The drafting rule (include/dots_ocr_hip.h; engine.predicted_draft states it on the host).  out[0 .. L) is the row's output, pred[0 .. P)
// its prediction, (cur, at) the slot's alignment: prediction index cur was the expected next token when the output was `at` long, so
// e* = cur + (L - at) is where the next token is expected now.
//   1. anchor   m = min(min_n, L, e*); if m >= 1, e* < P and pred[e* - m .. e*) == out[L - m .. L): e = e*
//   2. search   else, for n from min(max_n, L) down to min_n with key = out[L - n .. L): the candidates are the e = i + n < P with
//               pred[i .. i + n) == key; the first n that has one wins, among its candidates the one nearest to e*, the larger e on a tie
//   3. found    drafts = pred[e .. min(e + k, P)), cur = e, at = L, src = 1
//   4. else     (or no prediction) the slot keeps what ngram_draft_kernel left, cur and at stay — e* moves on with L — and src = 0
#include <climits>

#include "common.h"
#include "kernels.h"

namespace {

constexpr int PD_THREADS = 256;

// (|e - e*|, e) as one key whose minimum is the nearest candidate, the larger e on a tie
DEVI unsigned long long pd_key(long long es, int e) {
    long long d = es > e ? es - e : e - es;
    if (d > INT_MAX) d = INT_MAX;
    return ((unsigned long long)d << 32) | (unsigned)(INT_MAX - e);
}
constexpr unsigned long long PD_NONE = ~0ull;

// grid (B), PD_THREADS threads: the anchor is one compare per lane of wave 0; the search strides the threads over i, each keeps its best
// key, one wave reduction plus one LDS reduction per n (the shape of ngram_draft_kernel)
__global__ __launch_bounds__(PD_THREADS) void predict_draft_kernel(PredictState p, const int32_t* __restrict__ out_ids, const int32_t* __restrict__ out_lens,
                                                                   int out_stride, const int32_t* __restrict__ finished, const int32_t* __restrict__ sel,
                                                                   const int32_t* __restrict__ cls, int engine_greedy, int k, int min_n, int max_n,
                                                                   int32_t* __restrict__ drafts, int draft_stride, int32_t* __restrict__ n_draft,
                                                                   const int32_t* __restrict__ n_live) {
    __shared__ int32_t s_suf[DOTS_MAX_NGRAM_SIZE];
    __shared__ unsigned long long s_best[PD_THREADS / 64];
    __shared__ int s_anchor;
    const int b = blockIdx.x, tid = threadIdx.x;
    const bool speculates = engine_greedy && !(cls && cls[b] == SPEC_ROW_NONE);
    const int P = min(max(p.len[b], 0), p.stride);
    const int L = min(max(out_lens[b], 0), out_stride);
    // the counters: the drafts this kernel left at its last run were verified by the step that just ran (n_live of them, after the cap cut
    // them), and the step committed one token plus what the walk accepted — also at the run that finds the row finished
    if (tid == 0 && p.stats && n_live && !(sel && !sel[b])) {
        if (p.src[b] && n_live[b] >= 0) {
            p.stats[b * 2] += (unsigned long long)n_live[b];
            p.stats[b * 2 + 1] += (unsigned long long)max(L - p.seen[b] - 1, 0);
        }
        p.seen[b] = L;
    }
    if ((sel && !sel[b]) || (finished && finished[b]) || !speculates || P == 0) {      // uniform per workgroup
        if (tid == 0) p.src[b] = 0;
        return;
    }
    const int32_t* __restrict__ out = out_ids + (size_t)b * out_stride;
    const int32_t* __restrict__ pred = p.ids + (size_t)b * p.stride;
    const long long es = (long long)p.cur[b] + L - p.at[b];
    int e = -1;                                                       // uniform from every assignment on
    // ---- 1. the anchor: min_n <= DOTS_MAX_NGRAM_SIZE = 64 compares, one per lane of wave 0
    const int m = (int)min((long long)min(min_n, L), es);
    if (m >= 1 && es < P) {
        if (tid < 64) {
            const bool ok = tid >= m || pred[(int)es - m + tid] == out[L - m + tid];
            const bool all = __all(ok);
            if (tid == 0) s_anchor = all;
        }
        __syncthreads();
        if (s_anchor) e = (int)es;
    }
    // ---- 2. the search
    if (e < 0) {
        const int n_top = min(max_n, L);
        if (tid < n_top) s_suf[tid] = out[L - n_top + tid];
        __syncthreads();
        for (int n = n_top; n >= min_n && e < 0; --n) {
            const int32_t* key = s_suf + (n_top - n);
            unsigned long long best = PD_NONE;
            for (int i = tid; i + n < P; i += PD_THREADS) {
                bool hit = true;
                for (int j = n - 1; j >= 0; --j)
                    if (pred[i + j] != key[j]) { hit = false; break; }
                if (hit) best = min(best, pd_key(es, i + n));
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const unsigned hi = __shfl_xor((unsigned)(best >> 32), o, 64), lo = __shfl_xor((unsigned)best, o, 64);
                best = min(best, ((unsigned long long)hi << 32) | lo);
            }
            if ((tid & 63) == 0) s_best[tid >> 6] = best;
            __syncthreads();
            for (int w = 0; w < PD_THREADS / 64; ++w) best = min(best, s_best[w]);
            __syncthreads();                                          // the partials are read: the next n may overwrite them
            if (best != PD_NONE) e = INT_MAX - (int)(unsigned)best;
        }
    }
    // ---- 3. / 4.
    if (e < 0) {
        if (tid == 0) p.src[b] = 0;
        return;
    }
    const int cnt = min(k, P - e);                                    // e < P: at least one
    if (tid < cnt) drafts[(size_t)b * draft_stride + tid] = pred[e + tid];
    if (tid == 0) {
        n_draft[b] = cnt;
        p.cur[b] = e; p.at[b] = L; p.src[b] = 1;
    }
}

// len[row] = n with the alignment at the start; n == 0: the slot holds none, and drafts it took from the one it held are dropped
__global__ void predict_set_row_kernel(PredictState p, int32_t* n_draft, int row, int n) {
    p.len[row] = n;
    p.cur[row] = 0; p.at[row] = 0;
    if (n == 0) {
        if (p.src[row] && n_draft) n_draft[row] = 0;
        p.src[row] = 0;
    }
}

}  // namespace

hipError_t launch_predict_draft(hipStream_t s, const PredictState& p, const int32_t* out_ids, const int32_t* out_lens, int out_stride, const int32_t* finished,
                                const int32_t* sel, const int32_t* cls, int engine_greedy, int B, int k, int min_n, int max_n, int32_t* drafts, int draft_stride,
                                int32_t* n_draft, const int32_t* n_live) {
    if (!p.seen != !p.stats) return hipErrorInvalidValue;
    if (!p.ids || !p.len || !p.cur || !p.at || !p.src || p.stride < 1 || !out_ids || !out_lens || !drafts || !n_draft || out_stride < 1 || B < 1 ||
        B > DOTS_MAX_BATCH || k < 1 || k > DOTS_MAX_SPEC_DRAFTS || draft_stride < k || min_n < 1 || max_n < min_n || max_n > DOTS_MAX_NGRAM_SIZE)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(predict_draft_kernel, dim3(B), dim3(PD_THREADS), 0, s, p, out_ids, out_lens, out_stride, finished, sel, cls, engine_greedy, k, min_n,
                       max_n, drafts, draft_stride, n_draft, n_live);
    return hipGetLastError();
}

hipError_t launch_predict_set_row(hipStream_t s, const PredictState& p, int32_t* n_draft, int row, int n) {
    if (!p.len || !p.cur || !p.at || !p.src || row < 0 || row >= DOTS_MAX_BATCH || n < 0 || n > p.stride) return hipErrorInvalidValue;
    hipLaunchKernelGGL(predict_set_row_kernel, dim3(1), dim3(1), 0, s, p, n_draft, row, n);
    return hipGetLastError();
}
