// Device side of the loop guard: the check that runs after the commit of a token.  ONE definition: select_rows_kernel
// (decode.hip) runs it on the rows of a step that hold a rule, loop_probe_kernel (loop.hip) on explicit histories.
//
// The rule.  out[0 .. n] is the row's output, out[n] the token just committed.  Period p in [min_period, max_period] fires iff
// out[i] == out[i - p] for every i in [n + 1 - L(p) + p, n], L(p) = max(repeats * p, min_span), and n + 1 >= L(p): the last L(p) tokens
// repeat with period p.  That is "the last L(p) - p indices matched their predecessor at distance p", so each period keeps ONE number,
// the length of the run of such indices that ends at n: run = (n >= p && out[n] == out[n - p]) ? run + 1 : 0, and fires when
// run >= L(p) - p (a run counts indices >= p only, so n + 1 >= L(p) holds with it).  No history is scanned: a step costs one read of
// out[n - p] and one counter update per period.
//
// Every function here is called by all LOOP_THREADS threads of a workgroup with uniform arguments but `run`; thread t owns period t + 1.
#pragma once
#include "common.h"
#include "kernels.h"
#include "step_dev.h"

constexpr int LOOP_THREADS = 1024;
static_assert(LOOP_THREADS == DOTS_MAX_LOOP_PERIOD, "one thread per period");
constexpr int LOOP_NONE = 0x7fffffff;

// LDS of one workgroup: the waves' minima, double-buffered by the parity of n so that a caller that loops over tokens needs one barrier each
struct LoopLds { int wave_min[2][LOOP_THREADS / 64]; };

DEVI int loop_span(const RowLoop& r, int p) { return max(r.repeats * p, r.min_span); }

// The token `tok` was committed at output index n of a row whose earlier output is out[0 .. n) (out[n] itself is not read).  run: this
// thread's counter, updated in place.  Returns the smallest period that fires, the same value in every thread, or LOOP_NONE.
DEVI int loop_step(const RowLoop& r, int32_t& run, const int32_t* __restrict__ out, int n, int tok, LoopLds& L) {
    const int p = (int)threadIdx.x + 1;
    int mine = LOOP_NONE;
    if (p >= r.min_period && p <= r.max_period) {
        run = (n >= p && tok == out[n - p]) ? run + 1 : 0;
        if (run >= loop_span(r, p) - p) mine = p;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mine = min(mine, __shfl_xor(mine, o, 64));
    int* w = L.wave_min[n & 1];
    if ((threadIdx.x & 63) == 0) w[threadIdx.x >> 6] = mine;
    __syncthreads();
    int best = LOOP_NONE;
#pragma unroll
    for (int k = 0; k < LOOP_THREADS / 64; ++k) best = min(best, w[k]);
    return best;
}

// What the stage does with a row b that holds a rule, after thread 0 committed its token: what = commit_token's answer, n = the output
// index the token went to, both known to thread 0 only and handed to the workgroup through LDS.  A row that was finished already and a
// token that finished it as an EOS or stop id are not checked.  The hit: {hit_tok = n, period, span = L(period)}, and the row is finished.
struct LoopCommitLds { int what, n, tok; LoopLds L; };
DEVI void loop_after_commit(const LoopSel& ls, const StepState& st, int b, int what, int n, int tok, LoopCommitLds& S) {
    if (threadIdx.x == 0) { S.what = what; S.n = n; S.tok = tok; }
    __syncthreads();
    if (S.what != COMMIT_TOKEN) return;                               // uniform per workgroup
    const RowLoop r = ls.rows[b];
    int32_t* cell = ls.run + (size_t)b * DOTS_MAX_LOOP_PERIOD + threadIdx.x;
    const bool mine = (int)threadIdx.x + 1 >= r.min_period && (int)threadIdx.x + 1 <= r.max_period;
    int32_t run = mine ? *cell : 0;
    const int p = loop_step(r, run, st.out_ids + (size_t)b * st.out_stride, S.n, S.tok, S.L);
    if (mine) *cell = run;
    if (threadIdx.x == 0 && p != LOOP_NONE) {
        RowLoop& h = ls.rows[b];
        h.hit_tok = S.n; h.period = p; h.span = loop_span(r, p);
        st.finished[b] = 1;
    }
}
