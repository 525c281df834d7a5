// N-gram speculative decoding: the kernels a speculating decode step adds around the unchanged layer loop, and the
// stream-ordered writers of a row's drafts and of its speculation class.
//
// A slot b that holds d drafts occupies 1 + d rows of one step.  The step runs over R = rows x (k + 1) rows, draft-major: row
// r = j * rows + b carries token j of (last committed token, draft 1 .. k) of slot b at context ctx + j, and all the rows of a slot name
// the slot's KV pages.  dec_qkv appends the K/V of every row in a launch of its own before the attention launch, so row j attends over
// what rows 0 .. j - 1 appended and — every decode kernel being row-independent and batch-invariant bit for bit — its logits are those of
// the sequential step at that position.  The first `rows` rows are the rows of an unspeculated step: the existing selection stage
// commits their tokens with its present arguments.
//
//   spec_expand_kernel   head of the step: tokens, context lengths and block-table rows of the R rows from the slots' state and drafts
//   spec_argmax_kernel   after the lm_head: the arg-max partials of the live draft rows (the merge rule of argmax_partial_kernel)
//   spec_thresh_kernel, spec_draw_kernel   then, only while a row with parameters may speculate (dots_set_speculation_rows): the candidates
//                        of the live draft rows of SPEC_ROW_DRAW slots, by the selection stage's own arithmetic (select_dev.h)
//   spec_guide_chain_kernel, (guide_mask_drafts_kernel, guided.hip)   after spec_argmax_kernel, only while a guided row may speculate
//                        (dots_set_speculation_guided): the state every live draft row of a guided slot is selected under, and its allowed bits
//   (ngram_ban_drafts_kernel, ngram.hip)   only while a row with an n-gram rule may speculate (dots_set_speculation_shaped): the banned
//                        bits of every live draft row of such a slot, over the slot's output followed by the drafts before the row
//   spec_shape_select_kernel   then, while a guided, ruled, n-gram or penalised row may speculate: the arg-max partials (and values, for a
//                        sampled slot) of the live draft rows of such slots, shaped by the selection stage's own function (select_dev.h)
//   spec_accept_kernel   after the selection stage: walks a slot's drafts and commits through commit_token while they hold
//   (spec_logprob_partial_kernel, spec_logprob_final_kernel, logprobs.hip)   only while a row with logprobs may speculate
//                        (dots_set_speculation_logprobs) and some row has them on: the partials of the live draft rows of such slots beside
//                        spec_argmax_kernel, and after spec_accept_kernel the entries of the candidates it committed, from its accept record
//   ngram_draft_kernel   end of the step: the next step's drafts from the row's own output (prompt lookup without the prompt)
//   (predict_draft_kernel, predict.hip)   then, only while some slot holds a prediction (dots_set_row_prediction): the drafts of the slots
//                        whose output aligns with their prediction, from that prediction
//
// Draft row (b, j >= 1) is LIVE iff slot b is selected, not finished, a speculating row (sp.cls[b] != SPEC_ROW_NONE: the host's fact,
// kernels.h SpecRow; engine-wide arg max), holds at least j drafts and j < max_len[b] - out_lens[b]: a live row writes KV position ctx + j, and
// the last condition is "the sequence may still reach that position", which is also what its pages cover (the host lowers max_len when
// the pool runs dry).  Every other draft row idles like a released slot: context 0 on the scratch page.
#include <climits>

#include "kernels.h"
#include "select_dev.h"
#include "step_dev.h"

namespace {

constexpr int ND_THREADS = 256;

// the drafts slot b verifies in this step, or -1 when the slot takes no step at all (free or finished)
DEVI int spec_live_drafts(const SpecState& sp, const StepState& st, int b) {
    if ((st.sel && !st.sel[b]) || st.finished[b]) return -1;
    if (!sp.engine_greedy || sp.cls[b] == SPEC_ROW_NONE) return 0;
    const int room = (st.max_len ? st.max_len[b] : st.cap) - st.out_lens[b] - 1;      // draft rows whose token could still be committed
    return max(0, min(min(sp.n_draft[b], sp.k), room));
}

// grid (R = rows * (k + 1)), 64 threads
__global__ __launch_bounds__(64) void spec_expand_kernel(SpecState sp, StepState st, const int32_t* __restrict__ block_table, int max_pages,
                                                         int rows, int scratch_page) {
    const int r = blockIdx.x, j = r / rows, b = r - j * rows;
    const int nl = spec_live_drafts(sp, st, b);
    const bool live = j == 0 || j <= nl;
    const int32_t* __restrict__ src = block_table + (size_t)b * max_pages;
    int32_t* __restrict__ dst = sp.block_table + (size_t)r * max_pages;
    for (int p = threadIdx.x; p < max_pages; p += 64) dst[p] = live ? src[p] : scratch_page;
    if (threadIdx.x == 0) {
        sp.tokens[r] = j >= 1 && live ? sp.drafts[b * DOTS_MAX_SPEC_DRAFTS + j - 1] : st.cur_tokens[b];
        sp.ctx_len[r] = j == 0 ? st.ctx_len[b] : live ? st.ctx_len[b] + j : 0;
        if (j == 0) sp.n_live[b] = nl;
    }
}

// grid (ARGMAX_CHUNKS, R - rows): the partials of draft row rows + blockIdx.y, as argmax_partial_kernel (decode.hip) leaves them
__global__ __launch_bounds__(256) void spec_argmax_kernel(const float* __restrict__ logits, int V, int ld, int rows, const int32_t* __restrict__ n_live,
                                                          float* __restrict__ pval, int32_t* __restrict__ pidx) {
    __shared__ float sv[4];
    __shared__ int si[4];
    const int c = blockIdx.x, r = rows + blockIdx.y, j = r / rows, b = r - j * rows;
    if (j > n_live[b]) return;                                        // an idle row: nobody reads its partials
    const int per = (V + ARGMAX_CHUNKS - 1) / ARGMAX_CHUNKS;
    const int lo = c * per, hi = min(V, lo + per);
    const float* row = logits + (size_t)r * ld;
    float best = -INFINITY;
    int bi = 0x7fffffff;
    for (int i = lo + threadIdx.x; i < hi; i += 256) argmax_merge(best, bi, row[i], i);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) argmax_merge(best, bi, __shfl_xor(best, o, 64), __shfl_xor(bi, o, 64));
    if ((threadIdx.x & 63) == 0) { sv[threadIdx.x >> 6] = best; si[threadIdx.x >> 6] = bi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < 4; ++k) argmax_merge(best, bi, sv[k], si[k]);
        pval[r * ARGMAX_CHUNKS + c] = best;
        pidx[r * ARGMAX_CHUNKS + c] = bi;
    }
}

// The candidates of the draft rows of sampled slots.  grid (rows * k): workgroup x serves draft row r = rows + x = j * rows + b, and exits at
// once unless the row is live and its slot is SPEC_ROW_DRAW.  The row is selected exactly as select_thresh_kernel / select_rows_kernel
// (decode.hip) select row b of a sequential step at that position: the same device functions over logits row r (the raw logits are what
// the stage reads for a row that nothing shapes), rs.params[b], the softmax maximum from the partials left for r, and the counter out_lens[b] + j — out_lens as the head of the step saw it: both kernels run before the
// selection stage commits.
// A draft row whose selection is shaped (spec_row_shaped) reads its row of rs.pen instead, as select_thresh_kernel / select_rows_kernel read
// the shaped values of a guided, ruled, n-gram or penalised sampled row: spec_shape_select_kernel left them there, and their maximum in
// the partials of r.
//
// Which slots are shaped in this launch, from the device tables (uniform per workgroup).  rs is the RowSel of the draft rows: a table the
// host's switches (dots_set_speculation_guided / dots_set_speculation_shaped) do not open is a null pointer in it, and a slot that
// carries that feature is SPEC_ROW_NONE then — it has no live draft row.
DEVI bool spec_slot_guided(const SpecState& sp, const RowSel& rs, int b) { return sp.gstate && row_guided(rs, b); }
// is live draft row r of slot b selected from shaped values?  Under a guide only while the chain has a state for it: a dead row verifies nothing
DEVI bool spec_row_shaped(const SpecState& sp, const RowSel& rs, int b, int r) {
    if (spec_slot_guided(sp, rs, b)) return sp.gstate[r] >= 0;
    return row_ruled(rs, b) || row_ngram(rs, b) || row_penalised(rs, b);
}
DEVI const float* spec_draw_row(const SpecState& sp, const RowSel& rs, const float* logits, int ld, int V, int b, int r) {
    return spec_row_shaped(sp, rs, b, r) ? rs.pen + (size_t)r * V : logits + (size_t)r * ld;
}

__global__ __launch_bounds__(SEL_THREADS) void spec_thresh_kernel(const float* __restrict__ logits, int V, int ld, int rows, SpecState sp, RowSel rs,
                                                                  const float* __restrict__ pval, const int32_t* __restrict__ pidx) {
    __shared__ SelLds L;
    const int r = rows + blockIdx.x, j = r / rows, b = r - j * rows;
    if (j > sp.n_live[b] || sp.cls[b] != SPEC_ROW_DRAW) return;      // uniform per workgroup
    const RowParams p = rs.params[b];
    if (!(p.temperature > 0.f)) return;
    if (sel_unfiltered(p)) {
        if (threadIdx.x == 0) rs.thr[r] = SEL_NONE;
        return;
    }
    merge_partials(pval, pidx, r, &L.best, &L.bi);
    sel_threshold(spec_draw_row(sp, rs, logits, ld, V, b, r), V, p, L.best, rs.thr + r, L);
}

__global__ __launch_bounds__(SEL_THREADS) void spec_draw_kernel(const float* __restrict__ logits, int V, int ld, int rows, SpecState sp, RowSel rs,
                                                                const int32_t* __restrict__ out_lens, const float* __restrict__ pval,
                                                                const int32_t* __restrict__ pidx) {
    __shared__ float s_best;
    __shared__ int s_bi;
    __shared__ DrawLds D;
    const int r = rows + blockIdx.x, j = r / rows, b = r - j * rows;
    if (j > sp.n_live[b] || sp.cls[b] != SPEC_ROW_DRAW) return;      // uniform per workgroup
    merge_partials(pval, pidx, r, &s_best, &s_bi);
    const RowParams p = rs.params[b];
    int tok = -1;
    if (p.temperature > 0.f) tok = sel_draw(spec_draw_row(sp, rs, logits, ld, V, b, r), V, p, s_best, rs.thr[r], (uint32_t)(out_lens[b] + j), D);
    if (threadIdx.x == 0) sp.cand[b * DOTS_MAX_SPEC_DRAFTS + j - 1] = tok >= 0 ? tok : s_bi;      // no token: the arg max, as select_rows_kernel
}

// The states of the draft rows of guided slots.  grid (1), one wave: lane b serves slot b.  Draft row (b, j) carries draft j as its input, so
// the token it selects follows drafts 1 .. j: it is selected under rows[b].state — which nothing has moved yet in this step — walked over
// their bytes, a pure function of values known here.  If drafts 1 .. j are accepted that is bitwise the state commit_token will have left
// by then; if they are not, nobody reads the row.  A draft the guide could not have committed at its position — no bytes, an EOS id (it
// finishes the row and is not walked), a byte without a transition — ends the chain: its row and every later one get -1, and so do the
// rows past n_live and the rows of a slot without a guide.
__global__ __launch_bounds__(64) void spec_guide_chain_kernel(SpecState sp, GuideSel g, const int32_t* __restrict__ eos_ids, int n_eos, int rows,
                                                              const RowRules* __restrict__ rules) {
    const int b = threadIdx.x;
    if (b >= rows) return;
    const RowGuide rg = g.rows[b];
    const int nl = rg.table ? sp.n_live[b] : 0;
    const int n_stop = rules && (rules[b].flags & RULE_ON) ? min(rules[b].n_stop, DOTS_MAX_STOP_IDS) : 0;
    uint32_t s = (uint32_t)rg.state;
    bool dead = false;
    for (int j = 1; j <= sp.k; ++j) {
        dead = dead || j > nl;
        if (!dead) {
            const int tok = sp.drafts[b * DOTS_MAX_SPEC_DRAFTS + j - 1];
            dead = tok < 0 || tok >= g.V;
            int i = 0, end = 0;
            if (!dead) { i = g.tok_off[tok]; end = g.tok_off[tok + 1]; }
            dead = dead || i >= end;
            for (int e = 0; e < n_eos; ++e) dead = dead || tok == eos_ids[e];
            for (int e = 0; e < n_stop; ++e) dead = dead || tok == rules[b].stop[e];
            for (; i < end && !dead; ++i) {
                s = rg.table[(size_t)s * 256 + g.tok_bytes[i]];
                dead = s == GUIDE_DEAD;
            }
        }
        sp.gstate[j * rows + b] = dead ? -1 : (int32_t)s;
    }
}

// The arg-max partials of the draft rows whose selection is shaped, and the shaped values of those a sampler will read.  grid (ARGMAX_CHUNKS,
// rows * k) as spec_argmax_kernel, after it: a live row with spec_row_shaped overwrites the raw partials that kernel left for r, every other
// row exits at once.  Draft row r = (b, j) selects the token at output index out_lens[b] + j under the hypothesis that drafts 1 .. j were
// committed; if they were not, nobody reads the row.  Under that hypothesis everything that shapes it is known here, before anything
// commits: the rule image, the stop ids and the prompt-presence bits are the slot's own and do not move; "below min_tokens" is
// out_lens[b] + j < min_tokens; the guide's state is gstate[r] and its bits are row r of guide.mask (the chain and guide_mask_drafts_kernel);
// the n-gram bits are row r of ngram.mask (ngram_ban_drafts_kernel); the output counts are cnt[b] plus the occurrences among drafts
// 1 .. j, which the workgroup holds in LDS — cnt itself moves only in a commit, so a rejected draft leaves nothing behind.  The values
// are shape_logit's (select_dev.h), the function select_partial_kernel (decode.hip) shapes row b with, in the same chunks under the same
// merge rule, so the partials are what the stage would leave for the sequential step at that position.
__global__ __launch_bounds__(256) void spec_shape_select_kernel(const float* __restrict__ logits, int V, int ld, int rows, SpecState sp, RowSel rs,
                                                                StepState st, float* __restrict__ pval, int32_t* __restrict__ pidx) {
    __shared__ float sv[4];
    __shared__ int si[4];
    __shared__ int s_kill[16 + DOTS_MAX_STOP_IDS], s_nkill;
    __shared__ int32_t s_d[DOTS_MAX_SPEC_DRAFTS];
    const int c = blockIdx.x, r = rows + blockIdx.y, j = r / rows, b = r - j * rows;
    if (j > sp.n_live[b] || !spec_row_shaped(sp, rs, b, r)) return;  // uniform per workgroup
    const int per = (V + ARGMAX_CHUNKS - 1) / ARGMAX_CHUNKS;
    const int lo = c * per, hi = min(V, lo + per);
    const bool ruled = row_ruled(rs, b), guided = spec_slot_guided(sp, rs, b), ngram = row_ngram(rs, b), pen_on = row_penalised(rs, b);
    const RowParams p = pen_on ? rs.params[b] : RowParams{0.f, 1.f, 0, 1.f, 0.f, 0.f, 0};
    const int n_stop = ruled ? min(rs.rules[b].n_stop, DOTS_MAX_STOP_IDS) : 0;
    const bool early = ruled && st.out_lens[b] + j < rs.rules[b].min_tokens;
    const bool accepting = guided ? rs.guide.rows[b].accepting[sp.gstate[r]] != 0 : true;
    // the EOS / stop ids that fall into this chunk (-inf below min_tokens, and on a guided row whose state is not accepting), and the
    // drafts before the row (j <= n_live[b] <= DOTS_MAX_SPEC_DRAFTS)
    if (threadIdx.x == 0) s_nkill = 0;
    if ((int)threadIdx.x < j) s_d[threadIdx.x] = sp.drafts[b * DOTS_MAX_SPEC_DRAFTS + threadIdx.x];
    __syncthreads();
    if ((early || guided) && (int)threadIdx.x < min(st.n_eos, 16) + n_stop) {
        const int ne = min(st.n_eos, 16);
        const int id = (int)threadIdx.x < ne ? st.eos_ids[threadIdx.x] : rs.rules[b].stop[threadIdx.x - ne];
        if (id >= lo && id < hi) s_kill[atomicAdd(&s_nkill, 1)] = id;
    }
    __syncthreads();
    const int W = (V + 31) >> 5;
    RowShape sh;
    sh.img = ruled && (rs.rules[b].flags & RULE_IMG) ? rs.rule_img + (size_t)b * V : nullptr;
    sh.gbits = guided ? rs.guide.mask + (size_t)r * rs.guide.words : nullptr;
    sh.nbits = ngram ? rs.ngram.mask + (size_t)r * rs.ngram.words : nullptr;
    sh.cnt = pen_on ? rs.cnt + (size_t)b * V : nullptr;
    sh.seen = pen_on ? rs.seen + (size_t)b * W : nullptr;
    sh.kill = s_kill; sh.n_kill = s_nkill; sh.kill_on = early || !accepting;
    sh.drafts = s_d; sh.n_drafts = j;
    const float* row = logits + (size_t)r * ld;
    float* shaped = sp.cls[b] == SPEC_ROW_DRAW ? rs.pen + (size_t)r * V : nullptr;      // a greedy slot needs the arg max only
    float best = -INFINITY;
    int bi = 0x7fffffff;
    for (int i = lo + threadIdx.x; i < hi; i += 256) {
        const float l = shape_logit(row[i], i, sh, p);
        if (shaped) shaped[i] = l;
        argmax_merge(best, bi, l, i);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) argmax_merge(best, bi, __shfl_xor(best, o, 64), __shfl_xor(bi, o, 64));
    if ((threadIdx.x & 63) == 0) { sv[threadIdx.x >> 6] = best; si[threadIdx.x >> 6] = bi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < 4; ++k) argmax_merge(best, bi, sv[k], si[k]);
        pval[r * ARGMAX_CHUNKS + c] = best;
        pidx[r * ARGMAX_CHUNKS + c] = bi;
    }
}

// grid (rows), one wave.  Row 0's token is committed (the selection stage ran); draft j is right iff it equals the token committed before
// it, and then the candidate of draft row j + 1 — its arg max, or for a SPEC_ROW_DRAW slot the token spec_draw_kernel drew — is the next
// token of the sequential run.
// The commit is commit_row (select_dev.h), the function select_rows_kernel commits row b of a sequential step with, over rs, the RowSel of
// the draft rows: the output count of a penalised slot moves with every token of the walk and with nothing else, the slot's rules decide
// EOS / stop ids, its guide's automaton advances by the bytes of every token, its stop automaton walks them, and EOS, the cap and the hit
// record come out of the same code; any of them finishes the row mid-walk.  A table of rs that is null (the switch that opens it is off, or
// no row holds the feature) is one no speculating slot has an entry in.
// The walk of a guided slot also ends at a draft row the chain marked dead: the draft there is not a token the guide could have
// committed, so if it equals what was committed that was the all -inf fallback (id 0, the state did not move) and nothing past it is verified.
// sp.acc_n / sp.acc_tok (both set or both null): the walk also leaves how many candidates it committed and their ids, per slot.
__global__ __launch_bounds__(64) void spec_accept_kernel(SpecState sp, StepState st, int rows, int V, const float* __restrict__ pval,
                                                         const int32_t* __restrict__ pidx, RowSel rs) {
    __shared__ int32_t s_tok[DOTS_MAX_SPEC_DRAFTS];
    const int b = blockIdx.x, lane = threadIdx.x;
    const int nl = sp.n_live[b];                                      // uniform
    const bool drawn = sp.cand && sp.cls[b] == SPEC_ROW_DRAW;         // uniform
    const bool guided = spec_slot_guided(sp, rs, b);                  // uniform
    const bool pen = row_penalised(rs, b);                      // uniform
    for (int j = 0; j < nl; ++j) {
        if (drawn) {
            if (lane == 0) s_tok[j] = sp.cand[b * DOTS_MAX_SPEC_DRAFTS + j];
            continue;
        }
        const int r = (j + 1) * rows + b;
        float best = pval[r * ARGMAX_CHUNKS + lane];
        int bi = pidx[r * ARGMAX_CHUNKS + lane];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) argmax_merge(best, bi, __shfl_xor(best, o, 64), __shfl_xor(bi, o, 64));
        if (lane == 0) s_tok[j] = bi;
    }
    __syncthreads();
    if (lane != 0) return;
    sp.n_draft[b] = 0;                                                // the drafts are spent, whatever became of them
    if (sp.acc_n) sp.acc_n[b] = 0;
    if (nl < 0) return;
    int acc = 0;
    while (acc < nl && !st.finished[b] && sp.drafts[b * DOTS_MAX_SPEC_DRAFTS + acc] == st.cur_tokens[b]) {
        if (guided && sp.gstate[(acc + 1) * rows + b] < 0) break;
        commit_row(st, rs, b, V, pen, s_tok[acc]);
        if (sp.acc_tok) sp.acc_tok[b * DOTS_MAX_SPEC_DRAFTS + acc] = s_tok[acc];
        ++acc;
    }
    if (sp.acc_n) sp.acc_n[b] = acc;                                  // the accept record: what the walk committed (launch_spec_logprob_final)
    unsigned long long* mine = sp.stats + (size_t)b * 3;
    mine[0] += 1; mine[1] += (unsigned long long)nl; mine[2] += (unsigned long long)acc;
    unsigned long long* all = sp.stats + (size_t)DOTS_MAX_BATCH * 3;
    atomicAdd(all + 0, 1ull); atomicAdd(all + 1, (unsigned long long)nl); atomicAdd(all + 2, (unsigned long long)acc);
}

// The drafting rule (include/dots_ocr_hip.h): for n from max_n down to min_n with n + 1 <= L, key = out[L - n .. L); among the matches
// out[i .. i + n) == key with i + n < L the largest i with i + n + k <= L if there is one, else the smallest i; the draft is
// out[i + n .. min(i + n + k, L)).  The first n with a match wins.
// grid (B), ND_THREADS threads: the threads stride over i, each keeps (largest full, smallest any), one LDS reduction per n.
__global__ __launch_bounds__(ND_THREADS) void ngram_draft_kernel(const int32_t* __restrict__ out_ids, const int32_t* __restrict__ out_lens, int out_stride,
                                                                 const int32_t* __restrict__ finished, const int32_t* __restrict__ sel,
                                                                 const int32_t* __restrict__ cls, int engine_greedy, int k, int min_n, int max_n,
                                                                 int32_t* __restrict__ drafts, int draft_stride, int32_t* __restrict__ n_draft) {
    __shared__ int32_t s_suf[DOTS_MAX_NGRAM_SIZE];
    __shared__ int s_full[ND_THREADS / 64], s_any[ND_THREADS / 64];
    const int b = blockIdx.x, tid = threadIdx.x;
    const bool speculates = engine_greedy && !(cls && cls[b] == SPEC_ROW_NONE);
    if ((sel && !sel[b]) || (finished && finished[b]) || !speculates) {      // uniform per workgroup
        if (tid == 0) n_draft[b] = 0;
        return;
    }
    const int L = min(max(out_lens[b], 0), out_stride);
    const int32_t* __restrict__ out = out_ids + (size_t)b * out_stride;
    const int n_top = min(max_n, L - 1);                              // the longest key with n + 1 <= L
    if (tid < n_top) s_suf[tid] = out[L - n_top + tid];
    __syncthreads();
    for (int n = n_top; n >= min_n; --n) {
        const int32_t* key = s_suf + (n_top - n);
        int full = -1, any = INT_MAX;
        for (int i = tid; i + n < L; i += ND_THREADS) {
            bool hit = true;
            for (int j = n - 1; j >= 0; --j)
                if (out[i + j] != key[j]) { hit = false; break; }
            if (!hit) continue;
            any = min(any, i);
            if (i + n + k <= L) full = max(full, i);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            full = max(full, __shfl_xor(full, o, 64));
            any = min(any, __shfl_xor(any, o, 64));
        }
        if ((tid & 63) == 0) { s_full[tid >> 6] = full; s_any[tid >> 6] = any; }
        __syncthreads();
        for (int w = 0; w < ND_THREADS / 64; ++w) { full = max(full, s_full[w]); any = min(any, s_any[w]); }
        __syncthreads();                                              // the partials are read: the next n may overwrite them
        const int i = full >= 0 ? full : any;                         // uniform from here
        if (i == INT_MAX) continue;
        const int cnt = min(k, L - (i + n));
        if (tid < cnt) drafts[(size_t)b * draft_stride + tid] = out[i + n + tid];
        if (tid == 0) n_draft[b] = cnt;
        return;
    }
    if (tid == 0) n_draft[b] = 0;
}

struct DraftIds { int32_t v[DOTS_MAX_SPEC_DRAFTS]; };
__global__ void spec_set_drafts_kernel(int32_t* drafts, int32_t* n_draft, int row, DraftIds ids, int n) {
    for (int j = 0; j < n; ++j) drafts[row * DOTS_MAX_SPEC_DRAFTS + j] = ids.v[j];
    n_draft[row] = n;
}

__global__ void spec_set_class_kernel(int32_t* cls, int row, int value) { cls[row] = value; }

bool spec_ok(const SpecState& sp, int rows) {
    return sp.drafts && sp.n_draft && sp.n_live && sp.tokens && sp.ctx_len && sp.block_table && sp.stats && sp.cls && sp.k >= 1 && sp.k <= DOTS_MAX_SPEC_DRAFTS &&
           rows >= 1 && rows * (sp.k + 1) <= DOTS_MAX_BATCH;
}

}  // namespace

hipError_t launch_spec_expand(hipStream_t s, const SpecState& sp, const StepState& st, const int32_t* block_table, int max_pages, int rows, int scratch_page) {
    if (!spec_ok(sp, rows) || !block_table || max_pages < 1 || scratch_page < 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(spec_expand_kernel, dim3(rows * (sp.k + 1)), dim3(64), 0, s, sp, st, block_table, max_pages, rows, scratch_page);
    return hipGetLastError();
}

hipError_t launch_spec_argmax(hipStream_t s, const SpecState& sp, const float* logits, int V, int ld, int rows, float* pval, int32_t* pidx) {
    if (!spec_ok(sp, rows) || !logits || !pval || !pidx || V < 1 || ld < V) return hipErrorInvalidValue;
    hipLaunchKernelGGL(spec_argmax_kernel, dim3(ARGMAX_CHUNKS, rows * sp.k), dim3(256), 0, s, logits, V, ld, rows, (const int32_t*)sp.n_live, pval, pidx);
    return hipGetLastError();
}

namespace {
bool spec_shaped_sel(const SpecState& sp, const RowSel& rs) { return sp.gstate || rs.rules || rs.ngram.rows || rs.cnt; }
bool spec_row_sel_ok(const SpecState& sp, const RowSel& rs, int V) {
    if (!spec_shaped_sel(sp, rs)) return true;
    if (!rs.params || !rs.own || !rs.pen) return false;
    if (rs.rules && !rs.rule_img) return false;
    if (rs.cnt && !rs.seen) return false;
    if (rs.ngram.rows && (!rs.ngram.mask || rs.ngram.V != V || rs.ngram.words != ngram_mask_words(V))) return false;
    if (sp.gstate && (!rs.guide.rows || !rs.guide.mask || !rs.guide.tok_off || !rs.guide.tok_bytes || rs.guide.V != V || rs.guide.words != guide_mask_words(V)))
        return false;
    return true;
}
}  // namespace

hipError_t launch_spec_draw(hipStream_t s, const SpecState& sp, const float* logits, int V, int ld, int rows, const RowSel& rs, const int32_t* out_lens,
                            const float* pval, const int32_t* pidx) {
    if (!spec_ok(sp, rows) || !sp.cand || !logits || !rs.params || !rs.thr || !out_lens || !pval || !pidx || V < 1 || ld < V) return hipErrorInvalidValue;
    if (!spec_row_sel_ok(sp, rs, V)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(spec_thresh_kernel, dim3(rows * sp.k), dim3(SEL_THREADS), 0, s, logits, V, ld, rows, sp, rs, pval, pidx);
    hipLaunchKernelGGL(spec_draw_kernel, dim3(rows * sp.k), dim3(SEL_THREADS), 0, s, logits, V, ld, rows, sp, rs, out_lens, pval, pidx);
    return hipGetLastError();
}

namespace {
bool spec_guide_ok(const SpecState& sp, const GuideSel& g, const int32_t* eos_ids, int n_eos) {
    return sp.gstate && g.rows && g.mask && g.tok_off && g.tok_bytes && g.V >= 1 && g.words == guide_mask_words(g.V) && n_eos >= 0 && n_eos <= 16 &&
           (n_eos == 0 || eos_ids);
}
}  // namespace

hipError_t launch_spec_guide_chain(hipStream_t s, const SpecState& sp, const GuideSel& guide, const int32_t* eos_ids, int n_eos, int rows,
                                   const RowRules* rules) {
    // of sp the kernel reads drafts, n_live and k and writes gstate: the single-kernel entry point (ops.hip) fills in no more
    if (!sp.drafts || !sp.n_live || sp.k < 1 || sp.k > DOTS_MAX_SPEC_DRAFTS || rows < 1 || rows * (sp.k + 1) > DOTS_MAX_BATCH ||
        !spec_guide_ok(sp, guide, eos_ids, n_eos))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(spec_guide_chain_kernel, dim3(1), dim3(64), 0, s, sp, guide, eos_ids, n_eos, rows, rules);
    return hipGetLastError();
}

hipError_t launch_spec_shape_select(hipStream_t s, const SpecState& sp, const RowSel& rs, const StepState& st, const float* logits, int V, int ld, int rows,
                                    float* pval, int32_t* pidx) {
    if (!spec_ok(sp, rows) || !spec_shaped_sel(sp, rs) || !spec_row_sel_ok(sp, rs, V) || !logits || !pval || !pidx || V < 1 || ld < V || !st.out_lens ||
        st.n_eos < 0 || st.n_eos > 16 || (st.n_eos && !st.eos_ids))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(spec_shape_select_kernel, dim3(ARGMAX_CHUNKS, rows * sp.k), dim3(256), 0, s, logits, V, ld, rows, sp, rs, st, pval, pidx);
    return hipGetLastError();
}

hipError_t launch_spec_accept(hipStream_t s, const SpecState& sp, const StepState& st, int rows, int V, const float* pval, const int32_t* pidx,
                              const RowSel& rs) {
    if (!spec_ok(sp, rows) || !pval || !pidx || V < 1 || !spec_row_sel_ok(sp, rs, V)) return hipErrorInvalidValue;
    if (rs.stop.rows && (!rs.stop.tok_off || !rs.stop.tok_bytes)) return hipErrorInvalidValue;
    if (rs.guide.rows && (!sp.gstate || !rs.guide.tok_off || !rs.guide.tok_bytes)) return hipErrorInvalidValue;
    if (!sp.acc_n != !sp.acc_tok) return hipErrorInvalidValue;
    hipLaunchKernelGGL(spec_accept_kernel, dim3(rows), dim3(64), 0, s, sp, st, rows, V, pval, pidx, rs);
    return hipGetLastError();
}

hipError_t launch_ngram_draft(hipStream_t s, const int32_t* out_ids, const int32_t* out_lens, int out_stride, const int32_t* finished, const int32_t* sel,
                              const int32_t* cls, int engine_greedy, int B, int k, int min_n, int max_n, int32_t* drafts, int draft_stride,
                              int32_t* n_draft) {
    if (!out_ids || !out_lens || !drafts || !n_draft || out_stride < 1 || B < 1 || B > DOTS_MAX_BATCH || k < 1 || k > DOTS_MAX_SPEC_DRAFTS ||
        draft_stride < k || min_n < 1 || max_n < min_n || max_n > DOTS_MAX_NGRAM_SIZE)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(ngram_draft_kernel, dim3(B), dim3(ND_THREADS), 0, s, out_ids, out_lens, out_stride, finished, sel, cls, engine_greedy, k, min_n, max_n,
                       drafts, draft_stride, n_draft);
    return hipGetLastError();
}

hipError_t launch_spec_set_drafts(hipStream_t s, int32_t* drafts, int32_t* n_draft, int row, const int32_t* ids_host, int n) {
    if (!drafts || !n_draft || row < 0 || row >= DOTS_MAX_BATCH || n < 0 || n > DOTS_MAX_SPEC_DRAFTS || (n && !ids_host)) return hipErrorInvalidValue;
    DraftIds ids{};
    for (int j = 0; j < n; ++j) ids.v[j] = ids_host[j];
    hipLaunchKernelGGL(spec_set_drafts_kernel, dim3(1), dim3(1), 0, s, drafts, n_draft, row, ids, n);
    return hipGetLastError();
}

hipError_t launch_spec_set_class(hipStream_t s, int32_t* cls, int row, int value) {
    if (!cls || row < 0 || row >= DOTS_MAX_BATCH || value < SPEC_ROW_ARGMAX || value > SPEC_ROW_DRAW) return hipErrorInvalidValue;
    hipLaunchKernelGGL(spec_set_class_kernel, dim3(1), dim3(1), 0, s, cls, row, value);
    return hipGetLastError();
}
