// Rows of the dots.ocr engine: everything that decides what a row is selected with — the selection stage of a step, the per-row features
// (own sampling parameters, logit rules, guides, n-gram rules, stop strings), logprobs and speculation classes: their state, their
// validators and their C ABI.
#include "engine.h"

namespace engine {
namespace {
// The speculation class of a row (kernels.h SpecRow), from the host's record alone.  THE place that decides it: the stage
// features and the penalty of the row's parameters through RowStage::speculates, and logprobs (not a stage feature: a row that has them
// on speculates only under dots_set_speculation_logprobs).  The engine-wide
// temperature is not a row's fact: the kernels get it as engine_greedy.
int spec_row_class(const DotsEngine* e, int row) {
    const int mode = e->spec_rows | (e->spec_guided ? SPEC_ROWS_GUIDED : 0) | e->spec_shaped * SPEC_ROWS_NGRAM;      // DOTS_SPEC_SHAPED_* moved up by three bits
    if ((e->row_lp[row] >= 0 && !e->spec_logprobs) || !e->stage.speculates(row, e->row_pen[row], mode)) return SPEC_ROW_NONE;
    if (e->stage.staged(row) && !e->stage.has(row, ROW_PARAMS) && e->row_entry_sampled[row]) return SPEC_ROW_NONE;
    return e->stage.has(row, ROW_PARAMS) && e->row_sampled[row] ? SPEC_ROW_DRAW : SPEC_ROW_ARGMAX;
}

// the row's class to the device in stream order, after anything that may change it (the array exists once speculation was switched on)
int sync_spec_class(DotsEngine* e, int row) {
    if (e->sp_cls) CK(launch_spec_set_class(e->stream, e->sp_cls, row, spec_row_class(e, row)));
    return DOTS_OK;
}

// every row's class from the host's record in one copy (the setting changed, or the array is new); the call waits for it
int upload_spec_classes(DotsEngine* e) {
    if (!e->sp_cls) return DOTS_OK;
    int32_t cls[DOTS_MAX_BATCH];
    for (int b = 0; b < DOTS_MAX_BATCH; ++b) cls[b] = spec_row_class(e, b);
    CK(hipMemcpyAsync(e->sp_cls, cls, sizeof(cls), hipMemcpyHostToDevice, e->stream));
    CK(hipStreamSynchronize(e->stream));
    return DOTS_OK;
}

int ensure_row_table(DotsEngine* e) {
    if (e->d_rowp) return DOTS_OK;
    CK(e->alloc(&e->d_rowp, DOTS_MAX_BATCH));
    CK(e->alloc(&e->d_row_own, DOTS_MAX_BATCH));
    CK(e->alloc(&e->d_row_thr, DOTS_MAX_BATCH));
    return DOTS_OK;
}

int ensure_pen_state(DotsEngine* e) {
    if (e->pen_cnt) return DOTS_OK;
    const size_t rows = e->cfg.max_batch, V = e->cfg.vocab_size;
    CK(e->alloc(&e->pen_cnt, rows * V));
    CK(e->alloc(&e->pen_seen, rows * ((V + 31) / 32)));
    if (!e->pen_logits) CK(e->alloc(&e->pen_logits, rows * V));      // shared with the logit rules
    drop_step_graphs(e);                                   // graphs captured before hold no penalty state
    return DOTS_OK;
}

// table, image, shaped-logit scratch and staging of the logit rules, allocated by the first row that carries rules
int ensure_rules_state(DotsEngine* e) {
    if (e->d_rules) return DOTS_OK;
    // each piece is allocated once: a call that failed half way is resumed by the next one, nothing is allocated twice
    const size_t rows = e->cfg.max_batch, V = e->cfg.vocab_size, n_stage = V + 2 * DOTS_MAX_LOGIT_BIAS;
    if (!e->rule_img) CK(e->alloc(&e->rule_img, rows * V));
    if (!e->pen_logits) CK(e->alloc(&e->pen_logits, rows * V));
    if (!e->rule_stage) CK(e->alloc(&e->rule_stage, n_stage));
    if (!e->rule_stage_host) {
        CK(hipHostMalloc((void**)&e->rule_stage_host, n_stage * 4, hipHostMallocDefault));
        std::memset(e->rule_stage_host, 0, n_stage * 4);
    }
    if (!e->rule_ev) CK(hipEventCreateWithFlags(&e->rule_ev, hipEventDisableTiming));
    CK(e->alloc(&e->d_rules, DOTS_MAX_BATCH));             // zeroed by alloc(): no row carries rules; set last, it is the guard above
    drop_step_graphs(e);                                   // graphs captured before hold no shaped-logit scratch
    return DOTS_OK;
}

// row table and allowed bits of the guides, allocated by the first row that takes one
int ensure_guide_state(DotsEngine* e) {
    if (e->d_guides) return DOTS_OK;
    const size_t rows = e->cfg.max_batch, V = e->cfg.vocab_size;
    if (!e->guide_mask) CK(e->alloc(&e->guide_mask, rows * guide_mask_words((int)V)));
    if (!e->pen_logits) CK(e->alloc(&e->pen_logits, rows * V));       // the shaped logits of a sampled guided row
    CK(e->alloc(&e->d_guides, DOTS_MAX_BATCH));            // zeroed by alloc(): no row holds a guide; set last, it is the guard above
    drop_step_graphs(e);                                   // graphs captured before hold no guide state
    return DOTS_OK;
}

// row table and banned bits of the n-gram rules, allocated by the first row that takes one
int ensure_ngram_state(DotsEngine* e) {
    if (e->d_ngram) return DOTS_OK;
    // each piece is allocated once: a call that failed half way is resumed by the next one
    const size_t rows = e->cfg.max_batch, V = e->cfg.vocab_size;
    if (!e->ngram_mask) CK(e->alloc(&e->ngram_mask, rows * ngram_mask_words((int)V)));
    if (!e->pen_logits) CK(e->alloc(&e->pen_logits, rows * V));       // the shaped logits of a sampled n-gram row
    CK(e->alloc(&e->d_ngram, DOTS_MAX_BATCH));             // zeroed by alloc(): no row carries a rule; set last, it is the guard above
    drop_step_graphs(e);                                   // graphs captured before hold no n-gram state
    return DOTS_OK;
}

// row table of the stop strings, allocated by the first row that takes an automaton
int ensure_stop_state(DotsEngine* e) {
    if (e->d_stop) return DOTS_OK;
    CK(e->alloc(&e->d_stop, DOTS_MAX_BATCH));              // zeroed by alloc(): no row holds an automaton
    drop_step_graphs(e);                                   // graphs captured before hold no stop table
    return DOTS_OK;
}

// row table and run counters of the loop guard, allocated by the first row that takes a rule
int ensure_loop_state(DotsEngine* e) {
    if (e->d_loop) return DOTS_OK;
    if (!e->loop_run) CK(e->alloc(&e->loop_run, (size_t)DOTS_MAX_BATCH * DOTS_MAX_LOOP_PERIOD));
    CK(e->alloc(&e->d_loop, DOTS_MAX_BATCH));              // zeroed by alloc(): no row holds a rule; set last, it is the guard above
    drop_step_graphs(e);                                   // graphs captured before hold no loop table
    return DOTS_OK;
}

// what a row without parameters of its own is selected with once the per-row stage owns it (logit rules): the engine-wide setting as it stands
RowParams engine_row_params(const DotsEngine* e) { return RowParams{e->temperature, e->top_p, 0, 1.f, 0.f, 0.f, e->seed}; }

// row `row`, which has no parameters of its own, takes the engine-wide setting as its stage entry (stream ordered)
int write_engine_entry(DotsEngine* e, int row) {
    CK(launch_set_row_params(e->stream, e->d_rowp, e->d_row_own, row, engine_row_params(e), 1));
    e->row_entry_sampled[row] = e->temperature > 0.f;
    return DOTS_OK;
}

// Row `row` takes feature f: it enters the per-row stage unless another feature holds it there already, with the engine-wide setting as
// its entry and the own flag set (stream ordered).  Own parameters are that entry themselves: their setter has written it.
int enter_row_stage(DotsEngine* e, int row, RowFeature f) {
    RET(ensure_row_table(e));
    if (e->stage.attach(row, f) && f != ROW_PARAMS) RET(write_engine_entry(e, row));
    return sync_spec_class(e, row);
}

// Feature f comes off row `row`: with its last feature the row leaves the stage (entry and own flag zeroed); own parameters taken off a
// row that stays give the entry back to the engine-wide setting (stream ordered)
int leave_row_stage(DotsEngine* e, int row, RowFeature f) {
    if (!e->stage.has(row, f)) return DOTS_OK;
    if (e->stage.detach(row, f)) CK(launch_set_row_params(e->stream, e->d_rowp, e->d_row_own, row, RowParams{}, 0));
    else if (f == ROW_PARAMS) RET(write_engine_entry(e, row));
    return sync_spec_class(e, row);
}

// row `row` holds automaton id (a live one) from the root with no hit (stream ordered)
int assign_row_stop(DotsEngine* e, int row, int id, int min_tokens) {
    RET(ensure_row_table(e));
    RET(ensure_stop_state(e));
    const DotsEngine::Stop& a = e->stops[id];
    CK(launch_set_row_stop(e->stream, e->d_stop, row, RowStop{a.table, a.match_len, a.match_id, a.n_states, 0, min_tokens, -1, 0, 0, -1, 0}));
    return hold_row_stop(e, row, id, min_tokens);
}

// logprob outputs + scratch, allocated by the first row switched on; every output byte starts as 0xFF (NaN / -1)
int ensure_lp_state(DotsEngine* e) {
    if (e->lp_tok) return DOTS_OK;
    const size_t rows = e->cfg.max_batch, pos = (size_t)rows * e->cfg.max_seq_len, K = DOTS_MAX_TOP_LOGPROBS;
    hipStream_t s = e->stream;
    CK(e->alloc(&e->lp_ms, rows * LP_CHUNKS * 2));
    CK(e->alloc(&e->lp_pv, rows * LP_CHUNKS * K));
    CK(e->alloc(&e->lp_pi, rows * LP_CHUNKS * K));
    CK(e->alloc(&e->lp_pos, rows));
    CK(e->alloc(&e->lp_ids, pos * K));
    CK(e->alloc(&e->lp_top, pos * K));
    CK(e->alloc(&e->lp_tok, pos));
    CK(hipMemsetAsync(e->lp_tok, 0xFF, pos * 4, s));
    CK(hipMemsetAsync(e->lp_ids, 0xFF, pos * K * 4, s));
    CK(hipMemsetAsync(e->lp_top, 0xFF, pos * K * 4, s));
    return DOTS_OK;
}
}  // namespace

// the bookkeeping arrays of a slot-mode step, as select_tokens hands them to the selection kernels (the speculative kernels of spec.hip
// read and commit through the same state)
StepState step_state(const DotsEngine* e, int advance, const int32_t* sel) {
    StepState st;
    st.cur_tokens = e->cur_tokens; st.ctx_len = e->ctx_len; st.out_ids = e->out_ids; st.out_lens = e->out_lens; st.finished = e->finished;
    st.eos_ids = e->eos_ids; st.n_eos = e->n_eos; st.advance_ctx = advance;
    st.sel = sel; st.max_len = e->d_max_len; st.out_stride = e->cfg.max_seq_len; st.cap = e->cfg.max_seq_len;
    return st;
}

// does a speculating step draw the draft rows of sampled slots (launch_spec_draw)?  Only while rows with parameters may speculate and at
// least one row holds parameters: with dots_set_speculation_rows at 0 a step launches what it always did
bool spec_draws(const DotsEngine* e) {
    return e->slot_mode && e->spec_k > 0 && (e->spec_rows & SPEC_ROWS_SAMPLED) && e->stage.rows(ROW_PARAMS) > 0;
}

// may some guided row verify drafts in a speculating step (the launches under StepKey::gspec)?  A host count: the switch is on and at least
// one row holds a guide.  With dots_set_speculation_guided off a step launches what it always did
bool spec_guides(const DotsEngine* e) {
    return e->slot_mode && e->spec_k > 0 && e->spec_guided && e->stage.rows(ROW_GUIDE) > 0;
}

// may some row with logprobs on verify drafts in a speculating step (the launches under StepKey::lpspec)?  A host count: the switch is on
// and at least one row has logprobs on.  With dots_set_speculation_logprobs off a step launches what it always did
bool spec_lps(const DotsEngine* e) {
    return e->slot_mode && e->spec_k > 0 && e->spec_logprobs && e->n_lp > 0;
}

// Which shaped rows may verify drafts in a speculating step (StepKey::sspec; the DOTS_SPEC_SHAPED_* bits)?  Host counts: a bit is set while
// dots_set_speculation_shaped has it and at least one row holds the feature — an n-gram rule, logit rules, parameters with a penalty.  0:
// a step launches what it always did, and the draft-row kernels get no table of these features
int spec_shapes(const DotsEngine* e) {
    if (!e->slot_mode || e->spec_k <= 0 || !e->spec_shaped) return 0;
    int on = 0;
    if ((e->spec_shaped & DOTS_SPEC_SHAPED_NGRAM) && e->stage.rows(ROW_NGRAM) > 0) on |= DOTS_SPEC_SHAPED_NGRAM;
    if ((e->spec_shaped & DOTS_SPEC_SHAPED_RULES) && e->stage.rows(ROW_RULES) > 0) on |= DOTS_SPEC_SHAPED_RULES;
    if ((e->spec_shaped & DOTS_SPEC_SHAPED_PENALTY) && e->pen_cnt && e->stage.rows(ROW_PARAMS) > 0)
        for (int b = 0; b < e->cfg.max_batch; ++b)
            if (e->stage.has(b, ROW_PARAMS) && e->row_pen[b]) { on |= DOTS_SPEC_SHAPED_PENALTY; break; }
    return on;
}

// The RowSel of the draft rows of a speculating step (kernels.h): the stage's tables as far as the switches open them
RowSel spec_row_sel(const DotsEngine* e) {
    const int V = e->cfg.vocab_size, on = spec_shapes(e);
    RowSel rs{e->d_rowp, e->d_row_own, nullptr, nullptr, e->pen_logits, e->d_row_thr, e->temperature > 0.f ? 0 : 1, nullptr, nullptr, GuideSel{}, NgramSel{}, StopSel{}};
    if (on & DOTS_SPEC_SHAPED_PENALTY) { rs.cnt = e->pen_cnt; rs.seen = e->pen_seen; }
    if (on & DOTS_SPEC_SHAPED_RULES) { rs.rules = e->d_rules; rs.rule_img = e->rule_img; }
    if (on & DOTS_SPEC_SHAPED_NGRAM) rs.ngram = NgramSel{e->d_ngram, e->ngram_mask, ngram_mask_words(V), V};
    if (spec_guides(e)) rs.guide = guide_sel(e);
    if (e->d_stop) rs.stop = StopSel{e->d_stop, e->tok_off, e->tok_bytes, V, 0};
    rs.loop = loop_sel(e);                                 // a row that holds a rule verifies no draft: the accept walk never asks
    return rs;
}

// does a speculating step run the prediction drafter (StepKey::pred)?  A host count: the built-in drafter runs and at least one slot holds a
// prediction.  While no slot does, a step launches what it always did
bool spec_predicts(const DotsEngine* e) { return e->slot_mode && e->spec_k > 0 && e->spec_max_n > 0 && e->n_pred > 0; }

PredictState predict_state(const DotsEngine* e) {
    return PredictState{e->pr_ids, e->pr_len, e->pr_cur, e->pr_at, e->pr_src, (int32_t)e->cfg.max_seq_len, e->pr_seen, e->pr_stats};
}

SpecState spec_state(const DotsEngine* e) {
    return SpecState{e->sp_drafts, e->sp_ndraft, e->sp_nlive, e->sp_tokens, e->sp_ctx, e->sp_table, e->sp_stats, e->sp_cls,
                     spec_draws(e) ? e->sp_cand : nullptr, spec_guides(e) ? e->sp_gstate : nullptr, e->spec_k, e->temperature > 0.f ? 0 : 1,
                     spec_lps(e) ? e->sp_acc_n : nullptr, spec_lps(e) ? e->sp_acc_tok : nullptr};
}

// the row holds no prediction any more (stream ordered): dots_set_row_prediction with n = 0, dots_slot_release
int clear_row_prediction(DotsEngine* e, int row) {
    if (!e->pr_ids || !e->row_pred[row]) return DOTS_OK;
    CK(launch_predict_set_row(e->stream, predict_state(e), e->sp_ndraft, row, 0));
    e->row_pred[row] = 0;
    e->n_pred -= 1;
    return DOTS_OK;
}

// the loop rows' table and counters, once any row has held a rule (allocating them drops the captured steps, so no cache key changes)
LoopSel loop_sel(const DotsEngine* e) { return LoopSel{e->d_loop, e->d_loop ? e->loop_run : nullptr}; }

// what a launch needs to honour the guides (the row table exists once a row has taken one)
GuideSel guide_sel(const DotsEngine* e) {
    return GuideSel{e->d_guides, e->guide_mask, e->tok_off, e->tok_bytes, guide_mask_words(e->cfg.vocab_size), e->cfg.vocab_size};
}

// The per-row selection stage over `rs`: the n-gram rows' banned bits, the guided rows' allowed bits (neither kernel reads what the other
// writes), then the stage, which reads both.  ban_finished: the finished flags the ban kernel skips rows by (nullptr: it skips none)
hipError_t launch_row_stage(hipStream_t s, const float* logits, int V, int ld, int B, const RowSel& rs, float* am_val, int32_t* am_idx,
                            const StepState& st, const int32_t* ban_finished) {
    hipError_t r = hipSuccess;
    if (rs.ngram.rows) r = launch_ngram_ban(s, rs.ngram, B, st.out_ids, st.out_lens, st.out_stride, ban_finished, st.sel);
    if (r == hipSuccess && rs.guide.rows) r = launch_guide_mask(s, rs.guide, B, st.sel);
    return r == hipSuccess ? launch_select_rows(s, logits, V, ld, B, rs, am_val, am_idx, st) : r;
}

// greedy arg max or temperature / top-p sampling over the fp32 logits of the step
int select_tokens(DotsEngine* e, int advance) {
    const DotsConfig& c = e->cfg;
    StepState st = step_state(e, advance, e->sel_now);
    if (!e->slot_mode) { st.sel = nullptr; st.max_len = nullptr; st.out_stride = e->out_cap; st.cap = e->out_cap; }      // a static batch
    // logprobs: the partial kernel reads the logits and snapshots finished / out_lens before selection commits, the final kernel
    // reads the committed token after it
    const LogprobState ls{e->d_row_lp, st.sel, e->finished, e->out_lens, e->cur_tokens, e->lp_ms, e->lp_pv, e->lp_pi, e->lp_pos,
                          e->lp_tok, e->lp_ids, e->lp_top, c.max_seq_len};
    if (e->n_lp > 0) CK(launch_logprob_partial(e->stream, e->d_logits, c.vocab_size, c.vocab_size, e->B_sel, ls));
    if (e->stage.staged_rows() > 0) {      // per-row stage for the rows with their own parameters (+ the greedy rows that follow the engine)
        RowSel rs{e->d_rowp, e->d_row_own, e->pen_cnt, e->pen_seen, e->pen_logits, e->d_row_thr, e->temperature > 0.f ? 0 : 1,
                  e->stage.rows(ROW_RULES) > 0 ? e->d_rules : nullptr, e->rule_img, GuideSel{}, NgramSel{}, StopSel{}};
        // the stop-string rows' table, once any row has held one (allocating it drops the captured steps, so no cache key changes): the
        // commit of a row that holds an automaton walks it, no launch is added
        if (e->d_stop) rs.stop = StopSel{e->d_stop, e->tok_off, e->tok_bytes, c.vocab_size, 0};
        rs.loop = loop_sel(e);                     // as the stop table: the check runs inside the stage's commit kernel, no launch is added
        if (e->stage.rows(ROW_NGRAM) > 0)          // the n-gram rows' banned bits from their own output so far, before the stage reads the logits
            rs.ngram = NgramSel{e->d_ngram, e->ngram_mask, ngram_mask_words(c.vocab_size), c.vocab_size};
        if (e->stage.rows(ROW_GUIDE) > 0)          // the guided rows' allowed bits from their current states, before the stage reads the logits
            rs.guide = guide_sel(e);
        CK(launch_row_stage(e->stream, e->d_logits, c.vocab_size, c.vocab_size, e->B_sel, rs, e->am_val, e->am_idx, st, st.finished));
        if (e->temperature > 0.f)
            CK(launch_sample_step(e->stream, e->d_logits, c.vocab_size, c.vocab_size, e->B_sel, e->temperature, e->top_p, e->seed, st, e->d_row_own));
    } else if (e->temperature > 0.f)
        CK(launch_sample_step(e->stream, e->d_logits, c.vocab_size, c.vocab_size, e->B_sel, e->temperature, e->top_p, e->seed, st));
    else
        CK(launch_argmax_step(e->stream, e->d_logits, c.vocab_size, c.vocab_size, e->B_sel, e->am_val, e->am_idx, st));
    if (e->n_lp > 0) CK(launch_logprob_final(e->stream, e->d_logits, c.vocab_size, c.vocab_size, e->B_sel, ls));
    return DOTS_OK;
}

// feature f off row `row` (stream ordered): the feature's own table entry and reference count, then the stage
int clear_row_feature(DotsEngine* e, int row, RowFeature f) {
    if (!e->stage.has(row, f)) return DOTS_OK;
    switch (f) {
    case ROW_RULES:
        CK(launch_set_row_rules(e->stream, e->d_rules, e->rule_img, row, e->cfg.vocab_size, RowRules{}, nullptr, 0, nullptr, nullptr, 0));
        break;
    case ROW_GUIDE:
        CK(launch_set_row_guide(e->stream, e->d_guides, row, RowGuide{}));
        e->guides[e->row_guide[row] - 1].rows -= 1;
        e->row_guide[row] = 0;
        break;
    case ROW_NGRAM:
        CK(launch_set_row_ngram(e->stream, e->d_ngram, row, RowNgram{}));
        break;
    case ROW_STOP:
        CK(launch_set_row_stop(e->stream, e->d_stop, row, RowStop{}));
        e->stops[e->row_stop[row] - 1].rows -= 1;
        e->row_stop[row] = e->row_stop_min[row] = 0;
        break;
    case ROW_LOOP:
        CK(launch_set_row_loop(e->stream, e->d_loop, e->loop_run, row, RowLoop{}));
        e->row_loop[row] = DotsLoopRule{};
        break;
    default: break;                                        // own parameters: the stage entry is all there is
    }
    return leave_row_stage(e, row, f);
}

// host side of row `row` taking automaton id (a live one): stage membership, the automata's reference counts and the row's payload.  The
// caller writes the row's table entry (dots_set_row_stop one row, dots_slots_fork all children at once)
int hold_row_stop(DotsEngine* e, int row, int id, int min_tokens) {
    if (e->stage.has(row, ROW_STOP)) e->stops[e->row_stop[row] - 1].rows -= 1;
    RET(enter_row_stage(e, row, ROW_STOP));
    e->row_stop[row] = id + 1;
    e->row_stop_min[row] = min_tokens;
    e->stops[id].rows += 1;
    return DOTS_OK;
}

// host side of row `row` taking loop rule r (a checked one): stage membership and the row's payload.  The caller writes the row's table
// entry (dots_set_row_loop one row, dots_slots_fork all children at once)
int hold_row_loop(DotsEngine* e, int row, const DotsLoopRule& r) {
    RET(enter_row_stage(e, row, ROW_LOOP));
    e->row_loop[row] = r;
    return DOTS_OK;
}

int check_row_params(DotsEngine* e, const DotsSamplingParams& p, RowParams* out) {
    if (!(p.temperature >= 0.f) || !std::isfinite(p.temperature)) return e->fail(DOTS_E_INVALID, "temperature must be finite and >= 0");
    if (!(p.top_p > 0.f)) return e->fail(DOTS_E_INVALID, "top_p must be in (0, 1]");
    if (p.top_k < 0) return e->fail(DOTS_E_INVALID, "top_k must be 0 (off) or >= 1");
    if (!(p.repetition_penalty > 0.f) || !std::isfinite(p.repetition_penalty)) return e->fail(DOTS_E_INVALID, "repetition_penalty must be finite and > 0");
    if (!(p.frequency_penalty >= -2.f && p.frequency_penalty <= 2.f)) return e->fail(DOTS_E_INVALID, "frequency_penalty must be in [-2, 2]");
    if (!(p.presence_penalty >= -2.f && p.presence_penalty <= 2.f)) return e->fail(DOTS_E_INVALID, "presence_penalty must be in [-2, 2]");
    *out = RowParams{p.temperature, p.top_p > 1.f ? 1.f : p.top_p, p.top_k, p.repetition_penalty, p.frequency_penalty, p.presence_penalty, p.seed};
    return DOTS_OK;
}

// Validate one row's logit rules against vocabulary V and the engine's EOS ids -> the device entry.  Refused: a value out of range, a
// duplicate bias id, and rules that could never select a token (an empty allowed list, one that the bans cover, or — with min_tokens > 0 —
// one that the bans, the EOS ids and the stop ids cover together).
int check_logit_rules(DotsEngine* e, const DotsLogitRules& r, int V, const int32_t* eos, int n_eos, RowRules* out) {
    if (r.n_bias < 0 || r.n_bias > DOTS_MAX_LOGIT_BIAS || (r.n_bias && (!r.bias_ids || !r.bias_values)))
        return e->fail(DOTS_E_INVALID, "logit rules: n_bias must be in [0, %d]", DOTS_MAX_LOGIT_BIAS);
    if (r.n_allowed < 0 || r.n_allowed > V || (r.n_allowed && !r.allowed_ids)) return e->fail(DOTS_E_INVALID, "logit rules: n_allowed must be in [0, %d]", V);
    if (r.allowed_ids && r.n_allowed == 0) return e->fail(DOTS_E_INVALID, "logit rules: the allowed list is empty");
    if (r.min_tokens < 0) return e->fail(DOTS_E_INVALID, "logit rules: min_tokens must be >= 0");
    if (r.n_stop < 0 || r.n_stop > DOTS_MAX_STOP_IDS) return e->fail(DOTS_E_INVALID, "logit rules: n_stop must be in [0, %d]", DOTS_MAX_STOP_IDS);
    std::vector<uint8_t> mark(V, 0);                       // 1 = carries a bias, 2 = banned, 4 = allowed, 8 = EOS or stop id
    for (int j = 0; j < r.n_bias; ++j) {
        const int id = r.bias_ids[j];
        const float v = r.bias_values[j];
        if (id < 0 || id >= V) return e->fail(DOTS_E_INVALID, "logit rules: bias id %d outside [0, %d)", id, V);
        if (mark[id] & 1) return e->fail(DOTS_E_INVALID, "logit rules: bias id %d given twice", id);
        if (!(std::isfinite(v) || (std::isinf(v) && v < 0.f))) return e->fail(DOTS_E_INVALID, "logit rules: the bias of id %d must be finite or -inf", id);
        mark[id] |= std::isinf(v) ? 3 : 1;
    }
    for (int j = 0; j < r.n_stop; ++j) {
        if (r.stop_ids[j] < 0 || r.stop_ids[j] >= V) return e->fail(DOTS_E_INVALID, "logit rules: stop id %d outside [0, %d)", r.stop_ids[j], V);
        mark[r.stop_ids[j]] |= 8;
    }
    for (int j = 0; j < n_eos; ++j) if (eos[j] >= 0 && eos[j] < V) mark[eos[j]] |= 8;
    if (r.allowed_ids) {
        int free_now = 0, free_early = 0;                  // allowed ids that are not banned / and neither an EOS nor a stop id
        for (int j = 0; j < r.n_allowed; ++j) {
            const int id = r.allowed_ids[j];
            if (id < 0 || id >= V) return e->fail(DOTS_E_INVALID, "logit rules: allowed id %d outside [0, %d)", id, V);
            if (!(mark[id] & 2)) { free_now += 1; free_early += (mark[id] & 8) ? 0 : 1; }
        }
        if (!free_now) return e->fail(DOTS_E_INVALID, "logit rules: every allowed id is banned by the bias");
        if (r.min_tokens > 0 && !free_early) return e->fail(DOTS_E_INVALID, "logit rules: below min_tokens every allowed id is an EOS or a stop id");
    }
    RowRules rr{};
    rr.flags = RULE_ON | ((r.n_bias || r.allowed_ids) ? RULE_IMG : 0) | (r.ignore_eos ? RULE_IGNORE_EOS : 0);
    rr.min_tokens = r.min_tokens;
    rr.n_stop = r.n_stop;
    std::copy(r.stop_ids, r.stop_ids + r.n_stop, rr.stop);
    *out = rr;
    return DOTS_OK;
}

// Validate one row's n-gram rule against vocabulary V and the longest output max_len -> the device entry
int check_ngram_rule(DotsEngine* e, const DotsNgramRule& r, int V, int max_len, RowNgram* out) {
    if (V > NGRAM_MAX_V) return e->fail(DOTS_E_INVALID, "n-gram rule: the vocabulary %d exceeds the %d ids the ban kernel holds", V, NGRAM_MAX_V);
    if (r.size < 1 || r.size > DOTS_MAX_NGRAM_SIZE) return e->fail(DOTS_E_INVALID, "n-gram rule: size must be in [1, %d], got %d", DOTS_MAX_NGRAM_SIZE, r.size);
    if (r.window != 0 && (r.window < r.size || r.window > max_len))
        return e->fail(DOTS_E_INVALID, "n-gram rule: window must be 0 (the whole output) or in [size = %d, %d], got %d", r.size, max_len, r.window);
    if (r.n_whitelist < 0 || r.n_whitelist > DOTS_MAX_NGRAM_WHITELIST)
        return e->fail(DOTS_E_INVALID, "n-gram rule: n_whitelist must be in [0, %d]", DOTS_MAX_NGRAM_WHITELIST);
    RowNgram rn{};
    rn.n = r.size;
    rn.window = r.window;
    rn.n_white = r.n_whitelist;
    for (int j = 0; j < r.n_whitelist; ++j) {
        const int id = r.whitelist[j];
        if (id < 0 || id >= V) return e->fail(DOTS_E_INVALID, "n-gram rule: whitelist id %d outside [0, %d)", id, V);
        for (int k = 0; k < j; ++k)
            if (r.whitelist[k] == id) return e->fail(DOTS_E_INVALID, "n-gram rule: whitelist id %d given twice", id);
        rn.white[j] = id;
    }
    *out = rn;
    return DOTS_OK;
}

// positions of `row` back to NaN / -1 (at each prefill of the row once the outputs exist)
int clear_lp_row(DotsEngine* e, int row) {
    if (!e->lp_tok) return DOTS_OK;
    const size_t L = e->cfg.max_seq_len, K = DOTS_MAX_TOP_LOGPROBS;
    CK(hipMemsetAsync(e->lp_tok + (size_t)row * L, 0xFF, L * 4, e->stream));
    CK(hipMemsetAsync(e->lp_ids + (size_t)row * L * K, 0xFF, L * K * 4, e->stream));
    CK(hipMemsetAsync(e->lp_top + (size_t)row * L * K, 0xFF, L * K * 4, e->stream));
    return DOTS_OK;
}

// top_n of the row (-1 = off), in stream order; keeps n_lp, the count of rows that are on
int set_row_lp(DotsEngine* e, int row, int top_n) {
    const bool was = e->row_lp[row] >= 0;
    if (!was && top_n < 0) return DOTS_OK;
    CK(launch_set_row_lp(e->stream, e->d_row_lp, row, top_n));
    e->row_lp[row] = top_n;
    e->n_lp += (top_n >= 0 ? 1 : 0) - (was ? 1 : 0);
    return sync_spec_class(e, row);
}
}  // namespace engine

using namespace engine;
extern "C" {
int dots_set_sampling(DotsEngine* e, float temperature, float top_p, uint64_t seed) {
    if (!e) return DOTS_E_INVALID;
    if (!(temperature >= 0.f) || !(top_p > 0.f)) return e->fail(DOTS_E_INVALID, "temperature must be >= 0 and top_p in (0, 1]");
    e->temperature = temperature;
    e->top_p = top_p > 1.f ? 1.f : top_p;
    e->seed = seed;
    drop_step_graphs(e);                                   // the captured decode steps bake these values in
    return DOTS_OK;
}

int dots_set_row_sampling(DotsEngine* e, int row, const DotsSamplingParams* p) {
    if (!e) return DOTS_E_INVALID;
    if (row < 0 || row >= e->cfg.max_batch) return e->fail(DOTS_E_INVALID, "row %d out of range [0, %d)", row, e->cfg.max_batch);
    CK(hipSetDevice(e->device));
    if (!p) return clear_row_feature(e, row, ROW_PARAMS);
    if (beam_row(e, row)) return e->fail(DOTS_E_INVALID, BEAM_ROW_TAKES_NONE, row);
    RowParams rp;
    RET(check_row_params(e, *p, &rp));
    RET(ensure_row_table(e));
    if (rp.repetition_penalty != 1.f || rp.frequency_penalty != 0.f || rp.presence_penalty != 0.f) RET(ensure_pen_state(e));
    CK(launch_set_row_params(e->stream, e->d_rowp, e->d_row_own, row, rp, 1));
    e->row_pen[row] = rp.repetition_penalty != 1.f || rp.frequency_penalty != 0.f || rp.presence_penalty != 0.f;
    e->row_sampled[row] = rp.temperature > 0.f;
    return enter_row_stage(e, row, ROW_PARAMS);
}

int dots_set_row_logit_rules(DotsEngine* e, int row, const DotsLogitRules* r) {
    if (!e) return DOTS_E_INVALID;
    if (row < 0 || row >= e->cfg.max_batch) return e->fail(DOTS_E_INVALID, "row %d out of range [0, %d)", row, e->cfg.max_batch);
    CK(hipSetDevice(e->device));
    if (!r) return clear_row_feature(e, row, ROW_RULES);
    if (beam_row(e, row)) return e->fail(DOTS_E_INVALID, BEAM_ROW_TAKES_NONE, row);
    RowRules rr;
    RET(check_logit_rules(e, *r, e->cfg.vocab_size, e->h_eos, e->n_eos, &rr));
    RET(ensure_row_table(e));
    RET(ensure_rules_state(e));
    const int V = e->cfg.vocab_size, n_allowed = r->allowed_ids ? r->n_allowed : 0;
    if (rr.flags & RULE_IMG) {
        CK(hipEventSynchronize(e->rule_ev));               // the previous call's upload has left the pinned buffer (an unrecorded event: at once)
        int32_t* h = e->rule_stage_host;
        if (n_allowed) std::copy(r->allowed_ids, r->allowed_ids + n_allowed, h);
        if (r->n_bias) {
            std::copy(r->bias_ids, r->bias_ids + r->n_bias, h + V);
            std::memcpy(h + V + DOTS_MAX_LOGIT_BIAS, r->bias_values, (size_t)r->n_bias * 4);
        }
        if (n_allowed) CK(hipMemcpyAsync(e->rule_stage, h, (size_t)n_allowed * 4, hipMemcpyHostToDevice, e->stream));
        // ids and values in one copy: the whole [2][DOTS_MAX_LOGIT_BIAS] block, of which the kernel reads the first n_bias of each half
        if (r->n_bias) CK(hipMemcpyAsync(e->rule_stage + V, h + V, (size_t)2 * DOTS_MAX_LOGIT_BIAS * 4, hipMemcpyHostToDevice, e->stream));
        CK(hipEventRecord(e->rule_ev, e->stream));
    }
    CK(launch_set_row_rules(e->stream, e->d_rules, e->rule_img, row, V, rr, e->rule_stage, n_allowed, e->rule_stage + V,
                            reinterpret_cast<const float*>(e->rule_stage + V + DOTS_MAX_LOGIT_BIAS), r->n_bias));
    // not enter_row_stage(): the entry is rewritten whenever the row has no parameters of its own, staged already or not (known wart)
    if (!e->stage.has(row, ROW_PARAMS)) RET(write_engine_entry(e, row));
    e->stage.attach(row, ROW_RULES);
    return sync_spec_class(e, row);
}

int dots_set_token_bytes(DotsEngine* e, const int32_t* offsets, const uint8_t* bytes) {
    if (!e || !offsets) return e ? e->fail(DOTS_E_INVALID, "null argument") : DOTS_E_INVALID;
    const int V = e->cfg.vocab_size;
    if (offsets[0] != 0) return e->fail(DOTS_E_INVALID, "token bytes: offsets[0] must be 0");
    for (int t = 0; t < V; ++t)
        if (offsets[t + 1] < offsets[t]) return e->fail(DOTS_E_INVALID, "token bytes: offsets must not decrease (token %d)", t);
    const size_t n = (size_t)offsets[V];
    if (n && !bytes) return e->fail(DOTS_E_INVALID, "null argument");
    if (e->stage.rows(ROW_GUIDE) > 0) return e->fail(DOTS_E_STATE, "token bytes cannot change while %d row(s) hold a guide", e->stage.rows(ROW_GUIDE));
    if (e->stage.rows(ROW_STOP) > 0) return e->fail(DOTS_E_STATE, "token bytes cannot change while %d row(s) hold stop strings", e->stage.rows(ROW_STOP));
    CK(hipSetDevice(e->device));
    CK(hipStreamSynchronize(e->stream));                   // nothing in flight reads the previous image
    if (e->tok_off) { e->release(e->tok_off); e->tok_off = nullptr; }
    if (e->tok_bytes) { e->release(e->tok_bytes); e->tok_bytes = nullptr; }
    CK(e->alloc(&e->tok_bytes, n + 16));
    if (n) CK(hipMemcpyAsync(e->tok_bytes, bytes, n, hipMemcpyHostToDevice, e->stream));
    int32_t* off = nullptr;
    CK(e->alloc(&off, (size_t)V + 1));
    CK(hipMemcpyAsync(off, offsets, ((size_t)V + 1) * 4, hipMemcpyHostToDevice, e->stream));
    CK(hipStreamSynchronize(e->stream));                   // the caller's arrays are free again
    e->tok_off = off;
    drop_step_graphs(e);                                   // a captured step holds the previous pointers
    return DOTS_OK;
}

int dots_guide_create(DotsEngine* e, const uint16_t* table, int n_states, const uint8_t* accepting, int start, int32_t* id_out) {
    if (!e || !table || !accepting || !id_out) return e ? e->fail(DOTS_E_INVALID, "null argument") : DOTS_E_INVALID;
    if (n_states < 1 || n_states > DOTS_MAX_GUIDE_STATES) return e->fail(DOTS_E_INVALID, "guide: n_states must be in [1, %d]", DOTS_MAX_GUIDE_STATES);
    if (start < 0 || start >= n_states) return e->fail(DOTS_E_INVALID, "guide: start state %d outside [0, %d)", start, n_states);
    for (size_t i = 0; i < (size_t)n_states * 256; ++i)
        if (table[i] != GUIDE_DEAD && table[i] >= n_states)
            return e->fail(DOTS_E_INVALID, "guide: state %zu, byte %zu leads to state %d outside [0, %d)", i / 256, i % 256, (int)table[i], n_states);
    CK(hipSetDevice(e->device));
    DotsEngine::Guide g;
    g.n_states = n_states;
    g.start = start;
    CK(e->alloc(&g.table, (size_t)n_states * 256));
    CK(hipMemcpyAsync(g.table, table, (size_t)n_states * 512, hipMemcpyHostToDevice, e->stream));
    CK(e->alloc(&g.accepting, (size_t)n_states));
    CK(hipMemcpyAsync(g.accepting, accepting, (size_t)n_states, hipMemcpyHostToDevice, e->stream));
    CK(hipStreamSynchronize(e->stream));                   // the caller's arrays are free again
    size_t id = 0;
    while (id < e->guides.size() && e->guides[id].table) ++id;          // a destroyed guide's id is reused
    if (id == e->guides.size()) e->guides.push_back(g); else e->guides[id] = g;
    *id_out = (int32_t)id;
    return DOTS_OK;
}

int dots_guide_destroy(DotsEngine* e, int32_t id) {
    if (!e) return DOTS_E_INVALID;
    if (id < 0 || id >= (int)e->guides.size() || !e->guides[id].table) return e->fail(DOTS_E_INVALID, "no guide %d", id);
    if (e->guides[id].rows > 0) return e->fail(DOTS_E_STATE, "guide %d is held by %d row(s): clear them first (dots_set_row_guide(row, -1))", id, e->guides[id].rows);
    CK(hipSetDevice(e->device));
    CK(hipStreamSynchronize(e->stream));                   // steps in flight may still walk its table
    e->release(e->guides[id].table);
    e->release(e->guides[id].accepting);
    e->guides[id] = DotsEngine::Guide{};
    return DOTS_OK;
}

int dots_set_row_guide(DotsEngine* e, int row, int32_t id) {
    if (!e) return DOTS_E_INVALID;
    if (row < 0 || row >= e->cfg.max_batch) return e->fail(DOTS_E_INVALID, "row %d out of range [0, %d)", row, e->cfg.max_batch);
    CK(hipSetDevice(e->device));
    if (id < 0) return clear_row_feature(e, row, ROW_GUIDE);
    if (beam_row(e, row)) return e->fail(DOTS_E_INVALID, BEAM_ROW_TAKES_NONE, row);
    if (id >= (int)e->guides.size() || !e->guides[id].table) return e->fail(DOTS_E_INVALID, "no guide %d", id);
    if (!e->tok_off) return e->fail(DOTS_E_STATE, "the token bytes are not set (dots_set_token_bytes): a guide cannot judge any token");
    RET(ensure_row_table(e));
    RET(ensure_guide_state(e));
    const DotsEngine::Guide& g = e->guides[id];
    CK(launch_set_row_guide(e->stream, e->d_guides, row, RowGuide{g.table, g.accepting, g.n_states, g.start, g.start, 0}));
    if (e->stage.has(row, ROW_GUIDE)) e->guides[e->row_guide[row] - 1].rows -= 1;
    RET(enter_row_stage(e, row, ROW_GUIDE));
    e->row_guide[row] = id + 1;
    e->guides[id].rows += 1;
    return DOTS_OK;
}

int dots_set_row_ngram(DotsEngine* e, int row, const DotsNgramRule* r) {
    if (!e) return DOTS_E_INVALID;
    if (row < 0 || row >= e->cfg.max_batch) return e->fail(DOTS_E_INVALID, "row %d out of range [0, %d)", row, e->cfg.max_batch);
    CK(hipSetDevice(e->device));
    if (!r) return clear_row_feature(e, row, ROW_NGRAM);
    if (beam_row(e, row)) return e->fail(DOTS_E_INVALID, BEAM_ROW_TAKES_NONE, row);
    RowNgram rn;
    RET(check_ngram_rule(e, *r, e->cfg.vocab_size, e->cfg.max_seq_len, &rn));
    RET(ensure_row_table(e));
    RET(ensure_ngram_state(e));
    CK(launch_set_row_ngram(e->stream, e->d_ngram, row, rn));
    return enter_row_stage(e, row, ROW_NGRAM);
}

// ---------------------------------------------------------------------------------- stop strings
int dots_stop_create(DotsEngine* e, const uint16_t* table, int n_states, const uint16_t* match_len, const uint8_t* match_id, int32_t* handle_out) {
    if (!e || !table || !match_len || !match_id || !handle_out) return e ? e->fail(DOTS_E_INVALID, "null argument") : DOTS_E_INVALID;
    if (!e->tok_off) return e->fail(DOTS_E_STATE, "the token bytes are not set (dots_set_token_bytes): a stop string cannot be matched");
    if (n_states < 1 || n_states > STOP_MAX_STATES) return e->fail(DOTS_E_INVALID, "stop strings: n_states must be in [1, %d]", STOP_MAX_STATES);
    for (size_t i = 0; i < (size_t)n_states * 256; ++i)
        if (table[i] >= n_states)
            return e->fail(DOTS_E_INVALID, "stop strings: state %zu, byte %zu leads to state %d outside [0, %d)", i / 256, i % 256, (int)table[i], n_states);
    for (int i = 0; i < n_states; ++i)
        if (match_len[i] > DOTS_MAX_STOP_BYTES || (match_len[i] && match_id[i] >= DOTS_MAX_STOP_STRINGS))
            return e->fail(DOTS_E_INVALID, "stop strings: state %d matches %d bytes of string %d (at most %d bytes, %d strings)", i, (int)match_len[i],
                           (int)match_id[i], DOTS_MAX_STOP_BYTES, DOTS_MAX_STOP_STRINGS);
    if (match_len[0]) return e->fail(DOTS_E_INVALID, "stop strings: the root state cannot end a string");
    CK(hipSetDevice(e->device));
    DotsEngine::Stop a;
    a.n_states = n_states;
    CK(e->alloc(&a.table, (size_t)n_states * 256));
    CK(hipMemcpyAsync(a.table, table, (size_t)n_states * 512, hipMemcpyHostToDevice, e->stream));
    CK(e->alloc(&a.match_len, (size_t)n_states));
    CK(hipMemcpyAsync(a.match_len, match_len, (size_t)n_states * 2, hipMemcpyHostToDevice, e->stream));
    CK(e->alloc(&a.match_id, (size_t)n_states));
    CK(hipMemcpyAsync(a.match_id, match_id, (size_t)n_states, hipMemcpyHostToDevice, e->stream));
    CK(hipStreamSynchronize(e->stream));                   // the caller's arrays are free again
    size_t id = 0;
    while (id < e->stops.size() && e->stops[id].table) ++id;            // a destroyed automaton's id is reused
    if (id == e->stops.size()) e->stops.push_back(a); else e->stops[id] = a;
    *handle_out = (int32_t)id + 1;
    return DOTS_OK;
}

int dots_stop_destroy(DotsEngine* e, int32_t handle) {
    if (!e) return DOTS_E_INVALID;
    if (!e->tok_off) return e->fail(DOTS_E_STATE, "the token bytes are not set (dots_set_token_bytes): no stop automaton exists");
    const int id = handle - 1;
    if (id < 0 || id >= (int)e->stops.size() || !e->stops[id].table) return e->fail(DOTS_E_INVALID, "no stop automaton %d", handle);
    if (e->stops[id].rows > 0)
        return e->fail(DOTS_E_STATE, "stop automaton %d is held by %d row(s): clear them first (dots_set_row_stop(row, 0, 0))", handle, e->stops[id].rows);
    CK(hipSetDevice(e->device));
    CK(hipStreamSynchronize(e->stream));                   // steps in flight may still walk its table
    e->release(e->stops[id].table);
    e->release(e->stops[id].match_len);
    e->release(e->stops[id].match_id);
    e->stops[id] = DotsEngine::Stop{};
    return DOTS_OK;
}

int dots_set_row_stop(DotsEngine* e, int row, int32_t handle, int min_tokens) {
    if (!e) return DOTS_E_INVALID;
    if (!e->tok_off) return e->fail(DOTS_E_STATE, "the token bytes are not set (dots_set_token_bytes): a stop string cannot be matched");
    if (row < 0 || row >= e->cfg.max_batch) return e->fail(DOTS_E_INVALID, "row %d out of range [0, %d)", row, e->cfg.max_batch);
    CK(hipSetDevice(e->device));
    if (handle == 0) return clear_row_feature(e, row, ROW_STOP);
    if (beam_row(e, row)) return e->fail(DOTS_E_INVALID, BEAM_ROW_TAKES_NONE, row);
    const int id = handle - 1;
    if (id < 0 || id >= (int)e->stops.size() || !e->stops[id].table) return e->fail(DOTS_E_INVALID, "no stop automaton %d", handle);
    if (min_tokens < 0) return e->fail(DOTS_E_INVALID, "stop strings: min_tokens must be >= 0");
    return assign_row_stop(e, row, id, min_tokens);
}

int dots_row_stop_hit(DotsEngine* e, int row, int32_t* out) {
    if (!e || !out) return e ? e->fail(DOTS_E_INVALID, "null argument") : DOTS_E_INVALID;
    if (!e->tok_off) return e->fail(DOTS_E_STATE, "the token bytes are not set (dots_set_token_bytes): no row holds stop strings");
    if (row < 0 || row >= e->cfg.max_batch) return e->fail(DOTS_E_INVALID, "row %d out of range [0, %d)", row, e->cfg.max_batch);
    out[0] = -1; out[1] = 0; out[2] = 0; out[3] = -1;
    if (!e->stage.has(row, ROW_STOP)) return DOTS_OK;
    CK(hipSetDevice(e->device));
    RowStop rs;
    CK(hipMemcpyAsync(&rs, e->d_stop + row, sizeof(rs), hipMemcpyDeviceToHost, e->stream));
    CK(hipStreamSynchronize(e->stream));
    if (rs.hit_tok >= 0) { out[0] = rs.hit_tok; out[1] = rs.hit_bytes; out[2] = rs.hit_len; out[3] = rs.hit_id; }
    return DOTS_OK;
}

// ---------------------------------------------------------------------------------- loop guard
static int check_loop_rule(DotsEngine* e, const DotsLoopRule& r) {
    if (r.min_period < 1 || r.max_period < r.min_period || r.max_period > DOTS_MAX_LOOP_PERIOD)
        return e->fail(DOTS_E_INVALID, "loop guard: periods must satisfy 1 <= min_period <= max_period <= %d, got %d .. %d", DOTS_MAX_LOOP_PERIOD, r.min_period, r.max_period);
    if (r.repeats < 2 || r.repeats > 64) return e->fail(DOTS_E_INVALID, "loop guard: repeats must be in [2, 64], got %d", r.repeats);
    if (r.min_span < 0 || r.min_span > 65535) return e->fail(DOTS_E_INVALID, "loop guard: min_span must be in [0, 65535], got %d", r.min_span);
    return DOTS_OK;
}

int dots_set_row_loop(DotsEngine* e, int row, const DotsLoopRule* r) {
    if (!e) return DOTS_E_INVALID;
    if (row < 0 || row >= e->cfg.max_batch) return e->fail(DOTS_E_INVALID, "row %d out of range [0, %d)", row, e->cfg.max_batch);
    CK(hipSetDevice(e->device));
    if (!r) return clear_row_feature(e, row, ROW_LOOP);
    if (beam_row(e, row)) return e->fail(DOTS_E_INVALID, BEAM_ROW_TAKES_NONE, row);
    RET(check_loop_rule(e, *r));
    RET(ensure_row_table(e));
    RET(ensure_loop_state(e));
    CK(launch_set_row_loop(e->stream, e->d_loop, e->loop_run, row, RowLoop{r->min_period, r->max_period, r->repeats, r->min_span, -1, 0, 0, 0}));
    return hold_row_loop(e, row, *r);
}

int dots_row_loop_hit(DotsEngine* e, int row, int32_t* out) {
    if (!e || !out) return e ? e->fail(DOTS_E_INVALID, "null argument") : DOTS_E_INVALID;
    if (row < 0 || row >= e->cfg.max_batch) return e->fail(DOTS_E_INVALID, "row %d out of range [0, %d)", row, e->cfg.max_batch);
    out[0] = -1; out[1] = 0; out[2] = 0;
    if (!e->stage.has(row, ROW_LOOP)) return DOTS_OK;
    CK(hipSetDevice(e->device));
    RowLoop rl;
    CK(hipMemcpyAsync(&rl, e->d_loop + row, sizeof(rl), hipMemcpyDeviceToHost, e->stream));
    CK(hipStreamSynchronize(e->stream));
    if (rl.hit_tok >= 0) { out[0] = rl.hit_tok; out[1] = rl.period; out[2] = rl.span; }
    return DOTS_OK;
}

int dots_loop_probe(DotsEngine* e, const int32_t* ids, const int32_t* lens, int cases, int stride, const DotsLoopRule* rule, int32_t* hits_out) {
    if (!e || !ids || !lens || !rule || !hits_out) return e ? e->fail(DOTS_E_INVALID, "null argument") : DOTS_E_INVALID;
    if (cases < 1 || cases > 65535 || stride < 1 || (int64_t)cases * stride > (int64_t)1 << 28)
        return e->fail(DOTS_E_INVALID, "loop probe: cases must be in [1, 65535], stride >= 1 and cases x stride <= 2^28");
    for (int c = 0; c < cases; ++c)
        if (lens[c] < 0 || lens[c] > stride) return e->fail(DOTS_E_INVALID, "loop probe: case %d holds %d ids, the stride is %d", c, lens[c], stride);
    RET(check_loop_rule(e, *rule));
    CK(hipSetDevice(e->device));
    Scratch sc(e);
    int32_t *d_ids = nullptr, *d_lens = nullptr, *d_hits = nullptr;
    CK(sc.get(&d_ids, (size_t)cases * stride));
    CK(sc.get(&d_lens, (size_t)cases));
    CK(sc.get(&d_hits, (size_t)cases * 3));
    CK(hipMemcpyAsync(d_ids, ids, (size_t)cases * stride * 4, hipMemcpyHostToDevice, e->stream));
    CK(hipMemcpyAsync(d_lens, lens, (size_t)cases * 4, hipMemcpyHostToDevice, e->stream));
    CK(launch_loop_probe(e->stream, d_ids, d_lens, cases, stride, RowLoop{rule->min_period, rule->max_period, rule->repeats, rule->min_span, -1, 0, 0, 0}, d_hits));
    CK(hipMemcpyAsync(hits_out, d_hits, (size_t)cases * 12, hipMemcpyDeviceToHost, e->stream));
    CK(hipStreamSynchronize(e->stream));
    return DOTS_OK;
}

// ---------------------------------------------------------------------------------- n-gram speculative decoding
int dots_set_speculation(DotsEngine* e, int k, int min_n, int max_n) {
    if (!e) return DOTS_E_INVALID;
    if (k < 0 || k > DOTS_MAX_SPEC_DRAFTS) return e->fail(DOTS_E_INVALID, "k must be in [0, %d], got %d", DOTS_MAX_SPEC_DRAFTS, k);
    if (k > 0 && max_n != 0 && (min_n < 1 || max_n < min_n || max_n > DOTS_MAX_NGRAM_SIZE))
        return e->fail(DOTS_E_INVALID, "n-gram sizes must satisfy 1 <= min_n <= max_n <= %d (max_n = 0: host drafts only), got %d .. %d", DOTS_MAX_NGRAM_SIZE, min_n, max_n);
    if (k > 0 && e->cfg.max_batch / (k + 1) < 1)
        return e->fail(DOTS_E_CAPACITY, "%d drafts need %d rows per slot, max_batch is %d", k, k + 1, e->cfg.max_batch);
    if (e->slot_mode)
        for (int b = 0; b < e->cfg.max_batch; ++b)
            if (e->slot_active[b] || slot_filling(e, b)) return e->fail(DOTS_E_STATE, "speculation cannot change while slot %d is occupied or filling", b);
    if (k > 0 && e->pc) return e->fail(DOTS_E_STATE, "the engine cannot speculate while the prefix cache is on (dots_prefix_cache_enable)");
    CK(hipSetDevice(e->device));
    hipStream_t s = e->stream;
    if (k > 0 && !e->sp_stats) {
        // each piece is allocated once: a call that failed half way is resumed by the next one
        if (!e->sp_drafts) CK(e->alloc(&e->sp_drafts, (size_t)DOTS_MAX_BATCH * DOTS_MAX_SPEC_DRAFTS));
        if (!e->sp_ndraft) CK(e->alloc(&e->sp_ndraft, (size_t)DOTS_MAX_BATCH));
        if (!e->sp_nlive) CK(e->alloc(&e->sp_nlive, (size_t)DOTS_MAX_BATCH));
        if (!e->sp_tokens) CK(e->alloc(&e->sp_tokens, (size_t)DOTS_MAX_BATCH));
        if (!e->sp_ctx) CK(e->alloc(&e->sp_ctx, (size_t)DOTS_MAX_BATCH));
        if (!e->sp_table) {
            CK(e->alloc(&e->sp_table, (size_t)DOTS_MAX_BATCH * e->max_pages));
            const std::vector<int32_t> idle((size_t)DOTS_MAX_BATCH * e->max_pages, e->n_pool_pages);      // every row on the scratch page
            CK(hipMemcpyAsync(e->sp_table, idle.data(), idle.size() * 4, hipMemcpyHostToDevice, s));
            CK(hipStreamSynchronize(s));
        }
        if (!e->sp_cand) CK(e->alloc(&e->sp_cand, (size_t)DOTS_MAX_BATCH * DOTS_MAX_SPEC_DRAFTS));
        if (!e->sp_cls) CK(e->alloc(&e->sp_cls, (size_t)DOTS_MAX_BATCH));
        CK(e->alloc(&e->sp_stats, (size_t)(DOTS_MAX_BATCH + 1) * 3));      // set last, it is the guard above
        RET(upload_spec_classes(e));                                       // rows may have taken features before the array existed
    }
    if (e->sp_stats) {
        CK(hipMemsetAsync(e->sp_stats, 0, (size_t)(DOTS_MAX_BATCH + 1) * 3 * sizeof(unsigned long long), s));
        CK(hipMemsetAsync(e->sp_ndraft, 0, DOTS_MAX_BATCH * 4, s));
        CK(hipStreamSynchronize(s));
    }
    drop_step_graphs(e);                                     // a captured step bakes in the draft count and the drafter's sizes
    e->spec_k = k;
    e->spec_min_n = k > 0 && max_n > 0 ? min_n : 0;
    e->spec_max_n = k > 0 ? max_n : 0;
    return DOTS_OK;
}

int dots_set_speculation_rows(DotsEngine* e, int flags) {
    if (!e) return DOTS_E_INVALID;
    if (flags & ~SPEC_ROWS_ALL) return e->fail(DOTS_E_INVALID, "unknown speculation row flags 0x%x (DOTS_SPEC_ROWS_SAMPLED | DOTS_SPEC_ROWS_STOP)", flags);
    if (e->slot_mode)
        for (int b = 0; b < e->cfg.max_batch; ++b)
            if (e->slot_active[b]) return e->fail(DOTS_E_STATE, "the speculating rows cannot change while slot %d is occupied", b);
    CK(hipSetDevice(e->device));
    e->spec_rows = flags;
    drop_step_graphs(e);                                     // a captured step bakes in whether it draws the draft rows of sampled slots
    return upload_spec_classes(e);                           // free slots may hold features: every row's class under the new setting
}

int dots_set_speculation_guided(DotsEngine* e, int on) {
    if (!e) return DOTS_E_INVALID;
    if (e->slot_mode)
        for (int b = 0; b < e->cfg.max_batch; ++b)
            if (e->slot_active[b]) return e->fail(DOTS_E_STATE, "guided speculation cannot change while slot %d is occupied", b);
    CK(hipSetDevice(e->device));
    if (on && !e->sp_gstate) CK(e->alloc(&e->sp_gstate, (size_t)DOTS_MAX_BATCH));
    if ((on != 0) == (e->spec_guided != 0)) return DOTS_OK;
    e->spec_guided = on != 0;
    drop_step_graphs(e);                                     // a captured step bakes in whether it selects the draft rows of guided slots
    return upload_spec_classes(e);                           // free slots may hold guides: every row's class under the new setting
}

int dots_set_speculation_shaped(DotsEngine* e, int flags) {
    if (!e) return DOTS_E_INVALID;
    if (flags & ~(DOTS_SPEC_SHAPED_NGRAM | DOTS_SPEC_SHAPED_RULES | DOTS_SPEC_SHAPED_PENALTY))
        return e->fail(DOTS_E_INVALID, "unknown shaped speculation flags 0x%x (DOTS_SPEC_SHAPED_NGRAM | DOTS_SPEC_SHAPED_RULES | DOTS_SPEC_SHAPED_PENALTY)", flags);
    if (e->slot_mode)
        for (int b = 0; b < e->cfg.max_batch; ++b)
            if (e->slot_active[b]) return e->fail(DOTS_E_STATE, "shaped speculation cannot change while slot %d is occupied", b);
    if (flags == e->spec_shaped) return DOTS_OK;
    CK(hipSetDevice(e->device));
    e->spec_shaped = flags;
    drop_step_graphs(e);                                     // a captured step bakes in whether it shapes the draft rows of such slots
    return upload_spec_classes(e);                           // free slots may hold features: every row's class under the new setting
}

int dots_set_speculation_logprobs(DotsEngine* e, int on) {
    if (!e) return DOTS_E_INVALID;
    if (e->slot_mode)
        for (int b = 0; b < e->cfg.max_batch; ++b)
            if (e->slot_active[b]) return e->fail(DOTS_E_STATE, "logprob speculation cannot change while slot %d is occupied", b);
    CK(hipSetDevice(e->device));
    if (on && !e->sp_acc_tok) {
        // each piece is allocated once: a call that failed half way is resumed by the next one
        if (!e->sp_acc_n) CK(e->alloc(&e->sp_acc_n, (size_t)DOTS_MAX_BATCH));
        CK(e->alloc(&e->sp_acc_tok, (size_t)DOTS_MAX_BATCH * DOTS_MAX_SPEC_DRAFTS));      // set last, it is the guard above
    }
    if ((on != 0) == (e->spec_logprobs != 0)) return DOTS_OK;
    e->spec_logprobs = on != 0;
    drop_step_graphs(e);                                     // a captured step bakes in whether it reduces the draft rows of logprob slots
    return upload_spec_classes(e);                           // free slots may have logprobs on: every row's class under the new setting
}

int dots_set_row_drafts(DotsEngine* e, int row, const int32_t* ids_host, int n) {
    if (!e) return DOTS_E_INVALID;
    if (row < 0 || row >= e->cfg.max_batch) return e->fail(DOTS_E_INVALID, "row %d out of range [0, %d)", row, e->cfg.max_batch);
    if (n < 0 || n > e->spec_k) return e->fail(DOTS_E_INVALID, "%d drafts given, the engine speculates %d per step (dots_set_speculation)", n, e->spec_k);
    if (n > 0 && !ids_host) return e->fail(DOTS_E_INVALID, "null argument");
    for (int j = 0; j < n; ++j)
        if (ids_host[j] < 0 || ids_host[j] >= e->cfg.vocab_size) return e->fail(DOTS_E_INVALID, "draft id %d out of range [0, %d)", ids_host[j], e->cfg.vocab_size);
    if (!slot_occupied(e, row)) return e->fail(DOTS_E_STATE, "slot %d is not occupied", row);
    if (!e->spec_k) return DOTS_OK;                          // n == 0 with speculation off: nothing to clear
    CK(hipSetDevice(e->device));
    CK(launch_spec_set_drafts(e->stream, e->sp_drafts, e->sp_ndraft, row, ids_host, n));
    if (e->pr_src) CK(hipMemsetAsync(e->pr_src + row, 0, 4, e->stream));      // the host's drafts, not the prediction's
    return DOTS_OK;
}

int dots_spec_stats(DotsEngine* e, int row, int64_t* steps, int64_t* drafted, int64_t* accepted) {
    if (!e || !steps || !drafted || !accepted) return e ? e->fail(DOTS_E_INVALID, "null argument") : DOTS_E_INVALID;
    if (row < -1 || row >= e->cfg.max_batch) return e->fail(DOTS_E_INVALID, "row %d out of range [-1, %d)", row, e->cfg.max_batch);
    *steps = *drafted = *accepted = 0;
    if (!e->sp_stats) return DOTS_OK;
    CK(hipSetDevice(e->device));
    unsigned long long v[3] = {0, 0, 0};
    CK(hipMemcpyAsync(v, e->sp_stats + (size_t)(row < 0 ? DOTS_MAX_BATCH : row) * 3, sizeof(v), hipMemcpyDeviceToHost, e->stream));
    CK(hipStreamSynchronize(e->stream));
    *steps = (int64_t)v[0]; *drafted = (int64_t)v[1]; *accepted = (int64_t)v[2];
    return DOTS_OK;
}

// ---------------------------------------------------------------------------------- predicted outputs
int dots_set_row_prediction(DotsEngine* e, int row, const int32_t* ids_host, int n) {
    if (!e) return DOTS_E_INVALID;
    if (row < 0 || row >= e->cfg.max_batch) return e->fail(DOTS_E_INVALID, "row %d out of range [0, %d)", row, e->cfg.max_batch);
    if (n < 0) return e->fail(DOTS_E_INVALID, "prediction length must be >= 0, got %d", n);
    if (!ids_host) n = 0;
    if (n > e->cfg.max_seq_len) return e->fail(DOTS_E_CAPACITY, "a prediction of %d tokens is longer than a sequence can become (max_seq_len %d)", n, e->cfg.max_seq_len);
    for (int j = 0; j < n; ++j)
        if (ids_host[j] < 0 || ids_host[j] >= e->cfg.vocab_size)
            return e->fail(DOTS_E_INVALID, "prediction id %d at %d out of range [0, %d)", ids_host[j], j, e->cfg.vocab_size);
    CK(hipSetDevice(e->device));
    if (n == 0) return clear_row_prediction(e, row);
    hipStream_t s = e->stream;
    if (!e->pr_stats) {
        // each piece is allocated once: a call that failed half way is resumed by the next one
        if (!e->pr_ids) CK(e->alloc(&e->pr_ids, (size_t)e->cfg.max_batch * e->cfg.max_seq_len));
        if (!e->pr_len) CK(e->alloc(&e->pr_len, (size_t)DOTS_MAX_BATCH));
        if (!e->pr_cur) CK(e->alloc(&e->pr_cur, (size_t)DOTS_MAX_BATCH));
        if (!e->pr_at) CK(e->alloc(&e->pr_at, (size_t)DOTS_MAX_BATCH));
        if (!e->pr_src) CK(e->alloc(&e->pr_src, (size_t)DOTS_MAX_BATCH));
        if (!e->pr_seen) CK(e->alloc(&e->pr_seen, (size_t)DOTS_MAX_BATCH));
        CK(e->alloc(&e->pr_stats, (size_t)DOTS_MAX_BATCH * 2));             // set last, it is the guard above
    }
    CK(hipMemcpyAsync(e->pr_ids + (size_t)row * e->cfg.max_seq_len, ids_host, (size_t)n * 4, hipMemcpyHostToDevice, s));
    CK(launch_predict_set_row(s, predict_state(e), e->sp_ndraft, row, n));
    CK(hipStreamSynchronize(s));                             // ids_host is the caller's
    if (!e->row_pred[row]) e->n_pred += 1;
    e->row_pred[row] = n;
    return DOTS_OK;
}

int dots_row_prediction_stats(DotsEngine* e, int row, int64_t* drafted, int64_t* accepted) {
    if (!e || !drafted || !accepted) return e ? e->fail(DOTS_E_INVALID, "null argument") : DOTS_E_INVALID;
    if (row < 0 || row >= e->cfg.max_batch) return e->fail(DOTS_E_INVALID, "row %d out of range [0, %d)", row, e->cfg.max_batch);
    *drafted = *accepted = 0;
    if (!e->pr_stats) return DOTS_OK;
    CK(hipSetDevice(e->device));
    unsigned long long v[2] = {0, 0};
    CK(hipMemcpyAsync(v, e->pr_stats + (size_t)row * 2, sizeof(v), hipMemcpyDeviceToHost, e->stream));
    CK(hipStreamSynchronize(e->stream));
    *drafted = (int64_t)v[0]; *accepted = (int64_t)v[1];
    return DOTS_OK;
}

int dots_row_guide_state(DotsEngine* e, int row, int32_t* state_out) {
    if (!e || !state_out) return e ? e->fail(DOTS_E_INVALID, "null argument") : DOTS_E_INVALID;
    if (row < 0 || row >= e->cfg.max_batch) return e->fail(DOTS_E_INVALID, "row %d out of range [0, %d)", row, e->cfg.max_batch);
    *state_out = -1;
    if (!e->stage.has(row, ROW_GUIDE)) return DOTS_OK;
    CK(hipSetDevice(e->device));
    RowGuide rg;
    CK(hipMemcpyAsync(&rg, e->d_guides + row, sizeof(rg), hipMemcpyDeviceToHost, e->stream));
    CK(hipStreamSynchronize(e->stream));
    *state_out = rg.state;
    return DOTS_OK;
}

int dots_set_row_logprobs(DotsEngine* e, int row, int top_n) {
    if (!e) return DOTS_E_INVALID;
    if (row < 0 || row >= e->cfg.max_batch) return e->fail(DOTS_E_INVALID, "row %d out of range [0, %d)", row, e->cfg.max_batch);
    if (top_n < -1 || top_n > DOTS_MAX_TOP_LOGPROBS) return e->fail(DOTS_E_INVALID, "top_n must be -1 (off) or in [0, %d]", DOTS_MAX_TOP_LOGPROBS);
    if (top_n < 0 && !e->d_row_lp) return DOTS_OK;
    if (top_n >= 0 && beam_row(e, row)) return e->fail(DOTS_E_INVALID, BEAM_ROW_TAKES_NONE, row);
    if (e->cfg.vocab_size > LP_MAX_V) return e->fail(DOTS_E_INVALID, "logprobs support vocabularies up to %d", LP_MAX_V);
    CK(hipSetDevice(e->device));
    if (!e->d_row_lp) {
        CK(e->alloc(&e->d_row_lp, DOTS_MAX_BATCH));
        CK(hipMemsetAsync(e->d_row_lp, 0xFF, DOTS_MAX_BATCH * 4, e->stream));
    }
    if (top_n >= 0) RET(ensure_lp_state(e));
    return set_row_lp(e, row, top_n);
}

int dots_row_logprobs(DotsEngine* e, int row, int pos0, int n, float* tok_lp_host, int32_t* top_ids_host, float* top_lp_host, int32_t* n_out) {
    if (!e || !n_out || pos0 < 0 || n < 0 || (n > 0 && (!tok_lp_host || !top_ids_host || !top_lp_host)))
        return e ? e->fail(DOTS_E_INVALID, "bad row_logprobs arguments") : DOTS_E_INVALID;
    if (e->slot_mode) {
        if (!slot_occupied(e, row)) return e->fail(DOTS_E_STATE, "slot %d is not occupied", row);
    } else if (row < 0 || row >= e->B) {
        return e->fail(DOTS_E_STATE, "row %d is not a sequence of the current static batch (%d rows)", row, e->B);
    }
    CK(hipSetDevice(e->device));
    int32_t len = 0;
    CK(hipMemcpyAsync(&len, e->out_lens + row, 4, hipMemcpyDeviceToHost, e->stream));
    CK(hipStreamSynchronize(e->stream));
    const int take = std::max(0, std::min(n, std::min(len, e->cfg.max_seq_len) - pos0));
    *n_out = take;
    if (take <= 0) return DOTS_OK;
    const size_t K = DOTS_MAX_TOP_LOGPROBS;
    if (!e->lp_tok) {                                   // never switched on: every position was selected with the row off
        std::fill(tok_lp_host, tok_lp_host + take, std::nanf(""));
        std::fill(top_ids_host, top_ids_host + take * K, -1);
        std::fill(top_lp_host, top_lp_host + take * K, std::nanf(""));
        return DOTS_OK;
    }
    const size_t o = (size_t)row * e->cfg.max_seq_len + pos0;
    CK(hipMemcpyAsync(tok_lp_host, e->lp_tok + o, (size_t)take * 4, hipMemcpyDeviceToHost, e->stream));
    CK(hipMemcpyAsync(top_ids_host, e->lp_ids + o * K, (size_t)take * K * 4, hipMemcpyDeviceToHost, e->stream));
    CK(hipMemcpyAsync(top_lp_host, e->lp_top + o * K, (size_t)take * K * 4, hipMemcpyDeviceToHost, e->stream));
    CK(hipStreamSynchronize(e->stream));
    return DOTS_OK;
}
}  // extern "C"
