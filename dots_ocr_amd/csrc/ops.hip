// Single-kernel entry points of the dots.ocr engine (dots_op_* / dots_bench_*): the kernels of a step at caller-chosen dimensions over
// caller buffers, for the tests and the micro-benchmarks.  Nothing here runs in an engine step.
#include "engine.h"

using namespace engine;

namespace {
// Decode operand of a single-kernel entry point from a ROW-MAJOR bf16 weight: bf16 fragments (fp8 == 0), or a quantised copy packed
// as e4m3 fragments + its scales — the same kernels dots_finalize_weights runs.
int op_weight(DotsEngine* e, Scratch& sc, const bf16_t* w, int64_t rows, int K, int Hq, int Hkv, bool qkv, int fp8, void** wd, float** scale) {
    *scale = nullptr;
    if (fp8) {
        bf16_t* q = nullptr;
        uint8_t* d = nullptr;
        CK(sc.get(&q, (size_t)rows * K));
        CK(sc.get(scale, (size_t)rows));
        CK(sc.get(&d, (size_t)((rows + 15) / 16 * 16) * K));
        CK(hipMemcpyAsync(q, w, (size_t)rows * K * 2, hipMemcpyDeviceToDevice, e->stream));
        CK(launch_quant_rows_fp8(e->stream, q, *scale, rows, K));
        CK(launch_pack_frag_fp8(e->stream, q, d, rows, K, qkv ? (Hq + Hkv) * 128 : 0));
        *wd = d;
    } else {
        bf16_t* d = nullptr;
        CK(sc.get(&d, (size_t)((rows + 15) / 16 * 16) * K));
        if (qkv) CK(launch_pack_frag_qkv(e->stream, w, d, Hq, Hkv, K));
        else CK(launch_pack_frag(e->stream, w, d, rows, K));
        *wd = d;
    }
    return DOTS_OK;
}

// `iters` replays of run() between two events on the engine's stream (the caller has warmed up), *ms = the mean time of one replay
template <typename F>
int time_replays(DotsEngine* e, int iters, F&& run, float* ms) {
    hipEvent_t t0 = nullptr, t1 = nullptr;
    CK(hipEventCreate(&t0));
    CK(hipEventCreate(&t1));
    hipError_t r = hipEventRecord(t0, e->stream);
    for (int i = 0; i < iters && r == hipSuccess; ++i) r = run();
    if (r == hipSuccess) r = hipEventRecord(t1, e->stream);
    if (r == hipSuccess) r = hipEventSynchronize(t1);
    float total = 0.f;
    if (r == hipSuccess) r = hipEventElapsedTime(&total, t0, t1);
    hipEventDestroy(t0);
    hipEventDestroy(t1);
    CK(r);
    *ms = total / iters;
    return DOTS_OK;
}

// kv_scales == nullptr: a bf16 page pool; else an fp8 one with these [Hkv][2] scales (dots_op_dec_qkv_kv8 / dots_op_decode_attn_kv8)
int op_dec_qkv(DotsEngine* e, const void* h, const void* ln_w, const void* wqkv, const void* bias, const int32_t* ctx_len_dev,
               const int32_t* block_table_dev, int max_pages, void* pool_layer, void* q_out, int B, int H, int Hq, int Hkv, float eps,
               float rope_theta, int fp8, const float* kv_scales) {
    if (!e || !h || !ln_w || !wqkv || !ctx_len_dev || !block_table_dev || !pool_layer || !q_out) return e ? e->fail(DOTS_E_INVALID, "null argument") : DOTS_E_INVALID;
    CK(hipSetDevice(e->device));
    Scratch sc(e);
    void* wd = nullptr;
    float *freq = nullptr, *wscale = nullptr;
    CK(sc.get(&freq, 64));
    float f[64];
    for (int i = 0; i < 64; ++i) f[i] = 1.0f / powf(rope_theta, (float)(2 * i) / 128.0f);
    CK(hipMemcpyAsync(freq, f, sizeof(f), hipMemcpyHostToDevice, e->stream));
    RET(op_weight(e, sc, (const bf16_t*)wqkv, (int64_t)(Hq + 2 * Hkv) * 128, H, Hq, Hkv, true, fp8, &wd, &wscale));
    bf16_t* xn = nullptr;                            // scratch sized for THIS call's hidden size (the engine's own d_xn is sized for its model: the tests run the
    CK(sc.get(&xn, (size_t)DOTS_MAX_BATCH * H));     // BASELINE dimensions through a small-model engine)
    CK(launch_dec_qkv(e->stream, (const bf16_t*)h, (const bf16_t*)ln_w, wd, wscale, (const bf16_t*)bias, freq, ctx_len_dev, block_table_dev, max_pages,
                      pool_layer, (bf16_t*)q_out, B, H, Hq, Hkv, eps, e->force_part ? e->dec_cus : 0, xn, nullptr, nullptr, kv_scales));      // dots_set_decode_plan(1): the partition plan's kernels
    CK(hipStreamSynchronize(e->stream));
    return DOTS_OK;
}

// covered_pairs != nullptr (dots_op_decode_attn_shared): with the shared-prefix plan of the given block table, every row active and
// static_pages[b] = ctx_len[b] / 64; *covered_pairs = the (row, split) pairs the plan's items cover
int op_decode_attn(DotsEngine* e, const void* q, const void* pool_layer, const int32_t* ctx_len_dev, const int32_t* block_table_dev,
                   int max_pages, void* out, int B, int Hq, int Hkv, int max_seq_len, const float* kv_scales, int32_t* covered_pairs = nullptr) {
    if (!e || !q || !pool_layer || !ctx_len_dev || !block_table_dev || !out || B < 1 || B > DOTS_MAX_BATCH) return e ? e->fail(DOTS_E_INVALID, "bad decode_attn arguments") : DOTS_E_INVALID;
    if (max_pages < 1 || Hkv < 1 || Hq % Hkv != 0 || Hq / Hkv > 16) return e->fail(DOTS_E_INVALID, "bad decode_attn arguments");
    CK(hipSetDevice(e->device));
    Scratch sc(e);
    const int n_splits = splits_for_ctx(max_seq_len);
    SharePlanDev share{nullptr, 0};
    if (covered_pairs) {
        std::vector<int32_t> ctx(B), table((size_t)B * max_pages), active(B, 1), plan(SHARE_PLAN_WORDS, 0);
        uint64_t mask[DOTS_MAX_BATCH] = {0};
        CK(hipMemcpyAsync(ctx.data(), ctx_len_dev, (size_t)B * 4, hipMemcpyDeviceToHost, e->stream));
        CK(hipMemcpyAsync(table.data(), block_table_dev, table.size() * 4, hipMemcpyDeviceToHost, e->stream));
        CK(hipStreamSynchronize(e->stream));
        for (int b = 0; b < B; ++b) ctx[b] = std::min(std::max(ctx[b], 0) / PAGE, max_pages);
        const int waves = decode_attn_waves();
        const SharePlanCounts n = waves == 4 ? share_plan(active.data(), table.data(), max_pages, ctx.data(), B, n_splits, waves, max_pages, plan.data() + SHARE_ITEMS_OFF,
                                                          plan.data() + SHARE_MEMBERS_OFF, mask)
                                             : SharePlanCounts{0, 0, 0, 0};
        plan[0] = n.items;
        std::memcpy(plan.data() + SHARE_MASK_OFF, mask, sizeof(mask));
        *covered_pairs = n.pairs;
        if (n.items) {
            int32_t* d_plan = nullptr;
            CK(sc.get(&d_plan, (size_t)SHARE_PLAN_WORDS));
            CK(hipMemcpyAsync(d_plan, plan.data(), (size_t)SHARE_PLAN_WORDS * 4, hipMemcpyHostToDevice, e->stream));
            CK(hipStreamSynchronize(e->stream));                 // `plan` is a local
            share = SharePlanDev{d_plan, (int)round_up(n.items, SHARE_ITEM_QUANTUM)};
        }
    }
    float *po = nullptr, *pml = nullptr;
    bf16_t* att = nullptr;
    const size_t rb = (size_t)(B + 15) / 16 * 16;
    CK(sc.get(&po, rb * Hq * n_splits * 128));
    CK(sc.get(&pml, rb * Hq * n_splits * 2));
    CK(sc.get(&att, rb * Hq * 128));
    CK(hipMemsetAsync(po, 0xff, rb * Hq * n_splits * 128 * 4, e->stream));      // NaN: a partial read without having been written shows up
    CK(hipMemsetAsync(pml, 0xff, rb * Hq * n_splits * 2 * 4, e->stream));
    CK(launch_decode_attn(e->stream, (const bf16_t*)q, pool_layer, ctx_len_dev, block_table_dev, max_pages, po, pml, B, Hq, Hkv, n_splits,
                          1.0f / sqrtf(128.0f), e->force_part ? e->dec_cus : 0, e->attn_stream, kv_scales, share.cap ? &share : nullptr));      // dots_set_decode_plan: the plan's kernel choice
    CK(launch_decode_attn_combine(e->stream, po, pml, ctx_len_dev, att, B, Hq, Hkv, n_splits));
    CK(launch_unpack_x(e->stream, att, (bf16_t*)out, B, Hq * 128));
    CK(hipStreamSynchronize(e->stream));
    return DOTS_OK;
}

// dots_op_select_tokens / dots_bench_select_tokens.  mode 2 = the per-row stage once (the op); mode 0 / 1 / 2 with iters > 0 = the legacy
// arg max pair / the legacy sampler (params[0].temperature, top_p, seed) / the per-row stage, replayed iters times between two events
// with every row marked finished (nothing is appended), *ms = the mean time of one replay.
// rules_host != nullptr (mode 2 only): row b carries rules_host[b] unless that entry is empty (no bias, allowed list, min_tokens, stop id or
// ignore_eos), the engine's EOS ids are live, and n_gen_host[b] (or hist_lens - n_prompt when nullptr) is the row's generated count.
int select_op(DotsEngine* e, const float* logits_dev, int B, int V, const DotsSamplingParams* params_host, const int32_t* hist_dev,
              const int32_t* hist_lens_dev, int hist_stride, const int32_t* n_prompt_dev, int32_t* out_tokens_dev, int mode, int iters, float* ms,
              const DotsLogitRules* rules_host = nullptr, const int32_t* n_gen_host = nullptr, const int32_t* guide_ids_host = nullptr,
              const int32_t* states_host = nullptr, int32_t* states_out_host = nullptr, const DotsNgramRule* ngram_host = nullptr) {
    if (!e || !logits_dev || B < 1 || B > DOTS_MAX_BATCH || V < 1 || !params_host || !hist_dev || !hist_lens_dev || hist_stride < 1 || !n_prompt_dev ||
        (!out_tokens_dev && !ms) || mode < 0 || mode > 2 || (rules_host && mode != 2) || (n_gen_host && !rules_host) ||
        (guide_ids_host && (!rules_host || !states_host)) || (ngram_host && !rules_host))
        return e ? e->fail(DOTS_E_INVALID, "bad select_tokens arguments") : DOTS_E_INVALID;
    // ngram_host != nullptr: row b carries ngram_host[b] unless its size is 0; its history is hist[n_prompt[b] .. hist_lens[b]), copied to
    // the front of the stage's output rows (where the engine keeps a row's own output).  A window may reach hist_stride.
    std::vector<RowNgram> ngrams(ngram_host ? DOTS_MAX_BATCH : 0, RowNgram{});
    if (ngram_host)
        for (int b = 0; b < B; ++b)
            if (ngram_host[b].size != 0) RET(check_ngram_rule(e, ngram_host[b], V, hist_stride, &ngrams[b]));
    // guide_ids_host != nullptr: row b holds guide guide_ids_host[b] (-1: none) of this engine at state states_host[b]; V must be the engine's
    // vocabulary (the token bytes are its).  states_out_host (may be nullptr) receives the rows' states after the commit, -1 for a row without.
    if (guide_ids_host) {
        if (!e->tok_off) return e->fail(DOTS_E_STATE, "the token bytes are not set (dots_set_token_bytes)");
        if (V != e->cfg.vocab_size) return e->fail(DOTS_E_INVALID, "guided selection needs V = the engine's vocabulary %d", e->cfg.vocab_size);
        for (int b = 0; b < B; ++b) {
            const int id = guide_ids_host[b];
            if (id < 0) continue;
            if (id >= (int)e->guides.size() || !e->guides[id].table) return e->fail(DOTS_E_INVALID, "row %d: no guide %d", b, id);
            if (states_host[b] < 0 || states_host[b] >= e->guides[id].n_states)
                return e->fail(DOTS_E_INVALID, "row %d: state %d outside [0, %d)", b, states_host[b], e->guides[id].n_states);
        }
    }
    if (n_gen_host)
        for (int b = 0; b < B; ++b)
            if (n_gen_host[b] < 0 || n_gen_host[b] > hist_stride) return e->fail(DOTS_E_INVALID, "n_gen must be in [0, hist_stride]");
    std::vector<RowParams> rp(B);
    for (int b = 0; b < B; ++b) RET(check_row_params(e, params_host[b], &rp[b]));
    if (mode == 1 && !(rp[0].temperature > 0.f)) return e->fail(DOTS_E_INVALID, "the legacy sampler needs temperature > 0");
    const std::vector<int32_t> own(B, 1);
    CK(hipSetDevice(e->device));
    Scratch sc(e);
    const size_t W = ((size_t)V + 31) / 32;
    RowParams* tab = nullptr;
    int32_t *own_d = nullptr, *cnt = nullptr, *pidx = nullptr, *cur = nullptr, *ctx = nullptr, *ids = nullptr, *lens = nullptr, *fin = nullptr;
    uint32_t *seen = nullptr, *thr = nullptr;
    float *pen = nullptr, *pval = nullptr;
    CK(sc.get(&tab, B));
    CK(sc.get(&own_d, B));
    CK(sc.get(&thr, B));
    CK(sc.get(&cnt, (size_t)B * V));
    CK(sc.get(&seen, (size_t)B * W));
    CK(sc.get(&pen, (size_t)B * V));
    CK(sc.get(&pval, (size_t)B * 64));
    CK(sc.get(&pidx, (size_t)B * 64));
    CK(sc.get(&cur, B));
    CK(sc.get(&ctx, B));
    CK(sc.get(&ids, (size_t)B * (hist_stride + 1)));
    CK(sc.get(&lens, B));
    CK(sc.get(&fin, B));
    CK(hipMemcpyAsync(tab, rp.data(), B * sizeof(RowParams), hipMemcpyHostToDevice, e->stream));
    CK(hipMemcpyAsync(own_d, own.data(), B * 4, hipMemcpyHostToDevice, e->stream));
    CK(launch_pen_history(e->stream, hist_dev, hist_lens_dev, hist_stride, n_prompt_dev, B, V, cnt, seen, lens));
    StepState st;
    st.cur_tokens = cur; st.ctx_len = ctx; st.out_ids = ids; st.out_lens = lens; st.finished = fin;
    st.eos_ids = e->eos_ids; st.sel = nullptr; st.max_len = nullptr;
    st.n_eos = rules_host ? e->n_eos : 0; st.out_stride = hist_stride + 1; st.cap = hist_stride + 2; st.advance_ctx = 0;
    RowRules* rtab = nullptr;
    float* img = nullptr;
    if (rules_host) {
        int32_t* stage = nullptr;
        CK(sc.get(&rtab, DOTS_MAX_BATCH));
        CK(sc.get(&img, (size_t)B * V));
        CK(sc.get(&stage, (size_t)V + 2 * DOTS_MAX_LOGIT_BIAS));
        for (int b = 0; b < B; ++b) {
            const DotsLogitRules& r = rules_host[b];
            if (!r.n_bias && !r.allowed_ids && !r.min_tokens && !r.n_stop && !r.ignore_eos) continue;
            RowRules rr;
            RET(check_logit_rules(e, r, V, e->h_eos, e->n_eos, &rr));
            const int n_allowed = r.allowed_ids ? r.n_allowed : 0;
            if (n_allowed) CK(hipMemcpyAsync(stage, r.allowed_ids, (size_t)n_allowed * 4, hipMemcpyHostToDevice, e->stream));
            if (r.n_bias) {
                CK(hipMemcpyAsync(stage + V, r.bias_ids, (size_t)r.n_bias * 4, hipMemcpyHostToDevice, e->stream));
                CK(hipMemcpyAsync(stage + V + DOTS_MAX_LOGIT_BIAS, r.bias_values, (size_t)r.n_bias * 4, hipMemcpyHostToDevice, e->stream));
            }
            CK(launch_set_row_rules(e->stream, rtab, img, b, V, rr, stage, n_allowed, stage + V,
                                    reinterpret_cast<const float*>(stage + V + DOTS_MAX_LOGIT_BIAS), r.n_bias));
            CK(hipStreamSynchronize(e->stream));           // the caller's lists and the staging buffer are free again
        }
        if (n_gen_host) CK(hipMemcpyAsync(lens, n_gen_host, B * 4, hipMemcpyHostToDevice, e->stream));
    }
    RowSel rs{tab, own_d, cnt, seen, pen, thr, 0, rtab, img, GuideSel{}, NgramSel{}};
    if (ngram_host) {
        RowNgram* ntab = nullptr;
        uint32_t* nmask = nullptr;
        CK(sc.get(&ntab, DOTS_MAX_BATCH));
        CK(sc.get(&nmask, (size_t)B * ngram_mask_words(V)));
        CK(hipMemcpyAsync(ntab, ngrams.data(), DOTS_MAX_BATCH * sizeof(RowNgram), hipMemcpyHostToDevice, e->stream));
        CK(launch_ngram_history(e->stream, hist_dev, hist_lens_dev, hist_stride, n_prompt_dev, B, ids, st.out_stride));
        rs.ngram = NgramSel{ntab, nmask, ngram_mask_words(V), V};
    }
    RowGuide* gtab = nullptr;
    int32_t* gstates = nullptr;
    if (guide_ids_host) {
        uint32_t* gmask = nullptr;
        CK(sc.get(&gtab, DOTS_MAX_BATCH));
        CK(sc.get(&gstates, DOTS_MAX_BATCH));
        CK(sc.get(&gmask, (size_t)B * guide_mask_words(V)));
        std::vector<RowGuide> rows(DOTS_MAX_BATCH, RowGuide{});
        for (int b = 0; b < B; ++b) {
            if (guide_ids_host[b] < 0) continue;
            const DotsEngine::Guide& g = e->guides[guide_ids_host[b]];
            rows[b] = RowGuide{g.table, g.accepting, g.n_states, g.start, states_host[b], 0};
        }
        CK(hipMemcpyAsync(gtab, rows.data(), DOTS_MAX_BATCH * sizeof(RowGuide), hipMemcpyHostToDevice, e->stream));
        CK(hipMemcpyAsync(gstates, states_host, B * 4, hipMemcpyHostToDevice, e->stream));
        CK(hipStreamSynchronize(e->stream));               // `rows` is a local
        rs.guide = GuideSel{gtab, gmask, e->tok_off, e->tok_bytes, guide_mask_words(V), V};
    }
    auto run = [&]() -> hipError_t {
        if (rs.guide.rows) {
            // every replay starts from the given states (a timed replay commits nothing: its rows are marked finished)
            hipError_t r = launch_guide_set_states(e->stream, gtab, gstates, B);
            if (r != hipSuccess) return r;
        }
        if (mode == 0) return launch_argmax_step(e->stream, logits_dev, V, V, B, pval, pidx, st);
        if (mode == 1) return launch_sample_step(e->stream, logits_dev, V, V, B, rp[0].temperature, rp[0].top_p, rp[0].seed, st);
        // a timed replay marks its rows finished so that nothing is appended: the ban kernel is told of none, or it would skip them all
        return launch_row_stage(e->stream, logits_dev, V, V, B, rs, pval, pidx, st, iters > 0 ? nullptr : st.finished);
    };
    if (iters <= 0) {
        CK(run());
        CK(hipMemcpyAsync(out_tokens_dev, cur, B * 4, hipMemcpyDeviceToDevice, e->stream));
        std::vector<RowGuide> after(states_out_host ? B : 0);
        if (states_out_host) CK(hipMemcpyAsync(after.data(), gtab, B * sizeof(RowGuide), hipMemcpyDeviceToHost, e->stream));
        CK(hipStreamSynchronize(e->stream));
        for (size_t b = 0; b < after.size(); ++b) states_out_host[b] = after[b].table ? after[b].state : -1;
        return DOTS_OK;
    }
    const std::vector<int32_t> ones(B, 1);
    CK(hipMemcpyAsync(fin, ones.data(), B * 4, hipMemcpyHostToDevice, e->stream));
    for (int i = 0; i < 3; ++i) CK(run());                                  // warm-up
    return time_replays(e, iters, run, ms);
}

// dots_op_logprobs / dots_bench_logprobs: the two logprob kernels over caller logits, every row at position 0 of its own output row.
// which 0 = both kernels, 1 = partial only, 2 = final only; iters > 0 = replays between two events, *ms = mean time of one replay.
int logprobs_op(DotsEngine* e, const float* logits_dev, int B, int V, int ld, const int32_t* top_n_host, const int32_t* chosen_dev,
                float* tok_lp_dev, int32_t* top_ids_dev, float* top_lp_dev, int which, int iters, float* ms) {
    if (!e || !logits_dev || B < 1 || B > DOTS_MAX_BATCH || V < 1 || V > LP_MAX_V || ld < V || !top_n_host || which < 0 || which > 2)
        return e ? e->fail(DOTS_E_INVALID, "bad logprobs arguments") : DOTS_E_INVALID;
    for (int b = 0; b < B; ++b)
        if (top_n_host[b] < -1 || top_n_host[b] > DOTS_MAX_TOP_LOGPROBS) return e->fail(DOTS_E_INVALID, "top_n of row %d not in [-1, %d]", b, DOTS_MAX_TOP_LOGPROBS);
    CK(hipSetDevice(e->device));
    Scratch sc(e);
    const size_t K = DOTS_MAX_TOP_LOGPROBS;
    int32_t *tn = nullptr, *pi = nullptr, *pos = nullptr, *cho = nullptr, *ids = nullptr;
    float *ms_p = nullptr, *pv = nullptr, *tok = nullptr, *top = nullptr;
    CK(sc.get(&tn, B));
    CK(sc.get(&ms_p, (size_t)B * LP_CHUNKS * 2));
    CK(sc.get(&pv, (size_t)B * LP_CHUNKS * K));
    CK(sc.get(&pi, (size_t)B * LP_CHUNKS * K));
    CK(sc.get(&pos, B));
    if (!chosen_dev) { CK(sc.get(&cho, B)); chosen_dev = cho; }           // timing: token 0 of every row
    if (!tok_lp_dev) { CK(sc.get(&tok, B)); CK(sc.get(&ids, (size_t)B * K)); CK(sc.get(&top, (size_t)B * K)); tok_lp_dev = tok; top_ids_dev = ids; top_lp_dev = top; }
    CK(hipMemcpyAsync(tn, top_n_host, B * 4, hipMemcpyHostToDevice, e->stream));
    const LogprobState ls{tn, nullptr, nullptr, nullptr, chosen_dev, ms_p, pv, pi, pos, tok_lp_dev, top_ids_dev, top_lp_dev, 1};
    auto run = [&](int w) -> hipError_t {
        hipError_t r = hipSuccess;
        if (w != 2) r = launch_logprob_partial(e->stream, logits_dev, V, ld, B, ls);
        if (r == hipSuccess && w != 1) r = launch_logprob_final(e->stream, logits_dev, V, ld, B, ls);
        return r;
    };
    if (iters <= 0) {
        CK(run(0));
        CK(hipStreamSynchronize(e->stream));
        return DOTS_OK;
    }
    for (int i = 0; i < 3; ++i) CK(run(0));                              // warm-up; also leaves the partials the final kernel reads
    return time_replays(e, iters, [&] { return run(which); }, ms);
}
}  // namespace

extern "C" {
// ---------------------------------------------------------------- single-kernel entry points
int dots_op_rmsnorm(DotsEngine* e, const void* x, const void* w, void* y, int64_t rows, int dim, float eps) {
    if (!e) return DOTS_E_INVALID;
    CK(hipSetDevice(e->device));
    CK(launch_rmsnorm(e->stream, (const bf16_t*)x, (const bf16_t*)w, (bf16_t*)y, rows, dim, eps));
    return DOTS_OK;
}
int dots_op_layernorm(DotsEngine* e, const void* x, const void* w, const void* b, void* y, int64_t rows, int dim, float eps) {
    if (!e) return DOTS_E_INVALID;
    CK(hipSetDevice(e->device));
    CK(launch_layernorm(e->stream, (const bf16_t*)x, (const bf16_t*)w, (const bf16_t*)b, (bf16_t*)y, rows, dim, eps));
    return DOTS_OK;
}
int dots_op_gemm(DotsEngine* e, const void* A, const void* W, const void* bias, const void* residual, void* C,
                 int64_t M, int N, int K, int epilogue, const float* colscale) {
    if (!e) return DOTS_E_INVALID;
    CK(hipSetDevice(e->device));
    const int ldc = epilogue == EPI_SWIGLU ? N / 2 : N;
    CK(launch_gemm(e->stream, (const bf16_t*)A, (const bf16_t*)W, (const bf16_t*)bias, (const bf16_t*)residual, C, M, N, K, K, ldc, epilogue, colscale));
    return DOTS_OK;
}

int dots_op_gemm_fp8(DotsEngine* e, const void* A, const void* W, const void* bias, const void* residual, void* C, int64_t M, int N, int K,
                     int epilogue) {
    if (!e || !A || !W || !C) return e ? e->fail(DOTS_E_INVALID, "null argument") : DOTS_E_INVALID;
    if (!gemm_fp8_supports(N, K) || epilogue == EPI_F32) return e->fail(DOTS_E_INVALID, "fp8 GEMM needs N %% 256 == 0, K %% 64 == 0 and a bf16 output");
    CK(hipSetDevice(e->device));
    Scratch sc(e);
    bf16_t* wq = nullptr;
    uint8_t *w8 = nullptr, *a8 = nullptr;
    float *ws = nullptr, *as = nullptr;
    CK(sc.get(&wq, (size_t)N * K));
    CK(sc.get(&w8, (size_t)N * K));
    CK(sc.get(&ws, (size_t)N));
    CK(sc.get(&a8, (size_t)M * K));
    CK(sc.get(&as, (size_t)M));
    CK(hipMemcpyAsync(wq, W, (size_t)N * K * 2, hipMemcpyDeviceToDevice, e->stream));
    CK(launch_quant_rows_fp8(e->stream, wq, ws, N, K));
    CK(launch_bf16q_to_fp8(e->stream, wq, w8, (int64_t)N * K));
    CK(launch_quant_act_fp8(e->stream, (const bf16_t*)A, a8, as, M, K, K));
    const int ldc = epilogue == EPI_SWIGLU ? N / 2 : N;
    CK(launch_gemm_fp8(e->stream, a8, as, w8, ws, (const bf16_t*)bias, (const bf16_t*)residual, C, M, N, K, ldc, epilogue));
    CK(hipStreamSynchronize(e->stream));
    return DOTS_OK;
}

int dots_op_quant_fp8(DotsEngine* e, void* w_inout, float* scale_out, int64_t N, int K) {
    if (!e || !w_inout || !scale_out) return e ? e->fail(DOTS_E_INVALID, "null argument") : DOTS_E_INVALID;
    CK(hipSetDevice(e->device));
    CK(launch_quant_rows_fp8(e->stream, (bf16_t*)w_inout, scale_out, N, K));
    CK(hipStreamSynchronize(e->stream));
    return DOTS_OK;
}

static int upload_lists(DotsEngine* e, const int32_t* cu, int n_seq, int Hq, std::vector<Tile64>& tiles, std::vector<QBlock>& qb,
                        Tile64** d_tiles, QBlock** d_qb, int64_t* Tpad) {
    std::vector<int> lens(n_seq);
    for (int i = 0; i < n_seq; ++i) lens[i] = cu[i + 1] - cu[i];
    build_worklists(lens, Hq, tiles, qb, Tpad);
    CK(e->alloc(d_tiles, tiles.size() + 1));
    CK(e->alloc(d_qb, qb.size() + 1));
    CK(hipMemcpyAsync(*d_tiles, tiles.data(), tiles.size() * sizeof(Tile64), hipMemcpyHostToDevice, e->stream));
    CK(hipMemcpyAsync(*d_qb, qb.data(), qb.size() * sizeof(QBlock), hipMemcpyHostToDevice, e->stream));
    CK(hipStreamSynchronize(e->stream));
    return DOTS_OK;
}

int dots_op_flash_attn(DotsEngine* e, const void* q, const void* k, const void* vt, void* out, const int32_t* cu, int n_seq,
                       int Hq, int Hkv, int causal, float scale) {
    if (!e || !cu || n_seq < 1) return DOTS_E_INVALID;
    CK(hipSetDevice(e->device));
    std::vector<Tile64> tiles;
    std::vector<QBlock> qb;
    Tile64* dt = nullptr;
    QBlock* dq = nullptr;
    int64_t Tpad = 0;
    RET(upload_lists(e, cu, n_seq, Hq, tiles, qb, &dt, &dq, &Tpad));
    const int64_t T = cu[n_seq];
    const XcdPlan xcd_plan = make_xcd_plan(qb.data(), (int)qb.size());
    hipError_t r = launch_flash_attn(e->stream, (const bf16_t*)q, (const bf16_t*)k, (const bf16_t*)vt, (bf16_t*)out, dq, (int)qb.size(), T, Tpad, Hq, Hkv, causal, scale, &xcd_plan);
    hipStreamSynchronize(e->stream);
    e->release(dt);
    e->release(dq);
    CK(r);
    return DOTS_OK;
}

int dots_op_flash_attn_paged(DotsEngine* e, const void* q, const void* pool_layer, const int32_t* block_table_dev, int max_pages, int table_rows,
                             void* out, const int32_t* rows_host, const int32_t* prefix_host, const int32_t* n_new_host, int n_seq, int Hq, int Hkv,
                             float scale, const float* kv_scales_dev) {
    if (!e) return DOTS_E_INVALID;
    if (!q || !pool_layer || !block_table_dev || !out || !prefix_host || !n_new_host || n_seq < 1 || max_pages < 1 || table_rows < 1 || Hkv < 1 || Hq % Hkv)
        return e->fail(DOTS_E_INVALID, "bad flash_attn_paged arguments");
    CK(hipSetDevice(e->device));
    std::vector<PagedQBlock> items;
    int64_t T = 0;
    for (int b = 0; b < n_seq; ++b) {
        const int c = prefix_host[b], m = n_new_host[b], row = rows_host ? rows_host[b] : b;
        if (c < 0 || c % 64) return e->fail(DOTS_E_INVALID, "sequence %d: a prefix of %d positions is not a multiple of 64 (unaligned prefixes are not supported)", b, c);
        if (m < 1 || (int64_t)c + m > (int64_t)max_pages * 64 || row < 0 || row >= table_rows || T + m > INT32_MAX)
            return e->fail(DOTS_E_INVALID, "sequence %d: prefix %d + %d new rows on table row %d does not fit %d pages / %d rows", b, c, m, row, max_pages, table_rows);
        for (int r = 0; r < m; r += 64) items.push_back(PagedQBlock{(int32_t)(T + r), std::min(64, m - r), c + r, row});
        T += m;
    }
    Scratch sc(e);
    PagedQBlock* d_items = nullptr;
    CK(sc.get(&d_items, items.size()));
    CK(hipMemcpyAsync(d_items, items.data(), items.size() * sizeof(PagedQBlock), hipMemcpyHostToDevice, e->stream));
    CK(launch_flash_attn_paged(e->stream, (const bf16_t*)q, pool_layer, block_table_dev, max_pages, table_rows, items.data(), d_items, (int)items.size(),
                               (bf16_t*)out, T, Hq, Hkv, scale, kv_scales_dev));
    CK(hipStreamSynchronize(e->stream));
    return DOTS_OK;
}

int dots_plan_flash_xcd(const int32_t* lens, int n_seq, int Hq, int32_t* base8, int32_t* cnt8, int64_t* cost8) {
    if (!lens || n_seq < 1 || Hq < 1 || !base8 || !cnt8 || !cost8) return DOTS_E_INVALID;
    std::vector<int> L(lens, lens + n_seq);
    for (int n : L)
        if (n < 1) return DOTS_E_INVALID;
    std::vector<Tile64> tiles;
    std::vector<QBlock> qb;
    int64_t Tpad = 0;
    build_worklists(L, Hq, tiles, qb, &Tpad);
    const XcdPlan p = make_xcd_plan(qb.data(), (int)qb.size());
    for (int x = 0; x < 8; ++x) {
        base8[x] = p.base[x];
        cnt8[x] = p.cnt[x];
        cost8[x] = 0;
        for (int i = p.base[x]; i < p.base[x] + p.cnt[x]; ++i) cost8[x] += ((qb[i].n + 63) / 64 + 1) & ~1;
    }
    return (int)qb.size();
}

int dots_op_qkv_rope_split(DotsEngine* e, const void* qkv, void* q, void* k, void* vt, const int32_t* cu, int n_seq,
                           const int32_t* pos_host, int Hq, int Hkv, int rope2d, float theta) {
    if (!e || !cu || n_seq < 1 || !pos_host) return DOTS_E_INVALID;
    CK(hipSetDevice(e->device));
    std::vector<Tile64> tiles;
    std::vector<QBlock> qb;
    Tile64* dt = nullptr;
    QBlock* dq = nullptr;
    int64_t Tpad = 0;
    RET(upload_lists(e, cu, n_seq, Hq, tiles, qb, &dt, &dq, &Tpad));
    const int64_t T = cu[n_seq];
    int32_t* dpos = nullptr;
    float2* cs = nullptr;
    float* freq = nullptr;
    const int nf = rope2d ? 32 : 64;
    std::vector<float> f(nf);
    for (int i = 0; i < nf; ++i) f[i] = 1.0f / powf(theta, (float)(2 * i) / (rope2d ? 64.0f : 128.0f));
    CK(e->alloc(&dpos, (size_t)T * (rope2d ? 2 : 1)));
    CK(e->alloc(&cs, (size_t)T * 64));
    CK(e->alloc(&freq, (size_t)nf));
    CK(hipMemcpyAsync(dpos, pos_host, (size_t)T * (rope2d ? 2 : 1) * 4, hipMemcpyHostToDevice, e->stream));
    CK(hipMemcpyAsync(freq, f.data(), nf * 4, hipMemcpyHostToDevice, e->stream));
    CK(launch_rope_table(e->stream, dpos, freq, cs, T, rope2d));
    hipError_t r = launch_qkv_rope_split(e->stream, (const bf16_t*)qkv, cs, dt, (int)tiles.size(), (bf16_t*)q, (bf16_t*)k, (bf16_t*)vt, T, Tpad, Hq, Hkv);
    hipStreamSynchronize(e->stream);
    e->release(dt); e->release(dq); e->release(dpos); e->release(cs); e->release(freq);
    CK(r);
    return DOTS_OK;
}

// The qkv projection of a prefill pass + rope + head-major split, either as the engine's fused path (fused != 0: the GEMM's rope epilogue writes q / k,
// the split kernel only transposes v) or as the two kernels of rounds 1-5 — the test holds the two to the same bits.  fused != 0 fails with
// DOTS_E_INVALID when the process's GEMM plan / the shape has no fused kernel.
int dots_op_qkv_proj_rope(DotsEngine* e, const void* x, const void* w, const void* bias, void* qkv_ws, void* q, void* k, void* vt, const int32_t* cu, int n_seq,
                          const int32_t* pos_host, int K, int Hq, int Hkv, int rope2d, float theta, int fused) {
    if (!e || !x || !w || !qkv_ws || !q || !k || !vt || !cu || n_seq < 1 || !pos_host) return DOTS_E_INVALID;
    CK(hipSetDevice(e->device));
    std::vector<Tile64> tiles;
    std::vector<QBlock> qb;
    Tile64* dt = nullptr;
    QBlock* dq = nullptr;
    int64_t Tpad = 0;
    RET(upload_lists(e, cu, n_seq, Hq, tiles, qb, &dt, &dq, &Tpad));
    const int64_t T = cu[n_seq];
    const int N = (Hq + 2 * Hkv) * 128;
    int32_t* dpos = nullptr;
    float2* cs = nullptr;
    float* freq = nullptr;
    const int nf = rope2d ? 32 : 64;
    std::vector<float> f(nf);
    for (int i = 0; i < nf; ++i) f[i] = 1.0f / powf(theta, (float)(2 * i) / (rope2d ? 64.0f : 128.0f));
    CK(e->alloc(&dpos, (size_t)T * (rope2d ? 2 : 1)));
    CK(e->alloc(&cs, (size_t)T * 64));
    CK(e->alloc(&freq, (size_t)nf));
    CK(hipMemcpyAsync(dpos, pos_host, (size_t)T * (rope2d ? 2 : 1) * 4, hipMemcpyHostToDevice, e->stream));
    CK(hipMemcpyAsync(freq, f.data(), nf * 4, hipMemcpyHostToDevice, e->stream));
    CK(launch_rope_table(e->stream, dpos, freq, cs, T, rope2d));
    hipError_t r;
    if (fused) {
        r = launch_gemm_qk_rope(e->stream, (const bf16_t*)x, (const bf16_t*)w, (const bf16_t*)bias, (bf16_t*)qkv_ws, T, N, K, K, N, cs, (bf16_t*)q, (bf16_t*)k, Hq, Hkv);
        if (r == hipSuccess) r = launch_qkv_rope_split(e->stream, (const bf16_t*)qkv_ws, cs, dt, (int)tiles.size(), (bf16_t*)q, (bf16_t*)k, (bf16_t*)vt, T, Tpad, Hq, Hkv, true);
    } else {
        r = launch_gemm(e->stream, (const bf16_t*)x, (const bf16_t*)w, (const bf16_t*)bias, nullptr, qkv_ws, T, N, K, K, N, EPI_NONE);
        if (r == hipSuccess) r = launch_qkv_rope_split(e->stream, (const bf16_t*)qkv_ws, cs, dt, (int)tiles.size(), (bf16_t*)q, (bf16_t*)k, (bf16_t*)vt, T, Tpad, Hq, Hkv);
    }
    hipStreamSynchronize(e->stream);
    e->release(dt); e->release(dq); e->release(dpos); e->release(cs); e->release(freq);
    if (r == hipErrorNotSupported) { (void)hipGetLastError(); return e->fail(DOTS_E_INVALID, "no fused qkv + rope kernel for this shape / GEMM plan"); }
    CK(r);
    return DOTS_OK;
}

// ---- single decode kernels at caller-chosen dimensions (tests/test_decode_kernels_gpu.py).  Inputs are ROW-MAJOR bf16
// tensors as the HF state dict holds them; the fragment-order / permuted packing the decode step uses happens inside, with
// the same pack kernels the engine runs at dots_finalize_weights.

int dots_op_dec_qkv(DotsEngine* e, const void* h, const void* ln_w, const void* wqkv, const void* bias, const int32_t* ctx_len_dev,
                    const int32_t* block_table_dev, int max_pages, void* pool_layer, void* q_out, int B, int H, int Hq, int Hkv, float eps,
                    float rope_theta, int fp8) {
    return op_dec_qkv(e, h, ln_w, wqkv, bias, ctx_len_dev, block_table_dev, max_pages, pool_layer, q_out, B, H, Hq, Hkv, eps, rope_theta, fp8, nullptr);
}

int dots_op_dec_qkv_kv8(DotsEngine* e, const void* h, const void* ln_w, const void* wqkv, const void* bias, const int32_t* ctx_len_dev,
                        const int32_t* block_table_dev, int max_pages, void* pool_layer, void* q_out, int B, int H, int Hq, int Hkv, float eps,
                        float rope_theta, int fp8, const float* kv_scales_dev) {
    if (!kv_scales_dev) return e ? e->fail(DOTS_E_INVALID, "null kv_scales") : DOTS_E_INVALID;
    return op_dec_qkv(e, h, ln_w, wqkv, bias, ctx_len_dev, block_table_dev, max_pages, pool_layer, q_out, B, H, Hq, Hkv, eps, rope_theta, fp8, kv_scales_dev);
}

int dots_op_decode_attn(DotsEngine* e, const void* q, const void* pool_layer, const int32_t* ctx_len_dev, const int32_t* block_table_dev,
                        int max_pages, void* out, int B, int Hq, int Hkv, int max_seq_len) {
    return op_decode_attn(e, q, pool_layer, ctx_len_dev, block_table_dev, max_pages, out, B, Hq, Hkv, max_seq_len, nullptr);
}

int dots_op_decode_attn_shared(DotsEngine* e, const void* q, const void* pool_layer, const int32_t* ctx_len_dev, const int32_t* block_table_dev, int max_pages,
                               void* out, int B, int Hq, int Hkv, int max_seq_len, const float* kv_scales_dev, int32_t* covered_pairs_out) {
    if (!covered_pairs_out) return e ? e->fail(DOTS_E_INVALID, "null argument") : DOTS_E_INVALID;
    return op_decode_attn(e, q, pool_layer, ctx_len_dev, block_table_dev, max_pages, out, B, Hq, Hkv, max_seq_len, kv_scales_dev, covered_pairs_out);
}

int dots_plan_shared_prefix(const int32_t* active, const int32_t* block_table, int max_pages, const int32_t* static_pages, int rows, int n_splits, int waves,
                            int32_t* items3, int32_t* members, uint64_t* masks) {
    if (!active || !block_table || !static_pages || !items3 || !members || !masks || rows < 1 || rows > DOTS_MAX_BATCH || max_pages < 1 || n_splits < 1 || waves < 1)
        return DOTS_E_INVALID;
    for (int b = 0; b < rows; ++b)
        if (static_pages[b] < 0 || static_pages[b] > max_pages) return DOTS_E_INVALID;
    return share_plan(active, block_table, max_pages, static_pages, rows, n_splits, waves, max_pages, items3, members, masks).items;
}

int dots_op_decode_attn_kv8(DotsEngine* e, const void* q, const void* pool_layer, const int32_t* ctx_len_dev, const int32_t* block_table_dev,
                            int max_pages, void* out, int B, int Hq, int Hkv, int max_seq_len, const float* kv_scales_dev) {
    if (!kv_scales_dev) return e ? e->fail(DOTS_E_INVALID, "null kv_scales") : DOTS_E_INVALID;
    return op_decode_attn(e, q, pool_layer, ctx_len_dev, block_table_dev, max_pages, out, B, Hq, Hkv, max_seq_len, kv_scales_dev);
}

int dots_op_dec_proj(DotsEngine* e, const void* x, const void* w, void* h_inout, int B, int N, int K, int fp8) {
    if (!e || !x || !w || !h_inout || B < 1 || B > DOTS_MAX_BATCH) return e ? e->fail(DOTS_E_INVALID, "bad dec_proj arguments") : DOTS_E_INVALID;
    CK(hipSetDevice(e->device));
    Scratch sc(e);
    bf16_t* xi = nullptr;
    void* wd = nullptr;
    float* wscale = nullptr;
    CK(sc.get(&xi, (size_t)(B + 15) / 16 * 16 * K));
    CK(launch_pack_x(e->stream, (const bf16_t*)x, xi, B, K));
    RET(op_weight(e, sc, (const bf16_t*)w, N, K, 0, 0, false, fp8, &wd, &wscale));
    bool pend = false;
    float* part = nullptr;
    CK(sc.get(&part, (size_t)DEC_KSPLIT_PARTS * DOTS_MAX_BATCH * N));
    CK(launch_dec_proj(e->stream, xi, wd, wscale, (bf16_t*)h_inout, B, N, K, e->force_part ? e->dec_cus : 0, part, &pend));
    if (pend) CK(launch_dec_norm_ximg(e->stream, (const bf16_t*)h_inout, nullptr, nullptr, B, N, 0.f, part, wscale));        // the K-split kernel leaves the residual update to its consumer
    CK(hipStreamSynchronize(e->stream));
    return DOTS_OK;
}

int dots_op_dec_gateup(DotsEngine* e, const void* h, const void* ln_w, const void* gate_w, const void* up_w, void* act_out, int B, int H, int I, float eps,
                       int fp8) {
    if (!e || !h || !ln_w || !gate_w || !up_w || !act_out || B < 1 || B > DOTS_MAX_BATCH) return e ? e->fail(DOTS_E_INVALID, "bad dec_gateup arguments") : DOTS_E_INVALID;
    CK(hipSetDevice(e->device));
    Scratch sc(e);
    bf16_t *w13 = nullptr, *act = nullptr;
    void* w13d = nullptr;
    float* wscale = nullptr;
    CK(sc.get(&w13, (size_t)2 * I * H));
    CK(sc.get(&act, (size_t)(B + 15) / 16 * 16 * I));
    CK(launch_pack_w13(e->stream, (const bf16_t*)gate_w, (const bf16_t*)up_w, w13, I, H));
    RET(op_weight(e, sc, w13, (int64_t)2 * I, H, 0, 0, false, fp8, &w13d, &wscale));
    bf16_t* xn = nullptr;
    CK(sc.get(&xn, (size_t)DOTS_MAX_BATCH * H));
    CK(launch_dec_gateup(e->stream, (const bf16_t*)h, (const bf16_t*)ln_w, w13d, wscale, act, B, H, I, eps, e->force_part ? e->dec_cus : 0, xn));
    CK(launch_unpack_x(e->stream, act, (bf16_t*)act_out, B, I));
    CK(hipStreamSynchronize(e->stream));
    return DOTS_OK;
}

int dots_op_dec_lmhead(DotsEngine* e, const void* h, const void* ln_w, const void* w, void* logits_out, int B, int H, int V, float eps, int fp8) {
    if (!e || !h || !ln_w || !w || !logits_out || B < 1 || B > DOTS_MAX_BATCH) return e ? e->fail(DOTS_E_INVALID, "bad dec_lmhead arguments") : DOTS_E_INVALID;
    CK(hipSetDevice(e->device));
    Scratch sc(e);
    void* wd = nullptr;
    float* wscale = nullptr;
    RET(op_weight(e, sc, (const bf16_t*)w, V, H, 0, 0, false, fp8, &wd, &wscale));
    bf16_t* xn = nullptr;
    CK(sc.get(&xn, (size_t)DOTS_MAX_BATCH * H));
    CK(launch_dec_lmhead(e->stream, (const bf16_t*)h, (const bf16_t*)ln_w, wd, wscale, (float*)logits_out, B, H, V, eps, e->force_part ? e->dec_cus : 0, xn));
    CK(hipStreamSynchronize(e->stream));
    return DOTS_OK;
}

int dots_op_select_tokens(DotsEngine* e, const float* logits_dev, int B, int V, const DotsSamplingParams* params_host, const int32_t* hist_dev,
                          const int32_t* hist_lens_dev, int hist_stride, const int32_t* n_prompt_dev, int32_t* out_tokens_dev) {
    if (!out_tokens_dev) return e ? e->fail(DOTS_E_INVALID, "bad select_tokens arguments") : DOTS_E_INVALID;
    return select_op(e, logits_dev, B, V, params_host, hist_dev, hist_lens_dev, hist_stride, n_prompt_dev, out_tokens_dev, 2, 0, nullptr);
}

int dots_bench_select_tokens(DotsEngine* e, const float* logits_dev, int B, int V, const DotsSamplingParams* params_host, const int32_t* hist_dev,
                             const int32_t* hist_lens_dev, int hist_stride, const int32_t* n_prompt_dev, int mode, int iters, float* ms_out) {
    if (!ms_out || iters < 1) return e ? e->fail(DOTS_E_INVALID, "bad bench_select_tokens arguments") : DOTS_E_INVALID;
    return select_op(e, logits_dev, B, V, params_host, hist_dev, hist_lens_dev, hist_stride, n_prompt_dev, nullptr, mode, iters, ms_out);
}

int dots_op_select_tokens_rules(DotsEngine* e, const float* logits_dev, int B, int V, const DotsSamplingParams* params_host, const DotsLogitRules* rules_host,
                                const int32_t* n_gen_host, const int32_t* hist_dev, const int32_t* hist_lens_dev, int hist_stride,
                                const int32_t* n_prompt_dev, int32_t* out_tokens_dev) {
    if (!out_tokens_dev || !rules_host) return e ? e->fail(DOTS_E_INVALID, "bad select_tokens arguments") : DOTS_E_INVALID;
    return select_op(e, logits_dev, B, V, params_host, hist_dev, hist_lens_dev, hist_stride, n_prompt_dev, out_tokens_dev, 2, 0, nullptr, rules_host, n_gen_host);
}

int dots_bench_select_tokens_rules(DotsEngine* e, const float* logits_dev, int B, int V, const DotsSamplingParams* params_host, const DotsLogitRules* rules_host,
                                   const int32_t* n_gen_host, const int32_t* hist_dev, const int32_t* hist_lens_dev, int hist_stride,
                                   const int32_t* n_prompt_dev, int iters, float* ms_out) {
    if (!ms_out || iters < 1 || !rules_host) return e ? e->fail(DOTS_E_INVALID, "bad bench_select_tokens arguments") : DOTS_E_INVALID;
    return select_op(e, logits_dev, B, V, params_host, hist_dev, hist_lens_dev, hist_stride, n_prompt_dev, nullptr, 2, iters, ms_out, rules_host, n_gen_host);
}

int dots_op_select_tokens_guided(DotsEngine* e, const float* logits_dev, int B, int V, const DotsSamplingParams* params_host, const DotsLogitRules* rules_host,
                                 const int32_t* n_gen_host, const int32_t* guide_ids_host, const int32_t* states_host, const int32_t* hist_dev,
                                 const int32_t* hist_lens_dev, int hist_stride, const int32_t* n_prompt_dev, int32_t* out_tokens_dev, int32_t* states_out_host) {
    if (!out_tokens_dev || !rules_host || !guide_ids_host) return e ? e->fail(DOTS_E_INVALID, "bad select_tokens arguments") : DOTS_E_INVALID;
    return select_op(e, logits_dev, B, V, params_host, hist_dev, hist_lens_dev, hist_stride, n_prompt_dev, out_tokens_dev, 2, 0, nullptr, rules_host, n_gen_host,
                     guide_ids_host, states_host, states_out_host);
}

int dots_bench_select_tokens_guided(DotsEngine* e, const float* logits_dev, int B, int V, const DotsSamplingParams* params_host, const DotsLogitRules* rules_host,
                                    const int32_t* n_gen_host, const int32_t* guide_ids_host, const int32_t* states_host, const int32_t* hist_dev,
                                    const int32_t* hist_lens_dev, int hist_stride, const int32_t* n_prompt_dev, int iters, float* ms_out) {
    if (!ms_out || iters < 1 || !rules_host || !guide_ids_host) return e ? e->fail(DOTS_E_INVALID, "bad bench_select_tokens arguments") : DOTS_E_INVALID;
    return select_op(e, logits_dev, B, V, params_host, hist_dev, hist_lens_dev, hist_stride, n_prompt_dev, nullptr, 2, iters, ms_out, rules_host, n_gen_host,
                     guide_ids_host, states_host, nullptr);
}

int dots_op_select_tokens_ngram(DotsEngine* e, const float* logits_dev, int B, int V, const DotsSamplingParams* params_host, const DotsLogitRules* rules_host,
                                const DotsNgramRule* ngram_host, const int32_t* hist_dev, const int32_t* hist_lens_dev, int hist_stride,
                                const int32_t* n_prompt_dev, int32_t* out_tokens_dev) {
    if (!out_tokens_dev || !rules_host || !ngram_host) return e ? e->fail(DOTS_E_INVALID, "bad select_tokens arguments") : DOTS_E_INVALID;
    return select_op(e, logits_dev, B, V, params_host, hist_dev, hist_lens_dev, hist_stride, n_prompt_dev, out_tokens_dev, 2, 0, nullptr, rules_host, nullptr,
                     nullptr, nullptr, nullptr, ngram_host);
}

int dots_bench_select_tokens_ngram(DotsEngine* e, const float* logits_dev, int B, int V, const DotsSamplingParams* params_host, const DotsLogitRules* rules_host,
                                   const DotsNgramRule* ngram_host, const int32_t* hist_dev, const int32_t* hist_lens_dev, int hist_stride,
                                   const int32_t* n_prompt_dev, int iters, float* ms_out) {
    if (!ms_out || iters < 1 || !rules_host || !ngram_host) return e ? e->fail(DOTS_E_INVALID, "bad bench_select_tokens arguments") : DOTS_E_INVALID;
    return select_op(e, logits_dev, B, V, params_host, hist_dev, hist_lens_dev, hist_stride, n_prompt_dev, nullptr, 2, iters, ms_out, rules_host, nullptr,
                     nullptr, nullptr, nullptr, ngram_host);
}

int dots_op_ngram_draft(DotsEngine* e, const int32_t* hist_dev, const int32_t* hist_lens_dev, int hist_stride, int B, int k, int min_n, int max_n,
                        int32_t* drafts_dev, int32_t* n_drafts_dev) {
    if (!e || !hist_dev || !hist_lens_dev || !drafts_dev || !n_drafts_dev) return e ? e->fail(DOTS_E_INVALID, "null argument") : DOTS_E_INVALID;
    if (B < 1 || B > DOTS_MAX_BATCH || hist_stride < 1 || k < 1 || k > DOTS_MAX_SPEC_DRAFTS || min_n < 1 || max_n < min_n || max_n > DOTS_MAX_NGRAM_SIZE)
        return e->fail(DOTS_E_INVALID, "ngram_draft: B in [1, %d], k in [1, %d], 1 <= min_n <= max_n <= %d", DOTS_MAX_BATCH, DOTS_MAX_SPEC_DRAFTS, DOTS_MAX_NGRAM_SIZE);
    CK(hipSetDevice(e->device));
    CK(launch_ngram_draft(e->stream, hist_dev, hist_lens_dev, hist_stride, nullptr, nullptr, nullptr, 1, B, k, min_n, max_n, drafts_dev, k, n_drafts_dev));
    CK(hipStreamSynchronize(e->stream));
    return DOTS_OK;
}

int dots_op_predict_draft(DotsEngine* e, const int32_t* pred_dev, const int32_t* pred_lens_dev, int pred_stride, const int32_t* hist_dev,
                          const int32_t* hist_lens_dev, int hist_stride, int B, int k, int min_n, int max_n, int32_t* cur_dev, int32_t* at_dev,
                          int32_t* drafts_dev, int32_t* n_drafts_dev, int32_t* src_dev) {
    if (!e || !pred_dev || !pred_lens_dev || !hist_dev || !hist_lens_dev || !cur_dev || !at_dev || !drafts_dev || !n_drafts_dev || !src_dev)
        return e ? e->fail(DOTS_E_INVALID, "null argument") : DOTS_E_INVALID;
    if (B < 1 || B > DOTS_MAX_BATCH || pred_stride < 1 || hist_stride < 1 || k < 1 || k > DOTS_MAX_SPEC_DRAFTS || min_n < 1 || max_n < min_n ||
        max_n > DOTS_MAX_NGRAM_SIZE)
        return e->fail(DOTS_E_INVALID, "predict_draft: B in [1, %d], k in [1, %d], 1 <= min_n <= max_n <= %d", DOTS_MAX_BATCH, DOTS_MAX_SPEC_DRAFTS, DOTS_MAX_NGRAM_SIZE);
    CK(hipSetDevice(e->device));
    const PredictState p{pred_dev, const_cast<int32_t*>(pred_lens_dev), cur_dev, at_dev, src_dev, pred_stride, nullptr, nullptr};      // the drafter reads len only
    CK(launch_predict_draft(e->stream, p, hist_dev, hist_lens_dev, hist_stride, nullptr, nullptr, nullptr, 1, B, k, min_n, max_n, drafts_dev, k, n_drafts_dev, nullptr));
    CK(hipStreamSynchronize(e->stream));
    return DOTS_OK;
}

int dots_op_spec_guide_masks(DotsEngine* e, int rows, int k, const int32_t* guide_ids_host, const int32_t* states_host, const int32_t* drafts_host,
                             const int32_t* n_live_host, int32_t* states_out_host, uint32_t* mask_out_host) {
    if (!e || !guide_ids_host || !states_host || !drafts_host || !n_live_host || !states_out_host || !mask_out_host)
        return e ? e->fail(DOTS_E_INVALID, "null argument") : DOTS_E_INVALID;
    if (rows < 1 || k < 1 || k > DOTS_MAX_SPEC_DRAFTS || rows * (k + 1) > DOTS_MAX_BATCH)
        return e->fail(DOTS_E_INVALID, "spec_guide_masks: rows >= 1, k in [1, %d], rows x (k + 1) <= %d", DOTS_MAX_SPEC_DRAFTS, DOTS_MAX_BATCH);
    if (!e->tok_off) return e->fail(DOTS_E_STATE, "the token bytes are not set (dots_set_token_bytes): a guide cannot judge any token");
    const int V = e->cfg.vocab_size, R = rows * (k + 1), words = guide_mask_words(V);
    std::vector<RowGuide> tab(DOTS_MAX_BATCH, RowGuide{});
    std::vector<int32_t> drafts((size_t)DOTS_MAX_BATCH * DOTS_MAX_SPEC_DRAFTS, 0);
    for (int b = 0; b < rows; ++b) {
        for (int j = 0; j < k; ++j) {
            const int t = drafts_host[b * k + j];
            if (t < 0 || t >= V) return e->fail(DOTS_E_INVALID, "row %d: draft id %d out of range [0, %d)", b, t, V);
            drafts[(size_t)b * DOTS_MAX_SPEC_DRAFTS + j] = t;
        }
        const int id = guide_ids_host[b];
        if (id < 0) continue;
        if (id >= (int)e->guides.size() || !e->guides[id].table) return e->fail(DOTS_E_INVALID, "row %d: no guide %d", b, id);
        const DotsEngine::Guide& g = e->guides[id];
        if (states_host[b] < 0 || states_host[b] >= g.n_states) return e->fail(DOTS_E_INVALID, "row %d: state %d outside [0, %d)", b, states_host[b], g.n_states);
        tab[b] = RowGuide{g.table, g.accepting, g.n_states, g.start, states_host[b], 0};
    }
    CK(hipSetDevice(e->device));
    Scratch sc(e);
    RowGuide* gtab = nullptr;
    uint32_t* gmask = nullptr;
    int32_t *d_drafts = nullptr, *d_live = nullptr, *d_state = nullptr;
    CK(sc.get(&gtab, DOTS_MAX_BATCH));
    CK(sc.get(&gmask, (size_t)R * words));                 // zeroed: a row the kernels leave alone reads as "nothing allowed"
    CK(sc.get(&d_drafts, drafts.size()));
    CK(sc.get(&d_live, DOTS_MAX_BATCH));
    CK(sc.get(&d_state, DOTS_MAX_BATCH));
    CK(hipMemcpyAsync(gtab, tab.data(), DOTS_MAX_BATCH * sizeof(RowGuide), hipMemcpyHostToDevice, e->stream));
    CK(hipMemcpyAsync(d_drafts, drafts.data(), drafts.size() * 4, hipMemcpyHostToDevice, e->stream));
    CK(hipMemcpyAsync(d_live, n_live_host, (size_t)rows * 4, hipMemcpyHostToDevice, e->stream));
    CK(hipMemsetAsync(d_state, 0xFF, DOTS_MAX_BATCH * 4, e->stream));
    SpecState sp{};
    sp.drafts = d_drafts; sp.n_live = d_live; sp.gstate = d_state; sp.k = k;
    const GuideSel g{gtab, gmask, e->tok_off, e->tok_bytes, words, V};
    CK(launch_spec_guide_chain(e->stream, sp, g, e->eos_ids, e->n_eos, rows));
    CK(launch_guide_mask_drafts(e->stream, g, rows, k, d_state));
    CK(hipMemcpyAsync(states_out_host, d_state, (size_t)R * 4, hipMemcpyDeviceToHost, e->stream));
    CK(hipMemcpyAsync(mask_out_host, gmask, (size_t)R * words * 4, hipMemcpyDeviceToHost, e->stream));
    CK(hipStreamSynchronize(e->stream));                   // the host vectors above are free again, the outputs are there
    return DOTS_OK;
}

int dots_op_logprobs(DotsEngine* e, const float* logits_dev, int B, int V, int ld, const int32_t* top_n_host, const int32_t* chosen_dev,
                     float* tok_lp_dev, int32_t* top_ids_dev, float* top_lp_dev) {
    if (!chosen_dev || !tok_lp_dev || !top_ids_dev || !top_lp_dev) return e ? e->fail(DOTS_E_INVALID, "bad logprobs arguments") : DOTS_E_INVALID;
    return logprobs_op(e, logits_dev, B, V, ld, top_n_host, chosen_dev, tok_lp_dev, top_ids_dev, top_lp_dev, 0, 0, nullptr);
}

int dots_bench_logprobs(DotsEngine* e, const float* logits_dev, int B, int V, int ld, const int32_t* top_n_host, int which, int iters,
                        float* ms_out) {
    if (!ms_out || iters < 1) return e ? e->fail(DOTS_E_INVALID, "bad bench_logprobs arguments") : DOTS_E_INVALID;
    return logprobs_op(e, logits_dev, B, V, ld, top_n_host, nullptr, nullptr, nullptr, nullptr, which, iters, ms_out);
}

}  // extern "C"
