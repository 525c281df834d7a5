// Host orchestration + C ABI of the dots.ocr engine (include/dots_ocr_hip.h).
//
// One DotsEngine = one GPU = one HIP stream.  It owns the bf16 weights (packed once at
// dots_finalize_weights), the ViT / prefill workspaces, the paged KV pool and the decode buffers.
// The decode step is captured once per dots_generate call into a hipGraph and replayed: every
// per-step quantity (token ids, context lengths, block tables) lives in device memory and is read
// through pointers, so the graph never needs parameter updates (SURVEY §7 "hard parts").
#include "engine.h"

namespace engine {
namespace {
thread_local std::string g_create_error;

// One dense layer of ViT / prefill: bf16 MFMA GEMM, or in fp8 mode per-token activation quantisation + the fp8 MFMA GEMM.
int dense_on(DotsEngine* e, hipStream_t st, uint8_t* aq, float* as, const bf16_t* A, const bf16_t* W, const uint8_t* W8, const float* wscale,
             const bf16_t* bias, const bf16_t* R, void* C, int64_t M, int N, int K, int ldc, int epi) {
    if (!W8) {
        CK(launch_gemm(st, A, W, bias, R, C, M, N, K, K, ldc, epi, wscale));
        return DOTS_OK;
    }
    CK(launch_quant_act_fp8(st, A, aq, as, M, K, K));
    CK(launch_gemm_fp8(st, aq, as, W8, wscale, bias, R, C, M, N, K, ldc, epi));
    return DOTS_OK;
}
// LM prefill: the engine's main stream
int dense(DotsEngine* e, const bf16_t* A, const bf16_t* W, const uint8_t* W8, const float* wscale, const bf16_t* bias, const bf16_t* R, void* C,
          int64_t M, int N, int K, int ldc, int epi) {
    return dense_on(e, e->stream, e->act_q, e->act_s, A, W, W8, wscale, bias, R, C, M, N, K, ldc, epi);
}
// vision tower: whichever stream vit_forward runs on, its own scratch
int vdense(DotsEngine* e, const bf16_t* A, const bf16_t* W, const uint8_t* W8, const float* wscale, const bf16_t* bias, const bf16_t* R, void* C,
           int64_t M, int N, int K, int ldc, int epi) {
    return dense_on(e, e->vs, e->act_q_v, e->act_s_v, A, W, W8, wscale, bias, R, C, M, N, K, ldc, epi);
}

// qkv projection + rope + head-major split of a prefill pass (ViT block / LM layer).  bf16 weights on the one-wave-per-SIMD GEMM: the q / k heads
// leave the GEMM rotated and head-major (launch_gemm_qk_rope), the split kernel only transposes v; anything else: the two kernels of rounds 1-5.
// Same bits either way (tests/test_kernels_gpu.py).  `st` / scratch as dense_on.
int qkv_rope_on(DotsEngine* e, hipStream_t st, uint8_t* aq, float* as, const bf16_t* A, const bf16_t* W, const uint8_t* W8, const float* wscale, const bf16_t* bias,
                bf16_t* qkv, const float2* cs, const Tile64* tiles, int n_tiles, bf16_t* q, bf16_t* k, bf16_t* vt, int64_t T, int64_t Tpad, int K, int Hq, int Hkv) {
    const int N = (Hq + 2 * Hkv) * 128;
    if (!W8 && !wscale) {
        const hipError_t r = launch_gemm_qk_rope(st, A, W, bias, qkv, T, N, K, K, N, cs, q, k, Hq, Hkv);
        if (r == hipSuccess) {
            CK(launch_qkv_rope_split(st, qkv, cs, tiles, n_tiles, q, k, vt, T, Tpad, Hq, Hkv, true));
            return DOTS_OK;
        }
        if (r != hipErrorNotSupported) CK(r);
    }
    RET(dense_on(e, st, aq, as, A, W, W8, wscale, bias, nullptr, qkv, T, N, K, N, EPI_NONE));
    CK(launch_qkv_rope_split(st, qkv, cs, tiles, n_tiles, q, k, vt, T, Tpad, Hq, Hkv));
    return DOTS_OK;
}

// this layer's fp8-KV scales [Hkv][2] for the pool launchers, or nullptr for a bf16 pool
const float* layer_kv_scales(const DotsEngine* e, int layer) {
    return e->kv8 ? e->kv_scales + (size_t)layer * e->cfg.num_kv_heads * 2 : nullptr;
}

hipError_t attn_event(DotsEngine* e, int idx) {
    while ((int)e->attn_ev.size() <= idx) {
        hipEvent_t ev;
        hipError_t r = hipEventCreate(&ev);
        if (r != hipSuccess) return r;
        e->attn_ev.push_back(ev);
    }
    return hipEventRecord(e->attn_ev[idx], e->vs);
}

// Runs on e->vs (the main stream, or s_vit for a prefetch); the merged rows go to `vis_out`.
// Everything vit_forward can refuse, checked without touching the device: a prefetch whose launch is deferred behind a prefill
// (dots_vit_prefetch, after_prefill) is validated when it is REQUESTED, so that it cannot fail inside that prefill after the slots
// have been marked occupied.
int check_vision_request(DotsEngine* e, int64_t N, const int64_t* grid, int n_img) {
    const DotsConfig& c = e->cfg;
    const int m = c.v_merge;
    if (N > e->P) return e->fail(DOTS_E_CAPACITY, "total_patches %lld > max_patches %lld", (long long)N, (long long)e->P);
    if (c.v_temporal_patch != 1) return e->fail(DOTS_E_INVALID, "temporal_patch_size != 1 is not supported");
    int64_t off = 0, n_seq = 0;
    for (int i = 0; i < n_img; ++i) {
        const int64_t t = grid[i * 3], h = grid[i * 3 + 1], w = grid[i * 3 + 2];
        if (t < 1 || h < 1 || w < 1 || h % m || w % m) return e->fail(DOTS_E_INVALID, "grid_thw[%d] not divisible by merge size", i);
        if (t * h * w > N - off) return e->fail(DOTS_E_INVALID, "grid_thw does not match total_patches");
        off += t * h * w;
        n_seq += t;
    }
    if (off != N) return e->fail(DOTS_E_INVALID, "grid_thw covers %lld patches, total_patches is %lld", (long long)off, (long long)N);
    if (n_seq > 256) return e->fail(DOTS_E_CAPACITY, "more than 256 images per call");
    return DOTS_OK;
}

int vit_forward(DotsEngine* e, const float* pix_dev, int64_t N, const int64_t* grid, int n_img, void* out_dev, bf16_t* vis_out, int64_t* rows_out) {
    const DotsConfig& c = e->cfg;
    hipStream_t s = e->vs;
    const int E = c.v_embed_dim, Hh = c.v_heads, m = c.v_merge;
    RET(check_vision_request(e, N, grid, n_img));
    // ---- host: position ids (block-major over merge x merge groups), sequences
    e->h_pos.resize((size_t)N * 2);
    std::vector<int> lens;
    int64_t off = 0;
    double attn_flops = 0;
    for (int i = 0; i < n_img; ++i) {
        const int64_t t = grid[i * 3], h = grid[i * 3 + 1], w = grid[i * 3 + 2];
        if (h % m || w % m || t < 1) return e->fail(DOTS_E_INVALID, "grid_thw[%d] not divisible by merge size", i);
        if (off + t * h * w > N) return e->fail(DOTS_E_INVALID, "grid_thw does not match total_patches");
        for (int64_t tt = 0; tt < t; ++tt) {
            for (int64_t gh = 0; gh < h / m; ++gh)
                for (int64_t gw = 0; gw < w / m; ++gw)
                    for (int mh = 0; mh < m; ++mh)
                        for (int mw = 0; mw < m; ++mw) {
                            e->h_pos[off * 2] = (int32_t)(gh * m + mh);
                            e->h_pos[off * 2 + 1] = (int32_t)(gw * m + mw);
                            ++off;
                        }
            lens.push_back((int)(h * w));
            attn_flops += 4.0 * (double)(h * w) * (double)(h * w) * E;
        }
    }
    if (off != N) return e->fail(DOTS_E_INVALID, "grid_thw covers %lld patches, total_patches is %lld", (long long)off, (long long)N);
    if (lens.size() > 256) return e->fail(DOTS_E_CAPACITY, "more than 256 images per call");
    int64_t Tpad = 0;
    build_worklists(lens, Hh, e->h_tiles, e->h_qblocks, &Tpad);
    CK(hipMemcpyAsync(e->v_pos, e->h_pos.data(), e->h_pos.size() * 4, hipMemcpyHostToDevice, s));
    CK(hipMemcpyAsync(e->v_tiles, e->h_tiles.data(), e->h_tiles.size() * sizeof(Tile64), hipMemcpyHostToDevice, s));
    CK(hipMemcpyAsync(e->v_qblocks, e->h_qblocks.data(), e->h_qblocks.size() * sizeof(QBlock), hipMemcpyHostToDevice, s));

    CK(hipEventRecord(e->ev[0], s));
    CK(launch_patch_prep(s, pix_dev, e->v_xa, N, e->patch_k, e->patch_kpad));
    CK(launch_gemm(s, e->v_xa, e->patch_w, e->patch_b, nullptr, e->v_xn, N, E, e->patch_kpad, e->patch_kpad, E, EPI_NONE));
    CK(launch_rmsnorm(s, e->v_xn, e->patch_norm, e->v_x, N, E, c.v_rms_eps));
    CK(launch_rope_table(s, e->v_pos, e->v_inv_freq, e->v_cs, N, 1));
    const float scale = 1.0f / sqrtf(128.0f);
    e->attn_pairs = 0;
    const XcdPlan xcd_plan = make_xcd_plan(e->h_qblocks.data(), (int)e->h_qblocks.size());      // the XCDs' chunks of the attention work list, cut by cost
    // a prefetched tower: its last e->tail_now blocks and the merger run on the unmasked stream (DotsEngine::s_vit_full)
    hipStream_t const s_first = s;
    const bool prefetched = e->s_vit && s == e->s_vit && e->s_vit_full;
    const int switch_at = prefetched ? c.v_layers - std::max(0, std::min(e->tail_now, c.v_layers - 1)) : -1;
    if (prefetched) CK(hipEventRecord(e->ev_tw0, s));
    for (int i = 0; i < c.v_layers; ++i) {
        const VLayer& L = e->vl[i];
        if (i == switch_at) {
            CK(hipEventRecord(e->ev_tw_sw, s));
            e->tail_head_blocks = i;
            RET(chain_streams(e, s, e->s_vit_full));
            e->vs = s = e->s_vit_full;
        }
        CK(launch_rmsnorm(s, e->v_x, L.norm1, e->v_xn, N, E, c.v_rms_eps));
        RET(qkv_rope_on(e, s, e->act_q_v, e->act_s_v, e->v_xn, L.qkv_w, L.qkv_8, L.qkv_s, L.qkv_b, e->v_qkv, e->v_cs, e->v_tiles, (int)e->h_tiles.size(), e->v_q, e->v_k, e->v_vt,
                        N, Tpad, E, Hh, Hh));
        CK(attn_event(e, 2 * i));
        CK(launch_flash_attn(s, e->v_q, e->v_k, e->v_vt, e->v_att, e->v_qblocks, (int)e->h_qblocks.size(), N, Tpad, Hh, Hh, 0, scale, &xcd_plan));
        CK(attn_event(e, 2 * i + 1));
        e->attn_pairs = i + 1;
        RET(vdense(e, e->v_att, L.proj_w, L.proj_8, L.proj_s, L.proj_b, e->v_x, e->v_x, N, E, E, E, EPI_RESIDUAL));
        CK(launch_rmsnorm(s, e->v_x, L.norm2, e->v_xn, N, E, c.v_rms_eps));
        RET(vdense(e, e->v_xn, L.w13, L.w13_8, L.w13_s, L.b13, nullptr, e->v_act, N, 2 * c.v_intermediate, E, c.v_intermediate, EPI_SWIGLU));
        RET(vdense(e, e->v_act, L.w2, L.w2_8, L.w2_s, L.b2, e->v_x, e->v_x, N, E, c.v_intermediate, E, EPI_RESIDUAL));
        if (e->dbg_hidden && (size_t)(i + 1) * N * E <= e->dbg_cap) {
            CK(hipMemcpyAsync(e->dbg_hidden + (size_t)i * N * E, e->v_x, (size_t)N * E * 2, hipMemcpyDeviceToDevice, s));
            e->dbg_vit_rows = N;
        }
    }
    if (prefetched && switch_at == c.v_layers) {         // tail 0: the whole tower ran on the partition
        CK(hipEventRecord(e->ev_tw_sw, s));
        e->tail_head_blocks = c.v_layers;
    }
    const bf16_t* xin = e->v_x;
    if (c.v_post_norm) {
        CK(launch_rmsnorm(s, e->v_x, e->v_post_norm, e->v_xn, N, E, c.v_rms_eps));
        xin = e->v_xn;
    }
    CK(launch_layernorm(s, xin, e->m_ln_w, e->m_ln_b, e->v_att, N, E, c.v_ln_eps));
    const int g = m * m, Mg = E * g;
    const int64_t R = N / g;
    RET(vdense(e, e->v_att, e->m0_w, e->m0_8, e->m0_s, e->m0_b, nullptr, e->v_mh, R, Mg, Mg, Mg, EPI_GELU));
    RET(vdense(e, e->v_mh, e->m2_w, e->m2_8, e->m2_s, e->m2_b, nullptr, vis_out, R, c.hidden_size, Mg, c.hidden_size, EPI_NONE));
    if (s != s_first) {                                  // back to the stream the caller orders things on
        RET(chain_streams(e, s, s_first));
        e->vs = s = s_first;
    }
    CK(hipEventRecord(e->ev[1], s));
    *rows_out = R;
    if (out_dev) CK(hipMemcpyAsync(out_dev, vis_out, (size_t)R * c.hidden_size * 2, hipMemcpyDeviceToDevice, s));

    // algorithmic flops
    e->stats.vit_patches = N;
    e->stats.vit_attn_flops = attn_flops * c.v_layers;
    e->stats.vit_flops = e->stats.vit_attn_flops +
                         (double)c.v_layers * 2.0 * N * (4.0 * E * E + 3.0 * E * c.v_intermediate) +
                         2.0 * N * e->patch_k * E + 2.0 * (double)R * ((double)Mg * Mg + (double)Mg * c.hidden_size);
    return DOTS_OK;
}

// CU-masked side streams of the vision prefetch, created on first use.  Mask bit i = CU i / 8 of XCD i % 8 (profiles/r01_probe_cu_mask.txt):
// bits [0, dec_cus) for the decode loop, [dec_cus, 256) for the tower — each an equal share of every XCD.
int ensure_overlap_streams(DotsEngine* e) {
    if (e->s_vit) return DOTS_OK;
    if (const char* v = sw::read_now(sw::OVERLAP_DEC_CUS)) e->dec_cus = sw::parse_overlap_dec_cus(v);      // per engine, here: bench.py sets it between engines
    uint32_t wd[8] = {0}, wv[8] = {0};
    // DOTS_OCR_OVERLAP_BY_XCD=1 (experiment): whole XCDs instead of an equal share of every XCD — the decode loop gets XCDs 0 .. dec_cus / 32 - 1
    const bool by_xcd = launch_switches().overlap_by_xcd;
    for (int b = 0; b < 256; ++b) ((by_xcd ? (b % 8) < e->dec_cus / 32 : b < e->dec_cus) ? wd : wv)[b / 32] |= 1u << (b % 32);
    // A device that refuses CU masks (another compute-partition mode, fewer CUs) still gets correct results: plain streams then
    // time-slice the chip, i.e. the prefetch degenerates to the sequential schedule.
    if (hipExtStreamCreateWithCUMask(&e->s_dec, 8, wd) != hipSuccess || hipExtStreamCreateWithCUMask(&e->s_vit, 8, wv) != hipSuccess) {
        (void)hipGetLastError();
        if (e->s_dec) { hipStreamDestroy(e->s_dec); e->s_dec = nullptr; }
        fprintf(stderr, "[dots_ocr_hip] CU-masked streams are not available on this device: vision prefetch runs without CU partitioning\n");
        CK(hipStreamCreateWithFlags(&e->s_dec, hipStreamNonBlocking));
        CK(hipStreamCreateWithFlags(&e->s_vit, hipStreamNonBlocking));
    }
    CK(hipEventCreateWithFlags(&e->ev_vis_ready, hipEventDisableTiming));
    CK(hipEventCreateWithFlags(&e->ev_xs, hipEventDisableTiming));
    CK(hipStreamCreateWithFlags(&e->s_vit_full, hipStreamNonBlocking));
    CK(hipEventCreate(&e->ev_tw0));
    CK(hipEventCreate(&e->ev_tw_sw));
    CK(hipEventCreate(&e->ev_dec_end));
    return DOTS_OK;
}

// blocks of the next prefetched tower that run on the whole chip (see DotsEngine::s_vit_full)
int pick_tower_tail(DotsEngine* e) {
    const int L = e->cfg.v_layers;
    if (e->tail_fixed >= 0) return std::min(e->tail_fixed, L - 1);
    if (e->tail_head_blocks <= 0 || e->dec_end_seq <= e->dec_end_at_tw) return e->tail_now;      // nothing measured since the last tower started
    float head_ms = 0.f, d_ms = 0.f;
    if (hipEventElapsedTime(&head_ms, e->ev_tw0, e->ev_tw_sw) != hipSuccess || hipEventElapsedTime(&d_ms, e->ev_tw0, e->ev_dec_end) != hipSuccess) {
        (void)hipGetLastError();                         // not finished / not comparable: keep the current split
        return e->tail_now;
    }
    if (head_ms <= 0.f) return e->tail_now;
    const float t_block = head_ms / (float)e->tail_head_blocks;
    const int tail = d_ms <= 0.f ? L / 2 : (int)floorf((float)L - d_ms / t_block);
    return std::max(0, std::min(tail, L / 2));
}

int stage_pixels(DotsEngine* e, hipStream_t st, const float* pixel_values, int on_device, int64_t total_patches, const float** pix) {
    *pix = pixel_values;
    if (!on_device) {
        if (total_patches > e->P) return e->fail(DOTS_E_CAPACITY, "total_patches exceeds max_patches");
        if (!e->v_pix) CK(e->alloc(&e->v_pix, (size_t)e->P * e->patch_k));
        CK(hipMemcpyAsync(e->v_pix, pixel_values, (size_t)total_patches * e->patch_k * 4, hipMemcpyHostToDevice, st));
        *pix = e->v_pix;
    }
    return DOTS_OK;
}

// the tower of the prefetch request, on the side stream, behind everything the main stream holds so far
int launch_prefetched_tower(DotsEngine* e) {
    e->pref_deferred = false;
    e->tail_now = pick_tower_tail(e);
    e->dec_end_at_tw = e->dec_end_seq;
    ++e->tw_seq;
    RET(chain_streams(e, e->stream, e->s_vit));          // the pixels (dots_preprocess_image), an earlier tower pass, the prefill it was deferred behind
    e->vs = e->s_vit;
    int r = vit_forward(e, e->pref_pix, e->pref_patches, e->pref_grid.data(), (int)(e->pref_grid.size() / 3), nullptr, e->vis_pref, &e->vis_pref_rows);
    e->vs = e->stream;
    // a tower that failed AFTER switching to the unmasked tail stream returned without chaining it back: whatever it queued on
    // s_vit_full must still be covered by the event below, which the next tower / dots_vit_forward wait on before reusing v_x / v_qkv.
    // (After a complete tower this is one more event pair on already-ordered streams.)
    if (e->s_vit_full) {
        const int rc = chain_streams(e, e->s_vit_full, e->s_vit);
        if (r == DOTS_OK) r = rc;
    }
    CK(hipEventRecord(e->ev_vis_ready, e->s_vit));
    if (r != DOTS_OK) e->pref_pending = false;           // nothing to take
    return r;
}

// everything a captured step bakes in, from the engine's state as it stands (DotsEngine::StepKey)
DotsEngine::StepKey step_key(const DotsEngine* e, int rows, int n_splits, int out_cap, int part) {
    DotsEngine::StepKey k;
    k.rows = rows; k.splits = n_splits; k.out_cap = out_cap; k.n_eos = e->n_eos; k.part = part;
    k.rowp = e->stage.staged_rows() > 0;
    k.lp = e->n_lp > 0;
    k.rules = e->stage.rows(ROW_RULES) > 0;
    k.guided = e->stage.rows(ROW_GUIDE) > 0;
    k.ngram = e->stage.rows(ROW_NGRAM) > 0;
    k.spec = e->slot_mode ? e->spec_k : 0;
    k.draw = spec_draws(e);
    k.gspec = spec_guides(e);
    k.sspec = spec_shapes(e);
    k.lpspec = spec_lps(e);
    k.beam = e->slot_mode ? e->n_beam_hi : 0;
    k.share = out_cap == 0 ? share_plan_now(e).cap : 0;
    k.pred = spec_predicts(e);
    return k;
}

double decode_step_bytes(const DotsConfig& c) {
    const double H = c.hidden_size, Nq = c.num_heads * 128.0, Nkv = c.num_kv_heads * 128.0, I = c.intermediate_size;
    // every weight byte once per step.  bf16: 2 B per weight; fp8 mode: 1 B per linear weight + 4 B per output channel
    // (scale), norms and biases stay bf16
    const double lin = H * (Nq + 2 * Nkv) + Nq * H + 3 * H * I, chans = (Nq + 2 * Nkv) + H + 2 * I + H;
    const double small = 2.0 * ((c.attention_bias ? Nq + 2 * Nkv : 0) + 2 * H);
    if (c.fp8_weights) return c.num_layers * (lin + 4.0 * chans + small) + 2.0 * H + (double)c.vocab_size * (H + 4.0);
    return c.num_layers * (2.0 * lin + small) + 2.0 * H + 2.0 * (double)c.vocab_size * H;
}
}  // namespace

// sequences -> 64-token tiles and 128-row query blocks
// (Tile64.seq = the KV slot of the sequence: seq_ids[s], or s itself)
void build_worklists(const std::vector<int>& lens, int Hq, std::vector<Tile64>& tiles, std::vector<QBlock>& qblocks, int64_t* Tpad_used,
                     const int* seq_ids) {
    tiles.clear();
    qblocks.clear();
    int tok0 = 0, pad0 = 0;
    for (size_t s = 0; s < lens.size(); ++s) {
        const int n = lens[s];
        const int seq = seq_ids ? seq_ids[s] : (int)s;
        for (int t = 0; t * 64 < n; ++t) tiles.push_back(Tile64{tok0 + t * 64, std::min(64, n - t * 64), pad0 + t * 64, seq, t, 0});
        for (int h = 0; h < Hq; ++h)
            for (int q = 0; q < n; q += flash_rows_per_block()) qblocks.push_back(QBlock{q, n, tok0, pad0, h, 0});
        tok0 += n;
        pad0 += (int)round_up(n, 64);
    }
    *Tpad_used = pad0;
}

void drop_step_graphs(DotsEngine* e) {
    for (auto& g : e->step_graphs) {
        hipGraphExecDestroy(g.exec);
        hipGraphDestroy(g.graph);
    }
    e->step_graphs.clear();
}

// make `to` wait for everything enqueued on `from` so far
int chain_streams(DotsEngine* e, hipStream_t from, hipStream_t to) {
    if (from == to) return DOTS_OK;
    CK(hipEventRecord(e->ev_xs, from));
    CK(hipStreamWaitEvent(to, e->ev_xs, 0));
    return DOTS_OK;
}

// The stream the next decode chunk should be replayed on: the lower CU partition while a prefetched tower is still running (the two then
// share the chip instead of time-slicing it), the whole chip otherwise.  Hands the dependency over when the stream changes.
int pick_decode_stream(DotsEngine* e, hipStream_t* cur) {
    hipStream_t want = e->stream;
    if (e->s_vit && e->pref_pending && !e->pref_deferred && hipEventQuery(e->ev_vis_ready) == hipErrorNotReady) {
        (void)hipGetLastError();                   // "not ready" must not stay behind as the thread's last error (PyTorch / RCCL check it)
        want = e->s_dec;
    }
    if (want != *cur) {
        RET(chain_streams(e, *cur, want));
        *cur = want;
    }
    return DOTS_OK;
}

namespace {
// The Qwen2 layers of a prefill pass over the T packed rows of p_x (Tpad padded; the tiles of hp_tiles / p_tiles): K/V go to the pages that
// `table` names, attn(layer, pool_layer) launches the pass's attention into p_att.  capture: the residual stream after every layer is kept
// for dots_debug_capture_hidden
template <typename Attn>
int prefill_layers(DotsEngine* e, int64_t T, int64_t Tpad, const int32_t* table, bool capture, Attn attn) {
    const DotsConfig& c = e->cfg;
    hipStream_t s = e->stream;
    const int H = c.hidden_size, Hq = c.num_heads, Hkv = c.num_kv_heads, Nq = Hq * 128, n_tiles = (int)e->hp_tiles.size();
    for (int i = 0; i < c.num_layers; ++i) {
        const LLayer& Lw = e->ll[i];
        bf16_t* pool_l = e->pool + e->pool_layer_elems * i;
        CK(launch_rmsnorm(s, e->p_x, Lw.ln1, e->p_xn, T, H, c.rms_norm_eps));
        RET(qkv_rope_on(e, s, e->act_q, e->act_s, e->p_xn, Lw.qkv_w, Lw.qkv_8, Lw.qkv_s, Lw.qkv_b, e->p_qkv, e->p_cs, e->p_tiles, n_tiles, e->p_q, e->p_k, e->p_vt, T, Tpad, H, Hq, Hkv));
        CK(launch_kv_to_pages(s, e->p_k, e->p_qkv, e->p_tiles, n_tiles, table, e->max_pages, pool_l, T, Hq, Hkv, layer_kv_scales(e, i)));
        CK(attn(i, pool_l));
        RET(dense(e, e->p_att, Lw.o_w, Lw.o_8, Lw.o_s, nullptr, e->p_x, e->p_x, T, H, Nq, H, EPI_RESIDUAL));
        CK(launch_rmsnorm(s, e->p_x, Lw.ln2, e->p_xn, T, H, c.rms_norm_eps));
        RET(dense(e, e->p_xn, Lw.w13, Lw.w13_8, Lw.w13_s, nullptr, nullptr, e->p_act, T, 2 * c.intermediate_size, H, c.intermediate_size, EPI_SWIGLU));
        RET(dense(e, e->p_act, Lw.down_w, Lw.down_8, Lw.down_s, nullptr, e->p_x, e->p_x, T, H, c.intermediate_size, H, EPI_RESIDUAL));
        const size_t voff = (size_t)c.v_layers * e->dbg_vit_rows * c.v_embed_dim;       // LM layers are stored behind the ViT blocks
        if (capture && e->dbg_hidden && voff + (size_t)(i + 1) * T * H <= e->dbg_cap) {
            CK(hipMemcpyAsync(e->dbg_hidden + voff + (size_t)i * T * H, e->p_x, (size_t)T * H * 2, hipMemcpyDeviceToDevice, s));
            e->dbg_lm_rows = T;
        }
    }
    return DOTS_OK;
}
}  // namespace

// Prefill B packed prompts.  slots == nullptr: the static batch (sequence b -> slot b, every slot reset).
// slots != nullptr: continuous batching, sequence b goes into the free slot slots[b] with its own generation cap;
// the other slots' KV pages, contexts and outputs are not touched.
int prefill(DotsEngine* e, const int32_t* ids, const int32_t* lens, int B, const int32_t* slots, const int32_t* max_new) {
    const DotsConfig& c = e->cfg;
    hipStream_t s = e->stream;
    const int H = c.hidden_size, Hq = c.num_heads, Hkv = c.num_kv_heads, Nq = Hq * 128, Nkv = Hkv * 128, NQKV = Nq + 2 * Nkv;
    if (B < 1 || B > c.max_batch) return e->fail(DOTS_E_CAPACITY, "batch %d exceeds max_batch %d", B, c.max_batch);
    int64_t T = 0;
    std::vector<int> L(B), S(B);
    std::vector<LiveRow> live(slots ? B : 0);
    int rows = B;                                           // rows of the last-position / lm_head / selection stage
    for (int b = 0; b < B; ++b) {
        RET(check_prompt(e, b, lens[b], slots, max_new));
        L[b] = lens[b];
        T += lens[b];
        S[b] = slots ? slots[b] : b;
        if (slots) live[b] = LiveRow{S[b], L[b], max_new[b]};
    }
    if (T > e->TP) return e->fail(DOTS_E_CAPACITY, "packed prompt tokens %lld > max_prefill_tokens %lld", (long long)T, (long long)e->TP);
    e->fresh_slots.clear();                                 // the workspace of the previous prefill is about to be overwritten (dots_slots_fork)
    e->hp_pos.resize(T); e->hp_src.resize(T); e->hp_last.assign(DOTS_MAX_BATCH, 0);
    int64_t t = 0, vis_used = 0;
    for (int b = 0; b < B; t += L[b], ++b) {
        for (int i = 0; i < L[b]; ++i) e->hp_pos[t + i] = i;
        RET(map_prompt(e, ids + t, L[b], false, e->hp_src.data() + t, &vis_used));
        e->hp_last[b] = (int32_t)(t + L[b] - 1);
    }
    RET(check_vis_rows(e, vis_used));
    int64_t Tpad = 0;
    build_worklists(L, Hq, e->hp_tiles, e->hp_qblocks, &Tpad, S.data());
    CK(hipMemcpyAsync(e->p_pos, e->hp_pos.data(), T * 4, hipMemcpyHostToDevice, s));
    CK(hipMemcpyAsync(e->p_src, e->hp_src.data(), T * 4, hipMemcpyHostToDevice, s));
    CK(hipMemcpyAsync(e->p_last, e->hp_last.data(), DOTS_MAX_BATCH * 4, hipMemcpyHostToDevice, s));
    CK(hipMemcpyAsync(e->p_tiles, e->hp_tiles.data(), e->hp_tiles.size() * sizeof(Tile64), hipMemcpyHostToDevice, s));
    CK(hipMemcpyAsync(e->p_qblocks, e->hp_qblocks.data(), e->hp_qblocks.size() * sizeof(QBlock), hipMemcpyHostToDevice, s));
    // ---- KV pages: a static batch resets every slot and reserves prompt + generation cap (a closed batch: nothing competes for pages);
    // a slot prefill reserves the prompt plus KV_ADMIT_AHEAD tokens for its own sequences only — the rest is taken page by page as the
    // sequences actually grow (dots_slots_decode).  Entering slot mode returns the pages of the previous static batch first.
    if (slots && !e->slot_mode) RET(enter_slot_mode(e));
    if (!slots) {
        for (int b = 0; b < (int)e->slot_pages.size(); ++b) release_pages(e, b);
        RET(beam_clear_all(e));
    }
    {
        int need = 0;
        for (int b = 0; b < B; ++b) need += ((slots ? admit_tokens(e, L[b], max_new[b]) : std::min(L[b] + e->out_cap, c.max_seq_len)) + 63) / 64;
        ensure_free(e, need);
        if (need > (int)e->free_pages.size()) {
            const int have = free_count(e);
            if (!slots) CK(hipMemcpyAsync(e->block_table, e->hp_table.data(), e->hp_table.size() * 4, hipMemcpyHostToDevice, s));
            return e->fail(DOTS_E_CAPACITY, "KV pool exhausted: these sequences need %d pages of 64 tokens, %d of %d are free", need, have, e->n_pool_pages);
        }
        for (int b = 0; b < B; ++b) reserve_pages(e, S[b], slots ? admit_tokens(e, L[b], max_new[b]) : std::min(L[b] + e->out_cap, c.max_seq_len));
        if (!slots) CK(hipMemcpyAsync(e->block_table, e->hp_table.data(), e->hp_table.size() * 4, hipMemcpyHostToDevice, s));
        else for (int b = 0; b < B; ++b) CK(upload_table_row(e, S[b]));
    }
    // from here on a failed launch must give the pages back
    PageGuard page_guard{e, S.data(), B, true, slots != nullptr};
    if (!slots) {
        e->slot_mode = false;
        std::fill(e->slot_active, e->slot_active + DOTS_MAX_BATCH, 0);
        CK(hipMemcpyAsync(e->ctx_len, lens, B * 4, hipMemcpyHostToDevice, s));
        CK(hipMemsetAsync(e->out_lens, 0, c.max_batch * 4, s));
        CK(hipMemsetAsync(e->finished, 0, c.max_batch * 4, s));
        for (int b = 0; b < B; ++b) RET(clear_lp_row(e, b));           // logprob positions of the prefilled rows: NaN / -1 until written
    } else {
        // written ahead of the layer loop: only the selection stage below and the step after it read the rows' state
        RET(rows_go_live(e, live));
        RET(stage_new_rows(e, live, e->p_dst, &rows));
    }
    const int32_t* d_rows = slots ? e->p_dst : nullptr;     // the rows of the prompts, in order (static batch: rows [0, B))
    CK(hipEventRecord(e->ev[2], s));
    CK(launch_embed_gather(s, e->p_src, e->embed, e->vis, e->p_x, T, H));
    CK(launch_rope_table(s, e->p_pos, e->lm_inv_freq, e->p_cs, T, 0));
    RET(prefill_layers(e, T, Tpad, e->block_table, true, [&](int, bf16_t*) {
        return launch_flash_attn(s, e->p_q, e->p_k, e->p_vt, e->p_att, e->p_qblocks, (int)e->hp_qblocks.size(), T, Tpad, Hq, Hkv, 1, 1.0f / sqrtf(128.0f));
    }));
    // prompt-presence bits (repetition penalty) of the prefilled rows, once any row has used a penalty
    if (e->pen_cnt) CK(launch_pen_prompt(s, e->p_src, e->p_last, d_rows, B, c.image_token_id, c.vocab_size, e->pen_cnt, e->pen_seen));
    RET(restart_automata(e, d_rows, B));
    // last position of every sequence -> final norm -> lm_head -> first token
    CK(launch_gather_rows(s, e->p_x, e->p_last, d_rows, e->d_h, B, H));
    RET(select_first_tokens(e, rows, e->d_h));
    CK(hipEventRecord(e->ev[3], s));
    if (slots) {
        mark_live(e, live.data(), B);
        e->fresh_slots = S;                                // these sequences may be forked until the next step (dots_slots_fork)
        e->fresh_chunked = false;
    } else {
        e->B = B;
        e->h_prompt_lens = L;
    }
    page_guard.armed = false;
    if (e->pref_deferred) RET(launch_prefetched_tower(e));          // the next batch's tower starts behind this prefill (dots_vit_prefetch, after_prefill)
    e->steps_done = 0;
    e->vis_rows = 0;
    e->stats.prefill_tokens = T;
    double pf = 0;
    const double lin = (double)c.num_layers * ((double)H * NQKV + (double)Nq * H + 3.0 * H * c.intermediate_size);
    for (int b = 0; b < B; ++b) pf += 2.0 * lin * L[b] + (double)c.num_layers * 2.0 * L[b] * (double)L[b] * Nq + 2.0 * (double)c.vocab_size * H;
    e->stats.prefill_flops = pf;
    return DOTS_OK;
}

// ---- chunked prefill: the same prompts filled in passes of at most max_tokens positions over their own KV pages.
// begin: validates as prefill() does — except that the packed length is bounded by the pool only, not by the workspace — reserves the
// pages, embeds every prompt whole into the staging buffer (the tower's rows are consumed here) and leaves the slots FILLING.
// With leases / keys (dots_slots_prefill_begin_cached) a prompt that holds a lease names the lease's pages in the first
// entries of its table row, reserves and embeds the rest only, and starts with its cursor behind them; a lease stays the caller's until
// the call has succeeded.
int prefill_begin(DotsEngine* e, const int32_t* ids, const int32_t* lens, int B, const int32_t* slots, const int32_t* max_new, const int32_t* leases,
                  const uint8_t* const* keys) {
    const DotsConfig& c = e->cfg;
    hipStream_t s = e->stream;
    const int H = c.hidden_size;
    const bool cached = leases != nullptr;
    if (cached && !e->pc) return e->fail(DOTS_E_STATE, "the prefix cache is off (dots_prefix_cache_enable)");
    if (e->spec_k) return e->fail(DOTS_E_STATE, "a chunked prefill cannot begin while the engine speculates (dots_set_speculation), as a slot cannot be extended or suspended then");
    if (e->TP < 64) return e->fail(DOTS_E_CAPACITY, "a chunked prefill needs max_prefill_tokens >= 64, it is %lld", (long long)e->TP);
    if (B < 1 || B > c.max_batch) return e->fail(DOTS_E_CAPACITY, "batch %d exceeds max_batch %d", B, c.max_batch);
    for (int b = 0; b < B; ++b) RET(check_prompt(e, b, lens[b], slots, max_new));
    const std::vector<int> L(lens, lens + B), S(slots, slots + B);
    // a leased prompt: hit[b] positions are in the lease's pages; one whose lease needs no tower takes no rows of `vis`
    std::vector<const prefix_cache::Lease*> lease(B, nullptr);
    std::vector<int> hit(B, 0);
    for (int b = 0, t0 = 0; cached && b < B; t0 += L[b], ++b) {
        if (!leases[b]) continue;
        lease[b] = e->pc->lease(leases[b]);
        if (!lease[b]) return e->fail(DOTS_E_INVALID, "prompt %d: lease %d is not held", b, leases[b]);
        for (int a = 0; a < b; ++a)
            if (leases[a] == leases[b]) return e->fail(DOTS_E_INVALID, "lease %d given twice", leases[b]);
        hit[b] = lease[b]->hit_tokens;
        // the lease was taken for this very prompt: the prompt's blocks find the lease's pages
        if (!e->pc->eligible(ids + t0, L[b], keys[b]) || !e->pc->matches(leases[b], ids + t0, L[b], keys[b]))
            return e->fail(DOTS_E_INVALID, "prompt %d: lease %d was not taken for this prompt", b, leases[b]);
    }
    std::vector<std::vector<int32_t>> src(B);
    int64_t vis_used = 0;
    for (int b = 0, t0 = 0; b < B; t0 += L[b], ++b) {
        src[b].resize(L[b]);
        RET(map_prompt(e, ids + t0, L[b], lease[b] && !lease[b]->needs_tower, src[b].data(), &vis_used));
    }
    RET(check_vis_rows(e, vis_used));
    if (!e->slot_mode) RET(enter_slot_mode(e));
    int need = 0;
    for (int b = 0; b < B; ++b) need += (admit_tokens(e, L[b], max_new[b]) + 63) / 64 - hit[b] / 64;
    ensure_free(e, need);
    if (need > (int)e->free_pages.size())
        return e->fail(DOTS_E_CAPACITY, "KV pool exhausted: these sequences need %d pages of 64 tokens, %d of %d are free", need, free_count(e), e->n_pool_pages);
    // the buffers of the feature, once: nothing of the slots has changed if one cannot be had
    if (!e->fill_x) CK(e->alloc(&e->fill_x, (size_t)e->n_pool_pages * 64 * H));
    if (!e->fill_rows) CK(e->alloc(&e->fill_rows, (size_t)e->TP));
    if (!e->fill_table) CK(e->alloc(&e->fill_table, (size_t)DOTS_MAX_BATCH * e->max_pages));
    if (!e->fill_items) CK(e->alloc(&e->fill_items, (size_t)(e->TP / 64 + c.max_batch + 1)));
    PageGuard guard{e, slots, B, false};
    for (int b = 0; b < B; ++b) {
        if (hit[b]) share_pages(e, S[b], lease[b]->chain.data(), hit[b] / 64);      // the cached pages: the cursor starts behind them
        bool changed = false;
        grow_pages(e, S[b], admit_tokens(e, L[b], max_new[b]), &changed);      // cannot fall short: counted above
    }
    // the device table row of a filling slot stays on the scratch page (a decode step runs its row as a free one); the passes read fill_table
    for (int b = 0; b < B; ++b)
        CK(hipMemcpyAsync(e->fill_table + (size_t)S[b] * e->max_pages, e->hp_table.data() + (size_t)S[b] * e->max_pages, (size_t)e->max_pages * 4, hipMemcpyHostToDevice, s));
    // ---- embed every prompt whole, through the workspace in pieces of at most TP rows, into the rows of its own pages
    const int piece = (int)e->TP;
    e->hp_pos.resize(piece); e->hp_src.resize(piece); e->hp_rows.resize(piece);
    for (int b = 0; b < B; ++b) {
        const auto& pages = e->slot_pages[S[b]];
        for (int p0 = hit[b]; p0 < L[b]; p0 += piece) {
            const int n = std::min(piece, L[b] - p0);
            for (int i = 0; i < n; ++i) {
                e->hp_pos[i] = i;
                e->hp_src[i] = src[b][p0 + i] == INT32_MIN ? 0 : src[b][p0 + i];      // a row the cache retains: overwritten below
                e->hp_rows[i] = pages[(p0 + i) / 64] * 64 + (p0 + i) % 64;
            }
            CK(hipMemcpyAsync(e->p_src, e->hp_src.data(), (size_t)n * 4, hipMemcpyHostToDevice, s));
            CK(hipMemcpyAsync(e->p_pos, e->hp_pos.data(), (size_t)n * 4, hipMemcpyHostToDevice, s));
            CK(hipMemcpyAsync(e->fill_rows, e->hp_rows.data(), (size_t)n * 4, hipMemcpyHostToDevice, s));
            CK(launch_embed_gather(s, e->p_src, e->embed, e->vis, e->p_x, n, H));
            CK(launch_gather_rows(s, e->p_x, e->p_pos, e->fill_rows, e->fill_x, n, H));
            CK(hipStreamSynchronize(s));                   // the host lists are reused by the next piece
        }
        // image positions behind the hit of a prompt that ran no tower: the rows the lease's tail block retains, at the same offsets of
        // its page of the staging buffer (all of them lie in the first page the slot fills: prefix_cache.h)
        int pad0 = 0, pad_n = 0;
        if (lease[b] && lease[b]->tail_page >= 0 && e->pc->tail_rows(lease[b]->tail_page, &pad0, &pad_n)) {
            for (int i = 0; i < pad_n; ++i) {
                e->hp_pos[i] = lease[b]->tail_page * 64 + pad0 + i;
                e->hp_rows[i] = pages[hit[b] / 64] * 64 + pad0 + i;
            }
            CK(hipMemcpyAsync(e->p_pos, e->hp_pos.data(), (size_t)pad_n * 4, hipMemcpyHostToDevice, s));
            CK(hipMemcpyAsync(e->fill_rows, e->hp_rows.data(), (size_t)pad_n * 4, hipMemcpyHostToDevice, s));
            CK(launch_gather_rows(s, e->fill_x, e->p_pos, e->fill_rows, e->fill_x, pad_n, H));
            CK(hipStreamSynchronize(s));
        }
    }
    e->fresh_slots.clear();                                // p_src and p_x were overwritten (dots_slots_fork)
    const int W = (c.vocab_size + 31) / 32;
    for (int b = 0; b < B; ++b) {
        DotsEngine::Fill& f = e->fill[S[b]];
        f.on = true;
        f.L = L[b]; f.max_new = max_new[b]; f.cursor = hit[b];
        f.order = ++e->fill_order;
        f.src = std::move(src[b]);
        f.seen.assign(W, 0u);
        e->n_filling += 1;
    }
    for (int b = 0, t0 = 0; cached && b < B; t0 += L[b], ++b) {
        DotsEngine::Fill& f = e->fill[S[b]];
        for (int i = 0; i < hit[b]; ++i) f.seen[ids[t0 + i] >> 5] |= 1u << (ids[t0 + i] & 31);      // the presence bits of the skipped positions
        f.cache = e->pc->eligible(ids + t0, L[b], keys[b]);
        if (!f.cache) continue;
        f.ids.assign(ids + t0, ids + t0 + L[b]);
        f.keyed = keys[b] != nullptr;
        if (keys[b]) std::memcpy(f.key, keys[b], 16);
        f.cache_parent = hit[b] ? lease[b]->chain[hit[b] / 64 - 1] : -1;
    }
    guard.armed = false;
    for (int b = 0; cached && b < B; ++b)
        if (leases[b]) e->pc->release(leases[b]);          // the slot holds the pages now
    e->vis_rows = 0;                                       // the tower's rows are in the staging buffer: `vis` is free again
    if (e->pref_deferred) RET(launch_prefetched_tower(e));
    return DOTS_OK;
}

// advance: one pass of prefill()'s layer loop over up to max_tokens positions of the filling slots, oldest begin first; every cut falls on
// a multiple of 64 positions of its sequence or at its end.  Attention reads the pages (launch_flash_attn_paged), the page just written
// included, in the first pass of a prompt too — so what a position computes does not depend on where the cuts fall.
int prefill_advance(DotsEngine* e, int max_tokens, int32_t* remaining) {
    const DotsConfig& c = e->cfg;
    hipStream_t s = e->stream;
    const int H = c.hidden_size, V = c.vocab_size;
    if (max_tokens < 64 || max_tokens % 64 || max_tokens > e->TP)
        return e->fail(DOTS_E_INVALID, "max_tokens must be a positive multiple of 64 and at most max_prefill_tokens (%lld), got %d", (long long)e->TP, max_tokens);
    auto left = [&] {
        int64_t r = 0;
        for (int b = 0; b < c.max_batch; ++b)
            if (e->fill[b].on) r += e->fill[b].L - e->fill[b].cursor;
        return (int32_t)std::min<int64_t>(r, INT32_MAX);
    };
    if (!e->slot_mode || !e->n_filling) { *remaining = 0; return DOTS_OK; }
    // ---- what this pass takes
    std::vector<int> order;
    for (int b = 0; b < c.max_batch; ++b)
        if (e->fill[b].on) order.push_back(b);
    std::sort(order.begin(), order.end(), [&](int a, int b) { return e->fill[a].order < e->fill[b].order; });
    struct Part { int slot, take, tok0; bool done; };
    std::vector<Part> parts;
    int T = 0;
    for (int b : order) {
        const DotsEngine::Fill& f = e->fill[b];
        int take = std::min(f.L - f.cursor, max_tokens - T);
        if (take < f.L - f.cursor) take = take / 64 * 64;
        if (take <= 0) break;                              // FIFO: a later fill does not overtake
        parts.push_back(Part{b, take, T, f.cursor + take == f.L});
        T += take;
    }
    e->hp_pos.resize(T); e->hp_src.resize(T); e->hp_rows.resize(T); e->hp_last.assign(DOTS_MAX_BATCH, 0);
    e->hp_tiles.clear(); e->hp_items.clear();
    std::vector<LiveRow> done;                             // the slots whose last prompt token is in this pass
    int pad0 = 0;
    for (const Part& p : parts) {
        const DotsEngine::Fill& f = e->fill[p.slot];
        const auto& pages = e->slot_pages[p.slot];
        for (int i = 0; i < p.take; ++i) {
            const int pos = f.cursor + i;
            e->hp_pos[p.tok0 + i] = pos;
            e->hp_src[p.tok0 + i] = f.src[pos];
            e->hp_rows[p.tok0 + i] = pages[pos / 64] * 64 + pos % 64;
        }
        for (int r = 0; r < p.take; r += 64) {
            const int n = std::min(64, p.take - r);
            e->hp_tiles.push_back(Tile64{p.tok0 + r, n, pad0 + r, p.slot, (f.cursor + r) / 64, 0});
            e->hp_items.push_back(PagedQBlock{p.tok0 + r, n, f.cursor + r, p.slot});
        }
        pad0 += (int)round_up(p.take, 64);
        if (p.done) {
            e->hp_last[done.size()] = p.tok0 + p.take - 1;
            done.push_back(LiveRow{p.slot, f.L, f.max_new});
        }
    }
    const int64_t Tpad = pad0;
    const int n_tiles = (int)e->hp_tiles.size(), n_done = (int)done.size();
    e->fresh_slots.clear();                                // the workspace (and, with a completed slot, the logits) are about to be overwritten
    CK(hipMemcpyAsync(e->p_pos, e->hp_pos.data(), (size_t)T * 4, hipMemcpyHostToDevice, s));
    CK(hipMemcpyAsync(e->p_src, e->hp_src.data(), (size_t)T * 4, hipMemcpyHostToDevice, s));
    CK(hipMemcpyAsync(e->fill_rows, e->hp_rows.data(), (size_t)T * 4, hipMemcpyHostToDevice, s));
    CK(hipMemcpyAsync(e->p_tiles, e->hp_tiles.data(), (size_t)n_tiles * sizeof(Tile64), hipMemcpyHostToDevice, s));
    CK(hipMemcpyAsync(e->fill_items, e->hp_items.data(), (size_t)n_tiles * sizeof(PagedQBlock), hipMemcpyHostToDevice, s));
    CK(hipEventRecord(e->ev[2], s));
    CK(launch_gather_rows(s, e->fill_x, e->fill_rows, nullptr, e->p_x, T, H));
    CK(launch_rope_table(s, e->p_pos, e->lm_inv_freq, e->p_cs, T, 0));
    RET(prefill_layers(e, T, Tpad, e->fill_table, false, [&](int layer, bf16_t* pool_l) {
        return launch_flash_attn_paged(s, e->p_q, pool_l, e->fill_table, e->max_pages, c.max_batch, e->hp_items.data(), e->fill_items, n_tiles, e->p_att, T, c.num_heads,
                                       c.num_kv_heads, 1.0f / sqrtf(128.0f), layer_kv_scales(e, layer));
    }));
    // the pass has been issued: the cursors move and the presence bits of its tokens are accumulated
    for (const Part& p : parts) {
        DotsEngine::Fill& f = e->fill[p.slot];
        for (int i = 0; i < p.take; ++i) {
            const int id = f.src[f.cursor + i] >= 0 ? f.src[f.cursor + i] : c.image_token_id;
            if (id >= 0 && id < V) f.seen[id >> 5] |= 1u << (id & 31);
        }
        // the full prompt pages this pass completed enter the prefix cache, each behind the one before it
        for (int k = f.cursor / 64; f.cache && (k + 1) * 64 <= std::min(f.cursor + p.take, f.L); ++k) {
            const int32_t page = e->slot_pages[p.slot][k];
            if (e->pc && e->pc->insert(f.cache_parent, f.ids.data(), f.L, k, f.keyed ? f.key : nullptr, page)) f.cache_parent = page;
            else f.cache = false;                          // an equal block is resident: this one and what follows it stay the slot's own
        }
        f.cursor += p.take;
    }
    if (n_done) {
        // ---- the slots whose last prompt token is in this pass complete exactly as at the end of prefill()
        const int W = (V + 31) / 32;
        for (const LiveRow& r : done) {
            CK(upload_table_row(e, r.slot));               // the row becomes a live one: its pages, its context
            if (e->pen_cnt) {                              // the one-shot image: the prompt's presence bits, no generated token counted
                CK(hipMemsetAsync(e->pen_cnt + (size_t)r.slot * V, 0, (size_t)V * 4, s));
                CK(hipMemcpyAsync(e->pen_seen + (size_t)r.slot * W, e->fill[r.slot].seen.data(), (size_t)W * 4, hipMemcpyHostToDevice, s));
            }
        }
        // behind the layer loop, which reads none of it: until here the rows ran as free ones in every step
        int rows = 0;
        RET(rows_go_live(e, done));
        RET(stage_new_rows(e, done, e->p_dst, &rows));
        CK(hipMemcpyAsync(e->p_last, e->hp_last.data(), DOTS_MAX_BATCH * 4, hipMemcpyHostToDevice, s));
        RET(restart_automata(e, e->p_dst, n_done));
        CK(launch_gather_rows(s, e->p_x, e->p_last, e->p_dst, e->d_h, n_done, H));
        RET(select_first_tokens(e, rows, e->d_h));
    }
    CK(hipEventRecord(e->ev[3], s));
    CK(hipStreamSynchronize(s));                           // the host lists and the fills' presence bits were read by asynchronous copies
    if (n_done) {
        mark_live(e, done.data(), n_done);
        e->fresh_slots.clear();
        for (const LiveRow& r : done) {
            drop_fill(e, r.slot);
            e->fresh_slots.push_back(r.slot);              // may be forked until the next step, as after a prefill
        }
        e->fresh_chunked = true;
    }
    e->steps_done = 0;
    e->stats.prefill_tokens = T;
    *remaining = left();
    return DOTS_OK;
}

void drop_fill(DotsEngine* e, int slot) {
    if (slot < 0 || slot >= DOTS_MAX_BATCH || !e->fill[slot].on) return;
    DotsEngine::Fill& f = e->fill[slot];
    f.on = false;
    f.src.clear(); f.src.shrink_to_fit();
    f.seen.clear();
    f.ids.clear(); f.ids.shrink_to_fit();
    f.cache = false;
    e->n_filling -= 1;
}

// The layers of one decode step over B rows: embedding, then every layer's launches.  tokens / ctx_len [B] and block_table [B][max_pages]
// are the slots' own arrays in a plain step and step-private ones in a speculating step and in a chunk of dots_slots_extend.  *pend: the
// last down_proj left its K-quarter sums in d_part_h for the consumer of the residual stream to apply (with *pend_scale)
int decode_layers(DotsEngine* e, const int32_t* tokens, const int32_t* ctx_len, const int32_t* block_table, int B, int n_splits, int part, bool* pend_out,
                  const float** pend_scale_out, const SharePlanDev* share) {
    const DotsConfig& c = e->cfg;
    hipStream_t s = e->stream;
    const int H = c.hidden_size, Hq = c.num_heads, Hkv = c.num_kv_heads, Nq = Hq * 128, I = c.intermediate_size;
    const float scale = 1.0f / sqrtf(128.0f);
    CK(launch_dec_embed(s, tokens, e->embed, e->d_h, B, H));
    if (e->force_part) part = 1;                                                   // dots_set_decode_plan(1): the partition plan on every step (tests, A/B runs)
    const bool same_layer = launch_switches().debug_same_layer;   // experiment: all weight reads hit the Infinity Cache
    bool pend = false;                              // down_proj of the previous layer left its K-quarter sums in d_part_h: the next norm launch applies them
    const float* pend_scale = nullptr;
    for (int i = 0; i < c.num_layers; ++i) {
        const LLayer& L = e->ll[same_layer ? 0 : i];
        bf16_t* pool_l = e->pool + e->pool_layer_elems * i;
        CK(launch_dec_qkv(s, e->d_h, L.ln1, L.qkv_wd, L.qkv_s, L.qkv_b, e->lm_inv_freq, ctx_len, block_table, e->max_pages, pool_l, e->d_q, B, H, Hq,
                          Hkv, c.rms_norm_eps, part ? e->dec_cus : 0, e->d_xn, pend ? e->d_part_h : nullptr, pend_scale, layer_kv_scales(e, i)));
        CK(launch_decode_attn(s, e->d_q, pool_l, ctx_len, block_table, e->max_pages, e->d_part_o, e->d_part_ml, B, Hq, Hkv, n_splits, scale, part ? e->dec_cus : 0, e->attn_stream,
                              layer_kv_scales(e, i), share));
        CK(launch_decode_attn_combine(s, e->d_part_o, e->d_part_ml, ctx_len, e->d_att, B, Hq, Hkv, n_splits));
        bool pend_o = false;
        CK(launch_dec_proj(s, e->d_att, L.o_wd, L.o_s, e->d_h, B, H, Nq, part ? e->dec_cus : 0, e->d_part_h, &pend_o));
        CK(launch_dec_gateup(s, e->d_h, L.ln2, L.w13_wd, L.w13_s, e->d_act, B, H, I, c.rms_norm_eps, part ? e->dec_cus : 0, e->d_xn, pend_o ? e->d_part_h : nullptr, L.o_s));
        CK(launch_dec_proj(s, e->d_act, L.down_wd, L.down_s, e->d_h, B, H, I, part ? e->dec_cus : 0, e->d_part_h, &pend));
        pend_scale = L.down_s;
    }
    *pend_out = pend;
    *pend_scale_out = pend_scale;
    return DOTS_OK;
}

// every launch of one decode step; identical in eager mode and under graph capture
// part: the launch plan for a stream that is CU-masked to half the chip (whole 16-row tiles: half as many workgroups per projection)
int decode_step_launches(DotsEngine* e, int n_splits, int part) {
    const DotsConfig& c = e->cfg;
    hipStream_t s = e->stream;
    const int H = c.hidden_size;
    // A speculating step (slot mode, dots_set_speculation): `rows` slots become B = rows x (k + 1) rows whose tokens, contexts and
    // block-table rows spec_expand_kernel builds; the first `rows` of them are the rows of the plain step
    const int rows = e->B, spec_k = e->slot_mode ? e->spec_k : 0;
    const int B = rows * (spec_k + 1);
    const int32_t *tokens = e->cur_tokens, *ctx_len = e->ctx_len, *block_table = e->block_table;
    const SpecState sp = spec_state(e);
    if (spec_k) {
        CK(launch_spec_expand(s, sp, step_state(e, 1, e->d_sel), e->block_table, e->max_pages, rows, e->n_pool_pages));
        tokens = e->sp_tokens; ctx_len = e->sp_ctx; block_table = e->sp_table;
    }
    bool pend = false;
    const float* pend_scale = nullptr;
    // the shared-prefix plan describes the slots' own block table: the plain slot step alone takes it
    const SharePlanDev share = share_plan_now(e);
    RET(decode_layers(e, tokens, ctx_len, block_table, B, n_splits, part, &pend, &pend_scale, share.cap ? &share : nullptr));
    if (e->force_part) part = 1;                                                   // as the layers ran (decode_layers)
    CK(launch_dec_lmhead(s, e->d_h, e->final_norm, e->lm_head_d, e->lm_head_s, e->d_logits, B, H, c.vocab_size, c.rms_norm_eps, part ? e->dec_cus : 0, e->d_xn,
                         pend ? e->d_part_h : nullptr, pend_scale));
    if (spec_k) CK(launch_spec_argmax(s, sp, e->d_logits, c.vocab_size, c.vocab_size, rows, e->am_val, e->am_idx));
    // Slots whose selection is shaped and that speculate (dots_set_speculation_guided, dots_set_speculation_shaped), from the slots' state
    // before anything commits.  Guided: the state each live draft row is selected under and its allowed bits, into the rows of guide_mask
    // the stage does not use.  N-gram: the draft rows' banned bits, into the rows of ngram_mask the stage does not use.  Then the shaped
    // partials (and values) of every such draft row.  With both switches off (or no row holding such a feature) nothing is launched here
    const int sspec = spec_k ? spec_shapes(e) : 0;
    const RowSel spec_rs = spec_k ? spec_row_sel(e) : RowSel{};
    if (spec_k && (sp.gstate || sspec)) {
        if (B > c.max_batch) return e->fail(DOTS_E_CAPACITY, "%d rows x %d exceed max_batch %d", rows, spec_k + 1, c.max_batch);      // guide_mask / ngram_mask / pen_logits hold max_batch rows
        if (sp.gstate) {
            CK(launch_spec_guide_chain(s, sp, spec_rs.guide, e->eos_ids, e->n_eos, rows, spec_rs.rules));
            CK(launch_guide_mask_drafts(s, spec_rs.guide, rows, spec_k, sp.gstate));
        }
        if (spec_rs.ngram.rows)
            CK(launch_ngram_ban_drafts(s, spec_rs.ngram, rows, spec_k, e->out_ids, e->out_lens, c.max_seq_len, e->sp_drafts, e->sp_nlive));
        CK(launch_spec_shape_select(s, sp, spec_rs, step_state(e, 1, e->d_sel), e->d_logits, c.vocab_size, c.vocab_size, rows, e->am_val, e->am_idx));
    }
    // Slots with logprobs on that speculate (dots_set_speculation_logprobs): the partials of their live draft rows, from the raw logits, into
    // the rows of the logprob scratch the stage does not use.  With the switch off, or no row with logprobs on, nothing is launched here
    const bool lpspec = spec_k && spec_lps(e);
    const LogprobState spec_ls{e->d_row_lp, e->d_sel, e->finished, e->out_lens, e->cur_tokens, e->lp_ms, e->lp_pv, e->lp_pi, e->lp_pos,
                               e->lp_tok, e->lp_ids, e->lp_top, c.max_seq_len};
    if (lpspec) {
        if (B > c.max_batch) return e->fail(DOTS_E_CAPACITY, "%d rows x %d exceed max_batch %d", rows, spec_k + 1, c.max_batch);      // lp_ms / lp_pv / lp_pi hold max_batch rows
        CK(launch_spec_logprob_partial(s, e->d_logits, c.vocab_size, c.vocab_size, rows, spec_k, e->sp_nlive, spec_ls));
    }
    // the candidates of the draft rows of sampled slots, before the selection stage moves out_lens: draft row j draws with counter out_lens + j
    if (spec_k && sp.cand)
        CK(launch_spec_draw(s, sp, e->d_logits, c.vocab_size, c.vocab_size, rows, spec_rs, e->out_lens, e->am_val, e->am_idx));
    e->B_sel = rows;
    e->sel_now = e->d_sel;
    RET(select_tokens(e, 1));
    if (e->slot_mode && e->n_beam_hi > 0) RET(beam_step(e, rows));      // the beam groups' rows: masked out of the selection above
    if (spec_k) {
        // the selection stage committed row 0 of every slot; the accept walk commits what the drafts got right, then the drafter reads
        // the grown output
        const StepState st = step_state(e, 1, e->d_sel);
        CK(launch_spec_accept(s, sp, st, rows, c.vocab_size, e->am_val, e->am_idx, spec_rs));
        // the entries of the candidates the walk committed, at the positions their commits appended at
        if (lpspec) CK(launch_spec_logprob_final(s, e->d_logits, c.vocab_size, c.vocab_size, rows, spec_k, sp.acc_n, sp.acc_tok, spec_ls));
        if (e->spec_max_n > 0)
            CK(launch_ngram_draft(s, st.out_ids, st.out_lens, st.out_stride, st.finished, st.sel, sp.cls, sp.engine_greedy, rows, spec_k, e->spec_min_n,
                                  e->spec_max_n, e->sp_drafts, DOTS_MAX_SPEC_DRAFTS, e->sp_ndraft));
        // the slots that hold a prediction and whose output aligns with it draft from it instead.  While no slot holds
        // one nothing is launched here
        if (spec_predicts(e))
            CK(launch_predict_draft(s, predict_state(e), st.out_ids, st.out_lens, st.out_stride, st.finished, st.sel, sp.cls, sp.engine_greedy, rows, spec_k,
                                    e->spec_min_n, e->spec_max_n, e->sp_drafts, DOTS_MAX_SPEC_DRAFTS, e->sp_ndraft, e->sp_nlive));
    }
    return DOTS_OK;
}

int splits_for_ctx(int max_ctx) { return decode_attn_splits(max_ctx); }

// The captured decode step for (rows = e->B, splits, out_cap, e->n_eos): looked up in the cache or captured now.
int step_graph(DotsEngine* e, int rows, int n_splits, int out_cap, hipGraphExec_t* exec, int part) {
    const DotsEngine::StepKey key = step_key(e, rows, n_splits, out_cap, part);
    for (auto& g : e->step_graphs)
        if (g.key == key) {
            *exec = g.exec;
            return DOTS_OK;
        }
    if (e->step_graphs.size() >= 32) drop_step_graphs(e);
    DotsEngine::StepGraph g{key, nullptr, nullptr};
    CK(hipStreamBeginCapture(e->stream, hipStreamCaptureModeThreadLocal));
    int r = decode_step_launches(e, n_splits, part);
    hipError_t ce = hipStreamEndCapture(e->stream, &g.graph);
    if (r != DOTS_OK || ce != hipSuccess) {
        if (ce == hipSuccess && g.graph) hipGraphDestroy(g.graph);
        if (r != DOTS_OK) return r;
        CK(ce);
    }
    if (hipGraphInstantiate(&g.exec, g.graph, nullptr, nullptr, 0) != hipSuccess) {
        hipGraphDestroy(g.graph);
        return e->fail(DOTS_E_HIP, "hipGraphInstantiate failed for the decode step");
    }
    e->step_graphs.push_back(g);
    *exec = g.exec;
    return DOTS_OK;
}
}  // namespace engine

using namespace engine;

// ===================================================================================== C ABI
extern "C" {
const char* dots_last_error(DotsEngine* e) { return e ? e->err.c_str() : g_create_error.c_str(); }

void* dots_stream(DotsEngine* e) { return e ? (void*)e->stream : nullptr; }

int dots_create(const DotsConfig* cfg, int device, DotsEngine** out) {
    if (!cfg || !out) { g_create_error = "null argument"; return DOTS_E_INVALID; }
    const DotsConfig& c = *cfg;
    auto bad = [&](const char* m) { g_create_error = m; return DOTS_E_INVALID; };
    if (c.head_dim != 128) return bad("head_dim must be 128");
    if (c.v_embed_dim != c.v_heads * 128) return bad("vision head_dim must be 128");
    if (c.num_heads % c.num_kv_heads || c.num_heads / c.num_kv_heads > 16) return bad("unsupported GQA group");
    if (c.hidden_size % 128 || c.v_embed_dim % 128 || c.vocab_size % 128) return bad("hidden sizes and vocab must be multiples of 128");
    if (c.intermediate_size % 64 || c.v_intermediate % 64) return bad("intermediate sizes must be multiples of 64");
    if (c.hidden_size > 1536 || c.hidden_size % 256) return bad("hidden_size must be a multiple of 256 and <= 1536 (decode kernels keep a residual row in registers)");
    if (c.num_heads * 128 < 512 || c.intermediate_size < 512) return bad("projection K too small for the 16-way in-workgroup split");
    if (c.max_batch < 1 || c.max_batch > DOTS_MAX_BATCH) return bad("max_batch must be in [1,64]");
    if (c.max_seq_len < 64 || c.max_patches < 4 || c.max_prefill_tokens < 1) return bad("capacity fields too small");
    if (c.kv_pool_tokens < 0 || (c.kv_pool_tokens > 0 && c.kv_pool_tokens < 64)) return bad("kv_pool_tokens must be 0 (default) or >= 64");
    if (c.kv_cache_dtype != 0 && c.kv_cache_dtype != 1) return bad("kv_cache_dtype must be 0 (bf16) or 1 (fp8 e4m3)");
    if (c.v_merge < 1 || c.v_temporal_patch != 1) return bad("unsupported vision patching");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) { g_create_error = "no such HIP device"; return DOTS_E_HIP; }
    if (hipSetDevice(device) != hipSuccess) { g_create_error = "hipSetDevice failed"; return DOTS_E_HIP; }
    DotsEngine* e = new DotsEngine();
    std::fill(e->row_lp, e->row_lp + DOTS_MAX_BATCH, -1);
    e->cfg = c;
    e->device = device;
    // DOTS_OCR_CU_RANGE="lo-hi" (experiment, tools/overlap_probe.py): the engine's stream only uses CU-mask bits lo..hi (of 256; bit i = CU i / 8 of XCD i % 8)
    if (const char* cr = sw::read_now(sw::CU_RANGE)) {
        int lo = 0, hi = 255;
        if (!sw::parse_cu_range(cr, &lo, &hi)) { g_create_error = std::string("bad ") + sw::CU_RANGE; delete e; return DOTS_E_INVALID; }
        uint32_t words[8] = {0};
        for (int b = lo; b <= hi; ++b) words[b / 32] |= 1u << (b % 32);
        if (hipExtStreamCreateWithCUMask(&e->stream, 8, words) != hipSuccess) { g_create_error = "hipExtStreamCreateWithCUMask failed"; delete e; return DOTS_E_HIP; }
    } else
    if (hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking) != hipSuccess) { g_create_error = "hipStreamCreate failed"; delete e; return DOTS_E_HIP; }
    int r = alloc_workspaces(e);
    if (r != DOTS_OK) { g_create_error = e->err; dots_destroy(e); return r; }
    *out = e;
    return DOTS_OK;
}

void dots_destroy(DotsEngine* e) {
    if (!e) return;
    hipSetDevice(e->device);
    if (e->s_vit) hipStreamSynchronize(e->s_vit);
    if (e->s_vit_full) hipStreamSynchronize(e->s_vit_full);
    if (e->s_dec) hipStreamSynchronize(e->s_dec);
    if (e->stream) hipStreamSynchronize(e->stream);
    drop_step_graphs(e);
    for (hipEvent_t ev : {e->ev_tw0, e->ev_tw_sw, e->ev_dec_end}) if (ev) hipEventDestroy(ev);
    if (e->s_vit_full) hipStreamDestroy(e->s_vit_full);
    if (e->ev_vis_ready) hipEventDestroy(e->ev_vis_ready);
    if (e->ev_xs) hipEventDestroy(e->ev_xs);
    if (e->s_vit) hipStreamDestroy(e->s_vit);
    if (e->s_dec) hipStreamDestroy(e->s_dec);
    for (void* p : e->allocs) hipFree(p);
    if (e->rule_stage_host) hipHostFree(e->rule_stage_host);
    swap_free_host(e);
    stream_free_host(e);
    if (e->rule_ev) hipEventDestroy(e->rule_ev);
    for (auto& ev : e->ev) if (ev) hipEventDestroy(ev);
    for (auto& ev : e->attn_ev) hipEventDestroy(ev);
    if (e->stream) hipStreamDestroy(e->stream);
    delete e->pc;
    delete e;
}

int dots_vit_forward(DotsEngine* e, const float* pixel_values, int on_device, int64_t total_patches,
                     const int64_t* grid_thw, int n_img, void* out_embeds_dev) {
    if (!e) return DOTS_E_INVALID;
    if (!e->finalized) return e->fail(DOTS_E_STATE, "weights not finalized");
    if (!pixel_values || !grid_thw || n_img < 1 || total_patches < 1) return e->fail(DOTS_E_INVALID, "bad vit_forward arguments");
    CK(hipSetDevice(e->device));
    if (e->pref_deferred) RET(launch_prefetched_tower(e));
    if (e->s_vit) CK(hipStreamWaitEvent(e->stream, e->ev_vis_ready, 0));          // the tower's workspaces: one pass at a time
    const float* pix = nullptr;
    RET(stage_pixels(e, e->stream, pixel_values, on_device, total_patches, &pix));
    e->vs = e->stream;
    return vit_forward(e, pix, total_patches, grid_thw, n_img, out_embeds_dev, e->vis, &e->vis_rows);
}

int dots_vit_prefetch(DotsEngine* e, const float* pixel_values, int on_device, int64_t total_patches, const int64_t* grid_thw, int n_img,
                      int after_prefill) {
    if (!e) return DOTS_E_INVALID;
    if (!e->finalized) return e->fail(DOTS_E_STATE, "weights not finalized");
    if (!pixel_values || !grid_thw || n_img < 1 || total_patches < 1) return e->fail(DOTS_E_INVALID, "bad vit_prefetch arguments");
    if (e->pref_pending) return e->fail(DOTS_E_STATE, "a prefetched vision batch is waiting: dots_vit_take_prefetched first");
    CK(hipSetDevice(e->device));
    RET(check_vision_request(e, total_patches, grid_thw, n_img));          // now, not when the deferred tower is launched inside a prefill
    RET(ensure_overlap_streams(e));
    const float* pix = nullptr;
    RET(stage_pixels(e, e->stream, pixel_values, on_device, total_patches, &pix));      // host pixels: staged on the main stream, now
    e->pref_pix = pix;
    e->pref_patches = total_patches;
    e->pref_grid.assign(grid_thw, grid_thw + (size_t)n_img * 3);
    e->pref_pending = true;
    e->pref_deferred = true;
    if (!after_prefill) {
        int r = launch_prefetched_tower(e);
        if (r != DOTS_OK) { e->pref_pending = false; return r; }
    }
    return DOTS_OK;
}

int dots_vit_prefetch_ready(DotsEngine* e, int* ready) {
    if (!e || !ready) return e ? e->fail(DOTS_E_INVALID, "null argument") : DOTS_E_INVALID;
    if (!e->pref_pending) return e->fail(DOTS_E_STATE, "no prefetched vision batch (dots_vit_prefetch)");
    CK(hipSetDevice(e->device));
    *ready = 0;
    if (e->pref_deferred) return DOTS_OK;                 // not launched yet: it starts behind the next prefill
    const hipError_t q = hipEventQuery(e->ev_vis_ready);
    if (q == hipSuccess) *ready = 1;
    else if (q == hipErrorNotReady) (void)hipGetLastError();      // must not stay behind as the thread's last error
    else CK(q);
    return DOTS_OK;
}

int dots_vit_take_prefetched(DotsEngine* e) {
    if (!e) return DOTS_E_INVALID;
    if (!e->pref_pending) return e->fail(DOTS_E_STATE, "no prefetched vision batch (dots_vit_prefetch)");
    CK(hipSetDevice(e->device));
    if (e->pref_deferred) {                              // no prefill came by: run it now
        int r = launch_prefetched_tower(e);
        if (r != DOTS_OK) { e->pref_pending = false; return r; }
    }
    CK(hipStreamWaitEvent(e->stream, e->ev_vis_ready, 0));
    std::swap(e->vis, e->vis_pref);
    e->vis_rows = e->vis_pref_rows;
    e->pref_pending = false;
    return DOTS_OK;
}

int dots_prefill(DotsEngine* e, const int32_t* input_ids, const int32_t* prompt_lens, int B) {
    if (!e) return DOTS_E_INVALID;
    if (!e->finalized) return e->fail(DOTS_E_STATE, "weights not finalized");
    if (!input_ids || !prompt_lens) return e->fail(DOTS_E_INVALID, "null argument");
    CK(hipSetDevice(e->device));
    if (e->out_cap <= 0) e->out_cap = e->cfg.max_seq_len;
    return prefill(e, input_ids, prompt_lens, B);
}

int dots_decode_step(DotsEngine* e) {
    if (!e) return DOTS_E_INVALID;
    if (e->B < 1) return e->fail(DOTS_E_STATE, "no prefilled batch");
    CK(hipSetDevice(e->device));
    int max_ctx = 0;
    for (int b = 0; b < e->B; ++b) max_ctx = std::max(max_ctx, e->h_prompt_lens[b] + e->steps_done + 1);
    if (max_ctx >= e->cfg.max_seq_len) return e->fail(DOTS_E_CAPACITY, "sequence reached max_seq_len");
    e->fresh_slots.clear();
    RET(decode_step_launches(e, splits_for_ctx(e->cfg.max_seq_len)));
    e->steps_done += 1;
    return DOTS_OK;
}

int dots_generate(DotsEngine* e, const int32_t* input_ids, const int32_t* prompt_lens, int B,
                  const float* pixel_values, int on_device, int64_t total_patches, const int64_t* grid_thw, int n_img,
                  int max_new_tokens, const int32_t* eos_ids, int n_eos, int32_t* out_ids, int32_t* out_lens) {
    if (!e) return DOTS_E_INVALID;
    if (!e->finalized) return e->fail(DOTS_E_STATE, "weights not finalized");
    if (!input_ids || !prompt_lens || !out_ids || !out_lens || max_new_tokens < 1) return e->fail(DOTS_E_INVALID, "bad generate arguments");
    if (n_eos < 0 || n_eos > 16) return e->fail(DOTS_E_INVALID, "n_eos must be in [0,16]");
    CK(hipSetDevice(e->device));
    hipStream_t s = e->stream;
    int max_prompt = 0;
    for (int b = 0; b < B; ++b) max_prompt = std::max(max_prompt, prompt_lens[b]);
    if (max_prompt + max_new_tokens > e->cfg.max_seq_len)
        return e->fail(DOTS_E_CAPACITY, "prompt (%d) + max_new_tokens (%d) exceeds max_seq_len %d", max_prompt, max_new_tokens, e->cfg.max_seq_len);
    {   // the tower of a prefetch launched before this call (pipelined batches) keeps its stats; everything else starts from zero
        const DotsStats keep = e->stats;
        e->stats = DotsStats{};
        if (n_img == -1) { e->stats.vit_patches = keep.vit_patches; e->stats.vit_attn_flops = keep.vit_attn_flops; e->stats.vit_flops = keep.vit_flops; }
    }
    CK(hipEventRecord(e->ev[6], s));
    if (n_img != -1) e->vis_rows = 0;               // n_img == -1: the rows dots_vit_take_prefetched put in place
    if (n_img > 0) RET(dots_vit_forward(e, pixel_values, on_device, total_patches, grid_thw, n_img, nullptr));
    e->n_eos = n_eos;
    if (n_eos) CK(hipMemcpyAsync(e->eos_ids, eos_ids, n_eos * 4, hipMemcpyHostToDevice, s));
    if (n_eos) std::copy(eos_ids, eos_ids + n_eos, e->h_eos);
    e->out_cap = max_new_tokens;
    RET(prefill(e, input_ids, prompt_lens, B));

    // ---- decode loop: one captured graph replayed max_new_tokens-1 times
    CK(hipEventRecord(e->ev[4], s));
    const int n_splits = splits_for_ctx(e->cfg.max_seq_len);       // engine constant: results do not depend on the batch
    const bool use_graph = !sw::on_if_set(sw::read_now(sw::NO_GRAPH));           // read per call here, once per process in dots_step_chunk
    hipGraphExec_t exec = nullptr;
    hipGraphExec_t exec_part = nullptr;            // the step captured with the half-chip launch plan, for the masked stream
    if (use_graph && max_new_tokens > 1) {
        if (e->step_graphs.size() >= 30) drop_step_graphs(e);          // so that neither lookup below can evict the other's graph
        if (e->s_vit) RET(step_graph(e, B, n_splits, max_new_tokens, &exec_part, 1));
        RET(step_graph(e, B, n_splits, max_new_tokens, &exec));
    }
    std::vector<int32_t> fin(DOTS_MAX_BATCH);
    int steps = 0;
    hipStream_t cur = s;                           // where the decode graph is replayed: see pick_decode_stream
    for (int step = 1; step < max_new_tokens; ++step) {
        if (exec && (step & 15) == 1) RET(pick_decode_stream(e, &cur));
        if (exec) CK(hipGraphLaunch(cur != s && exec_part ? exec_part : exec, cur));
        else RET(decode_step_launches(e, n_splits));
        ++steps;
        if ((n_eos || e->stage.rows(ROW_STOP) > 0 || e->stage.rows(ROW_LOOP) > 0) && (step % 16 == 0)) {       // early exit once every sequence hit EOS (or its stop string, or its loop rule)
            CK(hipMemcpyAsync(fin.data(), e->finished, B * 4, hipMemcpyDeviceToHost, cur));
            CK(hipStreamSynchronize(cur));
            bool all = true;
            for (int b = 0; b < B; ++b) all = all && fin[b];
            if (all) break;
        }
        if (exec && !n_eos && cur != s && (step & 63) == 0) CK(hipStreamSynchronize(cur));     // let the host see the tower finish (the queue is 16 steps deep otherwise)
    }
    RET(chain_streams(e, cur, s));
    CK(hipEventRecord(e->ev[5], s));
    CK(hipEventRecord(e->ev[7], s));
    e->steps_done = steps;
    std::vector<int32_t> tmp((size_t)B * max_new_tokens);
    CK(hipMemcpyAsync(tmp.data(), e->out_ids, tmp.size() * 4, hipMemcpyDeviceToHost, s));
    CK(hipMemcpyAsync(out_lens, e->out_lens, B * 4, hipMemcpyDeviceToHost, s));
    CK(hipStreamSynchronize(s));
    std::memcpy(out_ids, tmp.data(), tmp.size() * 4);

    // ---- stats
    e->stats.decode_steps = steps;
    int64_t newtok = 0;
    double kvb = 0;
    const double kv_tok = (double)e->cfg.num_layers * e->cfg.num_kv_heads * 128 * 2 * (e->kv8 ? 1 : 2);      // bytes per cached token (K and V)
    for (int b = 0; b < B; ++b) {
        newtok += out_lens[b];
        for (int st = 0; st < steps; ++st) kvb += (double)(prompt_lens[b] + st + 1) * kv_tok;
    }
    e->stats.new_tokens = newtok;
    e->stats.decode_bytes = (double)steps * decode_step_bytes(e->cfg) + kvb;
    return DOTS_OK;
}

int dots_get_stats(DotsEngine* e, DotsStats* out) {
    if (!e || !out) return DOTS_E_INVALID;
    CK(hipSetDevice(e->device));
    CK(hipStreamSynchronize(e->stream));
    if (e->s_vit) CK(hipStreamSynchronize(e->s_vit));        // a prefetched tower's events (the next call would wait for it anyway)
    // An event pair that was never recorded (e.g. the static-batch events after a slot-mode run) makes hipEventElapsedTime fail; the
    // failure must not stay behind as the thread's "last error" (PyTorch / RCCL check hipGetLastError after their own launches).
    auto elapsed = [&](hipEvent_t a, hipEvent_t b) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, a, b) != hipSuccess) { (void)hipGetLastError(); ms = 0; }
        return ms;
    };
    auto el = [&](int a, int b) { return elapsed(e->ev[a], e->ev[b]); };
    e->stats.vit_ms = e->stats.vit_patches ? el(0, 1) : 0;
    e->stats.prefill_ms = e->stats.prefill_tokens ? el(2, 3) : 0;
    e->stats.decode_ms = e->stats.decode_steps ? el(4, 5) : 0;
    e->stats.total_ms = e->stats.decode_steps || e->stats.new_tokens ? el(6, 7) : 0;
    float a = 0;
    for (int i = 0; i < e->attn_pairs; ++i) a += elapsed(e->attn_ev[2 * i], e->attn_ev[2 * i + 1]);
    e->stats.vit_attn_ms = a;
    e->stats.vit_attn_launches = e->attn_pairs;
    *out = e->stats;
    return DOTS_OK;
}

int dots_preprocess_image(DotsEngine* e, const uint8_t* rgb, int on_device, int h, int w, int rh, int rw,
                          const int32_t* hcoef, const int32_t* hbounds, int hk, const int32_t* vcoef, const int32_t* vbounds, int vk,
                          const float* mean3, const float* std3, float rescale, float* out) {
    if (!e) return DOTS_E_INVALID;
    const DotsConfig& c = e->cfg;
    const int P = c.v_patch, m = c.v_merge;
    if (!rgb || !out || !mean3 || !std3 || h < 1 || w < 1 || rh < 1 || rw < 1) return e->fail(DOTS_E_INVALID, "bad preprocess arguments");
    if (rh % (P * m) || rw % (P * m)) return e->fail(DOTS_E_INVALID, "resized size %dx%d is not a multiple of patch*merge", rh, rw);
    if ((rw != w && (!hcoef || !hbounds || hk < 1)) || (rh != h && (!vcoef || !vbounds || vk < 1)))
        return e->fail(DOTS_E_INVALID, "missing resample table for a resized axis");
    if (c.v_channels != 3) return e->fail(DOTS_E_INVALID, "only 3-channel images are supported");
    CK(hipSetDevice(e->device));
    hipStream_t s = e->stream;
    auto grow = [&](uint8_t** p, size_t* cap, size_t need) -> hipError_t {
        if (need <= *cap) return hipSuccess;
        if (*p) { hipStreamSynchronize(s); e->release(*p); *p = nullptr; }
        *cap = need + need / 4;
        return e->alloc(p, *cap);
    };
    const size_t in_bytes = (size_t)h * w * 3, tmp_bytes = (size_t)h * rw * 3, out_bytes = (size_t)rh * rw * 3;
    const uint8_t* src = rgb;
    if (!on_device) {
        CK(grow(&e->pp_in, &e->pp_in_cap, in_bytes));
        CK(hipMemcpyAsync(e->pp_in, rgb, in_bytes, hipMemcpyHostToDevice, s));
        src = e->pp_in;
    }
    const size_t tab_ints = (rw != w ? (size_t)rw * (hk + 2) : 0) + (rh != h ? (size_t)rh * (vk + 2) : 0);
    if (tab_ints > e->pp_tab_cap) {
        if (e->pp_tab) { hipStreamSynchronize(s); e->release(e->pp_tab); e->pp_tab = nullptr; }
        e->pp_tab_cap = tab_ints + tab_ints / 4;
        CK(e->alloc(&e->pp_tab, e->pp_tab_cap));
    }
    int32_t* tab = e->pp_tab;
    if (rw != w) {
        CK(grow(&e->pp_tmp, &e->pp_tmp_cap, tmp_bytes));
        CK(hipMemcpyAsync(tab, hcoef, (size_t)rw * hk * 4, hipMemcpyHostToDevice, s));
        CK(hipMemcpyAsync(tab + (size_t)rw * hk, hbounds, (size_t)rw * 2 * 4, hipMemcpyHostToDevice, s));
        CK(launch_resize_h(s, src, e->pp_tmp, tab, tab + (size_t)rw * hk, hk, h, w, rw));
        src = e->pp_tmp;
        tab += (size_t)rw * (hk + 2);
    }
    if (rh != h) {
        CK(grow(&e->pp_out, &e->pp_out_cap, out_bytes));
        CK(hipMemcpyAsync(tab, vcoef, (size_t)rh * vk * 4, hipMemcpyHostToDevice, s));
        CK(hipMemcpyAsync(tab + (size_t)rh * vk, vbounds, (size_t)rh * 2 * 4, hipMemcpyHostToDevice, s));
        CK(launch_resize_v(s, src, e->pp_out, tab, tab + (size_t)rh * vk, vk, rw, rh));
        src = e->pp_out;
    }
    CK(launch_normalize_patchify(s, src, out, rw, rh / P, rw / P, P, m, rescale, mean3, std3));
    CK(hipStreamSynchronize(s));          // the host tables / image buffers may be reused by the caller
    return DOTS_OK;
}

int dots_set_decode_plan(DotsEngine* e, int plan) {
    if (!e) return DOTS_E_INVALID;
    if (plan < 0 || plan > 5 || (plan & 6) == 6)
        return e->fail(DOTS_E_INVALID, "decode plan must be 0 (by stream) or 1 (partition plan on every step), + 2 (streaming attention) or + 4 (per-split attention)");
    const int part = plan & 1, stream = (plan & 2) ? 1 : (plan & 4) ? 0 : -1;
    if (part != e->force_part || stream != e->attn_stream) {
        e->force_part = part;
        e->attn_stream = stream;
        drop_step_graphs(e);                               // the captured decode steps bake the launch plan in
    }
    return DOTS_OK;
}

int dots_tower_tail(DotsEngine* e, int set, int* now) {
    if (!e) return DOTS_E_INVALID;
    if (set < -2 || set > e->cfg.v_layers) return e->fail(DOTS_E_INVALID, "tower tail must be -2 (query), -1 (adaptive) or 0 .. v_layers");
    if (set >= -1) e->tail_fixed = set;
    if (now) *now = e->tail_now;
    return DOTS_OK;
}

int dots_set_gemm_plan(DotsEngine* e, int plan) {
    if (!e) return DOTS_E_INVALID;
    if (plan < 0 || plan > 1) return e->fail(DOTS_E_INVALID, "gemm plan must be 0 (8-wave ping-pong) or 1 (one wave per SIMD)");
    gemm_set_plan(plan);
    return DOTS_OK;
}

int dots_get_logits(DotsEngine* e, float* out) {
    if (!e || !out) return DOTS_E_INVALID;
    if (e->B < 1) return e->fail(DOTS_E_STATE, "no prefilled batch");
    CK(hipSetDevice(e->device));
    CK(hipMemcpyAsync(out, e->d_logits, (size_t)e->B * e->cfg.vocab_size * 4, hipMemcpyDeviceToHost, e->stream));
    CK(hipStreamSynchronize(e->stream));
    return DOTS_OK;
}

int dots_set_next_tokens(DotsEngine* e, const int32_t* tokens, int B) {
    if (!e || !tokens || B != e->B) return e ? e->fail(DOTS_E_INVALID, "bad set_next_tokens arguments") : DOTS_E_INVALID;
    CK(hipSetDevice(e->device));
    CK(hipMemcpyAsync(e->cur_tokens, tokens, B * 4, hipMemcpyHostToDevice, e->stream));
    CK(hipStreamSynchronize(e->stream));
    return DOTS_OK;
}

int dots_get_last_tokens(DotsEngine* e, int32_t* out) {
    if (!e || !out) return DOTS_E_INVALID;
    if (e->B < 1) return e->fail(DOTS_E_STATE, "no prefilled batch");
    CK(hipSetDevice(e->device));
    std::vector<int32_t> lens(DOTS_MAX_BATCH), ids((size_t)DOTS_MAX_BATCH * std::max(1, e->out_cap));
    CK(hipMemcpyAsync(lens.data(), e->out_lens, e->B * 4, hipMemcpyDeviceToHost, e->stream));
    CK(hipMemcpyAsync(ids.data(), e->out_ids, (size_t)e->B * e->out_cap * 4, hipMemcpyDeviceToHost, e->stream));
    CK(hipStreamSynchronize(e->stream));
    for (int b = 0; b < e->B; ++b) out[b] = lens[b] > 0 ? ids[(size_t)b * e->out_cap + lens[b] - 1] : -1;
    return DOTS_OK;
}

int dots_debug_capture_hidden(DotsEngine* e, int64_t capacity_elems) {
    if (!e || capacity_elems < 0) return DOTS_E_INVALID;
    CK(hipSetDevice(e->device));
    CK(hipStreamSynchronize(e->stream));
    if (e->dbg_hidden) { e->release(e->dbg_hidden); e->dbg_hidden = nullptr; }
    e->dbg_cap = 0; e->dbg_vit_rows = e->dbg_lm_rows = 0;
    if (capacity_elems > 0) {
        CK(e->alloc(&e->dbg_hidden, (size_t)capacity_elems));
        e->dbg_cap = (size_t)capacity_elems;
    }
    return DOTS_OK;
}

int dots_debug_read_hidden(DotsEngine* e, int which, int layer, void* out_host, int64_t* rows_out) {
    if (!e || !out_host || !rows_out || !e->dbg_hidden) return e ? e->fail(DOTS_E_STATE, "hidden-state capture is off") : DOTS_E_INVALID;
    CK(hipSetDevice(e->device));
    const DotsConfig& c = e->cfg;
    const int64_t rows = which == 0 ? e->dbg_vit_rows : e->dbg_lm_rows;
    const int dim = which == 0 ? c.v_embed_dim : c.hidden_size, n_layers = which == 0 ? c.v_layers : c.num_layers;
    if (rows <= 0 || layer < 0 || layer >= n_layers) return e->fail(DOTS_E_INVALID, "no captured hidden state for layer %d", layer);
    const size_t off = (which == 0 ? 0 : (size_t)c.v_layers * e->dbg_vit_rows * c.v_embed_dim) + (size_t)layer * rows * dim;
    if (off + (size_t)rows * dim > e->dbg_cap) return e->fail(DOTS_E_CAPACITY, "capture buffer too small for layer %d", layer);
    CK(hipMemcpyAsync(out_host, e->dbg_hidden + off, (size_t)rows * dim * 2, hipMemcpyDeviceToHost, e->stream));
    CK(hipStreamSynchronize(e->stream));
    *rows_out = rows;
    return DOTS_OK;
}

int dots_debug_read_kv(DotsEngine* e, int layer, int seq, int pos0, int n, int which, void* out_host) {
    if (!e || !out_host) return e ? e->fail(DOTS_E_INVALID, "null argument") : DOTS_E_INVALID;
    const DotsConfig& c = e->cfg;
    if (layer < 0 || layer >= c.num_layers || seq < 0 || seq >= c.max_batch || pos0 < 0 || n < 1 || (which != 0 && which != 1) ||
        (int64_t)pos0 + n > (int64_t)e->max_pages * PAGE)
        return e->fail(DOTS_E_INVALID, "bad dots_debug_read_kv arguments (layer %d, row %d, positions %d + %d, which %d)", layer, seq, pos0, n, which);
    RET(dots_synchronize(e));
    const int Hkv = c.num_kv_heads, es = e->kv8 ? 1 : 2;
    const size_t page_bytes = (size_t)PAGE_ELEMS * es;                                     // one (page, kv head, K|V)
    const uint8_t* base = reinterpret_cast<const uint8_t*>(e->pool) + e->pool_layer_elems * 2 * layer;
    std::vector<uint8_t> pg(page_bytes);
    uint8_t* out = static_cast<uint8_t*>(out_host);
    for (int p = pos0 / PAGE; p <= (pos0 + n - 1) / PAGE; ++p) {
        const int page = e->hp_table[(size_t)seq * e->max_pages + p];
        if (page >= e->n_pool_pages) return e->fail(DOTS_E_STATE, "position %d of row %d is not in the KV cache", std::max(pos0, p * PAGE), seq);
        for (int h = 0; h < Hkv; ++h) {
            CK(hipMemcpyAsync(pg.data(), base + ((size_t)(page * Hkv + h) * 2 + which) * page_bytes, page_bytes, hipMemcpyDeviceToHost, e->stream));
            CK(hipStreamSynchronize(e->stream));
            for (int pos = std::max(pos0, p * PAGE); pos < std::min(pos0 + n, (p + 1) * PAGE); ++pos)
                for (int d = 0; d < 128; ++d) {
                    const int key = pos & (PAGE - 1), el = which == 0 ? k_chunk(key, d) * 8 + (d & 7) : v_off(key, d);
                    const size_t o = ((size_t)h * n + (pos - pos0)) * 128 + d;
                    if (e->kv8) out[o] = pg[kv8_byte(el)];
                    else std::memcpy(out + o * 2, pg.data() + (size_t)el * 2, 2);
                }
        }
    }
    return DOTS_OK;
}

int dots_synchronize(DotsEngine* e) {
    if (!e) return DOTS_E_INVALID;
    CK(hipSetDevice(e->device));
    if (e->s_vit) CK(hipStreamSynchronize(e->s_vit));
    if (e->s_dec) CK(hipStreamSynchronize(e->s_dec));
    CK(hipStreamSynchronize(e->stream));
    return DOTS_OK;
}

int dots_dev_alloc(DotsEngine* e, int64_t bytes, void** out) {
    if (!e || !out || bytes < 0) return DOTS_E_INVALID;
    CK(hipSetDevice(e->device));
    uint8_t* p = nullptr;
    CK(e->alloc(&p, (size_t)bytes));
    *out = p;
    return DOTS_OK;
}
int dots_dev_free(DotsEngine* e, void* p) {
    if (!e) return DOTS_E_INVALID;
    CK(hipSetDevice(e->device));
    CK(hipStreamSynchronize(e->stream));
    e->release(p);
    return DOTS_OK;
}
int dots_memcpy_h2d(DotsEngine* e, void* dst, const void* src, int64_t bytes) {
    if (!e) return DOTS_E_INVALID;
    CK(hipSetDevice(e->device));
    CK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, e->stream));
    CK(hipStreamSynchronize(e->stream));
    return DOTS_OK;
}
int dots_memcpy_d2h(DotsEngine* e, void* dst, const void* src, int64_t bytes) {
    if (!e) return DOTS_E_INVALID;
    CK(hipSetDevice(e->device));
    CK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, e->stream));
    CK(hipStreamSynchronize(e->stream));
    return DOTS_OK;
}
}  // extern "C"
