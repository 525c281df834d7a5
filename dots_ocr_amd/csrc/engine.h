// Private header of the engine's host sources engine.hip, weights.hip, slots.hip, rows.hip and ops.hip (the map: DESIGN §6): the engine
// struct and the functions they call of each other.  Nothing outside csrc/ includes it.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>
#include <unordered_map>
#include <vector>

#include "common.h"
#include "decode_layout.h"
#include "dots_ocr_hip.h"
#include "kernels.h"
#include "prefix_cache.h"
#include "row_stage.h"
#include "share_plan.h"
#include "switches.h"

struct Tensor {
    bf16_t* p = nullptr;
    std::vector<int64_t> shape;
    int64_t numel() const { int64_t n = 1; for (auto s : shape) n *= s; return n; }
};

// *_s: per-output-channel fp32 scales of the fp8 configuration (cfg.fp8_weights; quant.hip), nullptr in bf16 mode.  In fp8 mode the
// row-major matrices hold bf16(q) (exact e4m3 values) and the decode copies (*_wd) hold the e4m3 bytes in fragment order.
// *_8: the e4m3 bytes row-major — the weight operand of the fp8-MFMA GEMMs (gemm.hip: gemm_fp8_256pp_kernel) of ViT / prefill.
struct VLayer {
    bf16_t *norm1, *qkv_w, *qkv_b, *proj_w, *proj_b, *norm2, *w13, *b13, *w2, *b2;
    float *qkv_s, *proj_s, *w13_s, *w2_s;
    uint8_t *qkv_8, *proj_8, *w13_8, *w2_8;
};
struct LLayer {
    bf16_t *ln1, *qkv_w, *qkv_b, *o_w, *ln2, *w13, *down_w;          // row-major [N][K]: prefill GEMMs
    void *qkv_wd, *o_wd, *w13_wd, *down_wd;                          // MFMA fragment order: decode skinny GEMMs
    float *qkv_s, *o_s, *w13_s, *down_s;
    uint8_t *qkv_8, *o_8, *w13_8, *down_8;
};

// a row that goes live in a slot: its context (the prompt length) and its generation cap ("what admitting a slot consists of")
struct LiveRow { int32_t slot, ctx, cap; };

struct DotsEngine {
    DotsConfig cfg{};
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;
    std::vector<void*> allocs;
    bool finalized = false;

    std::unordered_map<std::string, Tensor> raw;     // checkpoint tensors as loaded (bf16, device)

    // packed weights
    bf16_t *patch_w = nullptr, *patch_b = nullptr, *patch_norm = nullptr;
    int patch_k = 0, patch_kpad = 0;
    std::vector<VLayer> vl;
    bf16_t *v_post_norm = nullptr, *m_ln_w = nullptr, *m_ln_b = nullptr, *m0_w = nullptr, *m0_b = nullptr, *m2_w = nullptr, *m2_b = nullptr;
    bf16_t *embed = nullptr, *final_norm = nullptr, *lm_head = nullptr;
    void* lm_head_d = nullptr;
    float *m0_s = nullptr, *m2_s = nullptr, *lm_head_s = nullptr;
    uint8_t *m0_8 = nullptr, *m2_8 = nullptr;
    // fp8 mode: per-token quantised activations of the GEMM being launched (max rows x max K bytes) + their scales
    uint8_t* act_q = nullptr;
    float* act_s = nullptr;
    uint8_t* act_q_v = nullptr;            // the vision tower's own quantisation scratch (it may run beside a prefill: dots_vit_prefetch)
    float* act_s_v = nullptr;
    // ---- vision prefetch (dots_vit_prefetch): the tower of the NEXT page batch runs on `s_vit`, a stream masked to the upper
    // 256 - dec_cus CUs (an equal share of every XCD), while the decode loop of the current batch is replayed on `s_dec`, masked to
    // the lower dec_cus CUs.  Without the masks the two streams time-slice the chip and nothing overlaps (tools/overlap_probe.py).
    hipStream_t s_vit = nullptr, s_dec = nullptr;
    int dec_cus = 128;
    hipEvent_t ev_vis_ready = nullptr, ev_xs = nullptr;     // tower finished / cross-stream ordering
    bf16_t* vis_pref = nullptr;            // merged vision rows of the prefetched batch (swapped with `vis` when taken)
    int64_t vis_pref_rows = 0;
    bool pref_pending = false;             // a prefetch was requested and not yet taken
    bool pref_deferred = false;            // ... and its tower is still to be launched (behind the next prefill)
    const float* pref_pix = nullptr;       // deferred request
    int64_t pref_patches = 0;
    std::vector<int64_t> pref_grid;
    hipStream_t vs = nullptr;              // the stream vit_forward is currently enqueuing to (stream or s_vit)
    // ---- tower tail (round 5): the LAST `tail` blocks of a prefetched tower (and its merger) run on `s_vit_full`, a stream without a CU
    // mask.  The two partitions cannot be re-balanced in small steps (a partition has to be a whole number of CUs per shader engine of
    // every XCD — 32, 64, 96, ... CUs: with 56 every decode kernel ran at half speed, profiles/r05_decode_wide_ab.txt), so when the
    // decode loop of a step drains before the tower the decode partition would idle until the tower is done.  Instead the tower is split
    // in time: (L - tail) blocks beside the decode loop on its partition, the rest on the whole chip.  tail is chosen per launch from the
    // previous launch's measurements (events): tail = L - D / t_block, D = when the last decode chunk ended after the tower had started,
    // t_block = the partition's time per block — i.e. the head ends about when the decode loop does; a decode loop that outlasts the
    // tower gives tail = 0.  OFF by default (tail 0): the rule assumes that the decode work of a step is FINITE (bench.py's fixed
    // half_steps per admission); a serving loop whose host merely stopped issuing chunks while it waited for the tower would be read as
    // "decode drained".  Measured on the a4 bench: 5.74 (off) -> 5.81 pages/s (adaptive, 8 blocks) — the chip is power-limited, a block
    // on 256 CUs takes 27.6 ms against 30.4 on 192 (profiles/r05_tower_tail_ab.txt).
    hipStream_t s_vit_full = nullptr;
    hipEvent_t ev_tw0 = nullptr, ev_tw_sw = nullptr, ev_dec_end = nullptr;      // tower start / end of its partition part / end of the last decode chunk
    int tail_fixed = 0;                    // dots_tower_tail / DOTS_OCR_TOWER_TAIL_LAYERS: blocks on the whole chip (default 0 = off), -1 = adaptive
    int tail_now = 0;                      // tail of the tower being launched / launched last
    int tail_head_blocks = 0;              // blocks of the last prefetched tower that ran on the partition (0: no measurement yet)
    uint64_t tw_seq = 0, dec_end_seq = 0, dec_end_at_tw = 0;     // launch counters: was a decode chunk recorded after the last tower started?
    std::vector<LLayer> ll;
    float *v_inv_freq = nullptr, *lm_inv_freq = nullptr;

    // ---- ViT workspace (max_patches rows)
    int64_t P = 0, Ppad = 0;
    bf16_t *v_xa = nullptr, *v_x = nullptr, *v_xn = nullptr, *v_qkv = nullptr, *v_q = nullptr, *v_k = nullptr, *v_vt = nullptr,
           *v_att = nullptr, *v_act = nullptr, *v_mh = nullptr, *vis = nullptr;
    float* v_pix = nullptr;
    float2* v_cs = nullptr;
    int32_t* v_pos = nullptr;
    Tile64* v_tiles = nullptr;
    QBlock* v_qblocks = nullptr;
    int64_t vis_rows = 0;
    std::vector<int32_t> h_pos;
    std::vector<Tile64> h_tiles;
    std::vector<QBlock> h_qblocks;

    // ---- prefill workspace (max_prefill_tokens rows)
    int64_t TP = 0, TPpad = 0;
    bf16_t *p_x = nullptr, *p_xn = nullptr, *p_qkv = nullptr, *p_q = nullptr, *p_k = nullptr, *p_vt = nullptr, *p_att = nullptr, *p_act = nullptr;
    float2* p_cs = nullptr;
    int32_t *p_pos = nullptr, *p_src = nullptr, *p_last = nullptr;
    Tile64* p_tiles = nullptr;
    QBlock* p_qblocks = nullptr;
    std::vector<int32_t> hp_pos, hp_src, hp_last, hp_table;
    std::vector<Tile64> hp_tiles;
    std::vector<QBlock> hp_qblocks;

    // ---- KV pool + decode state
    int max_pages = 0;                     // block-table width: pages of one sequence at max_seq_len
    int n_pool_pages = 0;                  // allocatable pages; page n_pool_pages is the scratch page idle rows write to
    int kv_capped = 0;                     // sequences whose generation cap was lowered because the pool ran dry
    std::vector<int32_t> free_pages;       // LIFO free list
    // holders of every page (0 = in the free list).  Only dots_slots_fork makes a count exceed 1: the children's block-table rows name the
    // source's full prompt pages.  A page with more than one holder is never written
    std::vector<int32_t> page_refs;
    // dots_slots_fork: the slots the most recent dots_slots_prefill filled, in the order of its packed prompts (hp_last[i] = last packed
    // token of fresh_slots[i]); emptied by whatever invalidates that prefill's workspace (p_src, d_logits): any decode step, any other prefill
    std::vector<int> fresh_slots;
    int32_t* fk_dev = nullptr;             // [3][DOTS_MAX_BATCH] int32: a fork's destination slots, their tail pages, and (first entry) L - 1
    std::vector<std::vector<int32_t>> slot_pages;
    bf16_t* pool = nullptr;                // [layers][n_pool_pages + 1][Hkv][2][8192] bf16, or e4m3 bytes (kv8; decode.hip header)
    size_t pool_layer_elems = 0;           // per layer, in bf16 units (an fp8 pool's layer is half as many)
    bool kv8 = false;                      // DotsConfig.kv_cache_dtype == 1: the pool holds e4m3fn values
    float* kv_scales = nullptr;            // [layers][Hkv][K | V] fp32 (dots_set_kv_scales; 1.0 until set), read by the fp8 writers and reader
    int32_t *block_table = nullptr, *ctx_len = nullptr, *cur_tokens = nullptr, *out_ids = nullptr, *out_lens = nullptr,
            *finished = nullptr, *eos_ids = nullptr, *am_idx = nullptr;
    float* am_val = nullptr;
    int n_eos = 0;
    float temperature = 0.f, top_p = 1.f;      // temperature <= 0: greedy (arg max)
    uint64_t seed = 0;
    // which rows the per-row selection stage owns and for which features (row_stage.h): the only host record of it
    RowStage stage;
    // per-row selection (dots_set_row_sampling): device table + own flags, allocated on first use; penalty state
    // (output counts, prompt-presence bits, penalised-logit scratch) allocated when a row first carries a penalty
    RowParams* d_rowp = nullptr;
    int32_t* d_row_own = nullptr;
    uint32_t* d_row_thr = nullptr;
    int32_t* pen_cnt = nullptr;
    uint32_t* pen_seen = nullptr;
    float* pen_logits = nullptr;
    // logit rules (dots_set_row_logit_rules): per-row table + the dense "bias or -inf" image [max_batch][V], allocated by the
    // first row that carries rules.  rule_stage: pinned host staging of one call's id / value lists ([V + DOTS_MAX_LOGIT_BIAS] int32, then
    // [DOTS_MAX_LOGIT_BIAS] fp32) and its device twin; rule_ev guards the pinned buffer's reuse.
    RowRules* d_rules = nullptr;
    float* rule_img = nullptr;
    int32_t *rule_stage = nullptr, *rule_stage_host = nullptr;
    hipEvent_t rule_ev = nullptr;
    int32_t h_eos[16] = {0};               // host mirror of eos_ids (the never-selectable checks of the rules)
    // guided decoding (dots_set_row_guide): the packed bytes of the vocabulary (dots_set_token_bytes), the guides created on
    // this engine (device tables; rows = how many rows hold each), and — allocated by the first row that takes a guide — the row table and
    // the allowed bits [max_batch][guide_mask_words(V)].  row_guide[row] = guide id + 1 of a row that holds one.
    int32_t* tok_off = nullptr;
    uint8_t* tok_bytes = nullptr;
    struct Guide { uint16_t* table = nullptr; uint8_t* accepting = nullptr; int n_states = 0, start = 0, rows = 0; };
    std::vector<Guide> guides;
    RowGuide* d_guides = nullptr;
    uint32_t* guide_mask = nullptr;
    int row_guide[DOTS_MAX_BATCH] = {0};
    // no-repeat n-gram blocking (dots_set_row_ngram): allocated by the first row that takes a rule — the row table and the
    // banned bits [max_batch][ngram_mask_words(V)]
    RowNgram* d_ngram = nullptr;
    uint32_t* ngram_mask = nullptr;
    // stop strings (dots_set_row_stop): the automata created on this engine (device tables; rows = how many rows hold each) and
    // — allocated by the first row that takes one — the row table.  Of a row that holds one: row_stop[row] = automaton id + 1, row_stop_min its min_tokens.
    struct Stop { uint16_t* table = nullptr; uint16_t* match_len = nullptr; uint8_t* match_id = nullptr; int n_states = 0, rows = 0; };
    std::vector<Stop> stops;
    RowStop* d_stop = nullptr;
    int row_stop[DOTS_MAX_BATCH] = {0};
    int row_stop_min[DOTS_MAX_BATCH] = {0};
    // loop guard (dots_set_row_loop), allocated by the first row that takes a rule: the row table and the run counters
    // [DOTS_MAX_BATCH][DOTS_MAX_LOOP_PERIOD].  row_loop[row]: the rule of a row that holds one (what a fork hands its children)
    RowLoop* d_loop = nullptr;
    int32_t* loop_run = nullptr;
    DotsLoopRule row_loop[DOTS_MAX_BATCH] = {};
    // log-probabilities (dots_set_row_logprobs): top_n per row (-1 = off) on the device and its host mirror; the outputs
    // ([max_batch][max_seq_len] positions) and the stage's scratch are allocated by the first row switched on
    int32_t* d_row_lp = nullptr;
    float *lp_tok = nullptr, *lp_top = nullptr, *lp_ms = nullptr, *lp_pv = nullptr;
    int32_t *lp_ids = nullptr, *lp_pi = nullptr, *lp_pos = nullptr;
    int row_lp[DOTS_MAX_BATCH];
    int n_lp = 0;                          // rows with logprobs on: > 0 adds the two logprob kernels around the selection stage
    // streaming (dots_set_row_stream / dots_slots_drain), allocated by the first row switched on: the rows' cursors (output
    // tokens already delivered) and the mapped pinned block stream_drain_kernel stores into (st_dev: its device address).  row_stream is
    // host-only: a drain hands the kernel the streaming rows as a bit mask
    int32_t* stream_pos = nullptr;
    int32_t *st_host = nullptr, *st_dev = nullptr;
    int row_stream[DOTS_MAX_BATCH] = {0};
    // n-gram speculative decoding (dots_set_speculation): spec_k drafts per slot and step (0 = off), the drafter's n-gram
    // sizes (spec_max_n == 0: host drafts only), and — allocated by the first call that switches it on — the slots' drafts, the expanded
    // row arrays of a speculating step and the counters (kernels.h SpecState)
    int spec_k = 0, spec_min_n = 0, spec_max_n = 0;
    int32_t *sp_drafts = nullptr, *sp_ndraft = nullptr, *sp_nlive = nullptr, *sp_tokens = nullptr, *sp_ctx = nullptr, *sp_table = nullptr;
    unsigned long long* sp_stats = nullptr;
    // which staged rows speculate (dots_set_speculation_rows: DOTS_SPEC_ROWS_* bits, 0 = plain greedy rows only) and the device array of
    // every row's speculation class (kernels.h SpecRow), which spec_row_class() derives and the row setters write in stream order;
    // sp_cand: the candidates of the draft rows of sampled slots.  row_pen / row_sampled: of a row that holds ROW_PARAMS, whether its
    // parameters carry a penalty / a temperature > 0 (the two facts about them the class needs)
    int spec_rows = 0;
    int32_t *sp_cls = nullptr, *sp_cand = nullptr;
    // may a row that holds a guide verify drafts (dots_set_speculation_guided; spec_row_class() ORs SPEC_ROWS_GUIDED into the mode), and —
    // allocated by the first call that switches it on — the states of the draft rows of guided slots (kernels.h SpecState::gstate)
    int spec_guided = 0;
    int32_t* sp_gstate = nullptr;
    // which shaped rows may verify drafts (dots_set_speculation_shaped: DOTS_SPEC_SHAPED_* bits; spec_row_class() ORs them into the mode
    // three bits up): rows with an n-gram rule, with logit rules, with a penalty in their parameters.  No state of its own: the draft rows
    // use rows [rows, rows * (k + 1)) of ngram_mask and pen_logits, which hold max_batch rows
    int spec_shaped = 0;
    // may a row with logprobs on verify drafts (dots_set_speculation_logprobs; spec_row_class() asks it), and — allocated by the first call
    // that switches it on — the accept record of a step (kernels.h SpecState::acc_n / acc_tok).  The draft rows' partials use rows
    // [rows, rows * (k + 1)) of lp_ms / lp_pv / lp_pi, which hold max_batch rows
    int spec_logprobs = 0;
    int32_t *sp_acc_n = nullptr, *sp_acc_tok = nullptr;
    // predicted outputs (dots_set_row_prediction), allocated by the first call that sets one: the slots' predictions
    // ([max_batch][max_seq_len]) and per slot their length, the alignment (cur, at), the source flag of the current drafts, the output
    // length the drafter last saw and the two counters (kernels.h PredictState).  row_pred[row]: the length of the prediction the row holds, n_pred: how many
    // rows hold one — while it is 0 a step launches what it launched before (StepKey::pred)
    int32_t *pr_ids = nullptr, *pr_len = nullptr, *pr_cur = nullptr, *pr_at = nullptr, *pr_src = nullptr, *pr_seen = nullptr;
    unsigned long long* pr_stats = nullptr;
    int row_pred[DOTS_MAX_BATCH] = {0};
    int n_pred = 0;
    bool row_pen[DOTS_MAX_BATCH] = {false}, row_sampled[DOTS_MAX_BATCH] = {false};
    // of a staged row without ROW_PARAMS: the engine-wide setting its stage entry was written from had a temperature > 0.  Such a row is
    // drawn by the stage whatever dots_set_sampling says later, and its draft rows would be arg maxima: it verifies no draft
    bool row_entry_sampled[DOTS_MAX_BATCH] = {false};
    // beam search (dots_slots_beam): the groups' host records (B == 0: free), beam_of[row] = group index + 1 of a group row,
    // n_beam_hi = highest used index + 1 (what a step's group kernels are launched over; 0: a step launches nothing of this), and —
    // allocated by the first group — the device records, the completed-record buffers, the parents beside out_ids and the logprob
    // partials of the group rows with the tables (top_n = 2B / sel = 1 on group rows) their partial launch reads
    struct BeamGroup {
        int B = 0, L = 0, max_new = 0, done_ub = 0;      // done_ub: bound on the records waiting on the device
        int slots[DOTS_MAX_BEAMS] = {0};
        std::vector<BeamDone> done;                      // drained so far
    };
    std::vector<BeamGroup> beams;
    int beam_of[DOTS_MAX_BATCH] = {0};
    int n_beam_hi = 0;
    BeamGroupDev* d_beam = nullptr;
    BeamDone* d_beam_done = nullptr;
    int32_t *beam_parent = nullptr, *bm_pi = nullptr, *bm_pos = nullptr, *bm_topn = nullptr, *bm_sel = nullptr;
    float *bm_ms = nullptr, *bm_pv = nullptr;
    int out_cap = 0;                       // row stride of out_ids for the current generation
    bf16_t *d_h = nullptr, *d_q = nullptr, *d_att = nullptr, *d_act = nullptr, *d_xn = nullptr;      // d_xn: normalised rows of batches above 32 rows (decode_b64.hip)
    float* d_part_h = nullptr;                     // [DEC_KSPLIT_PARTS][DOTS_MAX_BATCH][hidden] fp32: the K-quarter sums of a projection above 32 rows (decode_b64.hip)
    float *d_part_o = nullptr, *d_part_ml = nullptr, *d_logits = nullptr;
    // decode launch plan forced on every step (dots_set_decode_plan): 0 = by stream (whole chip / CU partition), 1 = always the partition plan
    int force_part = 0;
    int attn_stream = -1;                  // decode attention kernel (dots_set_decode_plan bits 1-2): -1 = by items per CU, 1 = streaming wherever legal, 0 = per split
    int B = 0;                             // sequences of the current batch
    int B_sel = 0;                         // rows the token-selection kernel runs over
    // ---- continuous batching: every sequence slot b < max_batch is free or occupied; the decode graph runs over rows
    // [0, highest occupied slot] and only commits tokens for occupied, unfinished slots
    bool slot_mode = false;
    bool sel_dirty = true;
    int slot_active[DOTS_MAX_BATCH] = {0};
    int slot_limit[DOTS_MAX_BATCH] = {0};  // prompt length + generation cap of the slot's sequence (lowered when the page pool runs dry)
    int slot_prompt[DOTS_MAX_BATCH] = {0}; // prompt length
    int slot_ctx_ub[DOTS_MAX_BATCH] = {0}; // host-side upper bound of the slot's context: prompt + decode steps issued (finished rows stop earlier)
    int slot_done[DOTS_MAX_BATCH] = {0};   // seen finished at the last poll: grows no more
    int32_t *d_sel = nullptr, *d_sel_new = nullptr, *d_max_len = nullptr, *p_dst = nullptr;
    // shared-prefix attention (dots_set_shared_prefix_attention): the switch; share_dirty, raised with sel_dirty (whatever
    // changes slot_pages, slot_active, parked or slot_prompt) and lowered by the decode chunk that recomputes the plan; the plan's host and
    // device images (share_plan.h), allocated by the first chunk with the switch on; share_cap: the live item count rounded up to
    // SHARE_ITEM_QUANTUM (0: an empty plan — the step launches what it launches with the switch off); the last plan's counts and the
    // KV pages (one page of one kv head of one layer each) the chunks so far did not read
    bool share_on = false, share_dirty = true;
    int32_t* d_share = nullptr;
    std::vector<int32_t> h_share;
    int share_cap = 0;
    SharePlanCounts share_last{0, 0, 0, 0};
    int64_t share_pages_saved = 0;
    const int32_t* sel_now = nullptr;      // selection mask of the next select_tokens() call
    // what an admission uploads asynchronously, staged here so that it outlives the call (as hp_pos / hp_last do): the rows going live
    // (rows_go_live), and the mask [DOTS_MAX_BATCH] and slot list [DOTS_MAX_BATCH] of a first-token selection (stage_new_rows)
    std::vector<LiveRow> hp_live;
    std::vector<int32_t> hp_new;
    // ---- suspended sequences (dots_slot_suspend).  swap_host: pinned host memory of swap_total host pages, one host page =
    // one 64-token page of EVERY layer ([layer][page bytes], the staging layout of kv_swap.hip); swap_used[h] != 0: host page h is taken.
    // swap_stage / swap_list: the device staging buffer of KV_SWAP_CHUNK_PAGES host pages and the page list the kernels read, allocated by
    // the first suspend.  parked[slot]: the record of a suspended slot — per logical page of the row where its content is, and the
    // three device scalars of the row that an idle row loses
    uint8_t* swap_host = nullptr;
    int swap_total = 0, swap_free = 0, n_parked = 0;
    std::vector<uint8_t> swap_used;
    uint8_t* swap_stage = nullptr;
    int32_t* swap_list = nullptr;
    std::vector<int32_t> swap_list_host;
    struct Parked {
        bool on = false;
        // >= 0: a resident page the row still holds with others (page_refs > 1 at suspend); <= -2: host page -(v + 2); -1: a page without
        // content (taken ahead of the context), replaced by a fresh one at resume
        std::vector<int32_t> pages;
        int32_t cur_token = 0, ctx = 0, finished = 0;
    };
    Parked parked[DOTS_MAX_BATCH];
    // extending a live sequence (dots_slots_extend), allocated by the first call: the step-private row arrays of a chunk
    // (kernels.h ExtendRows), the hidden rows of the slots' last fed tokens ([max_batch][hidden], rows are slots: what the lm_head of the call
    // reads), and the call's staged lists (ex_stage, ex_stage_cap int32: regrown when a call packs more rows)
    int32_t *ex_tokens = nullptr, *ex_ctx = nullptr, *ex_table = nullptr, *ex_stage = nullptr;
    size_t ex_stage_cap = 0;
    bf16_t* ex_h = nullptr;
    // scoring given tokens (dots_slots_score), allocated by the first scoring call: the logits of a chunk's rows
    // ([max_batch][vocab] fp32 — not d_logits, whose rows are the slots'), the logprob stage's scratch over them and the entries' values
    // ([max_batch][max_seq_len], rows are slots); the top lists ([..][DOTS_MAX_TOP_LOGPROBS]) by the first call that asks for one.
    // sc_n[slot]: 1 + the entries the slot's last score recorded, 0 = not scored since it was filled or extended
    float *sc_logits = nullptr, *sc_ms = nullptr, *sc_pv = nullptr, *sc_tok = nullptr, *sc_top = nullptr;
    int32_t *sc_pi = nullptr, *sc_ids = nullptr;
    int sc_n[DOTS_MAX_BATCH] = {0};
    // chunked prefill (dots_slots_prefill_begin / dots_slots_prefill_advance).  fill[slot]: the record of a FILLING slot — not
    // occupied yet (slot_active == 0), so every step treats its row as a free one: context 0, and the DEVICE block-table row stays on the
    // scratch page until the fill completes, while hp_table and fill_table (the table the passes read) name its pages.  src: the prompt as
    // launch_embed_gather reads it; seen: its prompt-presence bits, accumulated pass by pass on the host; order: begin order (FIFO).
    // Allocated by the first begin: fill_x, the embedded prompts ([(n_pool_pages) * 64][hidden], position p of a slot at row page * 64 +
    // p % 64 of its own KV page — the pool's allocator is the staging buffer's), and the lists of a pass (staging rows, work items)
    struct Fill {
        bool on = false;
        int L = 0, max_new = 0, cursor = 0;
        uint64_t order = 0;
        std::vector<int32_t> src;
        std::vector<uint32_t> seen;
        // prefix cache: the pass that completes a full prompt page inserts it behind cache_parent (-1: the root) while
        // cache is set; ids: the prompt as given (the blocks' identity), key: its image's
        bool cache = false, keyed = false;
        int32_t cache_parent = -1;
        uint8_t key[16] = {0};
        std::vector<int32_t> ids;
    };
    Fill fill[DOTS_MAX_BATCH];
    int n_filling = 0;
    uint64_t fill_order = 0;
    bf16_t* fill_x = nullptr;
    int32_t *fill_rows = nullptr, *fill_table = nullptr;
    PagedQBlock* fill_items = nullptr;
    std::vector<int32_t> hp_rows;
    std::vector<PagedQBlock> hp_items;
    // prefix cache (dots_prefix_cache_enable): the block index (csrc/prefix_cache.h) over page_refs, nullptr = off.  The tower
    // rows a block retains are the rows of its page in fill_x, which nobody writes while the page is held
    prefix_cache::Index* pc = nullptr;
    bool fresh_chunked = false;            // fresh_slots were completed by a pass: p_src holds that pass only (dots_slots_fork copies the source's presence bits)
    // captured decode steps, keyed by everything the capture bakes in: rows, KV splits, static batch (out_cap = row stride of
    // the output buffer) or slot mode (out_cap = 0), number of EOS ids, whether any row carries its own parameters (rowp: the per-row
    // selection stage), whether any row returns logprobs (lp), whether any row carries logit rules (rules: the stage then gets their
    // table), whether any row holds a guide (guided: the mask kernel and the guides' tables), whether any row carries an n-gram rule (ngram:
    // the ban kernel and its bits), the draft count of a speculating step (spec: 0 = the plain step), whether that step draws the draft
    // rows of sampled slots (draw: the two launches of launch_spec_draw), whether some guided row may speculate in it (gspec: the three
    // launches that select the draft rows of guided slots under their guide), which shaped rows may (sspec: the
    // DOTS_SPEC_SHAPED_* bits that are switched on and held by some row — the draft rows' ban kernel and their shaped selection), whether
    // some row with logprobs may (lpspec: the draft rows' logprob pair and the accept record); engine-wide sampling changes drop
    // the cache (dots_set_sampling), per-row ones live in device memory; beam: the group entries a step's beam kernels run over (0: none);
    // share: the item capacity of a non-empty shared-prefix plan (the shared kernel's grid and the SKIP instantiation of the per-split
    // kernel; 0: neither — the live item count itself is device memory); pred: whether some slot holds a prediction while the built-in
    // drafter runs (the second drafter launch).  step_key() builds the key from the engine's state: a
    // feature that changes what a step launches adds a member here and a line there
    struct StepKey {
        int rows, splits, out_cap, n_eos, part, rowp, lp, rules, guided, ngram, spec, draw, gspec, sspec, lpspec, beam, share, pred;
        bool operator==(const StepKey& o) const { return std::memcmp(this, &o, sizeof(StepKey)) == 0; }
    };
    static_assert(std::has_unique_object_representations_v<StepKey>, "StepKey is compared bytewise: plain ints, no padding");
    struct StepGraph { StepKey key; hipGraph_t graph; hipGraphExec_t exec; };
    std::vector<StepGraph> step_graphs;
    std::vector<int> h_prompt_lens;
    int steps_done = 0;

    // ---- image preprocessing scratch (grown on demand)
    uint8_t *pp_in = nullptr, *pp_tmp = nullptr, *pp_out = nullptr;
    int32_t* pp_tab = nullptr;
    size_t pp_in_cap = 0, pp_tmp_cap = 0, pp_out_cap = 0, pp_tab_cap = 0;

    // ---- debug: residual stream after every ViT block / LM prefill layer (dots_debug_capture_hidden)
    bf16_t* dbg_hidden = nullptr;
    size_t dbg_cap = 0;                    // elements
    int64_t dbg_vit_rows = 0, dbg_lm_rows = 0;

    // ---- timing
    hipEvent_t ev[8]{};
    std::vector<hipEvent_t> attn_ev;
    DotsStats stats{};
    int attn_pairs = 0;

    int fail(int code, const char* fmt, ...) {
        char buf[1024];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(buf, sizeof(buf), fmt, ap);
        va_end(ap);
        err = buf;
        return code;
    }
    template <typename T>
    hipError_t alloc(T** p, size_t count) {
        void* q = nullptr;
        hipError_t e = hipMalloc(&q, std::max<size_t>(count * sizeof(T), 256));
        if (e != hipSuccess) return e;
        allocs.push_back(q);
        *p = reinterpret_cast<T*>(q);
        return hipMemsetAsync(q, 0, std::max<size_t>(count * sizeof(T), 256), stream);
    }
    void release(void* p) {
        if (!p) return;
        auto it = std::find(allocs.begin(), allocs.end(), p);
        if (it != allocs.end()) allocs.erase(it);
        hipFree(p);
    }
};

static_assert(sizeof(RowParams) == sizeof(DotsSamplingParams) && offsetof(RowParams, seed) == offsetof(DotsSamplingParams, seed) &&
                  offsetof(RowParams, presence_penalty) == offsetof(DotsSamplingParams, presence_penalty),
              "RowParams (kernels.h) must mirror DotsSamplingParams");

#define CK(expr)                                                                                         \
    do {                                                                                                 \
        hipError_t e_ = (expr);                                                                          \
        if (e_ != hipSuccess) return e->fail(DOTS_E_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

#define RET(x) do { int r_ = (x); if (r_ != DOTS_OK) return r_; } while (0)

// scratch device buffers of the single-kernel entry points, released (after a stream sync) on scope exit
struct Scratch {
    DotsEngine* e;
    std::vector<void*> ptrs;
    explicit Scratch(DotsEngine* e_) : e(e_) {}
    template <typename T>
    hipError_t get(T** p, size_t n) {
        hipError_t r = e->alloc(p, n);
        if (r == hipSuccess) ptrs.push_back(*p);
        return r;
    }
    ~Scratch() {
        hipStreamSynchronize(e->stream);
        for (void* p : ptrs) e->release(p);
    }
};

// ---- host functions called across the engine's sources.  A function one source alone uses is in an anonymous namespace there.
namespace engine {

inline int64_t round_up(int64_t a, int64_t b) { return (a + b - 1) / b * b; }

// weights.hip
int alloc_workspaces(DotsEngine* e);
// slots.hip: the KV page allocator
hipError_t upload_table_row(DotsEngine* e, int slot);
void release_pages(DotsEngine* e, int slot);
bool reserve_pages(DotsEngine* e, int slot, int tokens);
int admit_tokens(const DotsEngine* e, int prompt, int max_new);
int grow_pages(DotsEngine* e, int slot, int tokens, bool* changed);
// the first n entries of the slot's (empty) row name another holder's pages, which nobody writes any more: one more holder of each
void share_pages(DotsEngine* e, int slot, const int32_t* pages, int n);
// the prefix cache's evictable pages count as free: ensure_free moves up to `need` of them into the free list (off: nothing happens)
void ensure_free(DotsEngine* e, int64_t need);
int free_count(const DotsEngine* e);
inline size_t kv_page_bytes(const DotsEngine* e) { return (size_t)e->cfg.num_kv_heads * 2 * 8192 * (e->kv8 ? 1 : 2); }      // one page of one layer
// gives the pages of a list of slots back unless disarmed: between an admission's first page and its success the slots are not occupied,
// so dots_slot_release would refuse them.  upload: the device table rows follow (not a filling slot's, which stays on the scratch page)
struct PageGuard {
    DotsEngine* e; const int32_t* slots; int n; bool upload, armed = true;
    ~PageGuard() {
        for (int i = 0; armed && i < n; ++i) {
            release_pages(e, slots[i]);
            if (upload) (void)upload_table_row(e, slots[i]);
        }
    }
};
// slots.hip: what admitting a slot consists of, shared by prefill, chunked fill, fork, beam group and extend
inline bool slot_occupied(const DotsEngine* e, int slot) { return e->slot_mode && slot >= 0 && slot < e->cfg.max_batch && e->slot_active[slot]; }
int check_free_slot(DotsEngine* e, const int32_t* slots, int i, int src = -1, const char* src_of = "");
int check_prompt(DotsEngine* e, int b, int len, const int32_t* slots, const int32_t* max_new);
int map_prompt(DotsEngine* e, const int32_t* ids, int n, bool no_tower, int32_t* src, int64_t* vis_used);
int check_vis_rows(DotsEngine* e, int64_t vis_used);
int enter_slot_mode(DotsEngine* e);
int rows_go_live(DotsEngine* e, const std::vector<LiveRow>& rows, bool clear_lp = true);
int stage_new_rows(DotsEngine* e, const std::vector<LiveRow>& rows, int32_t* d_list, int* n_rows);
int restart_automata(DotsEngine* e, const int32_t* d_rows, int n, bool stops = true);
int select_first_tokens(DotsEngine* e, int rows, const bf16_t* h, bf16_t* xn = nullptr);
void mark_live(DotsEngine* e, const LiveRow* rows, int n, bool occupy = true);
// rows.hip: what a row is selected with
StepState step_state(const DotsEngine* e, int advance, const int32_t* sel);
bool spec_draws(const DotsEngine* e);
bool spec_guides(const DotsEngine* e);
bool spec_lps(const DotsEngine* e);
int spec_shapes(const DotsEngine* e);
RowSel spec_row_sel(const DotsEngine* e);
GuideSel guide_sel(const DotsEngine* e);
SpecState spec_state(const DotsEngine* e);
bool spec_predicts(const DotsEngine* e);
PredictState predict_state(const DotsEngine* e);
int clear_row_prediction(DotsEngine* e, int row);
hipError_t launch_row_stage(hipStream_t s, const float* logits, int V, int ld, int B, const RowSel& rs, float* am_val, int32_t* am_idx,
                            const StepState& st, const int32_t* ban_finished);
int select_tokens(DotsEngine* e, int advance);
int clear_row_feature(DotsEngine* e, int row, RowFeature f);
int hold_row_stop(DotsEngine* e, int row, int id, int min_tokens);
int hold_row_loop(DotsEngine* e, int row, const DotsLoopRule& r);
LoopSel loop_sel(const DotsEngine* e);
int check_row_params(DotsEngine* e, const DotsSamplingParams& p, RowParams* out);
int check_logit_rules(DotsEngine* e, const DotsLogitRules& r, int V, const int32_t* eos, int n_eos, RowRules* out);
int check_ngram_rule(DotsEngine* e, const DotsNgramRule& r, int V, int max_len, RowNgram* out);
int clear_lp_row(DotsEngine* e, int row);
int set_row_lp(DotsEngine* e, int row, int top_n);
// engine.hip: the step
void build_worklists(const std::vector<int>& lens, int Hq, std::vector<Tile64>& tiles, std::vector<QBlock>& qblocks, int64_t* Tpad_used,
                     const int* seq_ids = nullptr);
void drop_step_graphs(DotsEngine* e);
int chain_streams(DotsEngine* e, hipStream_t from, hipStream_t to);
int pick_decode_stream(DotsEngine* e, hipStream_t* cur);
int prefill(DotsEngine* e, const int32_t* ids, const int32_t* lens, int B, const int32_t* slots = nullptr, const int32_t* max_new = nullptr);
// chunked prefill: a filling slot holds pages and staged rows but is not occupied
// leases / keys (both or neither): dots_slots_prefill_begin_cached — a prompt with a lease starts behind its cached pages
int prefill_begin(DotsEngine* e, const int32_t* ids, const int32_t* lens, int B, const int32_t* slots, const int32_t* max_new, const int32_t* leases = nullptr,
                  const uint8_t* const* keys = nullptr);
int prefill_advance(DotsEngine* e, int max_tokens, int32_t* remaining);
inline bool slot_filling(const DotsEngine* e, int slot) { return slot >= 0 && slot < DOTS_MAX_BATCH && e->fill[slot].on; }
void drop_fill(DotsEngine* e, int slot);      // the record only: the pages go with release_pages
int decode_layers(DotsEngine* e, const int32_t* tokens, const int32_t* ctx_len, const int32_t* block_table, int B, int n_splits, int part, bool* pend,
                  const float** pend_scale, const SharePlanDev* share = nullptr);
// the shared-prefix plan of the step as the engine stands: the plain slot step with the switch on and a non-empty plan, else {nullptr, 0}
inline SharePlanDev share_plan_now(const DotsEngine* e) {
    return e->share_on && e->slot_mode && !e->spec_k && e->share_cap > 0 ? SharePlanDev{e->d_share, e->share_cap} : SharePlanDev{nullptr, 0};
}
int decode_step_launches(DotsEngine* e, int n_splits, int part = 0);
int splits_for_ctx(int max_ctx);
int step_graph(DotsEngine* e, int rows, int n_splits, int out_cap, hipGraphExec_t* exec, int part = 0);
// slots.hip: a suspended slot: occupied, its KV parked in host memory (dots_slot_suspend)
inline bool slot_parked(const DotsEngine* e, int slot) { return slot >= 0 && slot < DOTS_MAX_BATCH && e->parked[slot].on; }
void swap_free_host(DotsEngine* e);
// slots.hip: what a poll does to the host record with the device's finished / out_lens (dots_slots_poll, dots_slots_drain)
void poll_host_state(DotsEngine* e, int32_t* finished, int32_t* out_lens);
// stream.hip: the rows' stream cursors
int stream_restart_row(DotsEngine* e, int row);
int stream_reset(DotsEngine* e);
void stream_free_host(DotsEngine* e);
// beam.hip: beam groups
int beam_step(DotsEngine* e, int rows);
int beam_before_decode(DotsEngine* e, int n_steps);
int beam_release_group(DotsEngine* e, int slot);
int beam_clear_all(DotsEngine* e);
// a group row carries no stage feature and no logprobs: the row setters refuse it (BEAM_ROW_TAKES_NONE: their common sentence)
#define BEAM_ROW_TAKES_NONE "slot %d is a row of a beam group: it takes no row parameters, rules, guide, n-gram rule, stop strings, loop guard or logprobs"
inline bool beam_row(const DotsEngine* e, int row) { return row >= 0 && row < DOTS_MAX_BATCH && e->beam_of[row] != 0; }

}  // namespace engine
