// Host-side launchers of the gfx950 kernels (one per .hip translation unit).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

typedef uint16_t bf16_t;

#define DOTS_MAX_BATCH 64     // sequences per decode step: 4 tiles of 16 rows (decode_layout.h MAX_DECODE_ROWS)

enum { EPI_NONE = 0, EPI_RESIDUAL = 1, EPI_SWIGLU = 2, EPI_GELU = 3, EPI_F32 = 4, EPI_QKROPE = 5 /* launch_gemm_qk_rope only */ };

// ---- gemm.hip
hipError_t launch_gemm(hipStream_t s, const bf16_t* A, const bf16_t* W, const bf16_t* bias, const bf16_t* R,
                       void* C, int64_t M, int N, int K, int lda, int ldc, int epi, const float* colscale = nullptr);
int gemm_get_plan();            // 0 = 8-wave ping-pong kernel, 1 = one wave per SIMD (gemm.hip); process-wide
void gemm_set_plan(int plan);
// colscale: fp32 [N] multiplied into the accumulator column before bias (fp8 weights: W holds bf16(q), quant.hip), or nullptr

// ---- elementwise.hip
hipError_t launch_rmsnorm(hipStream_t s, const bf16_t* x, const bf16_t* w, bf16_t* y, int64_t rows, int dim, float eps);
hipError_t launch_layernorm(hipStream_t s, const bf16_t* x, const bf16_t* w, const bf16_t* b, bf16_t* y,
                            int64_t rows, int dim, float eps);
// f32 [rows, in_dim] -> bf16 [rows, out_dim] (zero padded columns), the patch-embed GEMM's A operand
hipError_t launch_patch_prep(hipStream_t s, const float* x, bf16_t* y, int64_t rows, int in_dim, int out_dim);
// cos/sin tables [T, 64] float2.  2-D: pos [T,2] (h,w), 32 frequencies per axis; 1-D: pos [T], 64 frequencies.
hipError_t launch_rope_table(hipStream_t s, const int32_t* pos, const float* inv_freq, float2* cs, int64_t T, int two_d);
// Work item of the 64-token tile kernels: tok0 = first packed token, n = valid tokens (<=64),
// pad0 = first padded position in the V^T buffer.
struct Tile64 { int32_t tok0, n, pad0, seq, page, _pad; };   // page = tile index inside its sequence
hipError_t launch_qkv_rope_split(hipStream_t s, const bf16_t* qkv, const float2* cs, const Tile64* tiles, int n_tiles,
                                 bf16_t* q, bf16_t* k, bf16_t* vt, int64_t T, int64_t Tpad, int Hq, int Hkv, bool v_only = false);
// ---- gemm.hip: the fused qkv projection of a prefill pass with the rotary embedding in its epilogue (round 6).  C = A W^T (+ bias) as launch_gemm
// with EPI_NONE, rounded to bf16 as that GEMM would store it, then: columns [0, (Hq + Hkv) * 128) — the q and k heads — are rotated with cs[t]
// (the arithmetic of qkv_rope_split_kernel, bit for bit) and written head-major into q [Hq][T][128] / k [Hkv][T][128]; the v columns go to
// qkv [T][ldc] unrotated (launch_qkv_rope_split(.., v_only = true) transposes them).  hipErrorNotSupported when the shape or the process's GEMM
// plan has no such kernel (the caller then runs launch_gemm + launch_qkv_rope_split).
struct QkRope { const float2* cs; bf16_t* q; bf16_t* k; long long T; int Hq; int n_rope_heads; };
hipError_t launch_gemm_qk_rope(hipStream_t s, const bf16_t* A, const bf16_t* W, const bf16_t* bias, bf16_t* qkv, int64_t M, int N, int K, int lda, int ldc,
                               const float2* cs, bf16_t* q, bf16_t* k, int Hq, int Hkv);
// x[t] = src[t] >= 0 ? embed[src[t]] : vision[-src[t]-1]
hipError_t launch_embed_gather(hipStream_t s, const int32_t* src, const bf16_t* embed, const bf16_t* vision, bf16_t* x,
                               int64_t T, int dim);
// y[dst ? dst[r] : r] = x[rows[r]]
hipError_t launch_gather_rows(hipStream_t s, const bf16_t* x, const int32_t* rows, const int32_t* dst, bf16_t* y, int n, int dim);

// ---- attn_prefill.hip
// One work item = (sequence, head, 128-row query block); the list is ordered seq-major, then head, then block, so that
// the XCD-contiguous remap of the 1-D grid gives one XCD (one L2) all query blocks that stream the same K/V.
struct QBlock { int32_t q0, n, tok0, pad0, head, _pad; };   // first row in seq, seq length, packed token offset, padded V^T offset
int flash_rows_per_block();      // 128 or 256 query rows per QBlock work item (what build_worklists must use)
// Which contiguous chunk of the QBlock list each XCD walks (workgroup i runs on XCD i % 8 and takes item base[i % 8] + i / 8; workgroups past
// cnt[] exit at once).  xcd_remap's chunks hold equal COUNTS; a block costs its sequence's KV tiles, so on a ragged batch (mixed page
// sizes) equal counts gave one XCD 1.32 x the mean work while the others idled (round 5, mixed64's towers).  make_xcd_plan cuts the list
// by COST instead (prefix-sum split: chunks stay contiguous, so the blocks of a (sequence, head) still share an L2); equal lengths give
// xcd_remap's chunks exactly.  nullptr = xcd_remap.
struct XcdPlan { int32_t base[8], cnt[8]; };
XcdPlan make_xcd_plan(const QBlock* blocks_host, int n_blocks);
hipError_t launch_flash_attn(hipStream_t s, const bf16_t* q, const bf16_t* k, const bf16_t* vt, bf16_t* out,
                             const QBlock* blocks, int n_blocks, int64_t T, int64_t Tpad, int Hq, int Hkv,
                             int causal, float scale, const XcdPlan* plan = nullptr);

// ---- attn_paged.hip: causal flash attention of a block of query rows over a sequence's own KV pages (chunked prefill)
// One work item = one 64-position query block of one sequence: positions [q0, q0 + n), q0 % 64 == 0, 1 <= n <= 64; its q rows are rows
// tok0 .. tok0 + n - 1 of q [Hq][T][128] (rope applied) and of out [T][Hq * 128]; its keys are pages 0 .. q0 / 64 of block-table row seq.
struct PagedQBlock { int32_t tok0, n, q0, seq; };
// items_host / items_dev: the same n_items work items; the host copy is checked before the launch (hipErrorInvalidValue for a q0 that is
// no multiple of 64, a block outside [1, 64] rows, T, max_pages or the table's table_rows rows).  kv_scales as below.
hipError_t launch_flash_attn_paged(hipStream_t s, const bf16_t* q, const void* pool_layer, const int32_t* block_table, int max_pages, int table_rows,
                                   const PagedQBlock* items_host, const PagedQBlock* items_dev, int n_items, bf16_t* out, int64_t T, int Hq, int Hkv,
                                   float scale, const float* kv_scales = nullptr);

// ---- decode.hip  (KV page pool layout documented there)
// Every launcher that touches the page pool takes kv_scales: nullptr = a bf16 pool; else pool_layer is an fp8 (e4m3fn) pool and kv_scales
// the device array [Hkv][K | V] of this layer's fp32 scales (DotsConfig.kv_cache_dtype = 1).
hipError_t launch_kv_to_pages(hipStream_t s, const bf16_t* k, const bf16_t* qkv, const Tile64* tiles, int n_tiles,
                              const int32_t* block_table, int max_pages, void* pool_layer, int64_t T, int Hq, int Hkv,
                              const float* kv_scales = nullptr);
// ---- kv_fork.hip: the tail-page copy of dots_slots_fork.  In every one of `layers` layers (layer_bytes apart) page src_page is
// copied whole (page_bytes = Hkv x 2 x 8192 elements, bf16 or e4m3) to the n pages dst_pages[0 .. n) (device array, n < DOTS_MAX_BATCH);
// the caller guarantees that every index names a page of the pool and that no destination is the source
hipError_t launch_kv_fork_pages(hipStream_t s, void* pool, size_t layer_bytes, size_t page_bytes, int layers, int src_page, const int32_t* dst_pages,
                                int n);
// ---- kv_swap.hip: the page moves of dots_slot_suspend / dots_slot_resume.  The n <= KV_SWAP_CHUNK_PAGES pages pages[0 .. n)
// (device array) of every one of `layers` layers are packed into / unpacked from the device staging buffer `stage`, laid out
// [page j][layer][page_bytes].  Pages are copied whole, as in kv_fork.hip; the caller guarantees that every index names a page of the pool
// and that `stage` holds n x layers x page_bytes bytes
constexpr int KV_SWAP_CHUNK_PAGES = 32;
hipError_t launch_kv_gather_pages(hipStream_t s, const void* pool, size_t layer_bytes, size_t page_bytes, int layers, void* stage, const int32_t* pages,
                                  int n);
hipError_t launch_kv_scatter_pages(hipStream_t s, void* pool, size_t layer_bytes, size_t page_bytes, int layers, const void* stage, const int32_t* pages,
                                   int n);
// ---- decode_fused.hip: dense layers of the decode step with in-workgroup split-K and fused prologues/epilogues.
// Activations between them travel as X images [K/8][XR][8], XR = 8 (B <= 8) or 16 (decode_layout.h).
hipError_t launch_dec_embed(hipStream_t s, const int32_t* tokens, const bf16_t* embed, bf16_t* h, int B, int dim);
// Wd + wscale: wscale == nullptr -> Wd is the bf16 fragment image (launch_pack_frag*); else Wd is the e4m3 fragment image
// (launch_pack_frag_fp8) and wscale[row] its fp32 per-output-channel scales (quant.hip).
// xn: scratch for the normalised rows of batches above 32 rows (MAX_DECODE_ROWS x H bf16; decode_b64.hip) or nullptr = the round-4 two-tile kernels.
// pend / pend_scale (qkv, gate|up, lm_head): the K-quarter sums a preceding launch_dec_proj left in `part` instead of updating h (+ that projection's fp8 weight scales or
// nullptr): the residual update is applied first — fused into the norm kernel on the xn path, by a launch of its own otherwise.
hipError_t launch_dec_qkv(hipStream_t s, const bf16_t* h, const bf16_t* ln_w, const void* Wd, const float* wscale, const bf16_t* bias,
                          const float* inv_freq, const int32_t* ctx_len, const int32_t* block_table, int max_pages,
                          void* pool_layer, bf16_t* q_out, int B, int H, int Hq, int Hkv, float eps, int part_cus = 0, bf16_t* xn = nullptr,
                          const float* pend = nullptr, const float* pend_scale = nullptr, const float* kv_scales = nullptr);
// h += X @ W^T.  part != nullptr (DEC_KSPLIT_PARTS x DOTS_MAX_BATCH x N fp32) allows the K-split kernel above 32 rows: *pending is then set and h is NOT
// updated by this launch — pass `part` (and wscale) as pend / pend_scale to the next launch_dec_qkv / launch_dec_gateup / launch_dec_lmhead, or call launch_dec_norm_ximg(.., part, ..)
hipError_t launch_dec_proj(hipStream_t s, const bf16_t* X, const void* Wd, const float* wscale, bf16_t* h, int B, int N, int K, int part_cus = 0,
                           float* part = nullptr, bool* pending = nullptr);
// part_cus > 0 (all dense launchers): the stream is CU-masked to that many CUs.  qkv / proj: whole 16-row weight tiles per workgroup at B <= 16,
// one round of wide workgroups above; gate|up: the grid is capped at what the CUs hold at once, the workgroups walk the (gate, up) tile pairs
hipError_t launch_dec_gateup(hipStream_t s, const bf16_t* h, const bf16_t* ln_w, const void* W13d, const float* wscale, bf16_t* act,
                             int B, int H, int I, float eps, int part_cus = 0, bf16_t* xn = nullptr, const float* pend = nullptr, const float* pend_scale = nullptr);
hipError_t launch_dec_lmhead(hipStream_t s, const bf16_t* h, const bf16_t* ln_w, const void* Wd, const float* wscale, float* logits,
                             int B, int H, int V, float eps, int part_cus = 0, bf16_t* xn = nullptr, const float* pend = nullptr, const float* pend_scale = nullptr);
// ---- decode_b64.hip (round 6): batches above 32 rows — all four 16-row batch tiles in one workgroup, every weight byte crosses a CU once
bool dec_stream64_supports(int B, int H);
// rows -> [pending residual update ->] rmsnorm -> X image (xn == nullptr with part != nullptr: the residual update only)
hipError_t launch_dec_norm_ximg(hipStream_t s, const bf16_t* h, const bf16_t* ln_w, bf16_t* xn, int B, int H, float eps, const float* part = nullptr, const float* pscale = nullptr);
hipError_t launch_dec_gateup64(hipStream_t s, const bf16_t* h, const bf16_t* ln_w, const void* W13d, const float* wscale, bf16_t* act, bf16_t* xn,
                               int B, int H, int I, float eps, int cus, const float* pend = nullptr, const float* pend_scale = nullptr);
hipError_t launch_dec_lmhead64(hipStream_t s, const bf16_t* h, const bf16_t* ln_w, const void* Wd, const float* wscale, float* logits, bf16_t* xn,
                               int B, int H, int V, float eps, int cus, const float* pend = nullptr, const float* pend_scale = nullptr);
constexpr int DEC_KSPLIT_PARTS = 4;          // K quarters of the K-split projection; part buffers hold DEC_KSPLIT_PARTS x DOTS_MAX_BATCH x N fp32
bool dec_proj_ksplit_supports(int B, int N, int K);
hipError_t launch_dec_proj_ksplit(hipStream_t s, const bf16_t* X, const void* Wd, bool fp8, float* part, int B, int N, int K, int cus);
// Shared-prefix attention: the device image of a plan (share_plan.h) and the item capacity the shared kernel's grid is sized
// for — workgroups at or past the live item count (plan[0], read on the device) exit at once.  nullptr / cap 0: the step launches nothing of it
struct SharePlanDev { const int32_t* plan; int cap; };
int decode_attn_waves();                       // pages in flight per decode-attention workgroup (engine constant)
int decode_attn_splits(int max_seq_len);       // KV splits for a context capacity: ceil(pages / waves), at most 64
hipError_t launch_decode_attn(hipStream_t s, const bf16_t* q, const void* pool_layer, const int32_t* ctx_len,
                              const int32_t* block_table, int max_pages, float* part_o, float* part_ml,
                              int B, int Hq, int Hkv, int n_splits, float scale, int part_cus = 0, int stream_mode = -1,
                              const float* kv_scales = nullptr, const SharePlanDev* share = nullptr);
// > 0: launch_decode_attn runs the streaming kernel (round 5) with that many resident workgroups; 0: one workgroup per (row, kv head, split).
// part_cus > 0: the stream is CU-masked to that many CUs; stream_mode 1 / 0 / -1 = always where legal / never / by items per CU; kv8: an fp8 pool (always 0)
int decode_attn_stream_wgs(int B, int Hkv, int n_splits, int max_pages, int part_cus, int stream_mode = -1, bool kv8 = false);
hipError_t launch_decode_attn_combine(hipStream_t s, const float* part_o, const float* part_ml, const int32_t* ctx_len, bf16_t* out,
                                      int B, int Hq, int Hkv, int n_splits);
// Per-step token bookkeeping state (device pointers), shared by the arg-max and the sampling kernels.
//   sel     rows (slots) to act on this call, or nullptr = all B rows
//   max_len per-row cap on generated tokens, or nullptr = `cap` for every row
struct StepState {
    int32_t *cur_tokens, *ctx_len, *out_ids, *out_lens, *finished;
    const int32_t *eos_ids, *sel, *max_len;
    int n_eos, out_stride, cap, advance_ctx;
};
hipError_t launch_argmax_step(hipStream_t s, const float* logits, int V, int ld, int B, float* pval, int32_t* pidx, const StepState& st);
// own != nullptr: skip the rows with own[b] != 0 (they carry per-row parameters: launch_select_rows)
hipError_t launch_sample_step(hipStream_t s, const float* logits, int V, int ld, int B, float temperature, float top_p, uint64_t seed,
                              const StepState& st, const int32_t* own = nullptr);
// Per-row token selection (decode.hip).  RowParams mirrors DotsSamplingParams (include/dots_ocr_hip.h) field for field.
struct RowParams { float temperature, top_p; int32_t top_k; float repetition_penalty, frequency_penalty, presence_penalty; uint64_t seed; };
// Device state of the stage.  params / own: [DOTS_MAX_BATCH]; a row with own[b] == 0 follows the engine-wide setting: the stage selects it
// only when legacy_greedy != 0 (arg max), otherwise launch_sample_step(.., own) does.  cnt [rows][V] int32 (generated-token counts),
// seen [rows][ceil(V / 32)] (prompt-presence bits) and pen [rows][V] fp32 (penalised logits, scratch) are nullptr until a penalty is used.
// Logit rules of a row.  flags: RULE_ON = the row carries rules (it always has own[b] != 0 too), RULE_IMG = its row of the
// dense "bias or -inf" image is live (a bias or an allowed list), RULE_IGNORE_EOS.  While the row has generated fewer than min_tokens
// tokens every engine EOS id and every stop id is -inf; a stop id finishes the row as an EOS id does.
#ifndef DOTS_MAX_STOP_IDS
#define DOTS_MAX_STOP_IDS 16
#endif
enum { RULE_ON = 1, RULE_IMG = 2, RULE_IGNORE_EOS = 4 };
struct RowRules { int32_t flags, min_tokens, n_stop, stop[DOTS_MAX_STOP_IDS]; };
// Guided decoding.  A guide is a byte DFA in device memory: table [n_states][256] uint16 (GUIDE_DEAD = no transition; every other
// entry < n_states) and accepting [n_states] uint8.  RowGuide: the guide a row holds (table == nullptr: none) and the state its automaton
// is in; the commit of a token walks that token's bytes from it.  GuideSel: what a launch of the per-row stage needs to honour the guides —
// the row table, the allowed bits guide_mask_kernel leaves ([rows][words] uint32, words = guide_mask_words(V): even, so that a wave's 64
// bits are one aligned 8-byte store), and the packed bytes of every vocabulary entry (tok_off [V + 1], tok_bytes; an entry without bytes can
// never be selected on a guided row).  rows == nullptr = no row of this launch is guided.
constexpr uint16_t GUIDE_DEAD = 0xFFFF;
struct RowGuide { const uint16_t* table; const uint8_t* accepting; int32_t n_states, start, state, _pad; };
struct GuideSel { RowGuide* rows; uint32_t* mask; const int32_t* tok_off; const uint8_t* tok_bytes; int32_t words, V; };
inline int guide_mask_words(int V) { return ((V + 63) / 64) * 2; }
// No-repeat n-gram blocking.  RowNgram: the rule a row carries (n == 0: none).  With out[0 .. L) the tokens the row has
// generated and P = out[L - n + 1 .. L), the id out[i + n - 1] is banned for every i in [max(0, L - window), L - n] (window == 0: from 0)
// with out[i .. i + n - 1) == P, unless it is one of the n_white ids of white.  NgramSel: what a launch of the per-row stage needs — the
// row table and the banned bits ngram_ban_kernel leaves ([rows][words] uint32, words = ngram_mask_words(V); bit t set = token t is -inf).
// rows == nullptr = no row of this launch carries an n-gram rule.
#ifndef DOTS_MAX_NGRAM_SIZE
#define DOTS_MAX_NGRAM_SIZE 64
#endif
#ifndef DOTS_MAX_NGRAM_WHITELIST
#define DOTS_MAX_NGRAM_WHITELIST 16
#endif
struct RowNgram { int32_t n, window, n_white, white[DOTS_MAX_NGRAM_WHITELIST]; };
struct NgramSel { const RowNgram* rows; uint32_t* mask; int32_t words, V; };
inline int ngram_mask_words(int V) { return (V + 31) / 32; }
constexpr int NGRAM_MAX_V = 64 * 1024 * 8;     // the banned bits of one row are built in LDS: 64 KB per workgroup
// Stop strings.  A stop automaton is the Aho-Corasick automaton of a row's stop strings with its failure links folded into a
// dense byte DFA in device memory: table [n_states][256] uint16 (every entry < n_states: there is no dead state; state 0 is the root),
// match_len [n_states] uint16 (bytes of the longest listed string that ends at the state, 0: none) and match_id [n_states] uint8 (its index
// in the caller's list).  RowStop: the automaton a row holds (table == nullptr: none), the state it is in, and the hit record the commit
// that finishes the row leaves (hit_tok == -1: no hit yet; step_dev.h stop_walk).  StopSel: what a launch of the per-row stage needs — the
// row table and the packed bytes of every vocabulary entry.  rows == nullptr = no row of this engine ever held stop strings.
#ifndef DOTS_MAX_STOP_STRINGS
#define DOTS_MAX_STOP_STRINGS 16
#endif
#ifndef DOTS_MAX_STOP_BYTES
#define DOTS_MAX_STOP_BYTES 64
#endif
constexpr int STOP_MAX_STATES = DOTS_MAX_STOP_STRINGS * DOTS_MAX_STOP_BYTES + 1;
struct RowStop {
    const uint16_t* table;
    const uint16_t* match_len;
    const uint8_t* match_id;
    int32_t n_states, state, min_tokens, hit_tok, hit_bytes, hit_len, hit_id, _pad;
};
struct StopSel { RowStop* rows; const int32_t* tok_off; const uint8_t* tok_bytes; int32_t V, _pad; };
// Loop guard.  RowLoop: the rule a row holds (max_period == 0: none) and the hit record the commit that fires it leaves
// (hit_tok == -1: no hit yet).  With out[0 .. n] the row's output, period p in [min_period, max_period] fires after the commit of out[n]
// iff out[i] == out[i - p] for the last L(p) - p indices i, L(p) = max(repeats * p, min_span) (loop_dev.h).  LoopSel: what a launch of the
// per-row stage needs — the row table and the run counters run[DOTS_MAX_BATCH][DOTS_MAX_LOOP_PERIOD] (run[b][p - 1] = the consecutive
// indices up to the last commit with out[i] == out[i - p]).  rows == nullptr = no row of this engine ever held a loop rule.
#ifndef DOTS_MAX_LOOP_PERIOD
#define DOTS_MAX_LOOP_PERIOD 1024
#endif
struct RowLoop { int32_t min_period, max_period, repeats, min_span, hit_tok, period, span, _pad; };
struct LoopSel { RowLoop* rows; int32_t* run; };
struct RowSel {
    const RowParams* params;
    const int32_t* own;
    int32_t* cnt;
    const uint32_t* seen;
    float* pen;                 // [rows][V] scratch: the shaped (ruled and / or penalised) logits of the rows that have any
    uint32_t* thr;              // [DOTS_MAX_BATCH] scratch: the largest key a sampled row keeps (decode.hip)
    int legacy_greedy;
    const RowRules* rules;      // [DOTS_MAX_BATCH], or nullptr = no row of this launch carries rules
    const float* rule_img;      // [rows][V] fp32: the bias of a token, -inf for a banned / not allowed one, 0 elsewhere
    GuideSel guide;             // guide.rows == nullptr = no row of this launch is guided
    NgramSel ngram;             // ngram.rows == nullptr = no row of this launch carries an n-gram rule
    StopSel stop;               // stop.rows == nullptr = no row of this engine ever held stop strings
    LoopSel loop;               // loop.rows == nullptr = no row of this engine ever held a loop rule
};
// pval / pidx: ARGMAX_CHUNKS (64) partials per row, as launch_argmax_step
hipError_t launch_select_rows(hipStream_t s, const float* logits, int V, int ld, int B, const RowSel& rs, float* pval, int32_t* pidx, const StepState& st);
// Prompt-presence bits of freshly prefilled rows from the packed prompt (src as launch_embed_gather: < 0 = an image row, i.e. image_token);
// sequence b ends at packed token last[b] and lives in row dst[b] (dst == nullptr: row b).  Clears the rows' counts too.
hipError_t launch_pen_prompt(hipStream_t s, const int32_t* src, const int32_t* last, const int32_t* dst, int B, int image_token, int V,
                             int32_t* cnt, uint32_t* seen);
// Penalty state from explicit histories (dots_op_select_tokens): row b holds hist[b][0, n_prompt[b]) prompt ids, then its generated ids up
// to hist_lens[b]; out_lens[b] = generated count.
hipError_t launch_pen_history(hipStream_t s, const int32_t* hist, const int32_t* hist_lens, int stride, const int32_t* n_prompt, int B, int V,
                              int32_t* cnt, uint32_t* seen, int32_t* out_lens);
// table[row] = p, own[row] = flag, in stream order
hipError_t launch_set_row_params(hipStream_t s, RowParams* table, int32_t* own, int row, const RowParams& p, int flag);
// Logit rules of one row, in stream order: its image row (when r.flags has RULE_IMG) = -inf everywhere but the n_allowed ids of allowed
// (n_allowed == 0: 0 everywhere), plus bias_val[j] at bias_ids[j] (n_bias distinct ids); then table[row] = r.  allowed / bias_ids /
// bias_val are device arrays of ids in [0, V).
hipError_t launch_set_row_rules(hipStream_t s, RowRules* table, float* img, int row, int V, const RowRules& r, const int32_t* allowed, int n_allowed,
                                const int32_t* bias_ids, const float* bias_val, int n_bias);
// ---- guided.hip: guided decoding
// The allowed bits of every guided row of the launch (rows without a guide and rows that sel masks out are skipped), from each row's
// current state: bit t = token t has bytes and walking them never leaves the automaton.  Runs before launch_select_rows.
hipError_t launch_guide_mask(hipStream_t s, const GuideSel& g, int B, const int32_t* sel);
// The allowed bits of the draft rows of a speculating step: row r = j * rows + b of g.mask, r in [rows, rows * (k + 1)), from
// the table of slot b at state gstate[r] (launch_spec_guide_chain); a row with gstate[r] < 0 (dead, idle, unguided) is left alone.  The
// same walk as launch_guide_mask; g.mask must hold rows * (k + 1) rows.
hipError_t launch_guide_mask_drafts(hipStream_t s, const GuideSel& g, int rows, int k, const int32_t* gstate);
// table[row] = g (with state = g.start), in stream order
hipError_t launch_set_row_guide(hipStream_t s, RowGuide* table, int row, const RowGuide& g);
// state = start for the n rows dst[0 .. n) (dst == nullptr: rows 0 .. n - 1) that hold a guide, in stream order (a prefill)
hipError_t launch_guide_reset_rows(hipStream_t s, RowGuide* table, const int32_t* dst, int n);
// table[row].state = state for rows [0, n) (explicit states of dots_op_select_tokens_guided)
hipError_t launch_guide_set_states(hipStream_t s, RowGuide* table, const int32_t* states, int n);
// ---- ngram.hip: no-repeat n-gram blocking
// The banned bits of every row of the launch that carries an n-gram rule, from the row's own output out_ids[b * out_stride + 0 .. out_lens[b])
// (StepState's arrays).  Rows without a rule, rows that sel masks out and rows with finished[b] != 0 (finished == nullptr: none) are
// skipped and keep the bits of their last step.  Runs before launch_select_rows.
hipError_t launch_ngram_ban(hipStream_t s, const NgramSel& g, int B, const int32_t* out_ids, const int32_t* out_lens, int out_stride,
                            const int32_t* finished, const int32_t* sel);
// The banned bits of the live draft rows of a speculating step: row r = j * rows + b of g.mask, r in [rows, rows * (k + 1)),
// for every slot b that carries a rule and every j <= n_live[b], from the history out_ids[b][0 .. out_lens[b]) followed by drafts[b][0 .. j)
// (drafts [DOTS_MAX_BATCH][DOTS_MAX_SPEC_DRAFTS], n_live as SpecState) by the rule of launch_ngram_ban; every other draft row is left
// alone.  After launch_spec_expand (n_live) and before anything commits; g.mask must hold rows * (k + 1) rows.
hipError_t launch_ngram_ban_drafts(hipStream_t s, const NgramSel& g, int rows, int k, const int32_t* out_ids, const int32_t* out_lens, int out_stride,
                                   const int32_t* drafts, const int32_t* n_live);
// table[row] = r, in stream order
hipError_t launch_set_row_ngram(hipStream_t s, RowNgram* table, int row, const RowNgram& r);
// out_ids[b * out_stride + j] = hist[b * stride + n_prompt[b] + j] for j < hist_lens[b] - n_prompt[b], the count launch_pen_history leaves
// in out_lens (explicit histories of dots_op_select_tokens_ngram; out_stride >= stride)
hipError_t launch_ngram_history(hipStream_t s, const int32_t* hist, const int32_t* hist_lens, int stride, const int32_t* n_prompt, int B,
                                int32_t* out_ids, int out_stride);
// ---- stop.hip: stop strings, the stream-ordered writers of the row table (the walk itself is step_dev.h stop_walk)
// table[row] = r with the automaton at the root and no hit (r.table == nullptr: the row holds none)
hipError_t launch_set_row_stop(hipStream_t s, RowStop* table, int row, const RowStop& r);
// root state and no hit for the n rows dst[0 .. n) (dst == nullptr: rows 0 .. n - 1) that hold an automaton, in stream order (a prefill)
hipError_t launch_stop_reset_rows(hipStream_t s, RowStop* table, const int32_t* dst, int n);
// table[dst[i]] = table[src] at the root with no hit, i < n (dots_slots_fork: the children inherit the source's automaton and min_tokens)
hipError_t launch_stop_fork_rows(hipStream_t s, RowStop* table, int src, const int32_t* dst, int n);
// ---- loop.hip: the loop guard, the stream-ordered writers of the row table and the run counters (the check itself is
// loop_dev.h loop_step, run by select_rows_kernel after the commit)
// table[row] = r with no hit and the row's counters zeroed (r.max_period == 0: the row holds none)
hipError_t launch_set_row_loop(hipStream_t s, RowLoop* table, int32_t* run, int row, const RowLoop& r);
// no hit and zeroed counters for the n rows dst[0 .. n) (dst == nullptr: rows 0 .. n - 1) that hold a rule, in stream order (the row's output starts over)
hipError_t launch_loop_reset_rows(hipStream_t s, RowLoop* table, int32_t* run, const int32_t* dst, int n);
// table[dst[i]] = table[src] with no hit and zeroed counters, i < n (dots_slots_fork: what an independent request holds before its first token)
hipError_t launch_loop_fork_rows(hipStream_t s, RowLoop* table, int32_t* run, int src, const int32_t* dst, int n);
// One workgroup per case: ids[c * stride + 0 .. lens[c]) go one by one through loop_step under rule r, the counters in registers;
// hits[c] = {hit_tok, period, span} of the first hit, {-1, 0, 0}: none.  A test entry (dots_loop_probe)
hipError_t launch_loop_probe(hipStream_t s, const int32_t* ids, const int32_t* lens, int cases, int stride, const RowLoop& r, int32_t* hits);
// ---- spec.hip: n-gram speculative decoding
// A speculating step runs over R = rows x (k + 1) rows, draft-major: row j * rows + b carries token j of (last token, draft 1 .. k) of slot
// b at context ctx + j on the slot's own KV pages.  SpecState: the slots' drafts of the next step (drafts [DOTS_MAX_BATCH]
// [DOTS_MAX_SPEC_DRAFTS], n_draft [DOTS_MAX_BATCH]), the expanded row arrays of the step (tokens / ctx_len [DOTS_MAX_BATCH], block_table
// [DOTS_MAX_BATCH][max_pages]), n_live [DOTS_MAX_BATCH] (draft rows of slot b this step verifies; -1: the slot takes no step) and the
// counters stats [DOTS_MAX_BATCH + 1][3] (steps, drafted, accepted; the last row holds the totals).
// cls [DOTS_MAX_BATCH]: the speculation class of every row (SpecRow), a host fact (rows.hip spec_row_class: the row's stage features, its
// parameters, its logprobs and dots_set_speculation_rows) that the stream-ordered row setters write, so it holds inside captured chunks.
// The kernels ask nothing else about a row; while engine_greedy == 0 (an engine-wide temperature) no row verifies a draft whatever its class.
// cand [DOTS_MAX_BATCH][DOTS_MAX_SPEC_DRAFTS]: the candidate tokens of the live draft rows of SPEC_ROW_DRAW slots (spec_draw_kernel);
// nullptr until a step runs that kernel.
// gstate [DOTS_MAX_BATCH]: while a guided row may speculate (dots_set_speculation_guided), the automaton state every live draft row of a
// guided slot is selected under, indexed by step row r = j * rows + b (launch_spec_guide_chain); -1 = the row verifies nothing under a
// guide: dead, idle, or its slot holds none.  nullptr: no step launch asks about guides.
// acc_n [DOTS_MAX_BATCH], acc_tok [DOTS_MAX_BATCH][DOTS_MAX_SPEC_DRAFTS]: the accept record, while a row with logprobs may speculate
// (dots_set_speculation_logprobs) — the number of candidates the accept walk of slot b committed in this step and their ids, for
// launch_spec_logprob_final.  nullptr (both): the walk records nothing.
#ifndef DOTS_MAX_SPEC_DRAFTS
#define DOTS_MAX_SPEC_DRAFTS 15
#endif
// 0 is what a row nobody touched holds: plain greedy
enum SpecRow : int32_t {
    SPEC_ROW_ARGMAX = 0,       // speculates; a draft row's candidate is its arg max
    SPEC_ROW_NONE = 1,         // verifies no draft and drafts nothing
    SPEC_ROW_DRAW = 2,         // speculates; a draft row's candidate is drawn by the row's own sampler (parameters with temperature > 0)
};
struct SpecState {
    int32_t *drafts, *n_draft, *n_live, *tokens, *ctx_len, *block_table;
    unsigned long long* stats;
    const int32_t* cls;
    int32_t* cand;
    int32_t* gstate;
    int32_t k, engine_greedy;
    int32_t *acc_n, *acc_tok;
};
// the step's row arrays from the slots' state (st: the StepState of the selection stage; block_table [rows][max_pages]); an idle draft row
// gets context 0 and a table row of scratch_page, like a released slot
hipError_t launch_spec_expand(hipStream_t s, const SpecState& sp, const StepState& st, const int32_t* block_table, int max_pages, int rows, int scratch_page);
// arg-max partials (as launch_argmax_step's first kernel) of the live draft rows [rows, rows * (k + 1)) of logits
hipError_t launch_spec_argmax(hipStream_t s, const SpecState& sp, const float* logits, int V, int ld, int rows, float* pval, int32_t* pidx);
// The RowSel of the draft rows (`rs` below): the stage's tables as the draft-row kernels may use them.  params / own / thr / pen as in the
// stage (thr and pen: the stage uses rows [0, rows), the draft rows [rows, rows * (k + 1))); guide = the launch's guides while sp.gstate
// is set, else GuideSel{}; rules (+ rule_img), ngram and cnt (+ seen) only while dots_set_speculation_shaped opens the feature and some row
// holds it, else null; stop as in the stage.  A slot that carries a feature whose table is null here is SPEC_ROW_NONE.
//
// The candidates of the live draft rows of SPEC_ROW_DRAW slots, after launch_spec_argmax and BEFORE the selection stage commits anything:
// draft row r = j * rows + b is selected with rs.params[b] over logits row r with counter out_lens[b] + j, by the selection stage's own
// arithmetic (select_dev.h), into sp.cand[b][j - 1].  Two launches of rows * k workgroups; every other draft row's workgroup exits at once.
// A draft row whose selection is shaped (a guided slot with sp.gstate[r] >= 0; a ruled, n-gram or penalised slot) reads row r of rs.pen
// instead of the logits (launch_spec_shape_select left the values and the partials of their maximum there).
hipError_t launch_spec_draw(hipStream_t s, const SpecState& sp, const float* logits, int V, int ld, int rows, const RowSel& rs, const int32_t* out_lens,
                            const float* pval, const int32_t* pidx);
// Shaped slots of a speculating step, after the lm_head and before anything is selected:
// chain (sp.gstate != nullptr): sp.gstate[j * rows + b], j = 1 .. k, = the state of slot b (guide.rows[b].state, which nothing has moved yet)
//   walked over the bytes of drafts 1 .. j, for j <= n_live[b]; -1 from the first draft on that has no bytes, is one of eos_ids or — rules
//   != nullptr — of the slot's own stop ids, or meets GUIDE_DEAD, for j > n_live[b] and for a slot without a guide.  One launch of one
//   wave: lane b serves slot b.
// shape_select: for every live draft row whose selection is shaped, the values of the stage's shape_logit (select_dev.h) under the
//   hypothesis that the drafts before the row were committed — the rule image, -inf for EOS / stop ids below min_tokens (at output index
//   out_lens[b] + j) or in a state that is not accepting, bit r of guide.mask, bit r of ngram.mask, the penalties over cnt[b] plus the
//   drafts before the row — as arg-max partials over pval / pidx row r (replacing launch_spec_argmax's) and, for a SPEC_ROW_DRAW slot, as
//   values in row r of rs.pen.  st: out_lens and the EOS ids are read, nothing is written.
hipError_t launch_spec_guide_chain(hipStream_t s, const SpecState& sp, const GuideSel& guide, const int32_t* eos_ids, int n_eos, int rows,
                                   const RowRules* rules = nullptr);
hipError_t launch_spec_shape_select(hipStream_t s, const SpecState& sp, const RowSel& rs, const StepState& st, const float* logits, int V, int ld, int rows,
                                    float* pval, int32_t* pidx);
// after the selection stage committed the first `rows` rows: per slot, while the row is not finished and draft j equals the token just
// committed, commit the candidate of draft row j + 1 (its arg max, or sp.cand for a SPEC_ROW_DRAW slot) as the stage commits a row
// (select_dev.h commit_row over rs): the output count of a penalised slot, then EOS / the slot's stop ids, the cap, the output, the guide's
// automaton and the stop automaton as in a sequential step; counts into sp.stats and clears the slot's drafts.  The walk of a guided slot
// also ends at a draft row with sp.gstate < 0
hipError_t launch_spec_accept(hipStream_t s, const SpecState& sp, const StepState& st, int rows, int V, const float* pval, const int32_t* pidx,
                              const RowSel& rs);
// drafts[b * draft_stride + 0 .. n_draft[b]) = the continuation of the longest suffix n-gram (min_n .. max_n) of out_ids[b * out_stride +
// 0 .. out_lens[b]) that occurred before, at most k ids (the rule: include/dots_ocr_hip.h).  Rows that sel masks out, finished rows, rows
// with cls[b] == SPEC_ROW_NONE, and every row while engine_greedy == 0 draft nothing (finished / sel / cls may be nullptr).
hipError_t launch_ngram_draft(hipStream_t s, const int32_t* out_ids, const int32_t* out_lens, int out_stride, const int32_t* finished, const int32_t* sel,
                              const int32_t* cls, int engine_greedy, int B, int k, int min_n, int max_n, int32_t* drafts, int draft_stride,
                              int32_t* n_draft);
// cls[row] = value, in stream order
hipError_t launch_spec_set_class(hipStream_t s, int32_t* cls, int row, int value);
// drafts[row][0 .. n) = ids_host, n_draft[row] = n, in stream order (the ids travel as a kernel argument)
hipError_t launch_spec_set_drafts(hipStream_t s, int32_t* drafts, int32_t* n_draft, int row, const int32_t* ids_host, int n);
// ---- predict.hip: predicted outputs, the drafter that proposes a caller-supplied text
// PredictState: the slots' predictions ids [rows][stride] and, per slot, len (0: the slot holds none), the alignment (cur: the prediction
// index the next token is expected at, at: the output length at which cur was set), src (did the slot's current drafts come from its
// prediction) and seen (the output length at the drafter's last run over the slot).  stats [DOTS_MAX_BATCH][2]: the prediction tokens
// the slot verified / committed, which the drafter accounts at its NEXT run over the slot — the one that finds it finished included —
// from src, the step's n_live and the growth of the output since `seen`.  seen and stats may be nullptr (both): nothing is counted.
struct PredictState {
    const int32_t* ids;
    int32_t *len, *cur, *at, *src;
    int32_t stride;
    int32_t* seen;
    unsigned long long* stats;
};
// After launch_ngram_draft, over the same rows and under the same early-out conditions: for every slot that holds a prediction and whose
// output the rule (include/dots_ocr_hip.h) aligns with it, drafts[b * draft_stride + 0 .. n_draft[b]) = the prediction from the aligned
// index on, at most k ids, cur / at = the new alignment, src = 1.  Every other slot keeps its drafts, n_draft, cur and at, and gets src = 0.
// n_live (SpecState::n_live of the step that just ran; nullptr: nothing is counted): a slot whose src was 1 and that took the step adds
// n_live[b] to stats[b][0] and out_lens[b] - seen[b] - 1, the tokens its accept walk committed, to stats[b][1].
hipError_t launch_predict_draft(hipStream_t s, const PredictState& p, const int32_t* out_ids, const int32_t* out_lens, int out_stride, const int32_t* finished,
                                const int32_t* sel, const int32_t* cls, int engine_greedy, int B, int k, int min_n, int max_n, int32_t* drafts, int draft_stride,
                                int32_t* n_draft, const int32_t* n_live);
// len[row] = n and the alignment at the start, in stream order (the ids are copied by the caller); n == 0: the slot holds none any more,
// src[row] = 0 and — n_draft != nullptr — the drafts it took from the prediction are dropped
hipError_t launch_predict_set_row(hipStream_t s, const PredictState& p, int32_t* n_draft, int row, int n);
// ---- extend.hip: more prompt tokens behind a live sequence (dots_slots_extend)
// ExtendRows: the packed rows of one call — row i feeds token[i] (-1: the slot's pending token, read on the device) to slot slot[i] at
// context ctx_len[slot] + off[i] — and the step-private arrays of a chunk (tokens / ctx_len [DOTS_MAX_BATCH], block_table [DOTS_MAX_BATCH]
// [max_pages]), which exist whether or not speculation was ever switched on.
struct ExtendRows {
    const int32_t *slot, *off, *token;
    int32_t *tokens, *ctx_len, *block_table;
};
// the arrays of the chunk that holds packed rows [r0, r0 + n_live): step row r < n_live names the slot's KV pages; rows [n_live, rows) idle
// at context 0 on scratch_page, like a released slot.  Reads the slots' state (cur_tokens .. block_table), writes none of it
hipError_t launch_extend_expand(hipStream_t s, const ExtendRows& ex, int r0, int n_live, int rows, const int32_t* cur_tokens, const int32_t* ctx_len,
                                const int32_t* finished, const int32_t* out_ids, const int32_t* out_lens, int out_stride, const int32_t* block_table,
                                int max_pages, int scratch_page);
// after the last chunk, for the n extended slots: ctx_len += fed, out_lens = 0, finished = 0, max_len = max_new
hipError_t launch_extend_commit(hipStream_t s, const int32_t* slots, const int32_t* fed, const int32_t* max_new, int n, int32_t* ctx_len,
                                int32_t* out_lens, int32_t* finished, int32_t* max_len);

// ---- logprobs.hip: log-probabilities of the raw logits of every selected row
#ifndef DOTS_MAX_TOP_LOGPROBS
#define DOTS_MAX_TOP_LOGPROBS 20
#endif
constexpr int LP_CHUNKS = 64;                  // vocabulary chunks per row (grid x of the partial kernel)
constexpr int LP_MAX_CHUNK = 4096;             // values of one chunk a 256-thread workgroup holds in registers
constexpr int LP_MAX_V = LP_CHUNKS * LP_MAX_CHUNK;
//   top_n    [rows] -1 = off (the row is skipped), 0 = the chosen token only, 1..DOTS_MAX_TOP_LOGPROBS
//   sel / finished / out_lens  as StepState (nullptr: every row / none finished / position 0); read BEFORE the selection kernels
//   chosen   [rows] the token selection committed (StepState.cur_tokens); read AFTER them
//   part_ms  [rows][LP_CHUNKS][2] (m, s), part_v / part_i [rows][LP_CHUNKS][DOTS_MAX_TOP_LOGPROBS], pos [rows]: scratch
//   tok_lp   [rows][stride], top_ids / top_lp [rows][stride][DOTS_MAX_TOP_LOGPROBS]: row b's token of this step goes to position
//            out_lens[b] (taken before the commit); a row already finished is not written
struct LogprobState {
    const int32_t *top_n, *sel, *finished, *out_lens, *chosen;
    float* part_ms;
    float* part_v;
    int32_t* part_i;
    int32_t* pos;
    float* tok_lp;
    int32_t* top_ids;
    float* top_lp;
    int stride;
};
// V <= LP_MAX_V, ld >= V; grid (LP_CHUNKS, B) / B
hipError_t launch_logprob_partial(hipStream_t s, const float* logits, int V, int ld, int B, const LogprobState& st);
hipError_t launch_logprob_final(hipStream_t s, const float* logits, int V, int ld, int B, const LogprobState& st);
// The draft rows of a speculating step (dots_set_speculation_logprobs), around the selection stage's own pair:
// partial: grid (LP_CHUNKS, rows * k), after the lm_head — the partials of every live draft row r = j * rows + b (j <= n_live[b]) of a slot
//   with top_n[b] >= 0, over logits row r into row r of part_ms / part_v / part_i (which hold rows * (k + 1) rows); takes no snapshot.
// final: grid (rows, k), after launch_spec_accept — for a < acc_n[b] the entry of candidate acc_tok[b][a] from draft row (a + 1) * rows + b,
//   at position pos[b] + 1 + a (pos: the snapshot launch_logprob_partial took for row b in this step).
hipError_t launch_spec_logprob_partial(hipStream_t s, const float* logits, int V, int ld, int rows, int k, const int32_t* n_live, const LogprobState& st);
hipError_t launch_spec_logprob_final(hipStream_t s, const float* logits, int V, int ld, int rows, int k, const int32_t* acc_n, const int32_t* acc_tok,
                                     const LogprobState& st);
// table[row] = top_n, in stream order
hipError_t launch_set_row_lp(hipStream_t s, int32_t* table, int row, int top_n);
// ---- score.hip: the logprob stage over the fed rows of a scoring extend (dots_slots_score)
// ScoreRows: per packed row of the call (score_plan.h) — its slot, the entry of that slot it records (-1: none), the token whose value
// the entry takes and the slot's top_n (0..DOTS_MAX_TOP_LOGPROBS).  The launches serve the chunk of `rows` packed rows from r0 on: logits
// row r and scratch row r of st (part_ms / part_v / part_i) are packed row r0 + r; the entry goes to tok_lp[slot * stride + entry] and
// top_ids / top_lp likewise (both nullptr: only tok_lp is written, every top_n then being 0).  Of st only those seven fields and stride
// are read.  partial: grid (LP_CHUNKS, rows); final: grid rows, one wave.
struct ScoreRows {
    const int32_t *slot, *entry, *target, *top_n;
};
hipError_t launch_score_logprob_partial(hipStream_t s, const float* logits, int V, int ld, const ScoreRows& sr, int r0, int rows, const LogprobState& st);
hipError_t launch_score_logprob_final(hipStream_t s, const float* logits, int V, int ld, const ScoreRows& sr, int r0, int rows, const LogprobState& st);
// ---- beam.hip: beam search over shared KV pages
// A group of B beams lives in B slots, in group order (beam i = slots[i]).  BeamGroupDev is its device record (B == 0: the entry is free):
// first = floor(L / 64), the first block-table entry the beams do not share with the prompt; cum the beams' cumulative log-probabilities
// (-inf: dead); spare the page each beam holds outside its table row; act / par / copy_src / copy_dst what one step's select kernel hands
// the reorder kernel and that one the copy kernel (copy_dst < 0: beam j copies nothing); n_done the completed records waiting in the
// group's BEAM_DONE_CAP entries of BeamState::done.
#ifndef DOTS_MAX_BEAMS
#define DOTS_MAX_BEAMS 8
#endif
constexpr int BEAM_MAX_GROUPS = DOTS_MAX_BATCH / 2;
constexpr int BEAM_DONE_CAP = 4096;
struct BeamGroupDev {
    int32_t B, first, n_done, act;
    int32_t slots[DOTS_MAX_BEAMS];
    float cum[DOTS_MAX_BEAMS];
    int32_t spare[DOTS_MAX_BEAMS], par[DOTS_MAX_BEAMS], copy_src[DOTS_MAX_BEAMS], copy_dst[DOTS_MAX_BEAMS];
};
struct BeamDone { int32_t step, parent, id; float s; };     // a completed candidate: an EOS id out of beam `parent` at `step`, s = its cum
// groups [BEAM_MAX_GROUPS], done [BEAM_MAX_GROUPS][BEAM_DONE_CAP], parent [rows][StepState::out_stride] (beside out_ids: -1 = a dead beam);
// part_*: the logprob partials of the group rows (launch_logprob_partial with top_n = 2B)
struct BeamState {
    BeamGroupDev* groups;
    BeamDone* done;
    int32_t* parent;
    const float *part_ms, *part_v;
    const int32_t* part_i;
};
// The selection of groups [g0, g0 + n): one workgroup per group merges the live beams' 2B best (lp, id) pairs, records the EOS candidates,
// commits the B best others (token, parent, cum, out_lens, ctx_len when st.advance_ctx, finished at the cap) and — reorder != 0 — arms the
// reorder of this step.  A group whose rows are finished is left alone.
hipError_t launch_beam_select(hipStream_t s, const BeamState& bs, const StepState& st, int g0, int n, int reorder);
// The mid-generation fork of groups [0, n), after launch_beam_select of the same step: every beam's block-table entries [first, g) become
// its parent's (g = the page of the position just written), its tail a copy of the parent's tail page in its own spare page, in every
// layer; the old tail becomes the spare.  A beam that is its own only child keeps its tail.  Bytes only: page_bytes of a bf16 or fp8 page.
hipError_t launch_beam_reorder(hipStream_t s, const BeamState& bs, int n, const int32_t* ctx_len, int32_t* block_table, int max_pages, void* pool,
                               size_t layer_bytes, size_t page_bytes, int layers);
// row-major [rows, K] -> MFMA fragment order (decode.hip): 16-row tiles x K/32 chunks of 1 KiB
hipError_t launch_pack_frag(hipStream_t s, const bf16_t* src, bf16_t* dst, int64_t rows, int K);
// fused qkv weight [(Hq + 2 Hkv) * 128, K]: as launch_pack_frag, q / k head rows permuted so that a 16-row tile holds whole RoPE pairs
hipError_t launch_pack_frag_qkv(hipStream_t s, const bf16_t* src, bf16_t* dst, int Hq, int Hkv, int K);
// row-major [rows <= 16, K] <-> X image [K/8][XR][8] (XR = 8 for rows <= 8, else 16): the single-kernel entry points' converters
hipError_t launch_pack_x(hipStream_t s, const bf16_t* src, bf16_t* x, int rows, int K);
hipError_t launch_unpack_x(hipStream_t s, const bf16_t* x, bf16_t* dst, int rows, int K);
// ---- quant.hip: fp8 (e4m3, per-output-channel scale) weights
// W[n][:] <- bf16(e4m3(W[n][:] / scale[n])) in place, scale[n] = max|W[n][:]| / 448 (1 for an all-zero row)
hipError_t launch_quant_rows_fp8(hipStream_t s, bf16_t* W, float* scale, int64_t N, int K);
// bf16(q) row-major [rows, K] -> e4m3 bytes in decode fragment order (512-B chunks); rot_rows = (Hq + Hkv) * 128 for the fused qkv weight, else 0
hipError_t launch_pack_frag_fp8(hipStream_t s, const bf16_t* src, uint8_t* dst, int64_t rows, int K, int rot_rows);
// activations: x bf16 [M][lda] -> q e4m3 [M][K] + scale[m] (per token); bf16(q) weights -> e4m3 bytes row-major
hipError_t launch_quant_act_fp8(hipStream_t s, const bf16_t* X, uint8_t* Q, float* scale, int64_t M, int K, int lda);
hipError_t launch_bf16q_to_fp8(hipStream_t s, const bf16_t* src, uint8_t* dst, int64_t n);
// ---- gemm.hip, fp8 MFMA: C = epilogue((Aq Wq^T) * rowscale[m] * colscale[n] + bias); Aq [M][K], Wq [N][K] e4m3 row-major;
// N % 256 == 0, K % 64 == 0, ldc % 8 == 0.  EPI_F32 is not offered.
hipError_t launch_gemm_fp8(hipStream_t s, const uint8_t* Aq, const float* rowscale, const uint8_t* Wq, const float* colscale, const bf16_t* bias,
                           const bf16_t* R, void* C, int64_t M, int N, int K, int ldc, int epi);
bool gemm_fp8_supports(int N, int K);
// ---- weights.hip helper kernels
hipError_t launch_pack_w13(hipStream_t s, const bf16_t* gate, const bf16_t* up, bf16_t* out, int I, int K);
hipError_t launch_convert_to_bf16(hipStream_t s, const void* src, int dtype, bf16_t* dst, int64_t n);

// ---- preprocess.hip: Pillow-exact bicubic resize + normalise + patchify on the GPU
hipError_t launch_resize_h(hipStream_t s, const uint8_t* in, uint8_t* out, const int32_t* coef, const int32_t* bounds,
                           int ksize, int H, int W, int rw);
hipError_t launch_resize_v(hipStream_t s, const uint8_t* in, uint8_t* out, const int32_t* coef, const int32_t* bounds,
                           int ksize, int W, int rh);
hipError_t launch_normalize_patchify(hipStream_t s, const uint8_t* img, float* out, int rw, int gh, int gw, int P, int m,
                                     float r255, const float* mean, const float* stdv);
