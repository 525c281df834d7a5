/* dots_ocr_hip.h — C ABI of the MI355X-native dots.ocr inference engine (libdots_ocr_hip.so).
 *
 * The reference (rednote-hilab/dots.ocr) has NO native layer: its hot path is the three HF
 * objects used in DotsOCRParser._inference_with_hf (dots_ocr/parser.py:78-117):
 *     self.model.generate(**inputs, max_new_tokens=...)         parser.py:110
 *     self.processor(...) / apply_chat_template / batch_decode  parser.py:93-105,114-116
 *     AutoModelForCausalLM.from_pretrained(...)                 parser.py:68-74
 * This header is the boundary a native binding for that path binds instead:
 * plain pointers and sizes, opaque handle, int status codes, no exceptions, no torch types.
 *
 * Conventions
 *   - every function returns 0 on success, a negative DOTS_E_* code on failure; the message is
 *     available from dots_last_error(handle) (or dots_last_error(NULL) for create failures);
 *   - the caller owns every buffer it passes; the engine owns all device memory it allocates;
 *   - one handle = one GPU = one HIP stream.  A handle is NOT thread-safe; different handles
 *     may be driven from different threads/processes (one per GPU);
 *   - pointers named *_dev are device pointers on the handle's GPU, *_host are host pointers;
 *     parameters named `x` with a companion `x_on_device` flag accept either;
 *   - bf16 tensors are raw uint16_t.
 */
#ifndef DOTS_OCR_HIP_H
#define DOTS_OCR_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DOTS_OK 0
#define DOTS_E_INVALID (-1)   /* bad argument / unsupported shape */
#define DOTS_E_HIP (-2)       /* HIP runtime error */
#define DOTS_E_STATE (-3)     /* call order (weights missing, sequence not prefetched, ...) */
#define DOTS_E_CAPACITY (-4)  /* exceeds max_batch / max_seq_len / workspace */

#define DOTS_DTYPE_BF16 0
#define DOTS_DTYPE_F32 1
#define DOTS_DTYPE_F16 2

typedef struct DotsEngine DotsEngine;

/* Mirrors the checkpoint's config.json (+ vision_config) that from_pretrained reads
 * (parser.py:68-74).  Hard-coded in the kernels: head_dim == 128; dots_create also requires hidden_size % 256 == 0 and
 * hidden_size <= 1536 (the decode kernels keep a residual row in 3 x 16-byte chunks per lane), the same for the vision embed_dim's
 * norm path — dots.ocr's 1536 / 1536 fit; a wider model needs NC_MAX raised in csrc/decode_dev.h. */
typedef struct DotsConfig {
    /* language model (Qwen2 architecture) */
    int32_t hidden_size, num_layers, num_heads, num_kv_heads, head_dim, intermediate_size, vocab_size;
    float rope_theta, rms_norm_eps;
    int32_t attention_bias;
    int32_t image_token_id;
    /* vision tower (NaViT) + patch merger */
    int32_t v_embed_dim, v_layers, v_heads, v_intermediate, v_patch, v_merge, v_channels, v_temporal_patch;
    float v_rms_eps, v_ln_eps;
    int32_t v_use_bias, v_post_norm;
    /* runtime capacity */
    int32_t max_batch;        /* sequences decoded together: <= 64; the decode kernels work in tiles of 16 rows (one MFMA column tile),
                                 batches above 16 re-read each weight slice once per tile from L2 / the Infinity Cache */
    int32_t max_seq_len;      /* prompt + generated tokens per sequence */
    int64_t max_patches;      /* vision patches per dots_vit_forward call (workspace) */
    int64_t max_prefill_tokens; /* packed prompt tokens per dots_prefill call */
    int64_t kv_pool_tokens;   /* paged KV cache: tokens the page pool holds across ALL sequences (pages of 64).  A static batch
                                 (dots_prefill / dots_generate) reserves prompt + generation cap per sequence; a slot sequence
                                 (dots_slots_prefill) reserves its prompt + 64 tokens and takes further pages on demand as it grows
                                 (dots_slots_decode).  0 = max_batch * max_seq_len (never refuses) */
    int32_t fp8_weights;      /* != 0: dots_finalize_weights quantises every ViT-block / merger / LM linear and the lm_head to OCP e4m3 with
                                 one fp32 scale per output channel (scale = max|row| / 448; csrc/quant.hip).  The decode step streams
                                 the e4m3 bytes (half the HBM traffic) against bf16 activations; the ViT / prefill GEMMs quantise
                                 their input activations per token the same way and run on the fp8 MFMA (W8A8).  Every quantised
                                 linear needs N % 256 == 0 and K % 64 == 0.  Embedding table, patch embedding, norms and biases
                                 stay bf16.  (BASELINE configs[4]) */
    int32_t kv_cache_dtype;   /* paged KV cache element type: 0 = bf16 (default), 1 = fp8 (OCP e4m3fn, vLLM's --kv-cache-dtype fp8), any other
                                 value is refused (DOTS_E_INVALID).  fp8: one fp32 scale s per (layer, kv head, K|V) (dots_set_kv_scales, default
                                 1.0); a cached value is e4m3fn(clamp(x / s, -448, 448)) rounded to nearest even, x = what the bf16 cache would
                                 hold, and reads back as float(stored) * s.  Pages still hold 64 tokens (half the bytes); prefill attention
                                 runs on its bf16 buffers, every decode step reads the fp8 cache.  DotsStats.decode_bytes counts 1 B per
                                 KV element.  (csrc/decode.hip header) */
} DotsConfig;

/* Per-phase device time of the last dots_generate / dots_vit_forward / ... call, measured with
 * HIP events on the engine's stream (what bench.py's roofline legs read). */
typedef struct DotsStats {
    float vit_ms, prefill_ms, decode_ms, total_ms;
    float vit_attn_ms;        /* sum of the ViT flash-attention launches */
    int32_t vit_attn_launches;
    float vit_gemm_ms;        /* sum of the ViT GEMM launches */
    int32_t decode_steps;
    int64_t vit_patches, prefill_tokens, new_tokens;
    double vit_attn_flops;    /* algorithmic: 4*N_i^2*E per layer summed over images */
    double vit_flops;         /* SURVEY §8(d) ViT formula */
    double prefill_flops;
    double decode_bytes;      /* steps*W + sum ctx*kv_bytes_per_token */
} DotsStats;

/* ---- lifecycle ------------------------------------------------------------------------ */
int dots_create(const DotsConfig* cfg, int device, DotsEngine** out);
void dots_destroy(DotsEngine* e);
const char* dots_last_error(DotsEngine* e);
/* HIP stream of the handle (hipStream_t as void*), for callers that record their own events. */
void* dots_stream(DotsEngine* e);

/* One call per checkpoint tensor, named as in the HF state dict the reference loads
 * (parser.py:68-74).  `data` is a host pointer; dtype bf16/f16/f32 (converted to bf16). */
int dots_load_weight(DotsEngine* e, const char* name, const void* data_host, int dtype,
                     const int64_t* shape, int ndim);
/* Verifies every tensor the config requires is present, builds fused/packed device copies. */
int dots_finalize_weights(DotsEngine* e);

/* ---- the hot path --------------------------------------------------------------------- */
/* Replaces DotsVisionTransformer.forward(pixel_values, grid_thw) (HF-hub modeling_dots_vision.py,
 * called inside model.generate at parser.py:110).  pixel_values f32 [total_patches, C*T*P*P],
 * grid_thw int64 [n_img,3] (host).  out_embeds_dev: bf16 [total_patches/merge^2, hidden] or NULL
 * (result then stays in the engine for the following dots_prefill). */
int dots_vit_forward(DotsEngine* e, const float* pixel_values, int pixel_values_on_device,
                     int64_t total_patches, const int64_t* grid_thw_host, int n_img,
                     void* out_embeds_dev);

/* Software pipelining across page batches (no counterpart in the reference's HF path, which is strictly sequential; vLLM overlaps
 * requests in its scheduler).  dots_vit_prefetch runs the tower of the NEXT batch asynchronously on a side stream that is masked to
 * the upper (256 - 128) CUs — an equal share of every XCD — and returns at once; while it runs, dots_generate replays its decode
 * graph on a stream masked to the lower 128 CUs (the two partitions then work side by side: two unmasked streams were measured to
 * time-slice the chip with no overlap at all), and on the whole chip again once the tower is done.  dots_vit_take_prefetched makes
 * the main stream wait for the tower and puts its rows in place for the next dots_prefill / dots_slots_prefill, or for
 * dots_generate with n_img = -1.  Order per batch k: take(k) -> [dots_preprocess_image(k+1)] -> prefetch(k+1) -> generate(k, n_img = -1).
 * after_prefill != 0: the tower is launched behind the NEXT prefill (dots_prefill / dots_generate / dots_slots_prefill) instead of at once,
 * so that it shares the chip with the latency-bound decode loop only, not with the MFMA-bound prefill (or at dots_vit_take_prefetched if no
 * prefill comes by).  pixel_values must stay valid until the rows are taken.  Results are bit-identical to the sequential calls.
 * Environment DOTS_OCR_OVERLAP_DEC_CUS (multiple of 8, default 128) sets the decode partition. */
int dots_vit_prefetch(DotsEngine* e, const float* pixel_values, int pixel_values_on_device, int64_t total_patches,
                      const int64_t* grid_thw_host, int n_img, int after_prefill);
int dots_vit_take_prefetched(DotsEngine* e);
/* *ready = 1 when the tower of the prefetched batch has finished (dots_vit_take_prefetched then makes nothing wait), 0 while it runs or has
 * not been launched yet (after_prefill).  A serving loop polls it between decode chunks and takes the batch only when its rows exist, so
 * that the sequences already decoding never queue behind a tower (dots_ocr_amd/scheduler.py).  DOTS_E_STATE without a pending prefetch. */
int dots_vit_prefetch_ready(DotsEngine* e, int* ready);

/* Replaces prepare_inputs_embeds + the prefill forward of Qwen2ForCausalLM.
 * Packed prompts: input_ids int32 [sum(prompt_lens)] (host), slot i of the batch gets prompt i.
 * Vision rows from the preceding dots_vit_forward are scattered at image_token_id positions. */
int dots_prefill(DotsEngine* e, const int32_t* input_ids_host, const int32_t* prompt_lens_host, int B);

/* One greedy decode step for the B prefilled sequences. */
int dots_decode_step(DotsEngine* e);

/* Replaces model.generate(**inputs, max_new_tokens=N) with do_sample=False (parser.py:110):
 * ViT over all images, prefill, greedy decode until every sequence hit an EOS id or N tokens.
 * out_ids int32 [B, max_new_tokens] (host, new tokens only), out_lens int32 [B].
 * n_eos == 0 disables EOS (fixed-length timing runs).
 * n_img == -1: skip the tower, the vision rows are the ones dots_vit_take_prefetched put in place. */
int dots_generate(DotsEngine* e, const int32_t* input_ids_host, const int32_t* prompt_lens_host, int B,
                  const float* pixel_values, int pixel_values_on_device, int64_t total_patches,
                  const int64_t* grid_thw_host, int n_img, int max_new_tokens,
                  const int32_t* eos_ids_host, int n_eos, int32_t* out_ids_host, int32_t* out_lens_host);

/* Replaces the image half of processor.__call__ (parser.py:99-105 -> Qwen2-VL image processor: Pillow BICUBIC resize to
 * (rh, rw) = smart_resize(h, w), x 1/255, (x - mean)/std, patchify) on the GPU, bit-identical to the host path.
 * rgb: uint8 [h, w, 3].  The per-axis tap tables are Pillow's 22-bit fixed-point coefficients, built on the host
 * (coef int32 [out, ksize], bounds int32 [out, 2] = first input index, tap count); pass NULL tables for an axis that
 * is not resized.  out_pixel_values_dev: float32 [(rh/P)*(rw/P), 3*P*P] on the device, ready for dots_vit_forward. */
int dots_preprocess_image(DotsEngine* e, const uint8_t* rgb, int rgb_on_device, int h, int w, int rh, int rw,
                          const int32_t* hcoef_host, const int32_t* hbounds_host, int hksize,
                          const int32_t* vcoef_host, const int32_t* vbounds_host, int vksize,
                          const float* mean3_host, const float* std3_host, float rescale, float* out_pixel_values_dev);

/* Token selection for the following prefill / decode / generate calls.  temperature == 0 (default): greedy arg max.
 * temperature > 0: sample from softmax(logits / temperature) restricted to the top_p nucleus — the sampling
 * parameters the reference passes to its vLLM backend (parser.py:27-28, model/inference.py:38-43).  Reproducible
 * from `seed` (counter-based: seed, batch slot, position). */
int dots_set_sampling(DotsEngine* e, float temperature, float top_p, uint64_t seed);

/* Per-row token selection.  One row = a slot (continuous batching) or sequence b of a static batch.
 *   temperature        >= 0; 0 = greedy (arg max of the penalised logits, the lowest index wins a tie)
 *   top_p              (0, 1]: nucleus over the softmax of the tokens top_k keeps
 *   top_k              0 = off, else keep every token whose tempered logit is >= the k-th largest (ties kept)
 *   repetition_penalty > 0, 1 = off: l' = l > 0 ? l / r : l * r for every token in the row's prompt or output (HF, vLLM)
 *   frequency_penalty, presence_penalty  [-2, 2]: l' -= f * c_t + p * (c_t > 0), c_t = count of t in the row's output (OpenAI)
 *   seed               the draw of a row's n-th generated token (the prefill's token is n = 0) uses u = hash(seed, n): neither the
 *                      row index nor the batch enters it
 * Penalties are applied first (repetition, then frequency / presence), never written over the logits dots_get_logits returns. */
typedef struct DotsSamplingParams {
    float temperature, top_p;
    int32_t top_k;
    float repetition_penalty, frequency_penalty, presence_penalty;
    uint64_t seed;
} DotsSamplingParams;
/* Give row `row` its own parameters (p == NULL: back to the dots_set_sampling setting), in stream order: they apply from the next token
 * the engine selects, the first token of a following dots_prefill / dots_slots_prefill included.  Captured decode graphs are kept.
 * dots_slot_release / dots_slots_reset clear the row.  DOTS_E_INVALID on a value out of range.
 * Penalty state is exact for a row that carries its penalty from before its prefill (set the row, then prefill it).  Limit: for a penalty
 * switched on while the row is already running, the counts c_t hold only the tokens selected after the switch, and the prompt-presence
 * bits exist only if some row of this engine had used a penalty before the row's prefill (the state is allocated on first use and
 * written by each prefill from then on); the prompt is not kept on the device to rebuild them. */
int dots_set_row_sampling(DotsEngine* e, int row, const DotsSamplingParams* p);

/* Per-row logit rules: which tokens a row may emit and when it stops.  One row = a slot, or sequence b of a static batch.
 *   bias_ids / bias_values  n_bias <= DOTS_MAX_LOGIT_BIAS pairs (id, value): the value is added to the token's logit; finite, or -inf = a
 *                           ban.  A duplicate id is refused.
 *   allowed_ids             NULL = every id is allowed, else n_allowed >= 1 ids: every id outside the list is -inf
 *   min_tokens              while the row has generated fewer than min_tokens tokens (the prefill's token is n = 0) every engine EOS id
 *                           (dots_set_eos) and every id of stop_ids is -inf
 *   stop_ids                n_stop <= DOTS_MAX_STOP_IDS ids that finish this row only, as an EOS id does: the id is appended, the row is finished
 *   ignore_eos              != 0: the engine's EOS ids do not finish this row (its stop ids and its length cap still do)
 * Order (vLLM's): raw logit + bias, -inf for banned / not allowed / min_tokens ids, then the penalties of DotsSamplingParams on that value
 * (-inf stays -inf), then the greedy arg max (lowest index on a tie) or the tempered top-k / top-p draw.  A -inf token has weight 0: it is
 * never drawn and never counted into top-k or the nucleus.  dots_get_logits and the logprobs stay on the raw logits. */
#define DOTS_MAX_LOGIT_BIAS 1024
#define DOTS_MAX_STOP_IDS 16
typedef struct DotsLogitRules {
    const int32_t* bias_ids;
    const float* bias_values;
    int32_t n_bias;
    const int32_t* allowed_ids;
    int32_t n_allowed;
    int32_t min_tokens;
    int32_t stop_ids[DOTS_MAX_STOP_IDS];
    int32_t n_stop;
    int32_t ignore_eos;
} DotsLogitRules;
/* Give row `row` logit rules (r == NULL: none), in stream order: they apply from the next token the engine selects, the first token of a
 * following dots_prefill / dots_slots_prefill included (set, then prefill).  The lists are copied before the call returns.  Values live in
 * device memory: captured decode graphs are kept (one more graph per step shape exists for "some row has rules").  dots_slot_release /
 * dots_slots_reset clear the row.  The first call allocates the state: an fp32 image and a shaped-logit scratch of max_batch x vocab each
 * (the latter shared with the penalties).
 * A row with rules is always selected by the per-row stage.  If it has no DotsSamplingParams of its own, the stage uses the engine-wide
 * temperature / top_p / seed of dots_set_sampling AS THEY STAND WHEN THE RULES ARE SET (or when its own parameters are cleared), with the
 * per-row draw u = hash(seed, n): a later dots_set_sampling does not reach it.
 * DOTS_E_INVALID: a value out of range, an id outside [0, vocab), a duplicate bias id, and rules that could never select a token — an empty
 * allowed list, one entirely banned by the bias, or (min_tokens > 0) one that bans, engine EOS ids and stop ids cover together.  The EOS ids
 * are those set at the call.  Should a row end up all -inf all the same (EOS ids changed later), it commits the lowest index, id 0. */
int dots_set_row_logit_rules(DotsEngine* e, int row, const DotsLogitRules* r);

/* ---- Guided decoding: a row's output follows a byte automaton that lives on the device and advances at every commit, so
 * that it holds inside captured decode chunks.  The host compiles a pattern to a trimmed DFA (dots_ocr_amd/guided.py).
 *
 * dots_set_token_bytes  the packed UTF-8 bytes of every vocabulary entry: offsets_host int32 [vocab + 1] (offsets[0] = 0, non-decreasing),
 *                       bytes_host the offsets[vocab] bytes.  An entry without bytes (give the special ids none) can never be selected on a
 *                       guided row.  Once per engine; DOTS_E_STATE while a row holds a guide.  Synchronises.
 * dots_guide_create     table_host uint16 [n_states][256] (0xFFFF = no transition, every other entry < n_states), accepting_host uint8
 *                       [n_states], start; n_states <= DOTS_MAX_GUIDE_STATES.  The automaton must be TRIMMED: from every state an accepting
 *                       one is reachable (then "the walk never meets 0xFFFF" is the whole test of a token).  Copied to device memory;
 *                       *id_out names it.  Any number of rows may hold one guide.  Synchronises.
 * dots_guide_destroy    DOTS_E_STATE while a row holds it.  Synchronises.
 * dots_set_row_guide    row `row` follows guide id from its start state (id < 0: none), written in stream order by a one-thread kernel:
 *                       captured decode graphs are kept (one more graph per step shape exists for "some row holds a guide").  A following
 *                       dots_prefill / dots_slots_prefill of the row starts the automaton over; the prefill's first token is already
 *                       selected under the guide.  dots_slot_release / dots_slots_reset clear the row.  DOTS_E_STATE before
 *                       dots_set_token_bytes.  The first call allocates the allowed bits (max_batch x vocab / 8 bytes) and the row table.
 * dots_row_guide_state  the state the row's automaton is in (-1: the row holds no guide).  Synchronises.
 *
 * A guided row at state s: token t is allowed iff it has bytes and walking them from s never leaves the automaton; the engine's EOS ids and
 * the row's stop ids are allowed iff s is accepting; every other id is -inf.  This enters where the allowed list of DotsLogitRules does
 * (raw logit + bias, -inf for banned / not allowed / min_tokens / guide, penalties, arg max or draw); dots_get_logits and the logprobs stay
 * on the raw logits.  The commit walks the chosen token's bytes.  An EOS id finishes a guided row whether or not ignore_eos is set.  Like a
 * row with rules, a guided row without DotsSamplingParams of its own is selected with the engine-wide setting as it stands at the call.
 * A row the guide (and min_tokens) leave nothing for commits id 0, as an all -inf row of the rules does; its state does not move. */
#define DOTS_MAX_GUIDE_STATES 4096
int dots_set_token_bytes(DotsEngine* e, const int32_t* offsets_host, const uint8_t* bytes_host);
int dots_guide_create(DotsEngine* e, const uint16_t* table_host, int n_states, const uint8_t* accepting_host, int start, int32_t* id_out);
int dots_guide_destroy(DotsEngine* e, int32_t id);
int dots_set_row_guide(DotsEngine* e, int row, int32_t id);
int dots_row_guide_state(DotsEngine* e, int row, int32_t* state_out);

/* ---- No-repeat n-gram blocking: a row never completes an n-gram it has already produced.  The ban is computed on the device
 * at every step from the row's own output, so it holds inside captured decode chunks.
 *
 * Let out[0 .. L) be the tokens the row has generated so far (the prefill's token is out[0]; the prompt is NOT part of the history, which is
 * the convention of vLLM's logits processors — Hugging Face generate() also feeds the prompt to its no_repeat_ngram_size processor).  With
 * n = size and W = window: if L < n - 1 nothing is banned; otherwise P = out[L - n + 1 .. L) (empty for n = 1), and for every i with
 * max(0, L - W) <= i <= L - n (W = 0: from 0) and out[i .. i + n - 1) == P the id out[i + n - 1] is banned unless it is in the whitelist.
 * So only n-grams lying wholly inside the last W generated tokens count.  With W = 0 and no whitelist this is what transformers'
 * NoRepeatNGramLogitsProcessor(n) bans when given out as input_ids.
 *
 * A banned id is -inf where the allowed list of DotsLogitRules and the guide's bit enter (raw logit + bias, -inf for banned / not allowed /
 * min_tokens / guide / n-gram, penalties, arg max or draw); dots_get_logits and the logprobs stay on the raw logits.  EOS and stop ids get no
 * special treatment: whitelist them if they must stay selectable.  Like a row with rules, an n-gram row without DotsSamplingParams of its
 * own is selected with the engine-wide setting as it stands at the call.  A row the ban, the rules and a guide together leave nothing for
 * commits id 0 (a guide's state does not move), as an all -inf row of the rules does.
 *
 * dots_set_row_ngram    row `row` carries *r from the next selected token on (NULL: none), written in stream order by a one-thread kernel:
 *                       captured decode graphs are kept (one more graph per step shape exists for "some row carries an n-gram rule").
 *                       Switching it on for a running row is exact from the next step: the history is always on the device.  A prefill
 *                       needs no reset, the row's output starts empty.  dots_slot_release / dots_slots_reset clear the row.  The first
 *                       call allocates the banned bits (max_batch x vocab / 8 bytes) and the row table.
 * DOTS_E_INVALID: size outside [1, DOTS_MAX_NGRAM_SIZE], window neither 0 nor in [size, max_seq_len], more than DOTS_MAX_NGRAM_WHITELIST
 * whitelist ids, one outside [0, vocab) or given twice, a vocabulary above 524 288. */
#define DOTS_MAX_NGRAM_SIZE 64
#define DOTS_MAX_NGRAM_WHITELIST 16
typedef struct DotsNgramRule {
    int32_t size;                /* n: 1 .. DOTS_MAX_NGRAM_SIZE */
    int32_t window;              /* W: 0 = the whole output, else size .. max_seq_len */
    int32_t n_whitelist;         /* 0 .. DOTS_MAX_NGRAM_WHITELIST */
    int32_t whitelist[DOTS_MAX_NGRAM_WHITELIST]; /* ids that are never banned by this rule */
} DotsNgramRule;
int dots_set_row_ngram(DotsEngine* e, int row, const DotsNgramRule* r);

/* ---- Stop strings: a row ends at the token that completes one of a few pieces of TEXT.  The check is a byte automaton on the
 * device that the commit of every token advances, so the stop is exact inside captured decode chunks and in dots_generate, and a stopped
 * row writes no further KV.  The host compiles 1 .. DOTS_MAX_STOP_STRINGS strings of 1 .. DOTS_MAX_STOP_BYTES bytes each into an
 * Aho-Corasick automaton with its failure links folded into a dense byte DFA (dots_ocr_amd/stop_strings.py).
 *
 * The matching rule: the row's output is scanned as a byte stream — the concatenated bytes (dots_set_token_bytes) of the tokens it has
 * generated; the prompt is not part of it, and a token without bytes contributes nothing and leaves the state alone.  The row stops at
 * the first byte at which any listed string ends; if several end there the longest (earliest start) is the match.  The token that holds
 * that byte is appended whole and is the row's last.  An engine EOS id or a stop id of the row's DotsLogitRules finishes the row as before
 * and is not walked.  While the index of the token (the prefill's token is 0) is below min_tokens the automaton advances but no match is
 * taken, so a string that straddles the boundary is still found.
 *
 * dots_stop_create    table_host uint16 [n_states][256] (every entry < n_states, state 0 = the root), match_len_host uint16 [n_states] (bytes
 *                     of the longest listed string ending at the state, 0 = none; <= DOTS_MAX_STOP_BYTES), match_id_host uint8 [n_states]
 *                     (its index, < DOTS_MAX_STOP_STRINGS); n_states <= DOTS_MAX_STOP_STRINGS x DOTS_MAX_STOP_BYTES + 1.  Copied to device
 *                     memory; *handle_out (>= 1) names it.  Any number of rows may hold one automaton.  Synchronises.
 * dots_stop_destroy   DOTS_E_STATE while a row holds it.  Synchronises.
 * dots_set_row_stop   row `row` (a slot, or sequence `row` of a static batch) holds the automaton from its root, with no hit (handle 0:
 *                     none), written in stream order by a one-thread kernel; captured decode graphs are kept and no graph is added.  A
 *                     following dots_prefill / dots_slots_prefill of the row starts the automaton over and clears the hit; the prefill's
 *                     first token is already walked.  dots_slot_release / dots_slots_reset clear the row; dots_slots_fork gives every child
 *                     the source's automaton and min_tokens at the root.  A row with stop strings is selected by the per-row stage (with the
 *                     engine-wide setting as it stands at the call if it has no DotsSamplingParams of its own) and verifies no draft of a
 *                     speculating step.
 * dots_row_stop_hit   out[4] = {index of the token that completed the match, bytes of that token consumed including the matching byte,
 *                     length of the matched string in bytes, its index in the list}, or {-1, 0, 0, -1}: no hit (yet), or the row holds no
 *                     stop strings.  Synchronises.
 * All four: DOTS_E_STATE before dots_set_token_bytes, DOTS_E_INVALID on a bad size, handle or row. */
#define DOTS_MAX_STOP_STRINGS 16
#define DOTS_MAX_STOP_BYTES 64
int dots_stop_create(DotsEngine* e, const uint16_t* table_host, int n_states, const uint16_t* match_len_host, const uint8_t* match_id_host,
                     int32_t* handle_out);
int dots_stop_destroy(DotsEngine* e, int32_t handle);
int dots_set_row_stop(DotsEngine* e, int row, int32_t handle, int min_tokens);
int dots_row_stop_hit(DotsEngine* e, int row, int32_t* out);

/* ---- Loop guard: a row ends at the token after which its output has started to cycle.  Opt-in per row; the check runs on
 * the device behind the commit of every token of the row, so the end is exact inside captured decode chunks and in dots_generate, and an
 * ended row writes no further KV.
 *
 * The rule: let out[0 .. n] be the row's output (the prefill's token is index 0) and L(p) = max(repeats * p, min_span).  After the token at
 * index n is committed, period p in [min_period, max_period] fires iff n + 1 >= L(p) and out[i] == out[i - p] for every i in
 * [n + 1 - L(p) + p, n].  The row fires at the first n at which any period fires, with the smallest such p: the firing token is appended
 * whole and is the row's last.  Ids are compared as ids.  A token that finishes the row as an engine EOS id or a stop id of its
 * DotsLogitRules is not checked; a hit at the token that reaches the generation cap is still recorded; a stop string that matches at the
 * same token leaves its own record too.  The window is the output since it last started over: a prefill, dots_slots_extend and setting
 * the rule start it over.
 *
 * dots_set_row_loop   row `row` (a slot, or sequence `row` of a static batch) holds the rule with no hit and its counters at zero (NULL:
 *                     none), written in stream order by one small kernel; the first call allocates the counters (max_batch-independent:
 *                     256 KiB) and drops the captured decode graphs once, later calls keep them.  dots_slot_release / dots_slots_reset
 *                     clear the row; dots_slots_fork gives every child the source's rule.  A row with a rule is selected by the per-row
 *                     stage (with the engine-wide setting as it stands at the call if it has no DotsSamplingParams of its own) and verifies
 *                     no draft of a speculating step, whatever dots_set_speculation_rows says.  Refused (DOTS_E_INVALID): limits outside
 *                     1 <= min_period <= max_period <= DOTS_MAX_LOOP_PERIOD, 2 <= repeats <= 64, 0 <= min_span <= 65535; a row of a beam
 *                     group.  dots_slots_beam refuses a source that holds a rule, dots_slots_score a slot that does (DOTS_E_STATE).
 * dots_row_loop_hit   out[3] = {index of the firing token, the period, the span L(period)}, or {-1, 0, 0}: no hit (yet), or the row holds
 *                     no rule.  Synchronises.
 * dots_loop_probe     a test entry: case c is the history ids_host[c * stride + 0 .. lens_host[c]), fed id by id through the device check
 *                     under `rule` from zeroed counters; hits_out_host[c * 3 ..] = the first hit as dots_row_loop_hit reports it.  One
 *                     launch, one workgroup per case.  Synchronises. */
#define DOTS_MAX_LOOP_PERIOD 1024
typedef struct DotsLoopRule {
    int32_t min_period;          /* 1 .. max_period */
    int32_t max_period;          /* .. DOTS_MAX_LOOP_PERIOD */
    int32_t repeats;             /* 2 .. 64: the cycle must stand this many times ... */
    int32_t min_span;            /* 0 .. 65535: ... over at least this many tokens */
} DotsLoopRule;
int dots_set_row_loop(DotsEngine* e, int row, const DotsLoopRule* r);
int dots_row_loop_hit(DotsEngine* e, int row, int32_t* out);
int dots_loop_probe(DotsEngine* e, const int32_t* ids_host, const int32_t* lens_host, int cases, int stride, const DotsLoopRule* rule,
                    int32_t* hits_out_host);

/* ---- N-gram speculative decoding: opt-in, engine-wide, slot mode only.  With k drafts a slot occupies up to
 * k + 1 rows of one decode step: row j carries token j of (last committed token, draft 1 .. k) at context ctx + j on the slot's own KV
 * pages, and sees the K/V rows 0 .. j - 1 appended in the step's qkv launch.  Every decode kernel is row-independent and batch-invariant
 * bit for bit, so row j's logits are those of the sequential step at that position; the step commits row 0's token as an unspeculated
 * step does and then, while draft j equals the token just committed, the arg max of row j + 1 — through the same bookkeeping (EOS ids,
 * generation cap, output, context).  The tokens of a greedy row are therefore EXACTLY those of the unspeculated engine; a step commits
 * 1 .. k + 1 of them, so dots_slots_decode(n) may finish a row before n steps have run.  The K/V of rejected drafts stay where they were
 * written; the next step overwrites those positions.
 *
 * By default only plain greedy rows speculate: a row with DotsSamplingParams, DotsLogitRules, a guide, an n-gram rule, stop strings or
 * logprobs of its own, and every row while dots_set_sampling has a temperature > 0, verifies no draft and decodes inside the speculating
 * step exactly as before.  dots_generate / dots_decode_step (the closed static batch) ignore the setting.
 *
 * dots_set_speculation_rows widens that: DOTS_SPEC_ROWS_SAMPLED lets a row with DotsSamplingParams speculate when they carry no penalty
 * (any temperature, top_k, top_p and seed), DOTS_SPEC_ROWS_STOP a row with stop strings; a row with both needs both bits.  A sampled
 * row's draft row j is selected by the row's own sampler with the counter of the output index it stands for (tokens generated + j), over
 * integer sums that do not depend on the order of the atomics: it is the token the unspeculated engine draws there, so the row's tokens
 * are EXACTLY those of the unspeculated engine for the same seed.  The accept walk advances the stop automaton through the commit a
 * sequential step uses: the row finishes at the same token, with the same hit record.
 *
 * dots_set_speculation_guided lets a row that holds a guide speculate too.  A guide's state depends on the committed tokens only, so the
 * state draft row j must be selected under — the slot's state walked over the bytes of drafts 1 .. j — is known at the head of the step:
 * the row's allowed bits, its arg max (or, for a sampled row under DOTS_SPEC_ROWS_SAMPLED, its draw) under the guide and the accept walk's
 * commits are those of the sequential step, so the tokens are again EXACTLY those of the unspeculated engine.  A draft the guide could not
 * have committed at its position (no bytes, an EOS id, a byte without a transition) verifies nothing from there on.  A row speculates iff
 * every feature it carries is let through: a guided row with DotsSamplingParams also needs DOTS_SPEC_ROWS_SAMPLED, one with stop strings
 * DOTS_SPEC_ROWS_STOP.
 *
 * dots_set_speculation_shaped closes the set: DOTS_SPEC_SHAPED_NGRAM lets a row with an n-gram rule speculate, DOTS_SPEC_SHAPED_RULES a
 * row with DotsLogitRules, DOTS_SPEC_SHAPED_PENALTY a row whose DotsSamplingParams carry a penalty (it needs DOTS_SPEC_ROWS_SAMPLED too,
 * as any row with parameters).  Draft row j is selected under the hypothesis that drafts 1 .. j were committed, and under it everything
 * that shapes the selection is known at the head of the step: the history the n-gram rule reads is the output followed by those drafts,
 * the output counts are the row's counts plus their occurrences, the output index min_tokens is compared with is tokens generated + j.
 * The counts change only when a token is committed, so a rejected draft leaves nothing behind, and the tokens are again EXACTLY those of
 * the unspeculated engine.  Under an engine-wide temperature no row speculates.
 *
 * dots_set_speculation_logprobs lets a row that returns logprobs (dots_set_row_logprobs) speculate.  A row's log-probabilities are a
 * function of its raw logits row alone, and the logits of draft row j are those of the sequential step at that position: the stage
 * reduces the live draft rows of such slots beside row 0, and after the accept walk the entries of the ACCEPTED candidates are written
 * at the output positions their commits appended at.  tok_lp, top_ids and top_lp of every position are EXACTLY, bit for bit, those of
 * the unspeculated engine; rejected and idle draft rows write nothing.  A row speculates iff every other feature it carries is let
 * through by the switches above.
 *
 * The built-in drafter looks the row's last tokens up in the row's OWN output (the prompt is not searched: image pads and a short
 * instruction).  With out[0 .. L) the tokens generated so far, for n from max_n down to min_n with n + 1 <= L: key = out[L - n .. L);
 * among the i with out[i .. i + n) == key and i + n < L take the largest i with i + n + k <= L if one exists, else the smallest i; the
 * draft is out[i + n .. min(i + n + k, L)).  The first n that has a match wins; no match = no drafts.
 *
 * dots_set_speculation  k drafts per slot and step: 0 = off (the default: a step launches exactly the kernels it launched before), 1 ..
 *                       DOTS_MAX_SPEC_DRAFTS.  1 <= min_n <= max_n <= DOTS_MAX_NGRAM_SIZE, or max_n = 0: no built-in drafter, the host
 *                       drafts (dots_set_row_drafts).  With k > 0 the usable slots are [0, max_batch / (k + 1)): dots_slots_prefill into a
 *                       higher slot returns DOTS_E_CAPACITY.  Allowed only while no slot is occupied (DOTS_E_STATE); zeroes the counters
 *                       and drops the captured steps.  DOTS_E_CAPACITY when max_batch < k + 1.
 * dots_set_speculation_rows  flags: DOTS_SPEC_ROWS_SAMPLED | DOTS_SPEC_ROWS_STOP; 0 (the default) = plain greedy rows only, and a step
 *                       launches exactly what it launched before.  The setting survives dots_set_speculation calls.  Allowed only while
 *                       no slot is occupied (DOTS_E_STATE); unknown bits: DOTS_E_INVALID.
 * dots_set_speculation_guided  on != 0: rows that hold a guide may verify drafts; 0 (the default): they never do, and a step launches
 *                       exactly what it launched before.  A call of its own, not a bit of dots_set_speculation_rows.  The setting
 *                       survives dots_set_speculation calls.  Allowed only while no slot is occupied (DOTS_E_STATE); a change drops the
 *                       captured steps.  The first call that switches it on allocates one int32 per step row.
 * dots_set_speculation_shaped  flags: DOTS_SPEC_SHAPED_NGRAM | DOTS_SPEC_SHAPED_RULES | DOTS_SPEC_SHAPED_PENALTY; 0 (the default): such rows
 *                       never verify a draft, and a step launches exactly what it launched before.  A call of its own, not bits of
 *                       dots_set_speculation_rows.  The setting survives dots_set_speculation calls.  Allowed only while no slot is
 *                       occupied (DOTS_E_STATE); unknown bits: DOTS_E_INVALID; a change drops the captured steps.  Allocates nothing.
 * dots_set_speculation_logprobs  on != 0: rows with logprobs on may verify drafts; 0 (the default): they never do, and a step launches
 *                       exactly what it launched before (as it does with the switch on while no row has logprobs on).  A call of its
 *                       own.  The setting survives dots_set_speculation calls.  Allowed only while no slot is occupied (DOTS_E_STATE); a
 *                       change drops the captured steps.  The first call that switches it on allocates the accept record (16 int32 per
 *                       step row).
 * dots_set_row_drafts   the n <= k drafts slot `row` verifies in its NEXT step, replacing what the drafter left (stream ordered; they are
 *                       spent by that step).  DOTS_E_INVALID: n > k or an id outside [0, vocab); DOTS_E_STATE: the slot is not occupied.
 *                       A row that does not speculate ignores them.
 * dots_spec_stats       speculating steps the row took, draft tokens it verified (after the generation cap cut them) and draft tokens it
 *                       committed, since the row's prefill; row = -1: the engine's totals since the last dots_set_speculation. */
#define DOTS_MAX_SPEC_DRAFTS 15
#define DOTS_SPEC_ROWS_SAMPLED 1
#define DOTS_SPEC_ROWS_STOP 2
#define DOTS_SPEC_SHAPED_NGRAM 1
#define DOTS_SPEC_SHAPED_RULES 2
#define DOTS_SPEC_SHAPED_PENALTY 4
int dots_set_speculation(DotsEngine* e, int k, int min_n, int max_n);
int dots_set_speculation_rows(DotsEngine* e, int flags);
int dots_set_speculation_guided(DotsEngine* e, int on);
int dots_set_speculation_shaped(DotsEngine* e, int flags);
int dots_set_speculation_logprobs(DotsEngine* e, int on);
int dots_set_row_drafts(DotsEngine* e, int row, const int32_t* ids_host, int n);
int dots_spec_stats(DotsEngine* e, int row, int64_t* steps, int64_t* drafted, int64_t* accepted);

/* Predicted outputs: a slot may hold a PREDICTION, a text the caller expects the output to resemble (a PDF's text layer,
 * another engine's result, an earlier run).  While the engine speculates with its built-in drafter (k > 0, max_n > 0) a second drafter
 * runs at the end of every step, on the GPU, and proposes the prediction's tokens as the slot's drafts where it can align the grown output
 * with it.  A prediction only changes which tokens are PROPOSED: every draft is verified by the step that follows exactly as an n-gram
 * draft is, so tokens, logprobs and stop hits are those of the unspeculated engine whatever the prediction holds.
 *
 * The rule.  out[0 .. L) is the slot's output, pred[0 .. P) its prediction; k, min_n, max_n are dots_set_speculation's.  The slot keeps an
 * alignment (cur, at): prediction index cur was where the next token was expected when the output was `at` long, so now it is expected
 * at e* = cur + (L - at).  cur = at = 0 when the prediction is set and when the slot is prefilled.
 *   1. anchor  m = min(min_n, L, e*).  If m >= 1, e* < P and pred[e* - m .. e*) == out[L - m .. L): e = e*.
 *   2. search  otherwise, for n from min(max_n, L) down to min_n with key = out[L - n .. L): the candidates are the e = i + n < P with
 *              pred[i .. i + n) == key.  The first n that has a candidate wins; among its candidates the one nearest to e*, the larger e
 *              on a tie.
 *   3. found   the slot's drafts are pred[e .. min(e + k, P)); cur = e, at = L.
 *   4. else    (or the slot holds no prediction) the slot keeps the drafts the own-output rule above left; cur and at stay, so e* moves on
 *              with L.
 * Rows that take no step, finished rows and rows that do not speculate are left alone, as by the built-in drafter.
 *
 * dots_set_row_prediction  slot `row` holds ids_host[0 .. n) from now on (copied; stream ordered), aligned with the start of its output.
 *                       n = 0 or ids_host = NULL: it holds none, and drafts it took from the one it held are dropped.  May be called
 *                       before the slot's prefill, like the other row setters.  dots_slots_prefill (and the chunked and cached forms)
 *                       restart the alignment and the counters; dots_slot_release and dots_slots_reset clear the prediction.  A fork's
 *                       children, beams, extends and scores carry none.  On an engine that does not speculate, or speculates with
 *                       max_n = 0, it is stored and inert.  While no slot holds one a step launches exactly what it launched before.  The
 *                       first call that sets one allocates max_batch x max_seq_len int32.  DOTS_E_INVALID: row out of range, n < 0, an id
 *                       outside [0, vocab); DOTS_E_CAPACITY: n > max_seq_len.
 * dots_row_prediction_stats  prediction tokens the row verified as drafts (after the generation cap cut them, as dots_spec_stats counts)
 *                       and prediction tokens it committed, since the row's prefill.  dots_spec_stats counts them too, unchanged. */
int dots_set_row_prediction(DotsEngine* e, int row, const int32_t* ids_host, int n);
int dots_row_prediction_stats(DotsEngine* e, int row, int64_t* drafted, int64_t* accepted);

/* Log-probabilities: log_softmax of the raw fp32 logits of the step (before penalties, temperature, top-k and top-p:
 * the values dots_get_logits returns), for every token a row commits, the prefill's first token included.  The top entries are
 * ordered by value descending, then index ascending.  lse comes from per-chunk (max, sum) pairs merged in a fixed chunk order, so a
 * row's values are bitwise the same alone, in any batch and in any slot.  Tokens and logits are the same with logprobs on or off. */
#define DOTS_MAX_TOP_LOGPROBS 20
/* Row `row` (a slot, or sequence b of a static batch) returns log-probabilities of the raw logits for every token selected from now on
 * (the first token of a following dots_prefill / dots_slots_prefill included).  top_n: -1 = off, 0 = the chosen token only, 1..20.
 * Stream ordered; captured decode graphs are kept.  dots_slot_release / dots_slots_reset switch the row off.  The output buffers
 * (max_batch x max_seq_len x 164 B) are allocated by the first call that switches a row on; from then on every prefill of a row
 * fills its positions with NaN / -1 first, whether or not the row is on.  DOTS_E_INVALID for a vocabulary above 262 144. */
int dots_set_row_logprobs(DotsEngine* e, int row, int top_n);
/* Positions [pos0, pos0 + n) of the row's generated tokens: tok_lp float [n], top_ids int32 [n][20], top_lp float [n][20]
 * (entries beyond the row's top_n, and positions selected while the row was off: -1 / NaN).  *n_out = positions that exist.
 * Slot mode: an occupied slot (read before dots_slot_release).  Static mode: rows < B after dots_generate / dots_decode_step. */
int dots_row_logprobs(DotsEngine* e, int row, int pos0, int n, float* tok_lp_host, int32_t* top_ids_host, float* top_lp_host, int32_t* n_out);
/* Launch plan of the decode step (results are bit-identical under either plan).  0 (default) = chosen by where the step runs: the
 * whole-chip plan (qkv / o_proj / down_proj as 8-row half tiles: 256 / 192 / 192 workgroups; one gate|up workgroup per tile pair), or —
 * while the step is replayed on the decode CU partition beside a prefetched vision tower (dots_vit_prefetch) — the PARTITION plan: the
 * projections as whole 16-row tiles (half as many workgroups) and gate|up as one resident round of workgroups that walk the tile pairs.
 * 1 = the partition plan on every step (tests, A/B runs; slower on the whole chip).  Environment DOTS_OCR_DECODE_PLAN sets the default.
 * Batches above 16 rows run the WIDE qkv / projection kernels under either plan (round 5: every batch tile in one workgroup, one dispatch
 * round sized for the CUs of the stream; DOTS_OCR_DEC_WIDE=0 = the per-tile kernels, same bits).
 * Round 5: + 2 = the STREAMING decode-attention kernel (one resident workgroup per CU walks the (row, kv head, split) items, pages arrive by
 * LDS-DMA one item ahead) wherever it is legal, + 4 = always one workgroup per item (also the default: the streaming kernel measured
 * slower at every batch size, profiles/r05_decode_attn_stream_ab.txt).  Same bits either way. */
int dots_set_decode_plan(DotsEngine* e, int plan);
/* Tower tail of the vision prefetch (round 5).  A prefetched tower (dots_vit_prefetch) runs on the upper CU partition beside the decode
 * loop; its LAST `tail` blocks (and the merger) run on the whole chip instead, so that the decode partition does not idle when the decode
 * loop of a step drains before the tower.  set = -1: adaptive — per launch, from the events of the previous one: the partition
 * part is sized to end when the last decode chunk did (a decode loop that outlasts the tower gives 0; for pipelines whose decode work per
 * admission is finite, as bench.py's); set >= 0: that many blocks on every launch (0 = off, the default); set = -2: leave it as it is.  Environment DOTS_OCR_TOWER_TAIL_LAYERS = the initial `set`.  *now (may be NULL) receives the tail of the tower
 * launched last.  Results do not depend on it (the same kernels in the same order). */
int dots_tower_tail(DotsEngine* e, int set, int* now);
/* Launch plan of the 256-wide bf16 MFMA GEMM behind the vision tower and the prefill (results are bit-identical under either plan:
 * the same MFMAs in the same k order per output element).  0 = 8 waves per workgroup, two per SIMD running half a K sub-tile apart
 * (round 2); 1 (default) = 4 waves, one per SIMD owning a 128 x 128 output block in 256 accumulator registers, K tiles of 64 streamed by
 * LDS-DMA through a 5-unit ring, one barrier per 64 MFMAs (round 5).  PROCESS-wide (the kernels are shared by every engine of the process);
 * environment DOTS_OCR_GEMM_PLAN sets the default. */
int dots_set_gemm_plan(DotsEngine* e, int plan);

/* ---- Continuous batching (the serving loop the reference delegates to vLLM: README "vLLM inference", parser.py:138-166
 * fires one request per page at it and the server keeps its batch full).  The engine's max_batch KV slots are
 * independent sequences: a finished sequence is read out, its slot released and refilled by a new prefill while the other
 * slots keep decoding.  Any static-batch call (dots_prefill / dots_generate) resets every slot.
 *
 * dots_slots_reset   enter slot mode with every slot free and every KV page back in the pool (a serving loop calls it once at start:
 *                    the pages of an earlier static batch would otherwise count as used until the first dots_slots_prefill); a prefetched
 *                    vision batch that was never taken is dropped.
 * dots_set_eos       stop tokens for the slot calls.
 * dots_slots_prefill n new sequences (packed ids, like dots_prefill) into the free slots `slots[i]`, each with its own
 *                    cap on generated tokens; if the prompts hold image tokens, run dots_vit_forward for exactly these
 *                    sequences first.  Selects each new sequence's first token.
 * dots_slots_decode  n_steps decode steps over all occupied slots (one captured graph per (rows, kv-split) shape).
 *                    Finished sequences idle in place: their context is frozen and nothing more is appended.  Before the steps
 *                    every running sequence is given the KV pages its next n_steps positions need (on-demand paging); if the pool
 *                    is dry the sequence keeps its pages and its generation cap is lowered to what they hold — it finishes there
 *                    (reason "length", as HF generate does at the context capacity); dots_slot_capacity reports the lowered cap.
 * dots_slots_poll    finished[b] = -1 free / 0 running / 1 finished / 2 suspended (dots_slot_suspend) / 3 filling (dots_slots_prefill_begin),
 *                    out_lens[b] = tokens generated so far; both
 *                    int32 [max_batch].  Synchronises the stream.
 * dots_slot_read     copies min(n, capacity) generated ids of one occupied slot, *n_out = n.
 * dots_slot_release  marks the slot free.
 * dots_slots_fork    parallel sampling: gives each of the n free slots dst_slots_host[i] a copy of the freshly prefilled sequence
 *                    in src_slot — same prompt, same KV, the source's cap on generated tokens — and its own first token, selected from the
 *                    source's last-position logits under the row parameters already set on that slot (sampling, logprobs, logit rules,
 *                    guide, n-gram rule: set, then fork, as with dots_slots_prefill).  From then on a child is an independent sequence: it
 *                    generates, bit for bit, what a dots_slots_prefill of the same prompt into that slot would have.  src_slot must have
 *                    been filled by the most recent dots_slots_prefill with no decode step issued since (DOTS_E_STATE otherwise); several
 *                    forks may follow one prefill.  A child's block-table row names the source's floor(L / 64) full prompt pages
 *                    (reference counted: a page returns to the pool when its last holder is released; dots_kv_pool_info counts physical
 *                    pages) and takes ceil(min(L + min(max_new, 64), max_seq_len) / 64) - floor(L / 64) pages of its own, the first of
 *                    which receives a copy of the source's partially filled page.  Refused with nothing changed: a destination out of
 *                    range, repeated or equal to the source (DOTS_E_INVALID), occupied (DOTS_E_STATE), not usable while speculating, or a
 *                    pool that cannot serve the children's pages (DOTS_E_CAPACITY).  Synchronises the stream. */
int dots_slots_reset(DotsEngine* e);
int dots_slots_fork(DotsEngine* e, int src_slot, const int32_t* dst_slots_host, int n);
int dots_set_eos(DotsEngine* e, const int32_t* eos_ids_host, int n_eos);
int dots_slots_prefill(DotsEngine* e, const int32_t* slots_host, int n, const int32_t* input_ids_host,
                       const int32_t* prompt_lens_host, const int32_t* max_new_tokens_host);
/* ---- Extend a live sequence: more prompt tokens behind the KV cache a slot already holds — several prompts over one
 * prefilled page, or a next turn behind a generated answer — without a second tower or prefill.
 *
 * dots_slots_extend  every listed slot holds the K/V of some context c and one pending token (selected, its K/V not yet written).  ids_host
 *                    packs lens_host[i] >= 1 tokens per slot.  keep_pending_host[i] = 1: the pending token stays in the sequence and the row
 *                    is fed [pending, ids...] (a next turn: the pending token is the answer's last token, normally its EOS);
 *                    0: the pending token is dropped and the row is fed [ids...] (a prefix that was prefilled only to be extended).
 *                    Afterwards the slot is what a dots_slots_prefill of the longer prompt would have left: prompt = c + tokens fed,
 *                    limit = prompt + max_new_tokens_host[i], no output, running, logprob positions cleared, guide and stop automata at
 *                    their start with no hit, the n-gram history and the sampler's counter from zero, and its first token selected from the
 *                    logits of its last fed token under everything set on the row (set, then extend, as with dots_slots_prefill).  The fed
 *                    rows run through the decode kernels at their positions, in chunks of at most max_batch rows: the state is, bit for
 *                    bit, that of feeding the same tokens one decode step at a time.  READ THE EARLIER OUTPUT FIRST (dots_slot_read,
 *                    dots_row_logprobs, dots_row_stop_hit): the call discards it.  A fork comes before an extend: the call ends the window
 *                    in which the most recent dots_slots_prefill can be forked.  Pages: every slot is grown to
 *                    ceil(min(prompt + min(max_new, 64), max_seq_len) / 64) pages.
 *                    Refused with nothing changed: a slot out of range or listed twice, lens < 1, max_new < 1, an id out of range or an image
 *                    token (DOTS_E_INVALID); a free or suspended slot, a row of a beam group, a row that carries a penalty, a speculating
 *                    engine, a static batch (DOTS_E_STATE); prompt + max_new_tokens above max_seq_len, or a pool that cannot serve the
 *                    pages (DOTS_E_CAPACITY).  Synchronises. */
int dots_slots_extend(DotsEngine* e, const int32_t* slots_host, int n, const int32_t* ids_host, const int32_t* lens_host,
                      const int32_t* keep_pending_host, const int32_t* max_new_tokens_host);
/* ---- Score given tokens on a live sequence: teacher-forced log-probabilities of a text the engine did not generate — vLLM's
 * prompt_logprobs over a suffix — in passes of max_batch positions instead of one decode step per token.
 *
 * dots_slots_score   dots_slots_extend with a record: the same arguments, checks, page arithmetic and launches, and every listed slot is
 *                    left in exactly the state dots_slots_extend with the same arguments leaves it (KV, context, first token selected from
 *                    its last fed row, automata restarted), so a scored prefix can be continued by ordinary decoding.  top_n_host[i] in
 *                    [0, DOTS_MAX_TOP_LOGPROBS] is slot i's top-list length.  Let F = [pending] + ids with keep_pending, else ids, f = |F|.
 *                    Entry j (0 <= j < f - 1) of the slot holds what the logprob stage (dots_set_row_logprobs) would have written had the
 *                    row at F[j]'s position selected F[j+1]: tok_lp = l[F[j+1]] - lse over the fp32 lm_head row l at F[j]'s position, and
 *                    the top_n largest raw logits as (id, l[id] - lse), value descending then id ascending; -1 / NaN beyond top_n.  Bit
 *                    for bit the entry of a sequential step forced to F[j+1].  The last fed row records nothing (its logits select the
 *                    slot's first token, as in an extend); f == 1 records zero entries.  The slot's entries are 0xFF-filled when the call
 *                    starts and stay readable until the next prefill, extend, score, release or reset of that slot.  The logits of the
 *                    fed rows go to a scratch of the call's own: dots_slot_logits of a slot outside the call is untouched.  The scratch
 *                    and the entries ([max_batch][max_seq_len]; the top lists once a call asks for top_n > 0) are allocated by the first
 *                    scoring call: an engine that never scores allocates and launches nothing of this.
 *                    Refused with nothing changed, as dots_slots_extend: a slot out of range or listed twice, lens < 1, max_new < 1, an id
 *                    out of range or an image token, top_n outside [0, 20] (DOTS_E_INVALID); a free, filling or suspended slot, a row of a
 *                    beam group, a row that carries a penalty, a speculating engine, a static batch (DOTS_E_STATE); prompt +
 *                    max_new_tokens above max_seq_len, or a pool that cannot serve the pages (DOTS_E_CAPACITY).  Synchronises.
 * dots_slot_scores   entries [pos0, pos0 + n) of the slot's row of the record (pos0 + n <= max_seq_len), in the layout of
 *                    dots_row_logprobs: tok_lp float [n], top_ids int32 [n][20], top_lp float [n][20].  *n_out = the number of entries the
 *                    slot's last score recorded; entries from there on read as 0xFF (NaN / -1).  DOTS_E_STATE for a free slot and for a
 *                    slot that has not been scored since it was filled or extended.  Synchronises. */
int dots_slots_score(DotsEngine* e, const int32_t* slots_host, int n, const int32_t* ids_host, const int32_t* lens_host,
                     const int32_t* keep_pending_host, const int32_t* max_new_tokens_host, const int32_t* top_n_host);
int dots_slot_scores(DotsEngine* e, int slot, int pos0, int n, float* tok_lp_host, int32_t* top_ids_host, float* top_lp_host, int32_t* n_out);
/* ---- Chunked prefill: the prompts of dots_slots_prefill filled in passes over their own KV pages, so that decode chunks of
 * the running slots can run between the passes and a prompt may be longer than max_prefill_tokens.
 *
 * dots_slots_prefill_begin    arguments and checks of dots_slots_prefill, except that the packed length is bounded by max_seq_len per prompt
 *                             and by the pool only.  Reserves every slot's admission pages (all or nothing), embeds every prompt whole —
 *                             vision rows included: run dots_vit_forward for exactly these sequences first, its rows are free again when the
 *                             call returns — and leaves the slots FILLING at position 0.  Refused on a speculating engine (DOTS_E_STATE).
 * dots_slots_prefill_advance  one pass of the prefill's layer loop over up to max_tokens positions (a positive multiple of 64, at most
 *                             max_prefill_tokens) of the filling slots, oldest begin first; a cut falls on a multiple of 64 positions of its
 *                             sequence or at its end.  A slot whose last prompt token is in the pass completes as at the end of
 *                             dots_slots_prefill (first token selected, running, forkable until the next step).  *remaining = positions
 *                             still to fill over all filling slots.  What a position computes does not depend on the cuts: logits, KV pages
 *                             and everything generated afterwards are identical in every bit for every max_tokens.
 * A filling slot is inert: decode steps, dots_slots_extend and dots_slots_prefill of other slots may run between passes and touch nothing
 * of it.  dots_slots_poll reports 3; dots_slot_release returns its pages; dots_slots_reset drops every fill; dots_slot_suspend,
 * dots_slots_extend, dots_slots_fork, dots_slots_beam, dots_slot_read and dots_slot_logits refuse it (DOTS_E_STATE), as do
 * dots_slots_prefill and dots_slots_prefill_begin into it. */
int dots_slots_prefill_begin(DotsEngine* e, const int32_t* slots_host, int n, const int32_t* input_ids_host, const int32_t* prompt_lens_host,
                             const int32_t* max_new_tokens_host);
int dots_slots_prefill_advance(DotsEngine* e, int max_tokens, int32_t* remaining);
/* ---- Prefix cache over the chunked prefill, off until switched on: full prompt pages (64 positions) that a pass of
 * dots_slots_prefill_advance wrote stay resident after their sequence is released, indexed by (the block before, the 64 token ids, the
 * 16-byte key of the prompt's image if a pad lies in the block or before it), and a later prompt that begins with the same blocks starts
 * its fill behind them.  Such a fill equals the cold chunked fill of the same prompt in every bit.  The index holds one reference on every
 * cached page; a page held by the index alone is evicted (least recently used first, deepest block first among equally old) whenever the
 * free list cannot serve a request, and counts as free in dots_kv_pool_info, dots_slots_pages_short and every admission check.  A prompt
 * with more than one image, or with an image and no key, is neither looked up nor inserted.  The key is the caller's promise that equal
 * keys mean equal pixels and grid.
 *
 * dots_prefix_cache_enable   on != 0 / 0.  DOTS_E_STATE while a slot is occupied or filling, and on a speculating engine (which in turn
 *                            cannot start to speculate while the cache is on).  Off drops every block and lease; the pages return.
 * dots_prefix_cache_lookup   walks the blocks of ids_host[0 .. len).  *hit_tokens = min(64 * matched, 64 * ((len - 1) / 64)): at least
 *                            one position is always computed.  *needs_tower = 0 when no image position lies at or behind *hit_tokens,
 *                            or when a resident block retains the tower's rows for all of them (they end in the page behind the hit).
 *                            *lease (> 0) holds a reference on every page the answer relies on until it is given to
 *                            dots_slots_prefill_begin_cached or to dots_prefix_cache_release; 0: nothing matched, or the prompt
 *                            bypasses the cache (then nothing is counted either).  image_key: 16 bytes or NULL.
 * dots_prefix_cache_release  gives an unused lease back (DOTS_E_INVALID: not held).
 * dots_slots_prefill_begin_cached  dots_slots_prefill_begin + per prompt a lease (0: none) and an image key (NULL: none).  A leased
 *                            prompt's table row names the lease's pages first; only the other pages are reserved and only positions
 *                            at or behind the hit are embedded and filled.  Run dots_vit_forward for exactly the prompts that hold
 *                            image tokens and no lease with needs_tower == 0.  The full prompt pages these fills complete are inserted
 *                            as their pass is issued.  A lease is consumed by success only: a refused call leaves it held.
 *                            dots_slots_prefill_begin itself never looks up and never inserts.
 * dots_prefix_cache_info     int64 [6]: lookups, hit tokens, blocks inserted, blocks evicted, resident pages, evictable pages. */
int dots_prefix_cache_enable(DotsEngine* e, int on);
int dots_prefix_cache_lookup(DotsEngine* e, const int32_t* ids_host, int len, const uint8_t* image_key, int32_t* lease, int32_t* hit_tokens,
                             int32_t* needs_tower);
int dots_prefix_cache_release(DotsEngine* e, int32_t lease);
int dots_slots_prefill_begin_cached(DotsEngine* e, const int32_t* slots_host, int n, const int32_t* input_ids_host, const int32_t* prompt_lens_host,
                                    const int32_t* max_new_tokens_host, const int32_t* leases_host, const uint8_t* const* image_keys);
int dots_prefix_cache_info(DotsEngine* e, int64_t* out6);
int dots_slots_decode(DotsEngine* e, int n_steps);
int dots_slots_poll(DotsEngine* e, int32_t* finished_host, int32_t* out_lens_host);
int dots_slot_read(DotsEngine* e, int slot, int32_t* out_ids_host, int capacity, int32_t* n_out);
int dots_slot_release(DotsEngine* e, int slot);
/* ---- Streaming: every streaming row's NEW tokens and logprob entries per scheduler chunk, in one launch and one stream
 * synchronisation however many rows stream.
 *
 * dots_set_row_stream   a row setting like dots_set_row_logprobs: set before the slot's prefill (or fork), switched off by
 *                       dots_slot_release and dots_slots_reset.  The row's cursor — the number of its output tokens already delivered —
 *                       starts at 0 wherever the engine starts the slot's output: an admission, a fork child, dots_slots_extend /
 *                       dots_slots_score.  DOTS_E_STATE for a row of a beam group (a group's outputs are reordered).  The first call
 *                       allocates the cursors and a pinned staging block; an engine that never streams allocates and launches nothing.
 * dots_slots_drain      a superset of dots_slots_poll: the same finished / out_lens and the same host-side effects, and for every
 *                       streaming row b the tokens out_ids[b][cursor, out_len), at most DOTS_STREAM_ROW_CAP of them (the oldest; the rest
 *                       come with the next drain), packed in slot order: tokens[first[b] .. first[b] + count[b]).  Rows that also return
 *                       logprobs get the matching entries in the layout of dots_row_logprobs behind lp_first[b] (-1: none).  The cursor
 *                       advances by what was delivered.  A suspended row delivers what it held at the suspend; a row that does not
 *                       stream, a free and a filling slot deliver nothing.  tokens_cap / lp_cap (entries) must hold
 *                       DOTS_STREAM_ROW_CAP per streaming row (per streaming row with logprobs): max_batch x DOTS_STREAM_ROW_CAP always
 *                       does.  With no streaming row the call IS dots_slots_poll.  Never part of a captured step. */
#define DOTS_STREAM_ROW_CAP 256
int dots_set_row_stream(DotsEngine* e, int row, int on);
int dots_slots_drain(DotsEngine* e, int32_t* finished_host, int32_t* out_lens_host, int32_t* first_host, int32_t* count_host, int32_t* lp_first_host,
                     int32_t* tokens_host, int tokens_cap, float* tok_lp_host, int32_t* top_ids_host, float* top_lp_host, int lp_cap,
                     int32_t* n_tokens, int32_t* n_lp);
/* ---- Beam search: a group of B beams, 2 <= B <= DOTS_MAX_BEAMS, over shared KV pages.  These are vLLM's beam-search
 * semantics with HF's length normalisation applied by the caller; they are not HF's BeamSearchScorer.
 *
 * Per step, on the raw logits: every live beam i offers its 2B best (lp, id) pairs (value descending, id ascending; lp = logit - lse,
 * bitwise what dots_row_logprobs returns for an ordinary row with the same prefix), a candidate is (i, rank r, id, s = fp32(cum[i] + lp));
 * candidates whose s is NaN or -inf do not exist; a candidate whose id is an EOS id (dots_set_eos) is recorded as completed
 * (step, parent beam, id, s); the B best others by (s descending, i ascending, r ascending) are the new beams, the rest of the beams is
 * dead (cum = -inf; token and parent read -1).  The group runs its cap of max_new_tokens steps (or until no beam is live); the first
 * selection is step 0.
 *
 * dots_slots_beam  src_slot and the n_dst free slots dst_slots_host become the group, in group order [src, dst...] (beam i = the i-th of
 *                  them).  src_slot as for dots_slots_fork: filled by the most recent dots_slots_prefill, no decode step since.  The
 *                  children share the source's floor(L / 64) full prompt pages; the group is fully reserved now: every beam owns
 *                  ceil((L + max_new) / 64) - floor(L / 64) pages plus one spare, and its block-table row belongs to the device from here
 *                  on (the mid-generation fork rewrites it inside the captured steps).  The source's own first token is replaced by the
 *                  group's first selection.  Refused with nothing changed: bad slots as dots_slots_fork, a pool that cannot serve the pages
 *                  (DOTS_E_CAPACITY), a speculating engine (DOTS_E_STATE), a group slot that carries row parameters, logit rules, a guide,
 *                  an n-gram rule, stop strings or logprobs (DOTS_E_INVALID; the row setters refuse a group row likewise).
 *                  dots_slots_decode steps the group with every other slot (a chunk that could complete more than 4096 hypotheses of one
 *                  group is refused: DOTS_E_CAPACITY); dots_slots_poll reports its rows finished together; dots_slot_release of any of
 *                  its slots releases all of them.  Synchronises.
 * dots_beam_info   B, steps done and completed records so far of the group that `slot` belongs to.  Synchronises.
 * dots_beam_read   + cum float [B]; tokens / parents int32 [B][step_capacity] (the first min(steps, step_capacity) steps of every beam:
 *                  parents[j][t] = the beam at step t - 1 that beam j of step t extends); done int32 [done_capacity][4] = (step, parent
 *                  beam, EOS id, the bits of s), every record since the group was made, in (step, beam, rank) order. */
#define DOTS_MAX_BEAMS 8
int dots_slots_beam(DotsEngine* e, int src_slot, const int32_t* dst_slots_host, int n_dst);
int dots_beam_info(DotsEngine* e, int slot, int32_t* n_beams, int32_t* steps, int32_t* n_done);
int dots_beam_read(DotsEngine* e, int slot, int32_t* n_beams, int32_t* steps, float* cum_host, int32_t* tokens_host, int32_t* parents_host,
                   int step_capacity, int32_t* done_host, int done_capacity, int32_t* n_done);
/* Paged KV pool: pages of 64 tokens in total / currently free (an admission policy checks this before dots_slots_prefill,
 * which refuses with DOTS_E_CAPACITY when prompt + 64 tokens of each new sequence do not fit). */
int dots_kv_pool_info(DotsEngine* e, int32_t* total_pages, int32_t* free_pages);
/* fp8 KV cache scales, fp32 [num_layers][num_kv_heads][2] (K, V), each finite and > 0, copied to the device array the decode kernels read
 * (captured decode graphs see them on replay).  DOTS_E_STATE while any sequence holds KV pages (after a static dots_generate: until
 * dots_slots_reset or the next dots_prefill releases them): a cached token keeps the scales it was written with.  Accepted for a bf16
 * cache too, where nothing reads them. */
int dots_set_kv_scales(DotsEngine* e, const float* scales_host);
/* Pages an occupied slot owns and its current limit on prompt + generated tokens (prompt + max_new_tokens unless the pool ran dry).  Of a
 * suspended slot: the pages that stayed resident. */
int dots_slot_capacity(DotsEngine* e, int slot, int32_t* pages_owned, int32_t* token_limit);
/* ---- Suspend and resume (vLLM's "swap" preemption): a running sequence is parked in its slot, its KV pages are moved to pinned
 * host memory and given back to the pool; later it continues on whatever pages are free then and generates, bit for bit, the tokens and
 * logprobs it would have generated undisturbed.  Opt-in: an engine that never calls these launches what it always did.
 *
 * dots_kv_swap_reserve    pinned host space for `pages` 64-token pages (each across all layers); regrown or, with 0, freed.  DOTS_E_STATE
 *                         while any slot is suspended.  Synchronises.
 * dots_kv_swap_info       host pages in total / currently free.
 * dots_slot_suspend       the slot must be occupied, running (not finished), not suspended, not a row of a beam group, and the engine must
 *                         not speculate (DOTS_E_STATE otherwise).  Every page the row holds alone is returned to the pool, those that hold
 *                         positions of its context after a copy to the host space; a page with other holders (the shared prompt pages of a
 *                         fork) stays resident and the row keeps its reference.  DOTS_E_CAPACITY when the host space cannot take the pages.
 *                         The slot stays occupied and keeps its row state (output, sampling / rule / guide / n-gram / stop state, logprobs):
 *                         dots_slot_read, dots_row_logprobs, dots_row_guide_state and dots_row_stop_hit work on it, dots_slots_poll reports
 *                         2 for it with out_lens as at the suspension, dots_slots_decode steps the others and gives it no pages,
 *                         dots_slot_release frees its host pages too, dots_slots_reset drops everything parked.  While a slot is
 *                         suspended, dots_set_speculation and dots_set_kv_scales are refused and the slot can be neither forked nor made a
 *                         beam group.  Synchronises.
 * dots_slot_resume        fresh pages from the free list, the KV copied back, the row running again.  DOTS_E_STATE: not suspended;
 *                         DOTS_E_CAPACITY: the pool cannot serve the row's pages.  Synchronises.
 * dots_slots_pages_short  *pages = how many pages the next dots_slots_decode(n_steps) would fail to obtain (0: no sequence would be capped),
 *                         by that call's own arithmetic.
 * Every refusal leaves pool, host space and slots unchanged. */
int dots_kv_swap_reserve(DotsEngine* e, int pages);
int dots_kv_swap_info(DotsEngine* e, int32_t* total_pages, int32_t* free_pages);
int dots_slot_suspend(DotsEngine* e, int slot);
int dots_slot_resume(DotsEngine* e, int slot);
int dots_slots_pages_short(DotsEngine* e, int n_steps, int32_t* pages);
/* ---- Shared-prefix decode attention (what vLLM calls cascade attention, here exact): rows that share prompt pages — the
 * children of a fork, a beam group, a prompts fan-out, two prefix-cache hits on one page image — read each shared KV split once per step
 * instead of once per row.  Opt-in, default off; tokens, logits, logprobs and KV are the same bits either way, on the bf16 and the fp8 pool.
 *
 * dots_set_shared_prefix_attention  on != 0 / 0, in stream order from the next dots_slots_decode; captured step graphs are kept.  The plan
 *                         (which rows name the same four full prompt pages in which KV split) is recomputed before a decode chunk only
 *                         after the slots changed, and lives in device arrays allocated by the first chunk with the switch on: an engine
 *                         that never switches it on allocates and launches nothing new, and a step whose plan is empty launches what
 *                         it launches with the switch off.  Inert, not refused, while the engine speculates, in dots_slots_extend /
 *                         dots_slots_score passes, in the static batch, and at max_seq_len above 16 k (n_splits * 4 < pages per row).
 * dots_shared_prefix_info int64 [4]: of the plan in force — items, rows in at least one item, (row, split) pairs covered — and,
 *                         cumulative, the KV pages not read: over steps and items, (members - 1) x 4 x kv heads x layers. */
int dots_set_shared_prefix_attention(DotsEngine* e, int on);
int dots_shared_prefix_info(DotsEngine* e, int64_t* out4);

/* fp32 logits [B, vocab] of the most recent prefill/decode step (tolerance checks). */
int dots_get_logits(DotsEngine* e, float* out_host);
/* fp32 logits [vocab] of an occupied slot's row as the most recent dots_slots_prefill, dots_slots_extend or decode step that ran over the
 * row left them (tolerance checks in slot mode; a plain step only: a speculating step lays its rows out differently).  Synchronises. */
int dots_slot_logits(DotsEngine* e, int slot, float* out_host);
/* Teacher forcing for per-step logit comparisons: overwrite the token the next decode step feeds. */
int dots_set_next_tokens(DotsEngine* e, const int32_t* tokens_host, int B);
/* Tokens chosen by the most recent prefill/decode step, int32 [B]. */
int dots_get_last_tokens(DotsEngine* e, int32_t* out_host);
int dots_get_stats(DotsEngine* e, DotsStats* out);
/* Debug / parity tooling (tools/layer_error_trace.py): keep a copy of the bf16 residual stream after every ViT block and every
 * LM prefill layer of the following dots_vit_forward / dots_prefill calls.  capacity_elems = 0 switches the capture off.
 * dots_debug_read_hidden: which = 0 ViT block `layer` -> [patches, v_embed_dim], which = 1 LM layer `layer` -> [tokens, hidden]. */
int dots_debug_capture_hidden(DotsEngine* e, int64_t capacity_elems);
int dots_debug_read_hidden(DotsEngine* e, int which, int layer, void* out_host, int64_t* rows_out);
/* Cached K (which = 0) or V (which = 1) of LM layer `layer`, positions pos0 .. pos0 + n - 1 of block-table row seq_or_slot (a static
 * batch's sequence index or a slot), in logical order [num_kv_heads][n][128] and the cache's storage type: bf16, or raw e4m3fn bytes
 * (kv_cache_dtype = 1).  DOTS_E_STATE if a position's page is not owned by that row.  Synchronises. */
int dots_debug_read_kv(DotsEngine* e, int layer, int seq_or_slot, int pos0, int n, int which, void* out_host);
int dots_synchronize(DotsEngine* e);

/* ---- device memory helpers (so a binding needs no other GPU library) ------------------- */
int dots_dev_alloc(DotsEngine* e, int64_t bytes, void** out_dev);
int dots_dev_free(DotsEngine* e, void* dev);
int dots_memcpy_h2d(DotsEngine* e, void* dst_dev, const void* src_host, int64_t bytes);
int dots_memcpy_d2h(DotsEngine* e, void* dst_host, const void* src_dev, int64_t bytes);

/* ---- single-kernel entry points (parity tests call the kernels through these) ---------- */
/* y = rmsnorm(x) * w : bf16 [rows, dim]; fp32 statistics; two roundings as modeling_qwen2.py:246-252 */
int dots_op_rmsnorm(DotsEngine* e, const void* x_dev, const void* w_dev, void* y_dev, int64_t rows, int dim, float eps);
int dots_op_layernorm(DotsEngine* e, const void* x_dev, const void* w_dev, const void* b_dev, void* y_dev,
                      int64_t rows, int dim, float eps);
/* C[M,N] = epilogue(A[M,K] @ W[N,K]^T + bias): bf16 in, fp32 accumulate.
 * epilogue: 0 none, 1 += residual (bf16 [M,N], may alias C), 2 SwiGLU (W rows interleaved in
 * 32-row gate/up groups, C is [M,N/2]), 3 exact GELU, 4 fp32 output. */
int dots_op_gemm(DotsEngine* e, const void* A_dev, const void* W_dev, const void* bias_dev,
                 const void* residual_dev, void* C_dev, int64_t M, int N, int K, int epilogue, const float* colscale_dev);
/* colscale_dev: NULL, or fp32 [N] multiplied into column n of the accumulator before the bias (the per-output-channel scale of
 * fp8 weights; W then holds the quantised values).
 * dots_op_quant_fp8: W bf16 [N,K] -> bf16(e4m3(W[n][:] / scale[n])) in place, scale_out[n] = max|W[n][:]| / 448 (1 for a zero row). */
int dots_op_quant_fp8(DotsEngine* e, void* w_inout_dev, float* scale_out_dev, int64_t N, int K);
/* The ViT / prefill GEMM of an fp8_weights engine: A bf16 [M,K] is quantised per token and W bf16 [N,K] per output channel to e4m3
 * (copies), then C = epilogue((Aq Wq^T) * a_scale[m] * w_scale[n] + bias) on the fp8 MFMA.  N % 256 == 0, K % 64 == 0; epilogues 0-3. */
int dots_op_gemm_fp8(DotsEngine* e, const void* A_dev, const void* W_dev, const void* bias_dev, const void* residual_dev, void* C_dev,
                     int64_t M, int N, int K, int epilogue);
/* Flash attention over packed sequences.  q [Hq, T, 128], k [Hkv, T, 128] bf16 (head-major),
 * vt [Hkv, 128, Tpad] (V transposed, every sequence padded to 64 keys, keys permuted inside
 * 16-groups as csrc/attn_prefill.hip documents), cu_seqlens int32 [n_seq+1] (host).
 * out bf16 [T, Hq*128]. */
int dots_op_flash_attn(DotsEngine* e, const void* q_dev, const void* k_dev, const void* vt_dev, void* out_dev,
                       const int32_t* cu_seqlens_host, int n_seq, int Hq, int Hkv, int causal, float scale);
/* Causal flash attention of blocks of NEW query rows over sequences whose keys already lie in the page pool (csrc/attn_paged.hip; what a
 * pass of dots_slots_prefill_advance runs).  Sequence b has prefix_host[b] positions in its pages (a multiple of 64; DOTS_E_INVALID
 * otherwise) and n_new_host[b] >= 1 new rows at positions prefix .. prefix + n_new - 1, whose keys and values are in the pages too; its
 * pages are row rows_host[b] (NULL: row b) of block_table_dev int32 [table_rows, max_pages].  q bf16 [Hq, T, 128] head-major, rope
 * applied, T = sum n_new, the sequences' rows packed in order; pool_layer as dots_op_decode_attn (kv_scales_dev == NULL) or
 * dots_op_decode_attn_kv8 (kv_scales_dev fp32 [Hkv][2]).  out bf16 [T, Hq*128].  Row at position p attends to keys 0 .. p. */
int dots_op_flash_attn_paged(DotsEngine* e, const void* q_dev, const void* pool_layer_dev, const int32_t* block_table_dev, int max_pages,
                             int table_rows, void* out_dev, const int32_t* rows_host, const int32_t* prefix_host, const int32_t* n_new_host,
                             int n_seq, int Hq, int Hkv, float scale, const float* kv_scales_dev);
/* Host-only (no device, no engine): how the flash-attention work list of a packed batch of sequences of lens[0 .. n_seq) patches and Hq heads
 * is cut across the 8 XCDs — base8[x] / cnt8[x] = the contiguous chunk of (sequence, head, query block) items XCD x walks, cost8[x] = its KV
 * tiles (csrc/kernels.h: XcdPlan; equal COST per XCD, not equal count: tests/test_cabi_cpu.py checks the balance on BASELINE configs[3]'s
 * page mix).  Returns the number of items, or a negative DOTS_E_*. */
int dots_plan_flash_xcd(const int32_t* lens, int n_seq, int Hq, int32_t* base8, int32_t* cnt8, int64_t* cost8);
/* Splits a packed qkv GEMM output [T, (Hq+2*Hkv)*128] into rope'd q/k and transposed v in the
 * layouts dots_op_flash_attn consumes.  rope2d != 0: vision 2-D rope from pos [T,2] int32;
 * else 1-D rope with positions pos [T] int32 and base theta. */
int dots_op_qkv_rope_split(DotsEngine* e, const void* qkv_dev, void* q_dev, void* k_dev, void* vt_dev,
                           const int32_t* cu_seqlens_host, int n_seq, const int32_t* pos_host,
                           int Hq, int Hkv, int rope2d, float theta);
/* x [T, K] bf16 @ w [(Hq+2*Hkv)*128, K]^T (+ bias) -> rope'd head-major q / k and transposed v (the layouts dots_op_flash_attn consumes), as the
 * prefill passes run it: fused != 0 = the GEMM's rope epilogue + the v transposition, fused == 0 = GEMM, then dots_op_qkv_rope_split's kernel.
 * Both give the same bits.  qkv_ws: [T, (Hq+2*Hkv)*128] bf16 workspace.  DOTS_E_INVALID if fused != 0 and no fused kernel serves the shape. */
int dots_op_qkv_proj_rope(DotsEngine* e, const void* x_dev, const void* w_dev, const void* bias_dev, void* qkv_ws_dev, void* q_dev, void* k_dev, void* vt_dev,
                          const int32_t* cu_seqlens_host, int n_seq, const int32_t* pos_host, int K, int Hq, int Hkv, int rope2d, float theta, int fused);
/* ---- single kernels of the decode step, at caller-chosen dimensions.  All tensors are device pointers in
 * the ROW-MAJOR layouts of the HF state dict / of a plain [B, features] activation; the MFMA fragment-order packing the
 * decode step uses (csrc/decode_layout.h) is applied inside with the engine's own pack kernels.  B <= 64.
 *
 * dots_op_dec_qkv      h [B,H] -> RMSNorm(ln_w) -> fused qkv projection wqkv [(Hq+2Hkv)*128, H] + bias -> 1-D RoPE at position
 *                      ctx_len[b] -> q_out bf16 [B, Hq*128]; the new key / value row of every sequence is appended to its
 *                      page: pool_layer [pages][Hkv][K|V][8192] bf16 (csrc/decode.hip header), block_table int32
 *                      [B, max_pages], ctx_len int32 [B] (tokens already in the cache).
 * dots_op_decode_attn  q bf16 [B, Hq*128] against the paged cache holding ctx_len[b] + 1 tokens per sequence (split-KV
 *                      kernel + combine kernel, KV split = the engine constant derived from max_seq_len) -> out bf16 [B, Hq*128].
 * dots_op_dec_proj     h_inout [B,N] += x [B,K] @ w [N,K]^T   (o_proj / down_proj with the residual add).
 * dots_op_dec_gateup   act_out [B,I] = silu(g) * u with g|u = RMSNorm(h) @ gate_w|up_w [I,H]^T.
 * dots_op_dec_lmhead   logits_out fp32 [B,V] = RMSNorm(h) @ w [V,H]^T.
 * fp8 != 0: the weight is quantised (dots_op_quant_fp8 on a copy), packed as e4m3 fragments and streamed by the fp8 instantiation
 * of the kernel — the path a DotsConfig.fp8_weights engine decodes with. */
int dots_op_dec_qkv(DotsEngine* e, const void* h_dev, const void* ln_w_dev, const void* wqkv_dev, const void* bias_dev,
                    const int32_t* ctx_len_dev, const int32_t* block_table_dev, int max_pages, void* pool_layer_dev, void* q_out_dev,
                    int B, int H, int Hq, int Hkv, float eps, float rope_theta, int fp8);
int dots_op_decode_attn(DotsEngine* e, const void* q_dev, const void* pool_layer_dev, const int32_t* ctx_len_dev,
                        const int32_t* block_table_dev, int max_pages, void* out_dev, int B, int Hq, int Hkv, int max_seq_len);
/* The same two kernels on an fp8 (e4m3fn) page pool [pages][Hkv][K|V][8192 B] (csrc/decode.hip header) with the fp32 scales
 * kv_scales_dev [Hkv][2] (K, V) — what a kv_cache_dtype = 1 engine decodes with. */
int dots_op_dec_qkv_kv8(DotsEngine* e, const void* h_dev, const void* ln_w_dev, const void* wqkv_dev, const void* bias_dev,
                        const int32_t* ctx_len_dev, const int32_t* block_table_dev, int max_pages, void* pool_layer_dev, void* q_out_dev,
                        int B, int H, int Hq, int Hkv, float eps, float rope_theta, int fp8, const float* kv_scales_dev);
int dots_op_decode_attn_kv8(DotsEngine* e, const void* q_dev, const void* pool_layer_dev, const int32_t* ctx_len_dev,
                            const int32_t* block_table_dev, int max_pages, void* out_dev, int B, int Hq, int Hkv, int max_seq_len,
                            const float* kv_scales_dev);
/* dots_op_decode_attn (kv_scales_dev_or_null == NULL) or dots_op_decode_attn_kv8 under the shared-prefix plan of the given
 * block table, every row active and static_pages[b] = ctx_len[b] / 64: the plan's items through the shared kernel, every other (row, split)
 * through the per-split kernel.  The partial buffers are filled with NaN first, so a (row, split) neither kernel wrote shows in out.
 * *covered_pairs_out = the (row, split) pairs the items cover (0: the call launched exactly what dots_op_decode_attn launches).  out equals
 * dots_op_decode_attn's in every bit. */
int dots_op_decode_attn_shared(DotsEngine* e, const void* q_dev, const void* pool_layer_dev, const int32_t* ctx_len_dev,
                               const int32_t* block_table_dev, int max_pages, void* out_dev, int B, int Hq, int Hkv, int max_seq_len,
                               const float* kv_scales_dev_or_null, int32_t* covered_pairs_out);
/* Host-only (no device, no engine): the shared-prefix plan (csrc/share_plan.h) of a step over rows <= 64 rows.  active / static_pages
 * int32 [rows], block_table int32 [rows, max_pages] (entries [0, static_pages[b]) of row b are read; 0 <= static_pages[b] <= max_pages).
 * Split s is pages [waves * s, waves * (s + 1)); row b is eligible for it iff it is active and waves * (s + 1) <= static_pages[b]; the
 * eligible rows of a split that name the same pages there, two or more, are one item.  items3 int32 [3 * 32 * n_splits] gets {split, first
 * member, members} per item (split by split, by lowest member within a split), members int32 [rows * n_splits] the member rows (ascending
 * within an item), masks uint64 [rows] bit s of row b = an item covers (b, s).  Empty when n_splits * waves < max_pages, n_splits > 64 or
 * waves > 8.  Returns the number of items, or a negative DOTS_E_*. */
int dots_plan_shared_prefix(const int32_t* active, const int32_t* block_table, int max_pages, const int32_t* static_pages, int rows,
                            int n_splits, int waves, int32_t* items3, int32_t* members, uint64_t* masks);
int dots_op_dec_proj(DotsEngine* e, const void* x_dev, const void* w_dev, void* h_inout_dev, int B, int N, int K, int fp8);
int dots_op_dec_gateup(DotsEngine* e, const void* h_dev, const void* ln_w_dev, const void* gate_w_dev, const void* up_w_dev, void* act_out_dev,
                       int B, int H, int I, float eps, int fp8);
int dots_op_dec_lmhead(DotsEngine* e, const void* h_dev, const void* ln_w_dev, const void* w_dev, void* logits_out_dev, int B, int H, int V,
                       float eps, int fp8);
/* The per-row selection stage on caller logits: logits_dev fp32 [B, V] (row stride V), params_host [B].  Row b's history hist_dev int32
 * [B, hist_stride] holds its prompt (n_prompt_dev[b] ids) followed by its generated tokens, hist_lens_dev[b] ids in all; the stage builds
 * the penalty state the decode loop keeps from it, draws with n = hist_lens - n_prompt, and writes the chosen ids to out_tokens_dev [B]. */
int dots_op_select_tokens(DotsEngine* e, const float* logits_dev, int B, int V, const DotsSamplingParams* params_host, const int32_t* hist_dev,
                          const int32_t* hist_lens_dev, int hist_stride, const int32_t* n_prompt_dev, int32_t* out_tokens_dev);
/* Timing of the selection stage on the same inputs (tools/sampling_bench.py): mode 0 = the arg max pair, 1 = the engine-wide sampler
 * (params_host[0].temperature / top_p / seed for every row), 2 = the per-row stage; iters replays between HIP events after a warm-up,
 * every row marked finished so that nothing is appended.  *ms_out = mean milliseconds per replay. */
int dots_bench_select_tokens(DotsEngine* e, const float* logits_dev, int B, int V, const DotsSamplingParams* params_host, const int32_t* hist_dev,
                             const int32_t* hist_lens_dev, int hist_stride, const int32_t* n_prompt_dev, int mode, int iters, float* ms_out);
/* dots_op_select_tokens with logit rules: rules_host [B] (an entry with no bias, allowed list, min_tokens, stop id and ignore_eos = a row
 * without rules), the engine's EOS ids live, and n_gen_host [B] = each row's generated count n in [0, hist_stride] (NULL: hist_lens -
 * n_prompt): it seeds the draw and is compared with min_tokens.  dots_bench_select_tokens_rules times the stage on the same inputs. */
int dots_op_select_tokens_rules(DotsEngine* e, const float* logits_dev, int B, int V, const DotsSamplingParams* params_host, const DotsLogitRules* rules_host,
                                const int32_t* n_gen_host, const int32_t* hist_dev, const int32_t* hist_lens_dev, int hist_stride,
                                const int32_t* n_prompt_dev, int32_t* out_tokens_dev);
int dots_bench_select_tokens_rules(DotsEngine* e, const float* logits_dev, int B, int V, const DotsSamplingParams* params_host, const DotsLogitRules* rules_host,
                                   const int32_t* n_gen_host, const int32_t* hist_dev, const int32_t* hist_lens_dev, int hist_stride,
                                   const int32_t* n_prompt_dev, int iters, float* ms_out);
/* dots_op_select_tokens_rules with guides: row b holds guide guide_ids_host[b] of this engine (-1: none) at state states_host[b]; V must be
 * the engine's vocabulary (the token bytes are the engine's).  states_out_host (may be NULL) receives each row's state after the commit,
 * -1 for a row without a guide.  dots_bench_select_tokens_guided times the stage, the mask kernel included, on the same inputs. */
int dots_op_select_tokens_guided(DotsEngine* e, const float* logits_dev, int B, int V, const DotsSamplingParams* params_host, const DotsLogitRules* rules_host,
                                 const int32_t* n_gen_host, const int32_t* guide_ids_host, const int32_t* states_host, const int32_t* hist_dev,
                                 const int32_t* hist_lens_dev, int hist_stride, const int32_t* n_prompt_dev, int32_t* out_tokens_dev, int32_t* states_out_host);
int dots_bench_select_tokens_guided(DotsEngine* e, const float* logits_dev, int B, int V, const DotsSamplingParams* params_host, const DotsLogitRules* rules_host,
                                    const int32_t* n_gen_host, const int32_t* guide_ids_host, const int32_t* states_host, const int32_t* hist_dev,
                                    const int32_t* hist_lens_dev, int hist_stride, const int32_t* n_prompt_dev, int iters, float* ms_out);
/* dots_op_select_tokens_rules with n-gram rules: row b carries ngram_host[b] unless its size is 0.  Its history is hist[n_prompt[b] ..
 * hist_lens[b]) — the generated part of the row — and a window may reach hist_stride.  No guides and no explicit n_gen here (min_tokens counts
 * hist_lens - n_prompt).  dots_bench_select_tokens_ngram times the stage, the ban kernel included, on the same inputs. */
int dots_op_select_tokens_ngram(DotsEngine* e, const float* logits_dev, int B, int V, const DotsSamplingParams* params_host, const DotsLogitRules* rules_host,
                                const DotsNgramRule* ngram_host, const int32_t* hist_dev, const int32_t* hist_lens_dev, int hist_stride,
                                const int32_t* n_prompt_dev, int32_t* out_tokens_dev);
int dots_bench_select_tokens_ngram(DotsEngine* e, const float* logits_dev, int B, int V, const DotsSamplingParams* params_host, const DotsLogitRules* rules_host,
                                   const DotsNgramRule* ngram_host, const int32_t* hist_dev, const int32_t* hist_lens_dev, int hist_stride,
                                   const int32_t* n_prompt_dev, int iters, float* ms_out);
/* The drafter alone on caller-supplied histories: hist int32 [B][hist_stride] holds row b's generated tokens hist[b][0 .. hist_lens[b]);
 * writes drafts int32 [B][k] and n_drafts int32 [B] by the rule above (every row drafts: no finished / selection state is read). */
/* The draft-row states and allowed bits of guided slots alone (launch_spec_guide_chain + launch_guide_mask_drafts), at the
 * engine's vocabulary, token bytes and EOS ids: slot b < rows holds guide guide_ids_host[b] (-1: none) at states_host[b], drafts
 * drafts_host[b][0 .. k) and n_live_host[b] live draft rows.  states_out_host int32 [rows * (k + 1)] and mask_out_host uint32
 * [rows * (k + 1)][2 * ceil(vocab / 64)], both indexed by step row r = j * rows + b: the state draft row (b, j) is selected under (-1: dead,
 * idle or unguided; every entry r < rows is -1) and its allowed bits (all clear where the state is -1). */
int dots_op_spec_guide_masks(DotsEngine* e, int rows, int k, const int32_t* guide_ids_host, const int32_t* states_host, const int32_t* drafts_host,
                             const int32_t* n_live_host, int32_t* states_out_host, uint32_t* mask_out_host);
int dots_op_ngram_draft(DotsEngine* e, const int32_t* hist_dev, const int32_t* hist_lens_dev, int hist_stride, int B, int k, int min_n, int max_n,
                        int32_t* drafts_dev, int32_t* n_drafts_dev);
/* The prediction drafter alone (predict_draft_kernel, the rule at dots_set_row_prediction) on caller-supplied device arrays: pred int32
 * [B][pred_stride] with pred_lens [B], hist int32 [B][hist_stride] with hist_lens [B], and the alignments cur / at int32 [B], read and —
 * for a row the rule finds a position for — written (0 <= cur, at < 2^30).  Such a row gets drafts [B][k], n_drafts [B] and src = 1;
 * every other row keeps drafts, n_drafts, cur and at as the caller set them and gets src = 0.  Every row drafts: no finished /
 * selection state is read. */
int dots_op_predict_draft(DotsEngine* e, const int32_t* pred_dev, const int32_t* pred_lens_dev, int pred_stride, const int32_t* hist_dev,
                          const int32_t* hist_lens_dev, int hist_stride, int B, int k, int min_n, int max_n, int32_t* cur_dev, int32_t* at_dev,
                          int32_t* drafts_dev, int32_t* n_drafts_dev, int32_t* src_dev);
/* The log-probability stage over caller logits: logits_dev fp32 [B, ld] (V <= ld), top_n_host [B] (-1 = row skipped, 0..20),
 * chosen_dev int32 [B] the chosen ids; writes tok_lp_dev float [B], top_ids_dev int32 [B][20], top_lp_dev float [B][20] of every row
 * with top_n >= 0 (entries beyond top_n: -1 / NaN).  The same two kernels the engine runs. */
int dots_op_logprobs(DotsEngine* e, const float* logits_dev, int B, int V, int ld, const int32_t* top_n_host,
                     const int32_t* chosen_dev, float* tok_lp_dev, int32_t* top_ids_dev, float* top_lp_dev);
/* Timing of that stage on the same inputs (tools/logprobs_bench.py): which 0 = both kernels, 1 = the partial kernel, 2 = the final
 * kernel; iters replays between HIP events after a warm-up.  *ms_out = mean milliseconds per replay. */
int dots_bench_logprobs(DotsEngine* e, const float* logits_dev, int B, int V, int ld, const int32_t* top_n_host, int which, int iters,
                        float* ms_out);

/* MFMA fragment-layout / LDS-DMA probe (csrc/probe_mfma.hip; tests/test_mfma_layout.py). */
int dots_probe_mfma(int which, const void* A, const void* Bt, void* D, void* stream);
/* Device-wide barrier probe inside one persistent kernel (csrc/probe_sync.hip): n_barriers bounded-spin barriers over
 * n_wg workgroups, each followed by cross-workgroup reads of freshly published data.  mode: 0 no fences, 1 agent-scope
 * fences, 2 nontemporal accesses, 3 agent-scope atomic accesses.  *ms_out = kernel time, stats_out[0] = stale reads,
 * stats_out[1] = barrier timeouts (the spin is bounded, the probe cannot hang). */
int dots_probe_grid_barrier(int n_wg, int threads, int n_barriers, int mode, int lds_bytes, float* ms_out, int32_t* stats_out);
/* CU-mask probe: runs n_wg workgroups on a stream created with hipExtStreamCreateWithCUMask(mask) (NULL: all CUs) and
 * returns each workgroup's raw HW_ID / XCC_ID registers, uint32 [n_wg][2]. */
int dots_probe_cu_mask(const uint32_t* mask, int words, int n_wg, int threads, int lds_bytes, uint32_t* ids_out_host);

#ifdef __cplusplus
}
#endif
#endif /* DOTS_OCR_HIP_H */
