// Every DOTS_OCR_* environment switch the library reads: its name, its parse rule and when it is read.  Host-only C++17, no HIP
// include (tests/switches_model.cpp compiles it alone).  None of these is on the product path: A/B switches of kept and rejected
// kernels, experiments, test hooks.  Unless noted a switch changes no result bit.
//
// Read times:
//   once per process  every field of LaunchSwitches, parsed at the first launch_switches() call
//   per engine        CU_RANGE, DECODE_PLAN, TOWER_TAIL_LAYERS at dots_create; OVERLAP_DEC_CUS at the engine's first ensure_overlap_streams
//                     (bench.py sets it between engines)
//   on every call     DEC_WIDE_CUS, DEC_KSPLIT, PAGED_ATTN_HEADS (the tests flip them inside one process) and NO_GRAPH in dots_generate
//                     (dots_step_chunk takes the per-process LaunchSwitches::no_graph)
// The per-engine and per-call readers are spelled sw::read_now(name) at the place that reads, so the read time shows where it happens.
#pragma once
#include <algorithm>
#include <cstdio>
#include <cstdlib>

namespace sw {

// ---- names: what each selects, and where the measurement that kept or rejected it is recorded
// decode launch plan (decode_fused.hip, decode_b64.hip)
constexpr const char* DEC_WIDE = "DOTS_OCR_DEC_WIDE";                    // =0: per-tile qkv / projection kernels above 16 rows instead of the wide ones (profiles/r05_decode_wide_ab.txt)
constexpr const char* DEC_WIDE_CUS = "DOTS_OCR_DEC_WIDE_CUS";            // =n: CUs the wide / K-split / streaming kernels size their round for (tests walk every workgroup shape)
constexpr const char* QKV_XIMG = "DOTS_OCR_QKV_XIMG";                    // =0: above 32 rows qkv normalises its own rows instead of reading the X image (tools/gpu_r6b.sh)
constexpr const char* PROJ_REG = "DOTS_OCR_PROJ_REG";                    // set: the register-round projection kernel for long K too, not the LDS-image one (profiles/r03_overlap_probe.txt)
constexpr const char* GATEUP_WG_CAP = "DOTS_OCR_GATEUP_WG_CAP";          // =n: gate|up grid capped at n workgroups, forcing the walking path (tests, A/B runs)
constexpr const char* GATEUP_PAIRS = "DOTS_OCR_GATEUP_PAIRS";            // =1|2: weight-tile pairs per gate|up workgroup (default by batch: timings at gateup_launch; profiles/r03_overlap_probe.txt)
constexpr const char* GATEUP_PER_TILE = "DOTS_OCR_GATEUP_PER_TILE";      // set: one gate|up workgroup set per 16-row tile at every batch size (profiles/r04_bench_a4_one_tile_kernels.json)
constexpr const char* LMHEAD_PER_TILE = "DOTS_OCR_LMHEAD_PER_TILE";      // set: the same for the lm_head (same file)
constexpr const char* TWO_TILE_FP8 = "DOTS_OCR_TWO_TILE_FP8";            // =0: e4m3 batches above 16 rows back on the per-tile kernels (profiles/HISTORY.md, round 5)
constexpr const char* DEC_S64 = "DOTS_OCR_DEC_S64";                      // =0: above 32 rows the two-tile gate|up / lm_head kernels instead of dec_stream64_kernel (profiles/r06_decode_b64_first_ab.txt)
constexpr const char* S64_WAVES = "DOTS_OCR_S64_WAVES";                  // =4|8|12: waves per dec_stream64_kernel workgroup (default by items per workgroup; same file)
constexpr const char* DEC_KSPLIT = "DOTS_OCR_DEC_KSPLIT";                // =0|1|2: K-quarter projections above 32 rows: off / down_proj (default) / o_proj too (profiles/r06_decode_ksplit_ab.txt)
// decode attention (decode.hip)
constexpr const char* ATTN_WAVES = "DOTS_OCR_ATTN_WAVES";                // =1|2|4|8: pages in flight per workgroup = the KV split; CHANGES the summation order (profiles/r06_decode_attn_waves_ab.txt)
constexpr const char* ATTN_STREAM = "DOTS_OCR_ATTN_STREAM";              // =1: the streaming kernel wherever legal, =0 never (slower everywhere: profiles/r05_decode_attn_stream_ab.txt)
constexpr const char* ATTN_STREAM_MIN = "DOTS_OCR_ATTN_STREAM_MIN";      // =n: the streaming kernel from n work items per CU (same file)
// GEMM (gemm.hip)
constexpr const char* GEMM_PLAN = "DOTS_OCR_GEMM_PLAN";                  // =0: 8-wave ping-pong kernel, else one wave per SIMD (profiles/r05_bench_a4_gemm_plan{0,1}.json); dots_set_gemm_plan overrides
constexpr const char* GEMM_LOCKSTEP = "DOTS_OCR_GEMM_LOCKSTEP";          // set: the one-barrier-per-K-tile schedule of round 1
constexpr const char* GEMM_128 = "DOTS_OCR_GEMM_128";                    // set: the 128-wide kernel for every shape (profiles/r01_xcdflash_bench_a4.json is the 256-wide one's line)
constexpr const char* QK_FUSE = "DOTS_OCR_QK_FUSE";                      // =0: qkv GEMM then qkv_rope_split_kernel instead of the rope epilogue (profiles/r06_qk_rope_fusion_ab.txt)
// prefill attention (attn_prefill.hip, attn_paged.hip)
constexpr const char* ATTN_MODE = "DOTS_OCR_ATTN_MODE";                  // =0|1|2: round-1 schedule / 8-wave ping-pong / 64-row DMA-ring kernel (default) (profiles/r04_flash_ab.txt)
constexpr const char* PREFILL_F64 = "DOTS_OCR_PREFILL_F64";              // =0: causal prefill on the 8-wave kernel of rounds 1-3 (tools/gpu_r6d.sh)
constexpr const char* ATTN_ROWS128 = "DOTS_OCR_ATTN_ROWS128";            // set: 128 query rows per work item, not 256 (+2-3 % for 256 in interleaved A/B, attn_prefill.hip)
constexpr const char* PAGED_ATTN_HEADS = "DOTS_OCR_PAGED_ATTN_HEADS";    // =1: one query head per wave in the paged prefill kernel (lost everywhere: profiles/chunked_prefill.txt)
// engine (engine.hip, weights.hip, slots.hip)
constexpr const char* OVERLAP_DEC_CUS = "DOTS_OCR_OVERLAP_DEC_CUS";      // =n: CUs of the decode partition beside the look-ahead tower (profiles/r06_a4_partition_sweep.txt)
constexpr const char* OVERLAP_BY_XCD = "DOTS_OCR_OVERLAP_BY_XCD";        // set: the partitions are whole XCDs (no gain: DESIGN §6)
constexpr const char* CU_RANGE = "DOTS_OCR_CU_RANGE";                    // =lo-hi: the engine's main stream on CU-mask bits lo..hi (profiles/r06_tower_kernels_vs_cus_power_cap.txt)
constexpr const char* DECODE_PLAN = "DOTS_OCR_DECODE_PLAN";              // =0..5: the default of dots_set_decode_plan (bit 0 partition plan, +2 streaming / +4 per-split attention)
constexpr const char* TOWER_TAIL_LAYERS = "DOTS_OCR_TOWER_TAIL_LAYERS";  // =n: the initial `set` of dots_tower_tail (profiles/r05_tower_tail_ab.txt)
constexpr const char* DEBUG_SAME_LAYER = "DOTS_OCR_DEBUG_SAME_LAYER";    // set: every decode layer reads layer 0's weights; WRONG results, an Infinity-Cache experiment
constexpr const char* NO_GRAPH = "DOTS_OCR_NO_GRAPH";                    // set: decode steps are launched directly, not replayed from a captured graph (profiler runs: profiles/stop_strings.txt)

// ---- parse rules: pure functions of the variable's text, nullptr = unset.  They differ on purpose: each is its switch's rule as first written.
inline bool on_unless_zero(const char* t) { return !(t && atoi(t) == 0); }       // "" and text count as 0: off
inline bool on_if_set(const char* t) { return t != nullptr; }                    // to anything, "0" and "" included
inline int int_or_auto(const char* t) { return t ? atoi(t) : 0; }                // 0 = automatic
inline int parse_attn_waves(const char* t) { const int v = t ? atoi(t) : 4; return (v == 1 || v == 2 || v == 8) ? v : 4; }
inline int parse_attn_stream(const char* t) { return t ? (atoi(t) != 0 ? 1 : 0) : -1; }
inline int parse_attn_stream_min(const char* t) { return t ? std::max(1, atoi(t)) : 0; }
inline int parse_attn_mode(const char* t) { return t ? atoi(t) : 2; }
inline int parse_gemm_plan(const char* t) { return t ? (atoi(t) != 0) : 1; }
inline int parse_dec_wide_cus(const char* t) { return t ? std::max(0, atoi(t)) : 0; }           // 0 = no override
inline int parse_dec_ksplit(const char* t) { return t ? atoi(t) : 1; }                          // <= 0 off, 1 long K only, >= 2 o_proj too
inline bool parse_paged_attn_one_head(const char* t) { return t && atoi(t) == 1; }
inline int parse_overlap_dec_cus(const char* t) { return std::max(32, std::min(224, atoi(t) / 8 * 8)); }       // t is set
inline int parse_tower_tail_layers(const char* t, int v_layers) { return std::max(-1, std::min(atoi(t), v_layers)); }      // t is set
inline bool parse_cu_range(const char* t, int* lo, int* hi) { return sscanf(t, "%d-%d", lo, hi) == 2 && *lo >= 0 && *hi <= 255 && *lo <= *hi; }      // t is set
// the same rule as dots_set_decode_plan: a bit field since round 5 — it used to be "any non-zero = partition plan", so an old setting of 2 or 3 now means
// the (slower) streaming attention kernel: values outside 0..5, and 6 / 7 (both attention bits), are refused instead of silently re-interpreted
struct DecodePlan { bool ok; int force_part, attn_stream; };
inline DecodePlan parse_decode_plan(const char* t) {      // t is set
    const int plan = atoi(t);
    if (plan < 0 || plan > 5 || (plan & 6) == 6) return {false, 0, -1};
    return {true, plan & 1, (plan & 2) ? 1 : (plan & 4) ? 0 : -1};
}

// KV splits of decode attention for a context capacity: ceil(pages / waves), at most 64 (an engine constant, never a function of the batch)
inline int attn_splits(int max_seq_len, int page, int waves) {
    const int pages = (max_seq_len + page - 1) / page;
    return std::max(1, std::min((pages + waves - 1) / waves, 64));
}

// ---- the per-process record
struct LaunchSwitches {
    bool dec_wide, qkv_ximg, two_tile_fp8, dec_s64, qk_fuse, prefill_f64;                                 // on_unless_zero
    bool proj_reg, gateup_per_tile, lmhead_per_tile, gemm_lockstep, gemm_128, attn_rows128, overlap_by_xcd, debug_same_layer, no_graph;      // on_if_set
    int gateup_wg_cap, gateup_pairs, s64_waves;                                                           // int_or_auto
    int attn_waves, attn_stream, attn_stream_min, attn_mode, gemm_plan;
};

// get(name) -> the variable's text or nullptr
template <class Get>
LaunchSwitches parse_launch_switches(Get get) {
    LaunchSwitches s;
    s.dec_wide = on_unless_zero(get(DEC_WIDE));
    s.qkv_ximg = on_unless_zero(get(QKV_XIMG));
    s.two_tile_fp8 = on_unless_zero(get(TWO_TILE_FP8));
    s.dec_s64 = on_unless_zero(get(DEC_S64));
    s.qk_fuse = on_unless_zero(get(QK_FUSE));
    s.prefill_f64 = on_unless_zero(get(PREFILL_F64));
    s.proj_reg = on_if_set(get(PROJ_REG));
    s.gateup_per_tile = on_if_set(get(GATEUP_PER_TILE));
    s.lmhead_per_tile = on_if_set(get(LMHEAD_PER_TILE));
    s.gemm_lockstep = on_if_set(get(GEMM_LOCKSTEP));
    s.gemm_128 = on_if_set(get(GEMM_128));
    s.attn_rows128 = on_if_set(get(ATTN_ROWS128));
    s.overlap_by_xcd = on_if_set(get(OVERLAP_BY_XCD));
    s.debug_same_layer = on_if_set(get(DEBUG_SAME_LAYER));
    s.no_graph = on_if_set(get(NO_GRAPH));
    s.gateup_wg_cap = int_or_auto(get(GATEUP_WG_CAP));
    s.gateup_pairs = int_or_auto(get(GATEUP_PAIRS));
    s.s64_waves = int_or_auto(get(S64_WAVES));
    s.attn_waves = parse_attn_waves(get(ATTN_WAVES));
    s.attn_stream = parse_attn_stream(get(ATTN_STREAM));
    s.attn_stream_min = parse_attn_stream_min(get(ATTN_STREAM_MIN));
    s.attn_mode = parse_attn_mode(get(ATTN_MODE));
    s.gemm_plan = parse_gemm_plan(get(GEMM_PLAN));
    return s;
}

inline const char* read_now(const char* name) { return std::getenv(name); }

inline const LaunchSwitches& launch_switches() {
    static const LaunchSwitches s = parse_launch_switches(read_now);
    return s;
}

}  // namespace sw

using sw::LaunchSwitches;
using sw::launch_switches;
