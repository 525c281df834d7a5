// Table check of the environment switches (dots_ocr_amd/csrc/switches.h), a stand-alone host program: tests/test_switches_cpu.py compiles
// it (plainly, and with the address and undefined-behaviour sanitizers) and runs it.  It lives here and not beside the header because the
// library build compiles every .cpp under csrc/.
//
// Every switch is fed the same seven texts — unset, "", "0", "1", "2", "-3", "abc" — and the result is compared with the rule the launchers
// had when each of them read its own variable (the EXPECT rows below restate those rules value by value, not by calling the header).
// The per-process switches go through parse_launch_switches with a fake environment that gives every variable the same text, so a
// field bound to the wrong rule shows.  Then the ATTN_WAVES whitelist, the OVERLAP_DEC_CUS clamp, the DECODE_PLAN refusals, CU_RANGE and
// decode_attn_splits' arithmetic.  Exit status 0 = no difference; the last line counts the checks.
#include <cstdio>
#include <cstring>

#include "switches.h"

namespace {

int n_checks = 0, n_bad = 0;

void check(bool ok, const char* what, const char* text, long got, long want) {
    ++n_checks;
    if (ok) return;
    if (++n_bad <= 30) std::fprintf(stderr, "MISMATCH %s for %s: got %ld, expected %ld\n", what, text ? (*text ? text : "\"\"") : "unset", got, want);
}
#define EXPECT(what, got, want) check((long)(got) == (long)(want), what, text, (long)(got), (long)(want))

constexpr int N_TEXTS = 7;
const char* const TEXTS[N_TEXTS] = {nullptr, "", "0", "1", "2", "-3", "abc"};
//                                  unset  ""  "0" "1" "2" "-3" "abc"
const int ON_UNLESS_ZERO[N_TEXTS] = {1,    0,  0,  1,  1,  1,   0};       // off only when set and atoi == 0
const int ON_IF_SET[N_TEXTS] =      {0,    1,  1,  1,  1,  1,   1};
const int INT_OR_AUTO[N_TEXTS] =    {0,    0,  0,  1,  2,  -3,  0};
const int ATTN_WAVES[N_TEXTS] =     {4,    4,  4,  1,  2,  4,   4};
const int ATTN_STREAM[N_TEXTS] =    {-1,   0,  0,  1,  1,  1,   0};
const int ATTN_STREAM_MIN[N_TEXTS] = {0,   1,  1,  1,  2,  1,   1};
const int ATTN_MODE[N_TEXTS] =      {2,    0,  0,  1,  2,  -3,  0};
const int GEMM_PLAN[N_TEXTS] =      {1,    0,  0,  1,  1,  1,   0};
const int DEC_WIDE_CUS[N_TEXTS] =   {0,    0,  0,  1,  2,  0,   0};       // 0 = no override
const int DEC_KSPLIT[N_TEXTS] =     {1,    0,  0,  1,  2,  -3,  0};
const int PAGED_ONE_HEAD[N_TEXTS] = {0,    0,  0,  1,  0,  0,   0};

const char* g_text = nullptr;
const char* same_text_for_all(const char* name) { return std::strncmp(name, "DOTS_OCR_", 9) == 0 ? g_text : nullptr; }

void per_process_switches() {
    for (int i = 0; i < N_TEXTS; ++i) {
        const char* text = g_text = TEXTS[i];
        const sw::LaunchSwitches s = sw::parse_launch_switches(same_text_for_all);
        EXPECT("DEC_WIDE", s.dec_wide, ON_UNLESS_ZERO[i]);
        EXPECT("QKV_XIMG", s.qkv_ximg, ON_UNLESS_ZERO[i]);
        EXPECT("TWO_TILE_FP8", s.two_tile_fp8, ON_UNLESS_ZERO[i]);
        EXPECT("DEC_S64", s.dec_s64, ON_UNLESS_ZERO[i]);
        EXPECT("QK_FUSE", s.qk_fuse, ON_UNLESS_ZERO[i]);
        EXPECT("PREFILL_F64", s.prefill_f64, ON_UNLESS_ZERO[i]);
        EXPECT("PROJ_REG", s.proj_reg, ON_IF_SET[i]);
        EXPECT("GATEUP_PER_TILE", s.gateup_per_tile, ON_IF_SET[i]);
        EXPECT("LMHEAD_PER_TILE", s.lmhead_per_tile, ON_IF_SET[i]);
        EXPECT("GEMM_LOCKSTEP", s.gemm_lockstep, ON_IF_SET[i]);
        EXPECT("GEMM_128", s.gemm_128, ON_IF_SET[i]);
        EXPECT("ATTN_ROWS128", s.attn_rows128, ON_IF_SET[i]);
        EXPECT("OVERLAP_BY_XCD", s.overlap_by_xcd, ON_IF_SET[i]);
        EXPECT("DEBUG_SAME_LAYER", s.debug_same_layer, ON_IF_SET[i]);
        EXPECT("NO_GRAPH", s.no_graph, ON_IF_SET[i]);
        EXPECT("GATEUP_WG_CAP", s.gateup_wg_cap, INT_OR_AUTO[i]);
        EXPECT("GATEUP_PAIRS", s.gateup_pairs, INT_OR_AUTO[i]);
        EXPECT("S64_WAVES", s.s64_waves, INT_OR_AUTO[i]);
        EXPECT("ATTN_WAVES", s.attn_waves, ATTN_WAVES[i]);
        EXPECT("ATTN_STREAM", s.attn_stream, ATTN_STREAM[i]);
        EXPECT("ATTN_STREAM_MIN", s.attn_stream_min, ATTN_STREAM_MIN[i]);
        EXPECT("ATTN_MODE", s.attn_mode, ATTN_MODE[i]);
        EXPECT("GEMM_PLAN", s.gemm_plan, GEMM_PLAN[i]);
    }
    // one variable set, every other unset: a field reads its own name and no other
    static const char* one_name = nullptr;
    auto only = [](const char* name) -> const char* { return std::strcmp(name, one_name) == 0 ? "0" : nullptr; };
    const char* text = "0";
    one_name = sw::DEC_WIDE;
    sw::LaunchSwitches s = sw::parse_launch_switches(only);
    EXPECT("DEC_WIDE alone", s.dec_wide, 0);
    EXPECT("QKV_XIMG beside DEC_WIDE", s.qkv_ximg, 1);
    EXPECT("NO_GRAPH beside DEC_WIDE", s.no_graph, 0);
    one_name = sw::GEMM_128;
    s = sw::parse_launch_switches(only);
    EXPECT("GEMM_128 alone", s.gemm_128, 1);
    EXPECT("GEMM_LOCKSTEP beside GEMM_128", s.gemm_lockstep, 0);
    EXPECT("GEMM_PLAN beside GEMM_128", s.gemm_plan, 1);
}

void per_call_and_per_engine_switches() {
    for (int i = 0; i < N_TEXTS; ++i) {
        const char* text = TEXTS[i];
        EXPECT("NO_GRAPH per call", sw::on_if_set(text), ON_IF_SET[i]);
        EXPECT("DEC_WIDE_CUS", sw::parse_dec_wide_cus(text), DEC_WIDE_CUS[i]);
        EXPECT("DEC_KSPLIT", sw::parse_dec_ksplit(text), DEC_KSPLIT[i]);
        EXPECT("PAGED_ATTN_HEADS", sw::parse_paged_attn_one_head(text), PAGED_ONE_HEAD[i]);
        if (!text) continue;                                          // the per-engine rules below are applied to a set variable only
        //                                      ""  "0" "1" "2" "-3" "abc"
        static const int DEC_CUS[N_TEXTS] = {0, 32, 32, 32, 32, 32, 32};
        static const int TAIL_OF_42[N_TEXTS] = {0, 0, 0, 1, 2, -1, 0};
        static const int PLAN_OK[N_TEXTS] = {0, 1, 1, 1, 1, 0, 1};
        static const int PLAN_PART[N_TEXTS] = {0, 0, 0, 1, 0, 0, 0};
        static const int PLAN_STREAM[N_TEXTS] = {0, -1, -1, -1, 1, -1, -1};
        EXPECT("OVERLAP_DEC_CUS", sw::parse_overlap_dec_cus(text), DEC_CUS[i]);
        EXPECT("TOWER_TAIL_LAYERS", sw::parse_tower_tail_layers(text, 42), TAIL_OF_42[i]);
        const sw::DecodePlan p = sw::parse_decode_plan(text);
        EXPECT("DECODE_PLAN ok", p.ok, PLAN_OK[i]);
        if (p.ok) {
            EXPECT("DECODE_PLAN partition", p.force_part, PLAN_PART[i]);
            EXPECT("DECODE_PLAN attention", p.attn_stream, PLAN_STREAM[i]);
        }
        int lo = -1, hi = -1;
        EXPECT("CU_RANGE", sw::parse_cu_range(text, &lo, &hi), 0);   // none of the seven texts is a range
    }
}

void named_cases() {
    const char* text;
    // ATTN_WAVES: 1, 2 or 8; anything else gives 4
    static const struct { const char* t; int want; } waves[] = {{"1", 1}, {"2", 2}, {"8", 8}, {"4", 4}, {"3", 4}, {"16", 4}, {"0", 4}, {"-1", 4}, {"8x", 8}};
    for (const auto& c : waves) { text = c.t; EXPECT("ATTN_WAVES whitelist", sw::parse_attn_waves(text), c.want); }
    // OVERLAP_DEC_CUS: atoi / 8 * 8, clamped to [32, 224]
    static const struct { const char* t; int want; } cus[] = {{"0", 32}, {"31", 32}, {"32", 32}, {"100", 96}, {"224", 224}, {"1000", 224}, {"64", 64}, {"128", 128}, {"39", 32}, {"40", 40}};
    for (const auto& c : cus) { text = c.t; EXPECT("OVERLAP_DEC_CUS clamp", sw::parse_overlap_dec_cus(text), c.want); }
    // DECODE_PLAN: 0 .. 5 accepted (bit 0 partition plan, + 2 streaming, + 4 per-split attention); 6, 7, -1 and 8 refused
    static const struct { const char* t; int ok, part, stream; } plans[] = {{"0", 1, 0, -1}, {"1", 1, 1, -1}, {"2", 1, 0, 1}, {"3", 1, 1, 1}, {"4", 1, 0, 0}, {"5", 1, 1, 0},
                                                                            {"6", 0, 0, 0},  {"7", 0, 0, 0},  {"-1", 0, 0, 0}, {"8", 0, 0, 0}};
    for (const auto& c : plans) {
        text = c.t;
        const sw::DecodePlan p = sw::parse_decode_plan(text);
        EXPECT("DECODE_PLAN accepted", p.ok, c.ok);
        if (c.ok) { EXPECT("DECODE_PLAN partition", p.force_part, c.part); EXPECT("DECODE_PLAN attention", p.attn_stream, c.stream); }
    }
    // TOWER_TAIL_LAYERS: clamped to [-1, v_layers]
    static const struct { const char* t; int want; } tails[] = {{"-1", -1}, {"-2", -1}, {"0", 0}, {"41", 41}, {"42", 42}, {"43", 42}};
    for (const auto& c : tails) { text = c.t; EXPECT("TOWER_TAIL_LAYERS clamp", sw::parse_tower_tail_layers(text, 42), c.want); }
    // CU_RANGE: lo-hi inside 0 .. 255, lo <= hi
    static const struct { const char* t; int ok, lo, hi; } ranges[] = {{"0-255", 1, 0, 255}, {"64-255", 1, 64, 255}, {"7-7", 1, 7, 7}, {"0-256", 0, 0, 0}, {"9-3", 0, 0, 0}, {"12", 0, 0, 0}, {"-1-5", 0, 0, 0}};
    for (const auto& c : ranges) {
        text = c.t;
        int lo = 0, hi = 255;
        EXPECT("CU_RANGE accepted", sw::parse_cu_range(text, &lo, &hi), c.ok);
        if (c.ok) { EXPECT("CU_RANGE lo", lo, c.lo); EXPECT("CU_RANGE hi", hi, c.hi); }
    }
    // decode_attn_splits = ceil(pages of 64 tokens / waves), at least 1, at most 64
    static const int seq[4] = {64, 256, 8192, 32768};
    static const struct { int waves; int want[4]; } splits[] = {{1, {1, 4, 64, 64}}, {2, {1, 2, 64, 64}}, {4, {1, 1, 32, 64}}, {8, {1, 1, 16, 64}}};
    text = "splits";
    for (const auto& c : splits)
        for (int i = 0; i < 4; ++i) EXPECT("decode_attn_splits", sw::attn_splits(seq[i], 64, c.waves), c.want[i]);
    EXPECT("decode_attn_splits ragged page", sw::attn_splits(65, 64, 1), 2);
}

}  // namespace

int main() {
    per_process_switches();
    per_call_and_per_engine_switches();
    named_cases();
    std::printf("%d checks, %d mismatches\n", n_checks, n_bad);
    return n_bad ? 1 : 0;
}
