// The plan of shared-prefix decode attention, in plain C++ so that a host program can hold it to a restatement
// (tests/test_shared_prefix_cpu.py through dots_plan_shared_prefix): which (rows, KV split) pairs of a decode step name the same four
// physical pages, so that one workgroup can load those pages once for all of their rows.
//
// A split s of a row is pages [waves * s, waves * (s + 1)) of its block-table row.  Row b is ELIGIBLE for split s iff it is active and
// waves * (s + 1) <= static_pages[b]: the leading pages that are full and that no step will write (the engine gives prompt / 64).  Per
// split the eligible rows are partitioned by their tuple of page ids; every class of two or more rows is one ITEM (split, member rows
// ascending), and mask[b] has bit s set iff some item covers (b, s).  So a row is in at most one item per split, and classes are formed
// per split: three rows of a prefix-cache tree that agree on 2 splits, two of them on 1 more, give 2 items of three and 1 item of two.
//
// The plan is empty when n_splits * waves < max_pages — a wave of the per-row kernel then walks more than one page, and a split's partial
// is no longer a function of four pages alone — and when waves or n_splits fall outside what an item and a 64-bit mask describe.
#pragma once
#include <cstdint>

// device image of a plan (int32 words): [0] = live items, then the items {split, first member, members}, the member rows, the rows' masks
constexpr int SHARE_MAX_ROWS = 64, SHARE_MAX_SPLITS = 64;
constexpr int SHARE_MAX_ITEMS = SHARE_MAX_SPLITS * (SHARE_MAX_ROWS / 2), SHARE_MAX_MEMBERS = SHARE_MAX_SPLITS * SHARE_MAX_ROWS;
constexpr int SHARE_ITEMS_OFF = 4, SHARE_MEMBERS_OFF = SHARE_ITEMS_OFF + 3 * SHARE_MAX_ITEMS, SHARE_MASK_OFF = SHARE_MEMBERS_OFF + SHARE_MAX_MEMBERS;
constexpr int SHARE_PLAN_WORDS = SHARE_MASK_OFF + 2 * SHARE_MAX_ROWS;
constexpr int SHARE_ITEM_QUANTUM = 64;      // a captured step's grid holds the item count rounded up to this (DotsEngine::StepKey::share)
static_assert(SHARE_MASK_OFF % 2 == 0, "the masks are 64-bit words");

struct SharePlanCounts { int items, rows, pairs, saved; };      // saved: sum over the items of (members - 1)

// active / static_pages [rows], table [rows][stride] (entries [0, static_pages[b]) of row b are read), items [3 * SHARE_MAX_ITEMS],
// members [SHARE_MAX_MEMBERS], mask [rows].  Items come split by split, within a split by their lowest member
inline SharePlanCounts share_plan(const int32_t* active, const int32_t* table, int stride, const int32_t* static_pages, int rows, int n_splits, int waves,
                                  int max_pages, int32_t* items, int32_t* members, uint64_t* mask) {
    SharePlanCounts c{0, 0, 0, 0};
    for (int b = 0; b < rows; ++b) mask[b] = 0;
    if (rows < 2 || rows > SHARE_MAX_ROWS || n_splits < 1 || n_splits > SHARE_MAX_SPLITS || waves < 1 || waves > 8) return c;
    if ((int64_t)n_splits * waves < max_pages) return c;
    int n_members = 0;
    for (int s = 0; s < n_splits; ++s) {
        bool taken[SHARE_MAX_ROWS] = {false};
        for (int a = 0; a < rows; ++a) {
            if (taken[a] || !active[a] || waves * (s + 1) > static_pages[a] || waves * (s + 1) > stride) continue;
            const int32_t* pa = table + (int64_t)a * stride + waves * s;
            const int first = n_members;
            members[n_members++] = a;
            for (int b = a + 1; b < rows; ++b) {
                if (taken[b] || !active[b] || waves * (s + 1) > static_pages[b]) continue;
                const int32_t* pb = table + (int64_t)b * stride + waves * s;
                bool same = true;
                for (int w = 0; w < waves; ++w) same = same && pa[w] == pb[w];
                if (!same) continue;
                taken[b] = true;
                members[n_members++] = b;
            }
            const int n = n_members - first;
            if (n < 2) { n_members = first; continue; }
            items[3 * c.items] = s; items[3 * c.items + 1] = first; items[3 * c.items + 2] = n;
            c.items += 1;
            c.pairs += n;
            c.saved += n - 1;
            for (int i = first; i < n_members; ++i) mask[members[i]] |= (uint64_t)1 << s;
        }
    }
    for (int b = 0; b < rows; ++b) c.rows += mask[b] != 0;
    return c;
}
