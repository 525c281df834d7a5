// Which rows the per-row selection stage owns, and why.  Host only: no HIP, no engine type, nothing but DOTS_MAX_BATCH
// (kernels.h; a stand-alone program defines it itself — tests/row_stage_model.cpp checks this record against a brute-force model).
//
// A row is selected by the per-row stage exactly while it carries at least one feature; its device `own` flag is 1 for as long.  This
// record is the only holder of that fact: the engine asks it, and acts on the entered / left transitions that attach / detach report.
#pragma once

#ifndef DOTS_MAX_BATCH
#error "row_stage.h needs DOTS_MAX_BATCH"
#endif

// ROW_FEATURES counts the features some speculation mode can let through (SpecRows below): what the stand-alone models of `speculates`
// enumerate.  ROW_LOOP (the loop guard) lies behind them — no mode opens it — and ROW_ALL_FEATURES counts every feature a row
// can be staged for: what the record's arrays and the engine's "every feature of the row" loops run over.
enum RowFeature { ROW_PARAMS, ROW_RULES, ROW_GUIDE, ROW_NGRAM, ROW_STOP, ROW_FEATURES, ROW_LOOP = ROW_FEATURES, ROW_ALL_FEATURES };
static_assert(ROW_ALL_FEATURES <= 8, "RowStage keeps a row's features in one byte");
// which staged rows may verify drafts: SAMPLED and STOP are the values of DOTS_SPEC_ROWS_* (dots_set_speculation_rows, whose
// every bit is SPEC_ROWS_ALL); the others are internal: the engine ORs SPEC_ROWS_GUIDED in from dots_set_speculation_guided, and NGRAM /
// RULES / PENALTY — the DOTS_SPEC_SHAPED_* bits moved up by three — from dots_set_speculation_shaped
enum SpecRows {
    SPEC_ROWS_SAMPLED = 1, SPEC_ROWS_STOP = 2, SPEC_ROWS_ALL = 3, SPEC_ROWS_GUIDED = 4,
    SPEC_ROWS_NGRAM = 8, SPEC_ROWS_RULES = 16, SPEC_ROWS_PENALTY = 32
};

struct RowStage {
    bool has(int row, RowFeature f) const { return (bits[row] >> f) & 1u; }
    bool staged(int row) const { return bits[row] != 0; }          // carries any feature
    int rows(RowFeature f) const { return n_rows[f]; }             // rows that carry f
    int staged_rows() const { return n_staged; }                   // rows that carry any feature: > 0 = the per-row stage runs
    // true: the row has just entered the stage.  A feature the row already holds changes nothing
    bool attach(int row, RowFeature f) {
        if (has(row, f)) return false;
        const bool entered = !staged(row);
        bits[row] |= 1u << f;
        n_rows[f] += 1;
        n_staged += entered;
        return entered;
    }
    // true: the row has just left the stage.  A feature the row does not hold changes nothing
    bool detach(int row, RowFeature f) {
        if (!has(row, f)) return false;
        bits[row] &= ~(1u << f);
        n_rows[f] -= 1;
        const bool left = !staged(row);
        n_staged -= left;
        return left;
    }
    // May the row verify drafts?  A row without features does (plain greedy).  A staged row does iff every feature it
    // carries is one the mode lets through — own parameters under SPEC_ROWS_SAMPLED, stop strings under SPEC_ROWS_STOP, a guide under
    // SPEC_ROWS_GUIDED, an n-gram rule under SPEC_ROWS_NGRAM, logit rules under SPEC_ROWS_RULES — and its parameters, if it has any, carry
    // no penalty or the mode has SPEC_ROWS_PENALTY (has_pen: the caller's fact about them; ignored for a row without ROW_PARAMS).  None
    // of these depends on a rejected token: draft row j is selected under the hypothesis that drafts 1 .. j were committed, and under it
    // the guide's state, the history an n-gram rule reads, the output counts and the output index are known at the head of the step;
    // rejected rows leave nothing behind.  The bits are opt-ins because each adds launches to a step, not because a row could go wrong.
    // Logprobs and the engine-wide temperature are not stage features: the caller adds them.
    // A loop rule (ROW_LOOP) is let through by no bit: its check is workgroup-wide behind every commit, and the accept walk
    // commits several tokens on one lane.  Such a row runs unspeculated beside speculating neighbours.
    bool speculates(int row, bool has_pen, int mode) const {
        const unsigned open = ((mode & SPEC_ROWS_SAMPLED) ? 1u << ROW_PARAMS : 0u) | ((mode & SPEC_ROWS_STOP) ? 1u << ROW_STOP : 0u) |
                              ((mode & SPEC_ROWS_GUIDED) ? 1u << ROW_GUIDE : 0u) | ((mode & SPEC_ROWS_NGRAM) ? 1u << ROW_NGRAM : 0u) |
                              ((mode & SPEC_ROWS_RULES) ? 1u << ROW_RULES : 0u);
        if (bits[row] & ~open) return false;
        return !(has(row, ROW_PARAMS) && has_pen && !(mode & SPEC_ROWS_PENALTY));
    }
    void reset() { *this = RowStage{}; }

private:
    unsigned char bits[DOTS_MAX_BATCH] = {0};
    int n_rows[ROW_ALL_FEATURES] = {0};
    int n_staged = 0;
};
