// RowStage::speculates (csrc/row_stage.h) with the internal bits SPEC_ROWS_NGRAM / SPEC_ROWS_RULES / SPEC_ROWS_PENALTY against the rule of
// DESIGN §6.6 stated by brute force, over every subset of the row features x {the row's parameters carry a penalty, they do not} x every
// value 0 .. 63 of the mode, on a row of its own and beside a neighbour that carries everything.  Stand-alone: no HIP, no engine.  The test
// compiles it with -fsanitize=address,undefined and runs it.
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#include "row_stage.h"

static_assert(SPEC_ROWS_SAMPLED == 1 && SPEC_ROWS_STOP == 2 && SPEC_ROWS_ALL == 3 && SPEC_ROWS_GUIDED == 4,
              "the public rows setting keeps its two bits and its ALL, the guide's bit its value");
static_assert(SPEC_ROWS_NGRAM == 8 && SPEC_ROWS_RULES == 16 && SPEC_ROWS_PENALTY == 32, "DOTS_SPEC_SHAPED_* = 1, 2, 4 moved up by three bits");

// The rule, in words: a row without features is plain greedy and speculates.  A row with features speculates iff every feature it carries
// is let through — parameters by SAMPLED, and with a penalty only under PENALTY too; stop strings by STOP; a guide by GUIDED; an n-gram
// rule by NGRAM; logit rules by RULES.
static bool model(unsigned features, bool has_pen, int mode) {
    for (int f = 0; f < ROW_FEATURES; ++f) {
        if (!((features >> f) & 1u)) continue;
        bool through = false;
        switch (f) {
        case ROW_PARAMS: through = (mode & 1) && (!has_pen || (mode & 32)); break;
        case ROW_STOP: through = (mode & 2) != 0; break;
        case ROW_GUIDE: through = (mode & 4) != 0; break;
        case ROW_NGRAM: through = (mode & 8) != 0; break;
        case ROW_RULES: through = (mode & 16) != 0; break;
        default: break;
        }
        if (!through) return false;
    }
    return true;
}

// the rule as it stood before the three bits existed (tests/spec_guided_model.cpp): what every mode below 8 must still answer
static bool model_before(unsigned features, bool has_pen, int mode) {
    for (int f = 0; f < ROW_FEATURES; ++f) {
        if (!((features >> f) & 1u)) continue;
        bool through = false;
        switch (f) {
        case ROW_PARAMS: through = (mode & 1) && !has_pen; break;
        case ROW_STOP: through = (mode & 2) != 0; break;
        case ROW_GUIDE: through = (mode & 4) != 0; break;
        default: break;
        }
        if (!through) return false;
    }
    return true;
}

int main() {
    long cases = 0;
    for (int row : {0, 1, DOTS_MAX_BATCH - 1})
        for (int neighbour = 0; neighbour < 2; ++neighbour)
            for (unsigned features = 0; features < (1u << ROW_FEATURES); ++features) {
                RowStage st;
                const int other = row == 0 ? 1 : 0;
                if (neighbour)
                    for (int f = 0; f < ROW_FEATURES; ++f) st.attach(other, (RowFeature)f);
                for (int f = 0; f < ROW_FEATURES; ++f)
                    if ((features >> f) & 1u) st.attach(row, (RowFeature)f);
                for (int pen = 0; pen < 2; ++pen)
                    for (int mode = 0; mode <= 63; ++mode) {
                        const bool got = st.speculates(row, pen != 0, mode), want = model(features, pen != 0, mode);
                        if (got != want) {
                            std::printf("row %d features 0x%x pen %d mode %d: speculates() = %d, the rule says %d\n", row, features, pen, mode, got, want);
                            return 1;
                        }
                        if (mode < 8 && got != model_before(features, pen != 0, mode)) {
                            std::printf("row %d features 0x%x pen %d mode %d: a mode below 8 answers %d, it used to answer %d\n", row, features, pen, mode, got, !got);
                            return 1;
                        }
                        // a bit changes nothing for a row that does not carry its feature
                        const bool ng = (features >> ROW_NGRAM) & 1u, ru = (features >> ROW_RULES) & 1u, pe = ((features >> ROW_PARAMS) & 1u) && pen;
                        const int idle = (ng ? 0 : SPEC_ROWS_NGRAM) | (ru ? 0 : SPEC_ROWS_RULES) | (pe ? 0 : SPEC_ROWS_PENALTY);
                        if (st.speculates(row, pen != 0, mode ^ idle) != got) {
                            std::printf("row %d features 0x%x pen %d mode %d: a bit of a feature the row does not carry changed the answer\n", row, features, pen, mode);
                            return 1;
                        }
                        ++cases;
                    }
                for (int f = 0; f < ROW_FEATURES; ++f) st.detach(row, (RowFeature)f);
                for (int mode = 0; mode <= 63; ++mode)
                    if (!st.speculates(row, true, mode)) {
                        std::printf("row %d: a row whose features are gone does not speculate under mode %d\n", row, mode);
                        return 1;
                    }
            }
    std::printf("%ld cases\n", cases);
    return 0;
}
