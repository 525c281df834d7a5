// RowStage::speculates (csrc/row_stage.h) with the internal bit SPEC_ROWS_GUIDED against the rule of DESIGN §6.6 stated by brute force, over
// every subset of the row features x {the row's parameters carry a penalty, they do not} x every value 0 .. 7 of the mode, on a row of its
// own and beside a neighbour that carries everything.  Stand-alone: no HIP, no engine.  The test compiles it with
// -fsanitize=address,undefined and runs it.
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#include "row_stage.h"

static_assert(SPEC_ROWS_SAMPLED == 1 && SPEC_ROWS_STOP == 2 && SPEC_ROWS_ALL == 3 && SPEC_ROWS_GUIDED == 4,
              "the public rows setting keeps its two bits and its ALL; the guide's bit is the next one");

// The rule, in words: a row without features is plain greedy and speculates.  A row with features speculates iff every feature it carries
// is let through — parameters by SAMPLED and only without a penalty, stop strings by STOP, a guide by GUIDED; rules and an n-gram rule by
// nothing.
static bool model(unsigned features, bool has_pen, int mode) {
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
                    for (int mode = 0; mode <= 7; ++mode) {
                        const bool got = st.speculates(row, pen != 0, mode), want = model(features, pen != 0, mode);
                        if (got != want) {
                            std::printf("row %d features 0x%x pen %d mode %d: speculates() = %d, the rule says %d\n", row, features, pen, mode, got, want);
                            return 1;
                        }
                        // without the guide's bit the answer is the one the modes 0 .. 3 always gave: a guided row never speculates
                        if ((features >> ROW_GUIDE) & 1u) {
                            if (st.speculates(row, pen != 0, mode & SPEC_ROWS_ALL)) {
                                std::printf("row %d features 0x%x pen %d mode %d: a guided row speculates without SPEC_ROWS_GUIDED\n", row, features, pen, mode & 3);
                                return 1;
                            }
                        } else if (st.speculates(row, pen != 0, mode & SPEC_ROWS_ALL) != got) {
                            std::printf("row %d features 0x%x pen %d mode %d: SPEC_ROWS_GUIDED changed a row without a guide\n", row, features, pen, mode);
                            return 1;
                        }
                        ++cases;
                    }
                for (int f = 0; f < ROW_FEATURES; ++f) st.detach(row, (RowFeature)f);
                for (int mode = 0; mode <= 7; ++mode)
                    if (!st.speculates(row, true, mode)) {
                        std::printf("row %d: a row whose features are gone does not speculate under mode %d\n", row, mode);
                        return 1;
                    }
            }
    std::printf("%ld cases\n", cases);
    return 0;
}
