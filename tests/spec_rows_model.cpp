// RowStage::speculates (csrc/row_stage.h) against the rule of DESIGN §6.6 stated by brute force, over every subset of the row features x
// {the row's parameters carry a penalty, they do not} x every value of the mode bits, on a row of its own and beside a neighbour that
// carries everything.  Stand-alone: no HIP, no engine.  The test compiles it with -fsanitize=address,undefined and runs it.
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#include "row_stage.h"

// The rule, in words: a row without features is plain greedy and speculates.  A row with features speculates iff the mode is on for every
// feature it carries — SAMPLED for parameters, STOP for stop strings; rules, a guide and an n-gram rule have no mode — and it does not
// hold parameters with a penalty.
static bool model(unsigned features, bool has_pen, int mode) {
    if (features == 0) return true;
    for (int f = 0; f < ROW_FEATURES; ++f) {
        if (!((features >> f) & 1u)) continue;
        if (f == ROW_PARAMS) {
            if (!(mode & SPEC_ROWS_SAMPLED) || has_pen) return false;
        } else if (f == ROW_STOP) {
            if (!(mode & SPEC_ROWS_STOP)) return false;
        } else {
            return false;
        }
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
                    for (int mode = 0; mode <= SPEC_ROWS_ALL; ++mode) {
                        const bool got = st.speculates(row, pen != 0, mode), want = model(features, pen != 0, mode);
                        if (got != want) {
                            std::printf("row %d features 0x%x pen %d mode %d: speculates() = %d, the rule says %d\n", row, features, pen, mode, got, want);
                            return 1;
                        }
                        ++cases;
                    }
                // mode 0 is the rule the engine had: exactly the rows outside the stage
                if (st.speculates(row, false, 0) != !st.staged(row) || st.speculates(row, true, 0) != !st.staged(row)) {
                    std::printf("row %d features 0x%x: mode 0 is not 'not staged'\n", row, features);
                    return 1;
                }
                // taking the features off again gives the plain row back under every mode
                for (int f = 0; f < ROW_FEATURES; ++f) st.detach(row, (RowFeature)f);
                for (int mode = 0; mode <= SPEC_ROWS_ALL; ++mode)
                    if (!st.speculates(row, true, mode)) {
                        std::printf("row %d: a row whose features are gone does not speculate under mode %d\n", row, mode);
                        return 1;
                    }
            }
    std::printf("%ld cases\n", cases);
    return 0;
}
