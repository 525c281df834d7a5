// RowStage (csrc/row_stage.h) with the loop guard's feature: a row that holds ROW_LOOP verifies no draft, under every
// mode 0 .. 63 (all SpecRows bits), whatever else it holds and whether or not its parameters carry a penalty — alone, and beside a
// neighbour that holds every feature; and ROW_LOOP changes nothing for a row that does not hold it.  Stand-alone: no HIP, no engine.
#include <cstdio>

#ifndef DOTS_MAX_BATCH
#define DOTS_MAX_BATCH 64
#endif
#include "row_stage.h"

static int fails = 0;
static long cases = 0;

static void check(bool ok, const char* what, int row, unsigned set, int pen, int mode, int beside) {
    ++cases;
    if (ok) return;
    if (++fails <= 20) std::fprintf(stderr, "%s: row %d features 0x%x pen %d mode %d neighbour %d\n", what, row, set, pen, mode, beside);
}

int main() {
    static_assert(ROW_LOOP >= ROW_FEATURES && ROW_LOOP < ROW_ALL_FEATURES, "ROW_LOOP is a stage feature behind the ones a speculation mode can open");
    static_assert(ROW_ALL_FEATURES <= 8, "RowStage keeps a row's features in one byte");
    const int rows[] = {0, 31, DOTS_MAX_BATCH - 1};
    for (int row : rows)
        for (int beside = 0; beside < 2; ++beside)
            for (unsigned set = 0; set < (1u << ROW_ALL_FEATURES); ++set) {
                RowStage with, without;                   // the same row with and without ROW_LOOP
                const int nb = row == 0 ? 1 : row - 1;
                if (beside)
                    for (int f = 0; f < ROW_ALL_FEATURES; ++f) { with.attach(nb, (RowFeature)f); without.attach(nb, (RowFeature)f); }
                for (int f = 0; f < ROW_ALL_FEATURES; ++f)
                    if ((set >> f) & 1u) {
                        with.attach(row, (RowFeature)f);
                        if (f != ROW_LOOP) without.attach(row, (RowFeature)f);
                    }
                const bool looped = (set >> ROW_LOOP) & 1u;
                for (int pen = 0; pen < 2; ++pen)
                    for (int mode = 0; mode < 64; ++mode) {
                        if (looped) {
                            check(!with.speculates(row, pen != 0, mode), "a loop row speculates", row, set, pen, mode, beside);
                            check(with.staged(row) && with.has(row, ROW_LOOP), "a loop row is not staged", row, set, pen, mode, beside);
                        } else {
                            check(with.speculates(row, pen != 0, mode) == without.speculates(row, pen != 0, mode), "ROW_LOOP changed another row", row, set,
                                  pen, mode, beside);
                        }
                        if (beside)                       // the neighbour holds everything, ROW_LOOP included: never
                            check(!with.speculates(nb, pen != 0, mode), "the full neighbour speculates", nb, set, pen, mode, beside);
                    }
                // the counts: the row's loop feature is counted once, and leaves with a detach
                check(with.rows(ROW_LOOP) == (looped ? 1 : 0) + beside, "rows(ROW_LOOP)", row, set, 0, 0, beside);
                if (looped) {
                    const bool left = with.detach(row, ROW_LOOP);
                    check(left == (set == (1u << ROW_LOOP)), "detach reports leaving the stage", row, set, 0, 0, beside);
                    check(with.rows(ROW_LOOP) == beside && !with.has(row, ROW_LOOP), "detach", row, set, 0, 0, beside);
                    for (int mode = 0; mode < 64; ++mode)
                        check(with.speculates(row, false, mode) == without.speculates(row, false, mode), "after the detach", row, set, 0, mode, beside);
                }
            }
    std::printf("%ld cases, %d failures\n", cases, fails);
    return fails ? 1 : 0;
}
