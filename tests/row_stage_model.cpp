// Exhaustive model check of RowStage (dots_ocr_amd/csrc/row_stage.h), a stand-alone host program: tests/test_row_stage_cpu.py compiles
// and runs it.  It lives here and not beside the header because the library build compiles every .cpp under csrc/.
//
// The model is a plain bool[rows][features], recounted from scratch after every operation.  Every sequence of up to 6 attach / detach
// operations over the five features on one row is walked (10 + 10^2 + ... + 10^6 operations), once with every other row empty and once
// with a second row that carries a fixed, different subset (cross-row leakage of the counters).  After every operation has / staged /
// rows / staged_rows and the operation's own return value (the entered / left transition) are compared with the model.  Exit status 0 =
// no difference.
#include <cstdio>
#include <cstring>

#ifndef DOTS_MAX_BATCH
#define DOTS_MAX_BATCH 64
#endif
#include "row_stage.h"

namespace {

constexpr int ROWS = DOTS_MAX_BATCH, DEPTH = 6;
long n_ops = 0;
int n_bad = 0;

struct Model {
    bool has[ROWS][ROW_FEATURES];
    bool staged(int row) const {
        for (int f = 0; f < ROW_FEATURES; ++f)
            if (has[row][f]) return true;
        return false;
    }
};

void bad(const char* what, const int* ops, int n) {
    if (++n_bad > 20) return;
    std::fprintf(stderr, "MISMATCH %s after", what);
    for (int i = 0; i < n; ++i) std::fprintf(stderr, " %s%d", ops[i] < ROW_FEATURES ? "+" : "-", ops[i] % ROW_FEATURES);
    std::fprintf(stderr, "\n");
}

void compare(const RowStage& s, const Model& m, const int* ops, int n) {
    int per_feature[ROW_FEATURES] = {0}, staged = 0;
    for (int r = 0; r < ROWS; ++r) {
        for (int f = 0; f < ROW_FEATURES; ++f) {
            per_feature[f] += m.has[r][f];
            if (s.has(r, (RowFeature)f) != m.has[r][f]) bad("has", ops, n);
        }
        staged += m.staged(r);
        if (s.staged(r) != m.staged(r)) bad("staged", ops, n);
    }
    for (int f = 0; f < ROW_FEATURES; ++f)
        if (s.rows((RowFeature)f) != per_feature[f]) bad("rows", ops, n);
    if (s.staged_rows() != staged) bad("staged_rows", ops, n);
}

// op < ROW_FEATURES: attach feature op; else detach feature op - ROW_FEATURES.  Returns whether stage and model agree on the transition
bool apply(RowStage& s, Model& m, int row, int op) {
    const RowFeature f = (RowFeature)(op % ROW_FEATURES);
    const bool before = m.staged(row);
    bool got, want;
    if (op < ROW_FEATURES) {
        got = s.attach(row, f);
        m.has[row][f] = true;
        want = !before;                                    // entered: only a row that carried nothing can enter
    } else {
        got = s.detach(row, f);
        m.has[row][f] = false;
        want = before && !m.staged(row);                   // left: it carried something and carries nothing now
    }
    return got == want;
}

void walk(const RowStage& s, const Model& m, int row, int* ops, int depth) {
    if (depth == DEPTH) return;
    for (int op = 0; op < 2 * ROW_FEATURES; ++op) {
        RowStage s2 = s;
        Model m2 = m;
        ops[depth] = op;
        ++n_ops;
        if (!apply(s2, m2, row, op)) bad("entered / left", ops, depth + 1);
        compare(s2, m2, ops, depth + 1);
        walk(s2, m2, row, ops, depth + 1);
    }
}

}  // namespace

int main() {
    int ops[DEPTH] = {0};
    const int subject = ROWS - 1, neighbour = 0;
    {   // one row alone
        RowStage s;
        Model m;
        std::memset(&m, 0, sizeof(m));
        compare(s, m, ops, 0);
        walk(s, m, subject, ops, 0);
    }
    {   // beside a row that carries rules and stop strings throughout
        RowStage s;
        Model m;
        std::memset(&m, 0, sizeof(m));
        if (!apply(s, m, neighbour, ROW_RULES) || !apply(s, m, neighbour, ROW_STOP)) bad("neighbour set-up", ops, 0);
        compare(s, m, ops, 0);
        walk(s, m, subject, ops, 0);
        // reset(): nothing is left, and the record works again from empty
        apply(s, m, subject, ROW_GUIDE);
        s.reset();
        std::memset(&m, 0, sizeof(m));
        compare(s, m, ops, 0);
        if (!apply(s, m, subject, ROW_PARAMS)) bad("attach after reset", ops, 0);
        compare(s, m, ops, 0);
    }
    std::printf("row_stage_model: %ld operations, %d mismatches\n", n_ops, n_bad);
    return n_bad ? 1 : 0;
}
