// The row plan of a scoring extend (csrc/score_plan.h) held to a brute-force restatement: for every call of up to 3 slots feeding up to 5
// ids each, with and without the pending token, at max_batch 2 and 4 — the packed rows, which rows record, their targets and entry
// indices, and where the chunks are cut.  Stand-alone: no GPU, no HIP.  Prints "<n> checks, <m> mismatches".
#include <cstdint>
#include <cstdio>
#include <vector>

#include "score_plan.h"

namespace {
long checks = 0, bad = 0;
void expect(bool ok, const char* what, int n, const int* lens, const int* keep, int mb, long r) {
    ++checks;
    if (ok) return;
    if (++bad <= 20) {
        std::printf("MISMATCH %s: n=%d mb=%d row=%ld lens/keep =", what, n, mb, r);
        for (int i = 0; i < n; ++i) std::printf(" %d/%d", lens[i], keep[i]);
        std::printf("\n");
    }
}

// the restatement: per slot its fed sequence F (the pending token as -1); a row is (slot, j); it records iff F has a j + 1
struct Row { int slot, j, tok, entry, target, chunk, in_chunk; };

void one_call(int n, const int* lens, const int* keep, int mb) {
    const int slot_ids[3] = {5, 2, 7};                         // not in order, not dense
    std::vector<int32_t> slots(n), ids, lens32(lens, lens + n), keep32(keep, keep + n);
    std::vector<std::vector<int>> F(n);
    int next_id = 100;
    for (int i = 0; i < n; ++i) {
        slots[i] = slot_ids[i];
        if (keep[i]) F[i].push_back(-1);
        for (int j = 0; j < lens[i]; ++j) {
            ids.push_back(next_id);
            F[i].push_back(next_id++);
        }
    }
    std::vector<Row> want;
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < (int)F[i].size(); ++j) {
            const bool rec = j + 1 < (int)F[i].size();
            const int r = (int)want.size();
            want.push_back(Row{slots[i], j, F[i][j], rec ? j : -1, rec ? F[i][j + 1] : -1, r / mb, r % mb});
        }
    const int64_t n_rows = extend_fed_rows(lens32.data(), keep32.data(), n);
    expect(n_rows == (int64_t)want.size(), "row count", n, lens, keep, mb, -1);
    std::vector<int32_t> slot(n_rows + 1, -77), off(n_rows + 1, -77), tok(n_rows + 1, -77), entry(n_rows + 1, -77), target(n_rows + 1, -77);
    expect(extend_pack_rows(slots.data(), ids.data(), lens32.data(), keep32.data(), n, slot.data(), off.data(), tok.data()) == n_rows, "packed count", n,
           lens, keep, mb, -1);
    const int64_t n_rec = score_plan_rows(slot.data(), off.data(), tok.data(), n_rows, entry.data(), target.data());
    long want_rec = 0;
    for (int64_t r = 0; r < n_rows; ++r) {
        const Row& w = want[r];
        want_rec += w.entry >= 0;
        expect(slot[r] == w.slot && off[r] == w.j && tok[r] == w.tok, "packed row", n, lens, keep, mb, r);
        expect((entry[r] >= 0) == (w.entry >= 0), "records", n, lens, keep, mb, r);
        expect(entry[r] == w.entry, "entry index", n, lens, keep, mb, r);
        expect(target[r] == w.target, "target", n, lens, keep, mb, r);
        expect(entry[r] < 0 || target[r] >= 100, "a target is an id of the call, never the pending token", n, lens, keep, mb, r);
    }
    expect(n_rec == want_rec, "recording rows", n, lens, keep, mb, -1);
    // nothing was written behind the lists
    expect(slot[n_rows] == -77 && off[n_rows] == -77 && tok[n_rows] == -77 && entry[n_rows] == -77 && target[n_rows] == -77, "guard", n, lens, keep, mb, n_rows);
    // ---- chunk cuts: every row in exactly one chunk, at the place the restatement says; a chunk records iff one of its rows does
    const int64_t n_chunks = score_chunks(n_rows, mb);
    expect(n_chunks == (n_rows + mb - 1) / mb, "chunk count", n, lens, keep, mb, -1);
    int64_t r = 0;
    for (int64_t k = 0; k < n_chunks; ++k) {
        const int cn = score_chunk_rows(n_rows, mb, k);
        expect(cn >= 1 && cn <= mb && (cn == mb || k == n_chunks - 1), "chunk rows", n, lens, keep, mb, k);
        bool any = false;
        for (int q = 0; q < cn; ++q, ++r) {
            expect(r < n_rows && want[r].chunk == k && want[r].in_chunk == q, "chunk cut", n, lens, keep, mb, r);
            any = any || (r < n_rows && want[r].entry >= 0);
        }
        expect(score_chunk_records(entry.data(), k * mb, cn) == any, "chunk records", n, lens, keep, mb, k);
    }
    expect(r == n_rows, "rows covered", n, lens, keep, mb, -1);
}
}  // namespace

int main() {
    for (int mb : {2, 4})
        for (int n = 1; n <= 3; ++n) {
            int lens[3] = {1, 1, 1}, keep[3] = {0, 0, 0};
            const int combos = n == 1 ? 10 : n == 2 ? 100 : 1000;
            for (int code = 0; code < combos; ++code) {
                int c = code;
                for (int i = 0; i < n; ++i, c /= 10) {
                    lens[i] = 1 + (c % 10) / 2;                // 1 .. 5
                    keep[i] = (c % 10) % 2;
                }
                one_call(n, lens, keep, mb);
            }
        }
    std::printf("%ld checks, %ld mismatches\n", checks, bad);
    return bad ? 1 : 0;
}
