// The row plan of dots_slots_extend and dots_slots_score, in plain C++ so that a host program can hold it to a
// restatement (tests/score_plan_model.cpp): how the tokens fed to the listed slots are packed into rows, and which packed row records
// which entry of a score.
//
// Slot i is fed F_i = [pending] + ids_i with keep_pending[i], else ids_i; f_i = |F_i|.  The packed rows are F_0, F_1, ... one after the
// other, and chunk k of a call is packed rows [k * max_batch, min((k + 1) * max_batch, n_rows)).  Packed row r = (slot i, offset j)
// carries F_i[j], -1 standing for the pending token (offset 0 alone can be it), which only the device knows.
//
// The row at F_i[j] records entry j of slot i iff j + 1 < f_i, and the token whose value it takes is F_i[j + 1] — the token of the NEXT
// packed row, in this chunk or the next one.  A slot's last row records nothing, whatever follows it in its chunk; a target is an id of
// the call's list, never the pending token.
#pragma once
#include <cstdint>

// rows the call packs
inline int64_t extend_fed_rows(const int32_t* lens, const int32_t* keep_pending, int n) {
    int64_t r = 0;
    for (int i = 0; i < n; ++i) r += lens[i] + (keep_pending[i] ? 1 : 0);
    return r;
}

// slot / off / tok [n_rows]: the packed rows, slot by slot in the caller's order.  Returns n_rows
inline int64_t extend_pack_rows(const int32_t* slots, const int32_t* ids, const int32_t* lens, const int32_t* keep_pending, int n, int32_t* slot,
                                int32_t* off, int32_t* tok) {
    int64_t r = 0, t = 0;
    for (int i = 0; i < n; ++i) {
        const int f = lens[i] + (keep_pending[i] ? 1 : 0);
        for (int j = 0; j < f; ++j, ++r) {
            slot[r] = slots[i];
            off[r] = j;
            tok[r] = keep_pending[i] ? (j == 0 ? -1 : ids[t + j - 1]) : ids[t + j];
        }
        t += lens[i];
    }
    return r;
}

// entry / target [n_rows] of the packed rows: entry[r] = the index of the entry row r records (its offset) or -1 = it records nothing,
// target[r] = the token whose value the entry takes (-1 where nothing is recorded).  A slot is listed once, so two neighbouring rows
// belong to one sequence iff they name the same slot and consecutive offsets.  Returns the number of rows that record
inline int64_t score_plan_rows(const int32_t* slot, const int32_t* off, const int32_t* tok, int64_t n_rows, int32_t* entry, int32_t* target) {
    int64_t n_rec = 0;
    for (int64_t r = 0; r < n_rows; ++r) {
        const bool rec = r + 1 < n_rows && slot[r + 1] == slot[r] && off[r + 1] == off[r] + 1;
        entry[r] = rec ? off[r] : -1;
        target[r] = rec ? tok[r + 1] : -1;
        n_rec += rec;
    }
    return n_rec;
}

// chunks of a call, and the rows of chunk k
inline int64_t score_chunks(int64_t n_rows, int max_batch) { return (n_rows + max_batch - 1) / max_batch; }
inline int score_chunk_rows(int64_t n_rows, int max_batch, int64_t k) {
    const int64_t left = n_rows - k * max_batch;
    return (int)(left < max_batch ? left : max_batch);
}
// does any of the cn rows from packed row r0 on record (a chunk whose rows record nothing runs no lm_head and no logprob stage)
inline bool score_chunk_records(const int32_t* entry, int64_t r0, int cn) {
    for (int r = 0; r < cn; ++r)
        if (entry[r0 + r] >= 0) return true;
    return false;
}
