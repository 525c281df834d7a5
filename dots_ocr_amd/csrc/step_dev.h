// Device helpers of the token-selection kernels (decode.hip) and of the speculative accept walk (spec.hip): the arg-max merge rule and the
// commit of one selected token.  ONE definition: a token a speculating step accepts goes through the bookkeeping of a sequential step.
#pragma once
#include "common.h"
#include "kernels.h"

constexpr int ARGMAX_CHUNKS = 64;

// The walk of a row's stop automaton over the bytes of token `tok`, which the row just appended at output index n.  At the first byte where
// a listed string ends (match_len[state] > 0) with n >= min_tokens: the hit record is written, the row is finished, the walk ends.  Below
// min_tokens the automaton still advances, so a string that straddles the boundary is found.  A token without bytes moves nothing.
DEVI void stop_walk(const StopSel& ss, const StepState& st, int b, int tok, int n) {
    RowStop& rs = ss.rows[b];
    if (!rs.table || tok < 0 || tok >= ss.V) return;
    uint32_t s = (uint32_t)rs.state < (uint32_t)rs.n_states ? (uint32_t)rs.state : 0u;
    const int j0 = ss.tok_off[tok], end = ss.tok_off[tok + 1];
    for (int j = j0; j < end; ++j) {
        s = rs.table[(size_t)s * 256 + ss.tok_bytes[j]];              // every entry < n_states (checked at dots_stop_create)
        const int len = rs.match_len[s];
        if (len > 0 && n >= rs.min_tokens) {
            rs.hit_tok = n; rs.hit_bytes = j - j0 + 1; rs.hit_len = len; rs.hit_id = rs.match_id[s];
            st.finished[b] = 1;
            break;
        }
    }
    rs.state = (int32_t)s;
}

// Commit one selected token of row (slot) b: append to its output, EOS / length bookkeeping, next-step input.
// A finished row keeps decoding (fixed-shape graph) but its context is frozen, so it rewrites the same KV position for ever
// and can idle in its slot until the host refills it (continuous batching).
// rules: the row's logit rules (per-row stage only) or nullptr: its stop ids finish it too, RULE_IGNORE_EOS takes the engine's
// EOS ids out of the test.  The arg-max and engine-wide sampler paths pass nullptr (a constant after inlining).
// guide: the launch's guides (per-row stage only) or nullptr.  A guided row that is not finished advances its automaton by the
// bytes of the committed token; an EOS or stop id moves nothing and finishes the row, RULE_IGNORE_EOS or not (the guide allowed it because
// the state is accepting; with nothing else left to allow, a row that ignored it could only repeat it).
// stop: the engine's stop-string rows (per-row stage only) or nullptr.  A row that holds an automaton and is not finished walks
// the bytes of the committed token (stop_walk); an EOS or stop id is not walked.
// Returns what the commit did, for the loop guard's check behind it (loop_dev.h): COMMIT_IDLE = the row was finished already and nothing
// was appended, COMMIT_EOS = the token finished the row as an EOS or stop id, COMMIT_TOKEN = anything else.
enum { COMMIT_IDLE = 0, COMMIT_TOKEN = 1, COMMIT_EOS = 2 };
DEVI int commit_token(const StepState& st, int b, int tok, const RowRules* rules = nullptr, const GuideSel* guide = nullptr,
                       const StopSel* stop = nullptr) {
    const bool done = st.finished[b] != 0;
    int what = COMMIT_IDLE;
    if (st.advance_ctx && !done) st.ctx_len[b] += 1;
    if (!done) {
        const int n = st.out_lens[b];
        const int cap = st.max_len ? st.max_len[b] : st.cap;
        st.out_ids[(size_t)b * st.out_stride + n] = tok;
        st.out_lens[b] = n + 1;
        bool eos = false;
        const bool guided = guide && guide->rows[b].table;
        if (guided || !(rules && (rules->flags & RULE_IGNORE_EOS)))
            for (int k = 0; k < st.n_eos; ++k) eos = eos || (tok == st.eos_ids[k]);
        if (rules)
            for (int k = 0; k < min(rules->n_stop, DOTS_MAX_STOP_IDS); ++k) eos = eos || (tok == rules->stop[k]);
        if (guided && !eos && tok >= 0 && tok < guide->V) {
            RowGuide& rg = guide->rows[b];
            uint32_t s = (uint32_t)rg.state;
            for (int j = guide->tok_off[tok], end = guide->tok_off[tok + 1]; j < end && s != GUIDE_DEAD; ++j)
                s = rg.table[(size_t)s * 256 + guide->tok_bytes[j]];
            if (s != GUIDE_DEAD) rg.state = (int32_t)s;              // a token the guide did not allow (the all -inf fallback) moves nothing
        }
        if (stop && !eos) stop_walk(*stop, st, b, tok, n);
        if (eos || n + 1 >= cap) st.finished[b] = 1;
        what = eos ? COMMIT_EOS : COMMIT_TOKEN;
    }
    st.cur_tokens[b] = tok;
    return what;
}

DEVI void argmax_merge(float& best, int& bi, float ov, int oi) {
    if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
}
