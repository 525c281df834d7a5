// Beam search over shared KV pages: a group of B beams in B slots pays one prefill and B decode rows; the per-step
// selection and the mid-generation fork of the beams run on the device, inside the captured decode step.
//
//   logprob_partial_kernel (logprobs.hip, launched here over the group rows with top_n = 2B): per-chunk (max, sum, top-2B) of every beam
//   beam_select_kernel   grid groups, one wave: per live beam the logprobs stage's final reduction (logprobs_dev.h: the same bits as an
//                        unbeamed row's logprobs), then lane 0 walks the B x 2B candidates in (beam, rank) order: s = cum + lp; an EOS id is
//                        a completed record, the others compete for the B places by (s desc, beam asc, rank asc).  Commits like
//                        commit_token: out_ids / beam_parent at out_lens, out_lens + 1, ctx_len + 1, finished at the cap.
//   beam_reorder_kernel  grid groups, 64 threads: the group's table entries [first, g] staged in LDS (all read before any is written),
//                        then row j's frozen entries [first, g) = its parent's and its tail entry g = its spare page, which
//                        beam_copy_kernel fills with the parent's tail; the old tail is the new spare.  The B tails and B spares are 2B
//                        distinct pages at all times, so no copy reads a page another one writes.
//   beam_copy_kernel     grid (page bytes / 4 KiB, layers, groups x 8), 256 threads: kv_fork_kernel's shape, 16-byte vectors, bytes only.
//
// All rows of a group share one context length, so every KV write of a step lands in entry g of a row: a tail owned by that row alone.
#include "engine.h"
#include "logprobs_dev.h"

namespace {

constexpr int BEAM_TOP = 2 * DOTS_MAX_BEAMS;

__global__ __launch_bounds__(64) void beam_select_kernel(BeamState bs, StepState st, int g0, int reorder) {
    __shared__ LpFinalLds l;
    __shared__ float clp[DOTS_MAX_BEAMS][BEAM_TOP];
    __shared__ int cid[DOTS_MAX_BEAMS][BEAM_TOP];
    __shared__ float sel_s[DOTS_MAX_BEAMS];
    __shared__ int sel_p[DOTS_MAX_BEAMS], sel_t[DOTS_MAX_BEAMS];
    const int gi = g0 + blockIdx.x, c = threadIdx.x;
    BeamGroupDev& g = bs.groups[gi];
    const int B = g.B;
    if (B < 2 || B > DOTS_MAX_BEAMS) return;
    const int row0 = g.slots[0];
    if (st.finished[row0]) return;                             // the rows of a group finish together
    const int step = st.out_lens[row0], n = 2 * B;
    if (step >= st.out_stride) return;
    for (int i = 0; i < B; ++i) {
        if (!(g.cum[i] > -INFINITY)) continue;                 // a dead beam has no candidates (uniform over the wave)
        const float lse = lp_final_load(l, bs.part_ms, bs.part_v, bs.part_i, g.slots[i], c, n);
        int h = 0;
        for (int r = 0; r < n; ++r) {
            float gv;
            int id;
            lp_final_next(l, c, n, h, gv, id);
            if (c == 0) {
                cid[i][r] = id == LP_NONE ? -1 : id;
                clp[i][r] = id == LP_NONE ? __builtin_nanf("") : gv - lse;
            }
        }
        __syncthreads();                                       // the next beam's load overwrites the lists
    }
    if (c != 0) return;
    int nsel = 0;
    for (int i = 0; i < B; ++i) {
        const float cum = g.cum[i];
        if (!(cum > -INFINITY)) continue;
        for (int r = 0; r < n; ++r) {
            const int id = cid[i][r];
            if (id < 0) continue;
            const float s = cum + clp[i][r];
            if (!(s > -INFINITY)) continue;                    // NaN or -inf: no such candidate
            bool eos = false;
            for (int k = 0; k < st.n_eos; ++k) eos = eos || (id == st.eos_ids[k]);
            if (eos) {
                const int k = g.n_done;
                if (k < BEAM_DONE_CAP) bs.done[(size_t)gi * BEAM_DONE_CAP + k] = BeamDone{step, i, id, s};
                g.n_done = k + 1;
                continue;
            }
            // candidates arrive in (beam, rank) order: a later one takes a place only from a strictly smaller score
            int pos = nsel;
            while (pos > 0 && s > sel_s[pos - 1]) --pos;
            if (pos >= B) continue;
            for (int k = min(nsel, B - 1); k > pos; --k) { sel_s[k] = sel_s[k - 1]; sel_p[k] = sel_p[k - 1]; sel_t[k] = sel_t[k - 1]; }
            sel_s[pos] = s; sel_p[pos] = i; sel_t[pos] = id;
            nsel = min(nsel + 1, B);
        }
    }
    for (int j = 0; j < B; ++j) {
        const int row = g.slots[j];
        const bool live = j < nsel;
        const size_t o = (size_t)row * st.out_stride + step;
        st.out_ids[o] = live ? sel_t[j] : -1;
        bs.parent[o] = live ? sel_p[j] : -1;
        st.cur_tokens[row] = live ? sel_t[j] : 0;
        g.cum[j] = live ? sel_s[j] : -INFINITY;
        g.par[j] = live ? sel_p[j] : (nsel ? sel_p[0] : j);    // a dead beam follows a live parent: the page invariant needs no special case
        st.out_lens[row] = step + 1;
        if (st.advance_ctx) st.ctx_len[row] += 1;
        const int cap = st.max_len ? st.max_len[row] : st.cap;
        if (step + 1 >= cap || nsel == 0) st.finished[row] = 1;
    }
    g.act = reorder;
}

__global__ __launch_bounds__(64) void beam_reorder_kernel(BeamState bs, const int32_t* __restrict__ ctx_len, int32_t* __restrict__ block_table,
                                                          int max_pages) {
    extern __shared__ int32_t tab[];                           // [B][max_pages]: entries [first, g] of every row
    __shared__ int par[DOTS_MAX_BEAMS], nch[DOTS_MAX_BEAMS];
    BeamGroupDev& g = bs.groups[blockIdx.x];
    const int B = g.B, t = threadIdx.x;
    if (B < 2 || B > DOTS_MAX_BEAMS) return;
    if (!g.act) {                                              // no selection this step (finished rows): nothing moves
        if (t < DOTS_MAX_BEAMS) g.copy_dst[t] = -1;
        return;
    }
    const int first = g.first, tail = (ctx_len[g.slots[0]] - 1) >> 6;          // the position the step just wrote
    const int W = tail - first + 1;
    if (W < 1 || tail >= max_pages) {
        if (t < DOTS_MAX_BEAMS) g.copy_dst[t] = -1;
        if (t == 0) g.act = 0;
        return;
    }
    if (t < DOTS_MAX_BEAMS) { par[t] = t < B ? g.par[t] : 0; nch[t] = 0; }
    for (int i = 0; i < B; ++i)
        for (int k = t; k < W; k += 64) tab[i * max_pages + k] = block_table[(size_t)g.slots[i] * max_pages + first + k];
    __syncthreads();
    if (t == 0)
        for (int j = 0; j < B; ++j) nch[par[j]] += 1;
    __syncthreads();
    for (int j = 0; j < B; ++j) {
        const int p = par[j];
        if (p != j)
            for (int k = t; k < W - 1; k += 64) block_table[(size_t)g.slots[j] * max_pages + first + k] = tab[p * max_pages + k];
    }
    if (t < B) {
        const int j = t, p = par[j];
        if (p == j && nch[j] == 1) g.copy_dst[j] = -1;         // its own only child: the tail stays where it is
        else {
            const int sp = g.spare[j];
            g.copy_src[j] = tab[p * max_pages + W - 1];
            g.copy_dst[j] = sp;
            block_table[(size_t)g.slots[j] * max_pages + tail] = sp;
            g.spare[j] = tab[j * max_pages + W - 1];
        }
    }
    if (t == 0) g.act = 0;
}

__global__ __launch_bounds__(256) void beam_copy_kernel(u32x4* __restrict__ pool, size_t layer_vec, int page_vec, const BeamGroupDev* __restrict__ groups) {
    const BeamGroupDev& g = groups[blockIdx.z / DOTS_MAX_BEAMS];
    const int j = blockIdx.z % DOTS_MAX_BEAMS, i = blockIdx.x * 256 + threadIdx.x;
    if (j >= g.B) return;
    const int dst = g.copy_dst[j];
    if (dst < 0 || i >= page_vec) return;
    u32x4* base = pool + (size_t)blockIdx.y * layer_vec;
    base[(size_t)dst * page_vec + i] = base[(size_t)g.copy_src[j] * page_vec + i];
}

}  // namespace

hipError_t launch_beam_select(hipStream_t s, const BeamState& bs, const StepState& st, int g0, int n, int reorder) {
    if (g0 < 0 || n < 1 || g0 + n > BEAM_MAX_GROUPS) return hipErrorInvalidValue;
    hipLaunchKernelGGL(beam_select_kernel, dim3(n), dim3(64), 0, s, bs, st, g0, reorder);
    return hipGetLastError();
}

hipError_t launch_beam_reorder(hipStream_t s, const BeamState& bs, int n, const int32_t* ctx_len, int32_t* block_table, int max_pages, void* pool,
                               size_t layer_bytes, size_t page_bytes, int layers) {
    const size_t lds = (size_t)DOTS_MAX_BEAMS * max_pages * 4;
    if (n < 1 || n > BEAM_MAX_GROUPS || max_pages < 1 || lds > 48 * 1024 || layers < 1 || page_bytes == 0 || (page_bytes & 15) || (layer_bytes & 15) ||
        page_bytes / 16 > (size_t)INT32_MAX)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(beam_reorder_kernel, dim3(n), dim3(64), lds, s, bs, ctx_len, block_table, max_pages);
    hipError_t r = hipGetLastError();
    if (r != hipSuccess) return r;
    const int page_vec = (int)(page_bytes / 16);
    hipLaunchKernelGGL(beam_copy_kernel, dim3((page_vec + 255) / 256, layers, n * DOTS_MAX_BEAMS), dim3(256), 0, s, reinterpret_cast<u32x4*>(pool),
                       layer_bytes / 16, page_vec, bs.groups);
    return hipGetLastError();
}

// ===================================================================================== host side
namespace engine {
namespace {

BeamState beam_state(const DotsEngine* e) { return BeamState{e->d_beam, e->d_beam_done, e->beam_parent, e->bm_ms, e->bm_pv, e->bm_pi}; }

LogprobState beam_partial_state(const DotsEngine* e) {
    return LogprobState{e->bm_topn, e->bm_sel, nullptr, nullptr, nullptr, e->bm_ms, e->bm_pv, e->bm_pi, e->bm_pos, nullptr, nullptr, nullptr, e->cfg.max_seq_len};
}

int ensure_beam_state(DotsEngine* e) {
    if (e->d_beam) return DOTS_OK;
    const size_t rows = e->cfg.max_batch, K = DOTS_MAX_TOP_LOGPROBS;
    CK(e->alloc(&e->d_beam, (size_t)BEAM_MAX_GROUPS));
    CK(e->alloc(&e->d_beam_done, (size_t)BEAM_MAX_GROUPS * BEAM_DONE_CAP));
    CK(e->alloc(&e->beam_parent, rows * e->cfg.max_seq_len));
    CK(e->alloc(&e->bm_ms, rows * LP_CHUNKS * 2));
    CK(e->alloc(&e->bm_pv, rows * LP_CHUNKS * K));
    CK(e->alloc(&e->bm_pi, rows * LP_CHUNKS * K));
    CK(e->alloc(&e->bm_pos, (size_t)DOTS_MAX_BATCH));
    CK(e->alloc(&e->bm_topn, (size_t)DOTS_MAX_BATCH));
    CK(e->alloc(&e->bm_sel, (size_t)DOTS_MAX_BATCH));
    e->beams.assign(BEAM_MAX_GROUPS, DotsEngine::BeamGroup{});
    return DOTS_OK;
}

// the tables the partial launch reads (top_n = 2B and sel = 1 on every group row), from the host records; stream ordered.  The caller
// synchronises before the stack arrays go
int upload_beam_rows(DotsEngine* e, int32_t* topn, int32_t* sel) {
    for (int b = 0; b < DOTS_MAX_BATCH; ++b) {
        const int gi = e->beam_of[b] - 1;
        topn[b] = gi >= 0 ? 2 * e->beams[gi].B : -1;
        sel[b] = gi >= 0 ? 1 : 0;
    }
    CK(hipMemcpyAsync(e->bm_topn, topn, DOTS_MAX_BATCH * 4, hipMemcpyHostToDevice, e->stream));
    CK(hipMemcpyAsync(e->bm_sel, sel, DOTS_MAX_BATCH * 4, hipMemcpyHostToDevice, e->stream));
    return DOTS_OK;
}

void recount_groups(DotsEngine* e) {
    e->n_beam_hi = 0;
    for (int g = 0; g < (int)e->beams.size(); ++g)
        if (e->beams[g].B) e->n_beam_hi = g + 1;
}

// completed records a step can add to a group at most: every beam's 2B distinct ids hold at most n_eos EOS ids
int done_per_step(const DotsEngine* e, const DotsEngine::BeamGroup& g) { return g.B * std::min(2 * g.B, e->n_eos); }

// the records waiting on the device move to the host record; synchronises
int drain_group(DotsEngine* e, int gi) {
    DotsEngine::BeamGroup& g = e->beams[gi];
    hipStream_t s = e->stream;
    int32_t n = 0;
    CK(hipMemcpyAsync(&n, &e->d_beam[gi].n_done, 4, hipMemcpyDeviceToHost, s));
    CK(hipStreamSynchronize(s));
    n = std::min<int32_t>(std::max<int32_t>(n, 0), BEAM_DONE_CAP);
    if (n > 0) {
        const size_t at = g.done.size();
        g.done.resize(at + n);
        CK(hipMemcpyAsync(g.done.data() + at, e->d_beam_done + (size_t)gi * BEAM_DONE_CAP, (size_t)n * sizeof(BeamDone), hipMemcpyDeviceToHost, s));
        CK(hipMemsetAsync(&e->d_beam[gi].n_done, 0, 4, s));
        CK(hipStreamSynchronize(s));
    }
    g.done_ub = 0;
    return DOTS_OK;
}

}  // namespace

// the group kernels of one decode step, behind the selection stage (which the group rows are masked out of)
int beam_step(DotsEngine* e, int rows) {
    const DotsConfig& c = e->cfg;
    hipStream_t s = e->stream;
    const size_t page_bytes = (size_t)c.num_kv_heads * 2 * 8192 * (e->kv8 ? 1 : 2);
    CK(launch_logprob_partial(s, e->d_logits, c.vocab_size, c.vocab_size, rows, beam_partial_state(e)));
    CK(launch_beam_select(s, beam_state(e), step_state(e, 1, nullptr), 0, e->n_beam_hi, 1));
    CK(launch_beam_reorder(s, beam_state(e), e->n_beam_hi, e->ctx_len, e->block_table, e->max_pages, e->pool, e->pool_layer_elems * 2, page_bytes, c.num_layers));
    return DOTS_OK;
}

// before a chunk of n_steps: no group's record buffer can overflow inside it
int beam_before_decode(DotsEngine* e, int n_steps) {
    for (int gi = 0; gi < e->n_beam_hi; ++gi) {
        DotsEngine::BeamGroup& g = e->beams[gi];
        if (!g.B) continue;
        const int64_t add = (int64_t)n_steps * done_per_step(e, g);
        if (add > BEAM_DONE_CAP)
            return e->fail(DOTS_E_CAPACITY, "a chunk of %d steps could complete %lld hypotheses of a beam group, its buffer holds %d: use shorter chunks", n_steps,
                           (long long)add, BEAM_DONE_CAP);
        if (g.done_ub + add > BEAM_DONE_CAP) RET(drain_group(e, gi));
        g.done_ub += (int)add;
    }
    return DOTS_OK;
}

// every slot of the group that `slot` belongs to is released (dots_slot_release of one of them)
int beam_release_group(DotsEngine* e, int slot) {
    const int gi = e->beam_of[slot] - 1;
    if (gi < 0) return DOTS_OK;
    DotsEngine::BeamGroup& g = e->beams[gi];
    hipStream_t s = e->stream;
    for (int i = 0; i < g.B; ++i) {
        const int b = g.slots[i];
        e->beam_of[b] = 0;
        e->slot_active[b] = 0;
        CK(hipMemsetAsync(e->ctx_len + b, 0, 4, s));
        release_pages(e, b);
        CK(upload_table_row(e, b));
    }
    CK(hipMemsetAsync(e->d_beam + gi, 0, sizeof(BeamGroupDev), s));
    g = DotsEngine::BeamGroup{};
    recount_groups(e);
    int32_t topn[DOTS_MAX_BATCH], sel[DOTS_MAX_BATCH];
    RET(upload_beam_rows(e, topn, sel));
    CK(hipStreamSynchronize(s));
    e->sel_dirty = true;
    return DOTS_OK;
}

// no group is left (dots_slots_reset, a static prefill): the caller gives the pages back
int beam_clear_all(DotsEngine* e) {
    if (!e->d_beam) return DOTS_OK;
    std::fill(e->beam_of, e->beam_of + DOTS_MAX_BATCH, 0);
    e->beams.assign(BEAM_MAX_GROUPS, DotsEngine::BeamGroup{});
    e->n_beam_hi = 0;
    CK(hipMemsetAsync(e->d_beam, 0, (size_t)BEAM_MAX_GROUPS * sizeof(BeamGroupDev), e->stream));
    CK(hipMemsetAsync(e->bm_topn, 0xFF, DOTS_MAX_BATCH * 4, e->stream));
    CK(hipMemsetAsync(e->bm_sel, 0, DOTS_MAX_BATCH * 4, e->stream));
    return DOTS_OK;
}

}  // namespace engine

using namespace engine;
extern "C" {

int dots_slots_beam(DotsEngine* e, int src_slot, const int32_t* dst_slots, int n_dst) {
    if (!e) return DOTS_E_INVALID;
    if (!e->finalized) return e->fail(DOTS_E_STATE, "weights not finalized");
    const int B = n_dst + 1;
    if (!dst_slots || B < 2 || B > DOTS_MAX_BEAMS)
        return e->fail(DOTS_E_INVALID, "dots_slots_beam: a group has 2 .. %d beams (the source and 1 .. %d free slots)", DOTS_MAX_BEAMS, DOTS_MAX_BEAMS - 1);
    const DotsConfig& c = e->cfg;
    const int mb = c.max_batch, V = c.vocab_size;
    if (src_slot < 0 || src_slot >= mb) return e->fail(DOTS_E_INVALID, "source slot %d out of range [0, %d)", src_slot, mb);
    if (e->spec_k) return e->fail(DOTS_E_STATE, "beam search cannot run while the engine speculates (dots_set_speculation)");
    const auto fresh = std::find(e->fresh_slots.begin(), e->fresh_slots.end(), src_slot);
    if (!e->slot_mode || !e->slot_active[src_slot] || fresh == e->fresh_slots.end() || slot_parked(e, src_slot))
        return e->fail(DOTS_E_STATE, "slot %d cannot start a beam group: only a sequence of the most recent dots_slots_prefill, before any decode step", src_slot);
    if (V > LP_MAX_V) return e->fail(DOTS_E_INVALID, "beam search supports vocabularies up to %d", LP_MAX_V);
    if ((size_t)e->max_pages * DOTS_MAX_BEAMS * 4 > 48 * 1024) return e->fail(DOTS_E_INVALID, "beam search supports max_seq_len up to %d", 48 * 1024 / (DOTS_MAX_BEAMS * 4) * 64);
    for (int i = 0; i < n_dst; ++i) RET(check_free_slot(e, dst_slots, i, src_slot, "group"));
    for (int i = 0; i < B; ++i) {
        const int r = i ? dst_slots[i - 1] : src_slot;
        if (e->stage.staged(r) || e->row_lp[r] >= 0)
            return e->fail(DOTS_E_INVALID, "slot %d carries row parameters, rules, a guide, an n-gram rule, stop strings, a loop guard or logprobs: a beam row takes none", r);
        if (e->row_stream[r]) return e->fail(DOTS_E_STATE, "slot %d streams (dots_set_row_stream): a group's outputs are reordered, its rows cannot", r);
    }
    int gi = 0;
    while (gi < (int)e->beams.size() && e->beams[gi].B) ++gi;
    if (!e->beams.empty() && gi == (int)e->beams.size()) return e->fail(DOTS_E_CAPACITY, "every beam group entry is in use");
    // ---- page arithmetic: full reservation.  Every beam owns pages for the positions [64 floor(L / 64), L + max_new) and one spare
    const int L = e->slot_prompt[src_slot], max_new = e->slot_limit[src_slot] - L;
    const int shared = L / 64, own = (L + max_new + 63) / 64 - shared;
    auto& src_pages = e->slot_pages[src_slot];
    if ((int)src_pages.size() < shared + (L % 64 ? 1 : 0)) return e->fail(DOTS_E_STATE, "slot %d does not hold its prompt pages", src_slot);
    const int src_has = (int)src_pages.size() - shared;
    const int64_t need = (int64_t)std::max(own - src_has, 0) + 1 + (int64_t)n_dst * (own + 1);
    ensure_free(e, need);
    if (shared + own > e->max_pages || need > (int64_t)e->free_pages.size())
        return e->fail(DOTS_E_CAPACITY, "KV pool exhausted: a group of %d beams needs %lld more pages of 64 tokens (%d per beam and a spare each), %d of %d are free", B,
                       (long long)need, own, free_count(e), e->n_pool_pages);
    CK(hipSetDevice(e->device));
    hipStream_t s = e->stream;
    RET(ensure_beam_state(e));
    // ---- from here on the call changes state; a failed launch gives the children's pages back (the source keeps what it grew by)
    PageGuard guard{e, dst_slots, n_dst, true};
    BeamGroupDev gd{};
    gd.B = B; gd.first = shared;
    int32_t stage[3 * DOTS_MAX_BATCH] = {0};
    std::vector<LiveRow> live(B);
    for (int i = 0; i < B; ++i) {
        const int d = i ? dst_slots[i - 1] : src_slot;
        auto& mine = e->slot_pages[d];
        if (i) share_pages(e, d, src_pages.data(), shared);
        bool changed = false;
        grow_pages(e, d, (shared + own) * 64, &changed);   // cannot fall short: counted above
        CK(upload_table_row(e, d));                        // the last upload of this row: from here on the device reorders it
        if (i) { stage[i - 1] = d; stage[DOTS_MAX_BATCH + i - 1] = mine[shared]; }
        gd.spare[i] = e->free_pages.back();                // held by the slot, named by no table row
        e->free_pages.pop_back();
        e->page_refs[gd.spare[i]] = 1;
        mine.push_back(gd.spare[i]);
        gd.slots[i] = d;
        gd.cum[i] = i ? -INFINITY : 0.f;
        gd.par[i] = 0;
        gd.copy_dst[i] = -1;
        live[i] = LiveRow{d, L, max_new};
    }
    CK(hipMemcpyAsync(e->fk_dev, stage, sizeof(stage), hipMemcpyHostToDevice, s));
    // the tail page, as a fork copies it
    if (L % 64) CK(launch_kv_fork_pages(s, e->pool, e->pool_layer_elems * 2, kv_page_bytes(e), c.num_layers, src_pages[shared], e->fk_dev + DOTS_MAX_BATCH, n_dst));
    // the source too: its own first token is replaced by the group's.  A group row's logprob positions stay as they are (rows_go_live)
    RET(rows_go_live(e, live, false));
    int rows = 0;
    for (int i = 0; i < B; ++i) {
        rows = std::max(rows, gd.slots[i] + 1);
        e->beam_of[gd.slots[i]] = gi + 1;
    }
    DotsEngine::BeamGroup& g = e->beams[gi];
    g = DotsEngine::BeamGroup{};
    g.B = B; g.L = L; g.max_new = max_new;
    std::copy(gd.slots, gd.slots + B, g.slots);
    struct GroupGuard {                                    // a failure below leaves no half-made group behind
        DotsEngine* e; int gi; bool armed = true;
        ~GroupGuard() {
            if (!armed) return;
            for (int i = 0; i < e->beams[gi].B; ++i) e->beam_of[e->beams[gi].slots[i]] = 0;
            e->beams[gi] = DotsEngine::BeamGroup{};
            (void)hipMemsetAsync(e->d_beam + gi, 0, sizeof(BeamGroupDev), e->stream);
        }
    } group_guard{e, gi};
    CK(hipMemcpyAsync(e->d_beam + gi, &gd, sizeof(gd), hipMemcpyHostToDevice, s));
    int32_t topn[DOTS_MAX_BATCH], sel[DOTS_MAX_BATCH];
    RET(upload_beam_rows(e, topn, sel));
    // ---- first selection: the source's last-position logits with cum = {0, -inf, ...}; every live beam's parent is beam 0 and every
    // child holds the source's KV already, so nothing is reordered
    CK(launch_logprob_partial(s, e->d_logits, V, V, rows, beam_partial_state(e)));
    CK(launch_beam_select(s, beam_state(e), step_state(e, 0, nullptr), gi, 1, 0));
    CK(hipStreamSynchronize(s));                           // the staged arrays are stack variables
    g.done_ub = done_per_step(e, g);
    mark_live(e, live.data() + 1, n_dst);                 // the source's record stands
    e->fresh_slots.erase(std::find(e->fresh_slots.begin(), e->fresh_slots.end(), src_slot));      // the source is no plain sequence any more
    recount_groups(e);
    guard.armed = false;
    group_guard.armed = false;
    return DOTS_OK;
}

int dots_beam_info(DotsEngine* e, int slot, int32_t* n_beams, int32_t* steps, int32_t* n_done) {
    if (!e || !n_beams || !steps || !n_done) return e ? e->fail(DOTS_E_INVALID, "null argument") : DOTS_E_INVALID;
    if (!e->slot_mode || slot < 0 || slot >= e->cfg.max_batch || !e->beam_of[slot]) return e->fail(DOTS_E_STATE, "slot %d belongs to no beam group", slot);
    CK(hipSetDevice(e->device));
    const int gi = e->beam_of[slot] - 1;
    RET(drain_group(e, gi));
    int32_t st = 0;
    CK(hipMemcpyAsync(&st, e->out_lens + e->beams[gi].slots[0], 4, hipMemcpyDeviceToHost, e->stream));
    CK(hipStreamSynchronize(e->stream));
    *n_beams = e->beams[gi].B;
    *steps = st;
    *n_done = (int32_t)e->beams[gi].done.size();
    return DOTS_OK;
}

int dots_beam_read(DotsEngine* e, int slot, int32_t* n_beams, int32_t* steps, float* cum, int32_t* tokens, int32_t* parents, int step_capacity,
                   int32_t* done, int done_capacity, int32_t* n_done) {
    if (!e || !n_beams || !steps || !cum || !n_done || step_capacity < 0 || done_capacity < 0 || (step_capacity && (!tokens || !parents)) ||
        (done_capacity && !done))
        return e ? e->fail(DOTS_E_INVALID, "bad beam_read arguments") : DOTS_E_INVALID;
    int32_t B = 0, st = 0, nd = 0;
    RET(dots_beam_info(e, slot, &B, &st, &nd));
    const DotsEngine::BeamGroup& g = e->beams[e->beam_of[slot] - 1];
    hipStream_t s = e->stream;
    float cum_all[DOTS_MAX_BEAMS];
    CK(hipMemcpyAsync(cum_all, e->d_beam[e->beam_of[slot] - 1].cum, sizeof(cum_all), hipMemcpyDeviceToHost, s));
    const int take = std::min<int>(st, step_capacity);
    for (int i = 0; i < B && take > 0; ++i) {
        const size_t o = (size_t)g.slots[i] * e->cfg.max_seq_len;
        CK(hipMemcpyAsync(tokens + (size_t)i * step_capacity, e->out_ids + o, (size_t)take * 4, hipMemcpyDeviceToHost, s));
        CK(hipMemcpyAsync(parents + (size_t)i * step_capacity, e->beam_parent + o, (size_t)take * 4, hipMemcpyDeviceToHost, s));
    }
    CK(hipStreamSynchronize(s));
    std::copy(cum_all, cum_all + B, cum);
    for (int k = 0; k < std::min<int>(nd, done_capacity); ++k) {
        const BeamDone& r = g.done[k];
        done[4 * k] = r.step; done[4 * k + 1] = r.parent; done[4 * k + 2] = r.id;
        std::memcpy(done + 4 * k + 3, &r.s, 4);
    }
    *n_beams = B; *steps = st; *n_done = nd;
    return DOTS_OK;
}

}  // extern "C"
