// Sequence slots of the dots.ocr engine: the host side of the paged KV pool, the steps of admitting a slot and the continuous-batching
// C ABI (prefill into free slots, fork, decode chunks, poll / read / release).
#include "engine.h"
#include "score_plan.h"

namespace engine {
// ---- KV page allocator (host side; the kernels only ever see the block table)
hipError_t upload_table_row(DotsEngine* e, int slot) {
    return hipMemcpyAsync(e->block_table + (size_t)slot * e->max_pages, e->hp_table.data() + (size_t)slot * e->max_pages, (size_t)e->max_pages * 4,
                          hipMemcpyHostToDevice, e->stream);
}
// the host pages of a suspended slot go back to the host space, and the slot is suspended no more (its resident pages: release_pages)
static void drop_parked(DotsEngine* e, int slot) {
    DotsEngine::Parked& pk = e->parked[slot];
    if (!pk.on) return;
    for (int32_t v : pk.pages)
        if (v <= -2) { e->swap_used[-(v + 2)] = 0; e->swap_free += 1; }
    pk.pages.clear();
    pk.on = false;
    e->n_parked -= 1;
}
void swap_free_host(DotsEngine* e) {
    if (e->swap_host) hipHostFree(e->swap_host);
    e->swap_host = nullptr;
    e->swap_total = e->swap_free = 0;
    e->swap_used.clear();
}
// the slot lets go of every page its row names; a page goes back to the free list when its last holder lets go (dots_slots_fork shares pages).
// Of a suspended slot these are the pages that stayed resident, and its host pages go back too
void release_pages(DotsEngine* e, int slot) {
    if (slot < DOTS_MAX_BATCH) drop_parked(e, slot);
    drop_fill(e, slot);                                    // a filling slot's staged rows live in the rows of its pages: they go with them
    auto& mine = e->slot_pages[slot];
    for (auto it = mine.rbegin(); it != mine.rend(); ++it)
        if (--e->page_refs[*it] == 0) e->free_pages.push_back(*it);
    mine.clear();
    std::fill(e->hp_table.begin() + (size_t)slot * e->max_pages, e->hp_table.begin() + (size_t)(slot + 1) * e->max_pages, e->n_pool_pages);
}
// ---- the prefix cache's pages in the allocator: a page whose only holder is the index is as good as free.  Every place
// that counts free pages or takes one calls ensure_free first; with the cache off that is a null test
void ensure_free(DotsEngine* e, int64_t need) {
    if (!e->pc || free_count(e) < need) return;           // a request the pool cannot serve evicts nothing
    while ((int64_t)e->free_pages.size() < need) {
        const int32_t page = e->pc->evict_one();
        if (page < 0) return;
        e->free_pages.push_back(page);
    }
}
int free_count(const DotsEngine* e) { return (int)e->free_pages.size() + (e->pc ? e->pc->evictable_pages() : 0); }

// pages for `tokens` positions of the sequence in `slot` (it holds none yet); false: the pool cannot serve them
bool reserve_pages(DotsEngine* e, int slot, int tokens) {
    const int need = (tokens + 63) / 64;
    ensure_free(e, need);
    if (need > (int)e->free_pages.size() || need > e->max_pages) return false;
    auto& mine = e->slot_pages[slot];
    for (int p = 0; p < need; ++p) {
        mine.push_back(e->free_pages.back());
        e->free_pages.pop_back();
        e->page_refs[mine.back()] = 1;
        e->hp_table[(size_t)slot * e->max_pages + p] = mine.back();
    }
    return true;
}

// On-demand growth (continuous batching): make the sequence in `slot` own pages for `tokens` positions; returns the positions its pages
// cover afterwards (< tokens when the pool ran dry).  *changed: the block-table row has to be uploaded.
int grow_pages(DotsEngine* e, int slot, int tokens, bool* changed) {
    auto& mine = e->slot_pages[slot];
    const int need = std::min((tokens + 63) / 64, e->max_pages);
    ensure_free(e, std::min<int64_t>(need - (int64_t)mine.size(), free_count(e)));      // a pool that runs dry gives what it has
    while ((int)mine.size() < need && !e->free_pages.empty()) {
        e->hp_table[(size_t)slot * e->max_pages + mine.size()] = e->free_pages.back();
        mine.push_back(e->free_pages.back());
        e->page_refs[mine.back()] = 1;
        e->free_pages.pop_back();
        *changed = true;
    }
    return (int)mine.size() * 64;
}

// ---- the paging arithmetic of a decode chunk, shared by dots_slots_decode and dots_slots_pages_short.  n counts positions: n_steps x
// (spec_k + 1).  A step at context c writes KV position c and brings the sequence to c + 2 tokens, so n more steps need positions
// [0, ctx + n), and a sequence limited to slot_limit tokens never writes beyond position slot_limit - 2.
// does the chunk give this slot pages: a running sequence that is neither a beam-group row (fully reserved at creation, and the device owns
// its table row: DESIGN §6.9) nor suspended
static bool slot_grows(const DotsEngine* e, int b) { return e->slot_active[b] && !e->slot_done[b] && !e->beam_of[b] && !e->parked[b].on; }
static int chunk_want(const DotsEngine* e, int b, int n) { return std::min(e->slot_ctx_ub[b] + n, e->slot_limit[b] - 1); }
// pages the slot lacks for chunk_want positions (what grow_pages would take)
static int chunk_pages_lacking(const DotsEngine* e, int b, int n) {
    const int need = std::min((chunk_want(e, b, n) + 63) / 64, e->max_pages);
    return std::max(0, need - (int)e->slot_pages[b].size());
}

// tokens a slot sequence reserves at admission: its prompt plus the first page-worth of generated tokens (the rest on demand)
constexpr int KV_ADMIT_AHEAD = 64;
int admit_tokens(const DotsEngine* e, int prompt, int max_new) { return std::min(prompt + std::min(max_new, KV_ADMIT_AHEAD), e->cfg.max_seq_len); }

void share_pages(DotsEngine* e, int slot, const int32_t* pages, int n) {
    auto& mine = e->slot_pages[slot];
    for (int p = 0; p < n; ++p) {
        mine.push_back(pages[p]);
        e->page_refs[pages[p]] += 1;
        e->hp_table[(size_t)slot * e->max_pages + p] = pages[p];
    }
}

// ---- what admitting a slot consists of: one implementation of every step that prefill(), prefill_begin() / prefill_advance(),
// dots_slots_fork, dots_slots_beam and dots_slots_extend share
// slots[i] of a list of free destination slots, against the engine and the entries before it; src: the source slot of a fork or group
int check_free_slot(DotsEngine* e, const int32_t* slots, int i, int src, const char* src_of) {
    const int d = slots[i], mb = e->cfg.max_batch, usable = e->spec_k ? mb / (e->spec_k + 1) : mb;
    if (d < 0 || d >= mb) return e->fail(DOTS_E_INVALID, "slot %d out of range [0, %d)", d, mb);
    if (d >= usable)
        return e->fail(DOTS_E_CAPACITY, "slot %d is not usable while speculating: with %d drafts a slot takes %d rows of a step, so only slots [0, max_batch / (k + 1)) = [0, %d) are",
                       d, e->spec_k, e->spec_k + 1, usable);
    if (d == src) return e->fail(DOTS_E_INVALID, "slot %d is the source of the %s", d, src_of);
    if (slot_occupied(e, d)) return e->fail(DOTS_E_STATE, "slot %d is occupied", d);
    if (e->slot_mode && slot_filling(e, d)) return e->fail(DOTS_E_STATE, "slot %d is filling (dots_slots_prefill_begin)", d);
    for (int a = 0; a < i; ++a)
        if (slots[a] == d) return e->fail(DOTS_E_INVALID, "slot %d listed twice", d);
    return DOTS_OK;
}

// prompt b of a prefill: its length, then (slots given) its destination slot and its generation cap
int check_prompt(DotsEngine* e, int b, int len, const int32_t* slots, const int32_t* max_new) {
    const int msl = e->cfg.max_seq_len;
    if (len < 1 || len >= msl) return e->fail(DOTS_E_CAPACITY, "prompt %d length %d not in [1, max_seq_len)", b, len);
    if (!slots) return DOTS_OK;
    RET(check_free_slot(e, slots, b));
    if (max_new[b] < 1 || len + max_new[b] > msl)
        return e->fail(DOTS_E_CAPACITY, "slot %d: prompt (%d) + max_new_tokens (%d) exceeds max_seq_len %d", slots[b], len, max_new[b], msl);
    return DOTS_OK;
}

// the ids of one prompt as launch_embed_gather reads them: the id, or -(k) for the k-th row of `vis` counted in *vis_used (no_tower: the
// prompt runs no tower, its image rows come from the prefix cache — INT32_MIN)
int map_prompt(DotsEngine* e, const int32_t* ids, int n, bool no_tower, int32_t* src, int64_t* vis_used) {
    for (int i = 0; i < n; ++i) {
        const int id = ids[i];
        if (id == e->cfg.image_token_id) src[i] = no_tower ? INT32_MIN : -(int32_t)(++*vis_used);
        else if (id < 0 || id >= e->cfg.vocab_size) return e->fail(DOTS_E_INVALID, "token id %d out of range", id);
        else src[i] = id;
    }
    return DOTS_OK;
}
int check_vis_rows(DotsEngine* e, int64_t vis_used) {
    if (vis_used == (vis_used ? e->vis_rows : 0)) return DOTS_OK;
    return e->fail(DOTS_E_STATE, "prompt has %lld image tokens but the vision tower produced %lld rows", (long long)vis_used, (long long)e->vis_rows);
}

// slot mode with every slot free, every page in the pool and every device table row on the scratch page
int enter_slot_mode(DotsEngine* e) {
    for (int b = 0; b < (int)e->slot_pages.size(); ++b) release_pages(e, b);
    RET(beam_clear_all(e));
    CK(hipMemcpyAsync(e->block_table, e->hp_table.data(), e->hp_table.size() * 4, hipMemcpyHostToDevice, e->stream));
    std::fill(e->slot_active, e->slot_active + DOTS_MAX_BATCH, 0);
    CK(hipMemsetAsync(e->ctx_len, 0, e->cfg.max_batch * 4, e->stream));
    e->slot_mode = true;
    e->B = 0;                                              // the static-batch entry points need a static prefill first
    return DOTS_OK;
}

// The device state of rows going live, which the selection stage and the step after it read: context, generation cap, nothing generated,
// not finished, no drafts and the speculation counters from zero, logprob positions unset.  Resets beyond what a caller did before it
// called this: a beam group's rows get the speculation counters zeroed, which nothing can show (a group is refused while the engine
// speculates, and dots_set_speculation zeroes every counter).  clear_lp = false keeps what a group's rows do show: they return no
// logprobs, and dots_row_logprobs of one reads the positions of the row's previous occupant
int rows_go_live(DotsEngine* e, const std::vector<LiveRow>& rows, bool clear_lp) {
    hipStream_t s = e->stream;
    e->hp_live = rows;
    for (const LiveRow& r : e->hp_live) {
        CK(hipMemcpyAsync(e->ctx_len + r.slot, &r.ctx, 4, hipMemcpyHostToDevice, s));
        CK(hipMemcpyAsync(e->d_max_len + r.slot, &r.cap, 4, hipMemcpyHostToDevice, s));
        CK(hipMemsetAsync(e->out_lens + r.slot, 0, 4, s));
        RET(stream_restart_row(e, r.slot));
        CK(hipMemsetAsync(e->finished + r.slot, 0, 4, s));
        if (e->sp_ndraft) {
            CK(hipMemsetAsync(e->sp_ndraft + r.slot, 0, 4, s));
            CK(hipMemsetAsync(e->sp_stats + (size_t)r.slot * 3, 0, 3 * sizeof(unsigned long long), s));
        }
        if (e->pr_stats) {                                  // a prediction the slot holds is aligned with the start of the new output
            CK(hipMemsetAsync(e->pr_cur + r.slot, 0, 4, s));
            CK(hipMemsetAsync(e->pr_at + r.slot, 0, 4, s));
            CK(hipMemsetAsync(e->pr_src + r.slot, 0, 4, s));
            CK(hipMemsetAsync(e->pr_seen + r.slot, 0, 4, s));
            CK(hipMemsetAsync(e->pr_stats + (size_t)r.slot * 2, 0, 2 * sizeof(unsigned long long), s));
        }
        if (clear_lp) RET(clear_lp_row(e, r.slot));
    }
    return DOTS_OK;
}

// the mask of the next first-token selection: these rows only; d_list (p_dst or nullptr) gets their slots in order.  *n_rows: the rows
// the lm_head and the selection stage run over
int stage_new_rows(DotsEngine* e, const std::vector<LiveRow>& rows, int32_t* d_list, int* n_rows) {
    e->hp_new.assign(2 * DOTS_MAX_BATCH, 0);
    *n_rows = 0;
    for (size_t i = 0; i < rows.size(); ++i) {
        e->hp_new[rows[i].slot] = 1;
        e->hp_new[DOTS_MAX_BATCH + i] = rows[i].slot;
        *n_rows = std::max(*n_rows, rows[i].slot + 1);
    }
    CK(hipMemcpyAsync(e->d_sel_new, e->hp_new.data(), DOTS_MAX_BATCH * 4, hipMemcpyHostToDevice, e->stream));
    if (d_list) CK(hipMemcpyAsync(d_list, e->hp_new.data() + DOTS_MAX_BATCH, rows.size() * 4, hipMemcpyHostToDevice, e->stream));
    return DOTS_OK;
}

// the automata of the rows that hold a guide start over (the first token is selected under the guide), and so do their stop automata,
// whose hit records are cleared: the first token's bytes are the first ones walked; and so do the run counters of the rows with a loop rule.  d_rows: device list of n rows, nullptr = rows [0, n)
int restart_automata(DotsEngine* e, const int32_t* d_rows, int n, bool stops) {
    if (e->stage.rows(ROW_GUIDE) > 0) CK(launch_guide_reset_rows(e->stream, e->d_guides, d_rows, n));
    if (stops && e->stage.rows(ROW_STOP) > 0) CK(launch_stop_reset_rows(e->stream, e->d_stop, d_rows, n));
    // the loop guard's window is the output since it last started over: counters zeroed, no hit
    if (e->stage.rows(ROW_LOOP) > 0) CK(launch_loop_reset_rows(e->stream, e->d_loop, e->loop_run, d_rows, n));
    return DOTS_OK;
}

// the first tokens: final norm and lm_head over the rows of h (nullptr: the logits are in place), then the selection stage over the mask
// of stage_new_rows
int select_first_tokens(DotsEngine* e, int rows, const bf16_t* h, bf16_t* xn) {
    const DotsConfig& c = e->cfg;
    if (h) CK(launch_dec_lmhead(e->stream, h, e->final_norm, e->lm_head_d, e->lm_head_s, e->d_logits, rows, c.hidden_size, c.vocab_size, c.rms_norm_eps, 0, xn));
    e->B_sel = rows;
    e->sel_now = e->d_sel_new;
    return select_tokens(e, 0);
}

// the host record of live slots; occupy = false: the slots are occupied already (an extend)
void mark_live(DotsEngine* e, const LiveRow* rows, int n, bool occupy) {
    for (int i = 0; i < n; ++i) {
        const int b = rows[i].slot;
        if (occupy) e->slot_active[b] = 1;
        e->slot_limit[b] = rows[i].ctx + rows[i].cap;
        e->slot_prompt[b] = rows[i].ctx;
        e->slot_ctx_ub[b] = rows[i].ctx;
        e->slot_done[b] = 0;
        e->sc_n[b] = 0;                                     // whatever a score recorded belongs to the sequence before
    }
    e->sel_dirty = true;
}

// the device's finished / out_lens as a poll reports them, and what the host record takes from them
void poll_host_state(DotsEngine* e, int32_t* finished, int32_t* out_lens) {
    const int mb = e->cfg.max_batch;
    for (int b = 0; b < mb; ++b) {
        if (e->slot_mode && e->fill[b].on) { finished[b] = 3; out_lens[b] = 0; }             // filling (dots_slots_prefill_begin): nothing generated yet
        else if (!e->slot_mode || !e->slot_active[b]) { finished[b] = -1; out_lens[b] = 0; }      // -1: free slot
        else if (e->parked[b].on) finished[b] = 2;                                           // suspended: out_lens as they stood at suspend
        else {
            if (finished[b]) e->slot_done[b] = 1;                                            // takes no more pages
            // every issued step has run: the context is prompt + generated - 1 exactly.  A speculating step advances a row by 1 .. k + 1
            // positions, so dots_slots_decode counts k + 1 per step; without this the bound (and the pages taken ahead) would run away
            if (e->spec_k) e->slot_ctx_ub[b] = std::min(e->slot_ctx_ub[b], e->slot_prompt[b] + out_lens[b] - 1);
        }
    }
}
}  // namespace engine

using namespace engine;
extern "C" {
// ---------------------------------------------------------------------------------- continuous batching
int dots_set_eos(DotsEngine* e, const int32_t* eos_ids, int n_eos) {
    if (!e) return DOTS_E_INVALID;
    if (n_eos < 0 || n_eos > 16 || (n_eos && !eos_ids)) return e->fail(DOTS_E_INVALID, "n_eos must be in [0,16]");
    CK(hipSetDevice(e->device));
    if (n_eos) CK(hipMemcpyAsync(e->eos_ids, eos_ids, n_eos * 4, hipMemcpyHostToDevice, e->stream));
    CK(hipStreamSynchronize(e->stream));
    e->n_eos = n_eos;
    std::copy(eos_ids, eos_ids + n_eos, e->h_eos);
    return DOTS_OK;
}

int dots_slots_prefill(DotsEngine* e, const int32_t* slots, int n, const int32_t* input_ids, const int32_t* prompt_lens,
                       const int32_t* max_new_tokens) {
    if (!e) return DOTS_E_INVALID;
    if (!e->finalized) return e->fail(DOTS_E_STATE, "weights not finalized");
    if (!slots || !input_ids || !prompt_lens || !max_new_tokens) return e->fail(DOTS_E_INVALID, "null argument");
    CK(hipSetDevice(e->device));
    return prefill(e, input_ids, prompt_lens, n, slots, max_new_tokens);
}

// Chunked prefill: begin reserves and stages, every advance fills up to max_tokens positions
int dots_slots_prefill_begin(DotsEngine* e, const int32_t* slots, int n, const int32_t* input_ids, const int32_t* prompt_lens,
                             const int32_t* max_new_tokens) {
    if (!e) return DOTS_E_INVALID;
    if (!e->finalized) return e->fail(DOTS_E_STATE, "weights not finalized");
    if (!slots || !input_ids || !prompt_lens || !max_new_tokens) return e->fail(DOTS_E_INVALID, "null argument");
    CK(hipSetDevice(e->device));
    return prefill_begin(e, input_ids, prompt_lens, n, slots, max_new_tokens);
}

int dots_slots_prefill_advance(DotsEngine* e, int max_tokens, int32_t* remaining) {
    if (!e) return DOTS_E_INVALID;
    if (!e->finalized) return e->fail(DOTS_E_STATE, "weights not finalized");
    if (!remaining) return e->fail(DOTS_E_INVALID, "null argument");
    CK(hipSetDevice(e->device));
    return prefill_advance(e, max_tokens, remaining);
}

// ---------------------------------------------------------------------------------- prefix cache
int dots_prefix_cache_enable(DotsEngine* e, int on) {
    if (!e) return DOTS_E_INVALID;
    if (!e->finalized) return e->fail(DOTS_E_STATE, "weights not finalized");
    if (e->spec_k) return e->fail(DOTS_E_STATE, "the prefix cache cannot be used while the engine speculates (dots_set_speculation)");
    for (int b = 0; b < e->cfg.max_batch; ++b)
        if ((e->slot_mode && e->slot_active[b]) || slot_filling(e, b))
            return e->fail(DOTS_E_STATE, "the prefix cache cannot change while slot %d is occupied or filling", b);
    if (on && !e->pc) e->pc = new prefix_cache::Index(&e->page_refs, e->n_pool_pages, e->cfg.image_token_id);
    if (!on && e->pc) {
        e->pc->clear(&e->free_pages);
        delete e->pc;
        e->pc = nullptr;
    }
    return DOTS_OK;
}

int dots_prefix_cache_lookup(DotsEngine* e, const int32_t* ids, int len, const uint8_t* image_key, int32_t* lease, int32_t* hit_tokens, int32_t* needs_tower) {
    if (!e) return DOTS_E_INVALID;
    if (!ids || !lease || !hit_tokens || !needs_tower) return e->fail(DOTS_E_INVALID, "null argument");
    if (!e->pc) return e->fail(DOTS_E_STATE, "the prefix cache is off (dots_prefix_cache_enable)");
    if (len < 1 || len >= e->cfg.max_seq_len) return e->fail(DOTS_E_CAPACITY, "prompt length %d not in [1, max_seq_len)", len);
    *lease = *hit_tokens = 0;
    if (!e->pc->eligible(ids, len, image_key)) {           // bypass: not looked up, not counted
        *needs_tower = prefix_cache::find_pads(ids, len, e->cfg.image_token_id).n > 0;
        return DOTS_OK;
    }
    int hit = 0, tower = 0;
    *lease = e->pc->lookup(ids, len, image_key, &hit, &tower);
    *hit_tokens = hit;
    *needs_tower = tower;
    return DOTS_OK;
}

int dots_prefix_cache_release(DotsEngine* e, int32_t lease) {
    if (!e) return DOTS_E_INVALID;
    if (!e->pc) return e->fail(DOTS_E_STATE, "the prefix cache is off (dots_prefix_cache_enable)");
    if (!e->pc->release(lease)) return e->fail(DOTS_E_INVALID, "lease %d is not held", lease);
    return DOTS_OK;
}

int dots_slots_prefill_begin_cached(DotsEngine* e, const int32_t* slots, int n, const int32_t* input_ids, const int32_t* prompt_lens,
                                    const int32_t* max_new_tokens, const int32_t* leases, const uint8_t* const* image_keys) {
    if (!e) return DOTS_E_INVALID;
    if (!e->finalized) return e->fail(DOTS_E_STATE, "weights not finalized");
    if (!slots || !input_ids || !prompt_lens || !max_new_tokens || !leases || !image_keys) return e->fail(DOTS_E_INVALID, "null argument");
    CK(hipSetDevice(e->device));
    return prefill_begin(e, input_ids, prompt_lens, n, slots, max_new_tokens, leases, image_keys);
}

int dots_prefix_cache_info(DotsEngine* e, int64_t* out6) {
    if (!e || !out6) return e ? e->fail(DOTS_E_INVALID, "null argument") : DOTS_E_INVALID;
    if (!e->pc) return e->fail(DOTS_E_STATE, "the prefix cache is off (dots_prefix_cache_enable)");
    const prefix_cache::Info& i = e->pc->info();
    out6[0] = i.lookups; out6[1] = i.hit_tokens; out6[2] = i.inserted; out6[3] = i.evicted;
    out6[4] = e->pc->resident_pages(); out6[5] = e->pc->evictable_pages();
    return DOTS_OK;
}

// Parallel sampling: n free slots become copies of the freshly prefilled sequence in src_slot.  Everything is validated and
// counted before anything changes; the children then share the source's full prompt pages (reference counts), get a copy of its tail page
// and select their own first token from the source's last-position logits.
int dots_slots_fork(DotsEngine* e, int src_slot, const int32_t* dst_slots, int n) {
    if (!e) return DOTS_E_INVALID;
    if (!e->finalized) return e->fail(DOTS_E_STATE, "weights not finalized");
    if (!dst_slots || n < 1 || n >= DOTS_MAX_BATCH) return e->fail(DOTS_E_INVALID, "dots_slots_fork: n must be in [1, %d) and dst_slots given", DOTS_MAX_BATCH);
    const DotsConfig& c = e->cfg;
    const int mb = c.max_batch, V = c.vocab_size;
    if (src_slot < 0 || src_slot >= mb) return e->fail(DOTS_E_INVALID, "source slot %d out of range [0, %d)", src_slot, mb);
    const auto fresh = std::find(e->fresh_slots.begin(), e->fresh_slots.end(), src_slot);
    if (!e->slot_mode || !e->slot_active[src_slot] || fresh == e->fresh_slots.end() || slot_parked(e, src_slot))
        return e->fail(DOTS_E_STATE, "slot %d cannot be forked: only a sequence of the most recent dots_slots_prefill, before any decode step", src_slot);
    for (int i = 0; i < n; ++i) RET(check_free_slot(e, dst_slots, i, src_slot, "fork"));
    // ---- page arithmetic: the children name the source's floor(L / 64) full prompt pages and own the rest of the admission reserve
    const int L = e->slot_prompt[src_slot], max_new = e->slot_limit[src_slot] - L;
    const int shared = L / 64, own = (admit_tokens(e, L, max_new) + 63) / 64 - shared;          // own >= 1: the reserve is at least L + 1 tokens
    const auto& src_pages = e->slot_pages[src_slot];
    if ((int)src_pages.size() < shared + (L % 64 ? 1 : 0)) return e->fail(DOTS_E_STATE, "slot %d does not hold its prompt pages", src_slot);
    ensure_free(e, (int64_t)n * own);
    if (shared + own > e->max_pages || (int64_t)n * own > (int64_t)e->free_pages.size())
        return e->fail(DOTS_E_CAPACITY, "KV pool exhausted: %d forked sequences need %d pages of 64 tokens each, %d of %d are free", n, own,
                       free_count(e), e->n_pool_pages);
    CK(hipSetDevice(e->device));
    hipStream_t s = e->stream;
    // ---- from here on the call changes state; a failed launch gives the children's pages back (the slots are not marked occupied yet)
    PageGuard guard{e, dst_slots, n, true};
    int32_t stage[3 * DOTS_MAX_BATCH] = {0};
    std::vector<LiveRow> live(n);
    for (int i = 0; i < n; ++i) {
        const int d = dst_slots[i];
        share_pages(e, d, src_pages.data(), shared);       // every row appends at positions >= L
        bool changed = false;
        grow_pages(e, d, (shared + own) * 64, &changed);   // cannot fall short: counted above
        CK(upload_table_row(e, d));
        stage[i] = d;
        stage[DOTS_MAX_BATCH + i] = e->slot_pages[d][shared];
        live[i] = LiveRow{d, L, max_new};
    }
    stage[2 * DOTS_MAX_BATCH] = L - 1;
    CK(hipMemcpyAsync(e->fk_dev, stage, sizeof(stage), hipMemcpyHostToDevice, s));
    const int32_t *fk_dst = e->fk_dev, *fk_pages = e->fk_dev + DOTS_MAX_BATCH, *fk_last = e->fk_dev + 2 * DOTS_MAX_BATCH;
    // the tail page: behind the prefill's page writers on the same stream; its source is written by nobody until the source's first step
    if (L % 64) CK(launch_kv_fork_pages(s, e->pool, e->pool_layer_elems * 2, kv_page_bytes(e), c.num_layers, src_pages[shared], fk_pages, n));
    RET(rows_go_live(e, live));
    // the source's last-position logits row (rows of d_logits are slots; nothing has run over them since the prefill)
    for (int i = 0; i < n; ++i)
        CK(hipMemcpyAsync(e->d_logits + (size_t)dst_slots[i] * V, e->d_logits + (size_t)src_slot * V, (size_t)V * 4, hipMemcpyDeviceToDevice, s));
    int rows = 0;
    RET(stage_new_rows(e, live, nullptr, &rows));
    if (e->pen_cnt && e->fresh_chunked) {
        // a source filled in passes: p_src holds its last pass only, but its own presence bits are the whole prompt's and nothing has been counted yet
        const size_t W = (size_t)(V + 31) / 32;
        for (int i = 0; i < n; ++i) {
            CK(hipMemsetAsync(e->pen_cnt + (size_t)dst_slots[i] * V, 0, (size_t)V * 4, s));
            CK(hipMemcpyAsync(e->pen_seen + dst_slots[i] * W, e->pen_seen + src_slot * W, W * 4, hipMemcpyDeviceToDevice, s));
        }
    } else if (e->pen_cnt) {
        // prompt-presence bits and zeroed counts of every child from the source's packed prompt, still in p_src: one sequence per launch,
        // so that each starts at the source's first token
        const int b = (int)(fresh - e->fresh_slots.begin());
        const int32_t* src0 = e->p_src + (b ? e->hp_last[b - 1] + 1 : 0);
        for (int i = 0; i < n; ++i) CK(launch_pen_prompt(s, src0, fk_last, fk_dst + i, 1, c.image_token_id, V, e->pen_cnt, e->pen_seen));
    }
    const bool inherits = e->stage.has(src_slot, ROW_STOP);
    RET(restart_automata(e, fk_dst, n, !inherits));
    if (inherits) {
        // the children inherit the source's stop strings (automaton and min_tokens) at the root with no hit: one launch writes all their entries
        for (int i = 0; i < n; ++i) RET(hold_row_stop(e, dst_slots[i], e->row_stop[src_slot] - 1, e->row_stop_min[src_slot]));
        CK(launch_stop_fork_rows(s, e->d_stop, src_slot, fk_dst, n));
    }
    if (e->stage.has(src_slot, ROW_LOOP)) {
        // ... and its loop rule, with no hit and the counters at zero: what an independent request holds before its first token
        for (int i = 0; i < n; ++i) RET(hold_row_loop(e, dst_slots[i], e->row_loop[src_slot]));
        CK(launch_loop_fork_rows(s, e->d_loop, e->loop_run, src_slot, fk_dst, n));
    }
    CK(hipStreamSynchronize(s));                           // `stage` is a stack array
    // ---- the children's first tokens, from the logits in place
    RET(select_first_tokens(e, rows, nullptr));
    mark_live(e, live.data(), n);
    guard.armed = false;
    return DOTS_OK;
}

// More prompt tokens behind live sequences.  Everything is validated and counted before anything changes; the packed rows
// then run through the layer loop of a decode step in chunks of at most max_batch rows, and the slots end as slots prefilled with the
// longer prompt, their first token selected from the logits of their last fed row.
//
// top_n != nullptr: the call scores (dots_slots_score).  The same checks, page arithmetic and launches, and per chunk an
// lm_head over all its rows into the scoring logits scratch and the logprob stage of score.hip over the rows that record an entry
// (score_plan.h).  An extend (top_n == nullptr) launches and allocates nothing of that.
namespace {
int extend_slots(DotsEngine* e, const char* call, const int32_t* slots, int n, const int32_t* ids, const int32_t* lens, const int32_t* keep_pending,
                 const int32_t* max_new_tokens, const int32_t* top_n) {
    const DotsConfig& c = e->cfg;
    const int mb = c.max_batch, V = c.vocab_size, H = c.hidden_size;
    if (n < 1 || n > mb) return e->fail(DOTS_E_INVALID, "%s: n must be in [1, %d]", call, mb);
    if (!e->slot_mode) return e->fail(DOTS_E_STATE, "%s: the engine runs a static batch; only a slot sequence can be extended", call);
    if (e->spec_k) return e->fail(DOTS_E_STATE, "a slot cannot be extended while the engine speculates (dots_set_speculation)");
    int64_t n_ids = 0;
    for (int i = 0; i < n; ++i) {
        const int b = slots[i];
        if (b < 0 || b >= mb) return e->fail(DOTS_E_INVALID, "slot %d out of range [0, %d)", b, mb);
        if (!e->slot_active[b]) return e->fail(DOTS_E_STATE, "slot %d is not occupied", b);
        if (e->parked[b].on) return e->fail(DOTS_E_STATE, "slot %d is suspended: resume it first", b);
        if (e->beam_of[b]) return e->fail(DOTS_E_STATE, "slot %d is a row of a beam group: a group cannot be extended", b);
        for (int a = 0; a < i; ++a)
            if (slots[a] == b) return e->fail(DOTS_E_INVALID, "slot %d listed twice", b);
        if (lens[i] < 1) return e->fail(DOTS_E_INVALID, "slot %d: at least one token must be fed, got %d", b, lens[i]);
        if (max_new_tokens[i] < 1) return e->fail(DOTS_E_INVALID, "slot %d: max_new_tokens must be >= 1, got %d", b, max_new_tokens[i]);
        if (top_n && (top_n[i] < 0 || top_n[i] > DOTS_MAX_TOP_LOGPROBS))
            return e->fail(DOTS_E_INVALID, "slot %d: top_n must be in [0, %d], got %d", b, DOTS_MAX_TOP_LOGPROBS, top_n[i]);
        if (top_n && e->stage.has(b, ROW_LOOP))
            return e->fail(DOTS_E_STATE, "slot %d carries a loop guard: a scored row selects nothing it could guard (clear it first: dots_set_row_loop(row, NULL))", b);
        if (e->stage.has(b, ROW_PARAMS) && e->row_pen[b])
            return e->fail(DOTS_E_STATE, "slot %d carries a penalty: its prompt-presence image would have to absorb the earlier output, so it cannot be extended", b);
        for (int j = 0; j < lens[i]; ++j) {
            const int id = ids[n_ids + j];
            if (id < 0 || id >= V) return e->fail(DOTS_E_INVALID, "token id %d out of range", id);
            if (id == c.image_token_id) return e->fail(DOTS_E_INVALID, "slot %d: an image token cannot be fed by an extend (the vision rows enter at the prefill)", b);
        }
        n_ids += lens[i];
    }
    if (top_n && V > LP_MAX_V) return e->fail(DOTS_E_INVALID, "logprobs support vocabularies up to %d", LP_MAX_V);
    CK(hipSetDevice(e->device));
    hipStream_t s = e->stream;
    // ---- the true contexts (slot_ctx_ub is only a bound once a row has finished early), then the page arithmetic, before anything changes
    int32_t ctx[DOTS_MAX_BATCH] = {0};
    CK(hipMemcpyAsync(ctx, e->ctx_len, (size_t)mb * 4, hipMemcpyDeviceToHost, s));
    CK(hipStreamSynchronize(s));
    int fed[DOTS_MAX_BATCH], new_prompt[DOTS_MAX_BATCH], old_pages[DOTS_MAX_BATCH];
    int64_t n_rows = 0, lacking = 0;
    for (int i = 0; i < n; ++i) {
        const int b = slots[i], cb = ctx[b];
        fed[i] = lens[i] + (keep_pending[i] ? 1 : 0);
        new_prompt[i] = cb + fed[i];
        const auto& mine = e->slot_pages[b];
        old_pages[i] = (int)mine.size();
        if (cb < 1 || (cb + 63) / 64 > (int)mine.size())
            return e->fail(DOTS_E_STATE, "slot %d: context %d is not covered by its %d pages", b, cb, (int)mine.size());
        if ((int64_t)new_prompt[i] + max_new_tokens[i] > c.max_seq_len)
            return e->fail(DOTS_E_CAPACITY, "slot %d: extended prompt (%d + %d) + max_new_tokens (%d) exceeds max_seq_len %d", b, cb, fed[i], max_new_tokens[i],
                           c.max_seq_len);
        // every fed position is written: its page must be the row's alone (the shared prompt pages of a fork all lie below the context)
        for (int p = cb / 64; p < (int)mine.size(); ++p)
            if (e->page_refs[mine[p]] != 1) return e->fail(DOTS_E_STATE, "slot %d: page %d of its row has other holders and cannot be written", b, p);
        const int need = std::min((admit_tokens(e, new_prompt[i], max_new_tokens[i]) + 63) / 64, e->max_pages);
        if (need * 64 < new_prompt[i]) return e->fail(DOTS_E_CAPACITY, "slot %d: %d tokens exceed the block table", b, new_prompt[i]);
        lacking += std::max(0, need - (int)mine.size());
        n_rows += fed[i];
    }
    ensure_free(e, lacking);
    if (lacking > (int64_t)e->free_pages.size())
        return e->fail(DOTS_E_CAPACITY, "KV pool exhausted: the extended sequences need %d more pages of 64 tokens, %d of %d are free", (int)lacking,
                       free_count(e), e->n_pool_pages);
    // ---- the call's device buffers (nothing of the slots changes if one cannot be had)
    if (!e->ex_tokens) CK(e->alloc(&e->ex_tokens, DOTS_MAX_BATCH));
    if (!e->ex_ctx) CK(e->alloc(&e->ex_ctx, DOTS_MAX_BATCH));
    if (!e->ex_table) CK(e->alloc(&e->ex_table, (size_t)DOTS_MAX_BATCH * e->max_pages));
    if (!e->ex_h) CK(e->alloc(&e->ex_h, (size_t)DOTS_MAX_BATCH * H));
    const size_t n_stage = (top_n ? 6 : 3) * (size_t)n_rows + 5 * (size_t)n;
    bool any_top = false;
    for (int i = 0; top_n && i < n; ++i) any_top |= top_n[i] > 0;
    if (top_n) {
        const size_t K = DOTS_MAX_TOP_LOGPROBS, pos = (size_t)mb * c.max_seq_len;
        if (!e->sc_logits) CK(e->alloc(&e->sc_logits, (size_t)mb * V));
        if (!e->sc_ms) CK(e->alloc(&e->sc_ms, (size_t)mb * LP_CHUNKS * 2));
        if (!e->sc_pv) CK(e->alloc(&e->sc_pv, (size_t)mb * LP_CHUNKS * K));
        if (!e->sc_pi) CK(e->alloc(&e->sc_pi, (size_t)mb * LP_CHUNKS * K));
        if (!e->sc_tok) {
            CK(e->alloc(&e->sc_tok, pos));
            CK(hipMemsetAsync(e->sc_tok, 0xFF, pos * 4, s));
        }
        if (any_top && !e->sc_ids) {
            CK(e->alloc(&e->sc_ids, pos * K));
            CK(hipMemsetAsync(e->sc_ids, 0xFF, pos * K * 4, s));
        }
        if (any_top && !e->sc_top) {
            CK(e->alloc(&e->sc_top, pos * K));
            CK(hipMemsetAsync(e->sc_top, 0xFF, pos * K * 4, s));
        }
    }
    if (e->ex_stage_cap < n_stage) {
        CK(hipStreamSynchronize(s));
        e->release(e->ex_stage);
        e->ex_stage = nullptr;
        e->ex_stage_cap = 0;
        CK(e->alloc(&e->ex_stage, n_stage));
        e->ex_stage_cap = n_stage;
    }
    // packed rows, slot by slot in the caller's order: (slot, offset from the slot's context, token or -1 = its pending token); then the
    // per-slot lists; then, in chunk order, the step row that holds a slot's last fed token and the slot it belongs to; then, of a score,
    // per packed row the entry it records, its target and its slot's top_n
    std::vector<int32_t> st(n_stage);
    int32_t *h_slot = st.data(), *h_off = h_slot + n_rows, *h_tok = h_off + n_rows, *h_slots = h_tok + n_rows, *h_fed = h_slots + n, *h_new = h_fed + n,
            *h_gsrc = h_new + n, *h_gdst = h_gsrc + n, *h_entry = top_n ? h_gdst + n : nullptr, *h_target = top_n ? h_entry + n_rows : nullptr,
            *h_topn = top_n ? h_target + n_rows : nullptr;
    std::vector<int> chunk_g0((size_t)(n_rows + mb - 1) / mb + 1, 0);
    std::vector<LiveRow> live(n);
    int rows = 0;
    {
        extend_pack_rows(slots, ids, lens, keep_pending, n, h_slot, h_off, h_tok);
        int64_t r = 0;
        int g = 0;
        for (int i = 0; i < n; ++i) {
            r += fed[i];
            if (top_n) std::fill(h_topn + (r - fed[i]), h_topn + r, top_n[i]);
            h_slots[i] = slots[i]; h_fed[i] = fed[i]; h_new[i] = max_new_tokens[i];
            h_gsrc[g] = (int32_t)((r - 1) % mb); h_gdst[g] = slots[i];      // slots end in row order, so the lists are in chunk order
            chunk_g0[(size_t)((r - 1) / mb) + 1] = ++g;
            live[i] = LiveRow{slots[i], new_prompt[i], max_new_tokens[i]};
        }
        for (size_t k = 1; k < chunk_g0.size(); ++k) chunk_g0[k] = std::max(chunk_g0[k], chunk_g0[k - 1]);
        if (top_n) score_plan_rows(h_slot, h_off, h_tok, n_rows, h_entry, h_target);
    }
    CK(hipMemcpyAsync(e->ex_stage, st.data(), n_stage * 4, hipMemcpyHostToDevice, s));
    RET(stage_new_rows(e, live, nullptr, &rows));
    CK(hipStreamSynchronize(s));                             // the staged lists are local variables
    const int32_t *d_slot = e->ex_stage, *d_off = d_slot + n_rows, *d_tok = d_off + n_rows, *d_slots = d_tok + n_rows, *d_fed = d_slots + n,
                  *d_new = d_fed + n, *d_gsrc = d_new + n, *d_gdst = d_gsrc + n, *d_entry = top_n ? d_gdst + n : nullptr,
                  *d_target = top_n ? d_entry + n_rows : nullptr, *d_topn = top_n ? d_target + n_rows : nullptr;
    // ---- from here on the call changes state; a failed launch gives the new pages back
    struct ExtendGuard {
        DotsEngine* e; const int32_t* slots; const int* old_pages; int n; bool armed = true;
        ~ExtendGuard() {
            if (!armed) return;
            for (int i = 0; i < n; ++i) {
                auto& mine = e->slot_pages[slots[i]];
                while ((int)mine.size() > old_pages[i]) {
                    e->page_refs[mine.back()] = 0;
                    e->free_pages.push_back(mine.back());
                    mine.pop_back();
                    e->hp_table[(size_t)slots[i] * e->max_pages + mine.size()] = e->n_pool_pages;
                }
                (void)upload_table_row(e, slots[i]);
            }
        }
    } guard{e, slots, old_pages, n};
    for (int i = 0; i < n; ++i) {
        bool changed = false;
        grow_pages(e, slots[i], admit_tokens(e, new_prompt[i], max_new_tokens[i]), &changed);      // cannot fall short: counted above
        if (changed) CK(upload_table_row(e, slots[i]));
    }
    e->fresh_slots.clear();                                  // the call overwrites the logits a fork selects from: a fork comes before an extend
    const ExtendRows ex{d_slot, d_off, d_tok, e->ex_tokens, e->ex_ctx, e->ex_table};
    const ScoreRows sr{d_slot, d_entry, d_target, d_topn};
    const LogprobState sc_ls{nullptr, nullptr, nullptr, nullptr, nullptr, e->sc_ms, e->sc_pv, e->sc_pi, nullptr, e->sc_tok, e->sc_ids, e->sc_top, c.max_seq_len};
    if (top_n) {
        // the slots' entries of an earlier score are gone whatever happens from here on
        const size_t L = (size_t)c.max_seq_len, K = DOTS_MAX_TOP_LOGPROBS;
        for (int i = 0; i < n; ++i) {
            e->sc_n[slots[i]] = 0;
            CK(hipMemsetAsync(e->sc_tok + slots[i] * L, 0xFF, L * 4, s));
            if (e->sc_ids) CK(hipMemsetAsync(e->sc_ids + slots[i] * L * K, 0xFF, L * K * 4, s));
            if (e->sc_top) CK(hipMemsetAsync(e->sc_top + slots[i] * L * K, 0xFF, L * K * 4, s));
        }
    }
    const int n_splits = splits_for_ctx(c.max_seq_len);
    for (int64_t r0 = 0, k = 0; r0 < n_rows; r0 += mb, ++k) {
        const int cn = (int)std::min<int64_t>(mb, n_rows - r0);
        CK(launch_extend_expand(s, ex, (int)r0, cn, cn, e->cur_tokens, e->ctx_len, e->finished, e->out_ids, e->out_lens, c.max_seq_len, e->block_table,
                                e->max_pages, e->n_pool_pages));
        bool pend = false;
        const float* pend_scale = nullptr;
        RET(decode_layers(e, e->ex_tokens, e->ex_ctx, e->ex_table, cn, n_splits, 0, &pend, &pend_scale));
        const int g0 = chunk_g0[k], g1 = chunk_g0[k + 1];
        const bool records = top_n && score_chunk_records(h_entry, r0, cn);
        if (g1 == g0 && !records) continue;                  // no slot's last token is in this chunk: nothing reads its residual rows
        // the lm_head's prologue would apply the pending K-quarter sums of the last down_proj; the gather needs the finished rows
        if (pend) CK(launch_dec_norm_ximg(s, e->d_h, nullptr, nullptr, cn, H, c.rms_norm_eps, e->d_part_h, pend_scale));
        if (g1 > g0) CK(launch_gather_rows(s, e->d_h, d_gsrc + g0, d_gdst + g0, e->ex_h, g1 - g0, H));
        if (!records) continue;
        // ---- a score: every row's logits (row r of the scratch = packed row r0 + r), then the entries of the rows that record one
        CK(launch_dec_lmhead(s, e->d_h, e->final_norm, e->lm_head_d, e->lm_head_s, e->sc_logits, cn, H, V, c.rms_norm_eps, 0, e->d_xn));
        CK(launch_score_logprob_partial(s, e->sc_logits, V, V, sr, (int)r0, cn, sc_ls));
        CK(launch_score_logprob_final(s, e->sc_logits, V, V, sr, (int)r0, cn, sc_ls));
    }
    // ---- the slots' state: that of slots prefilled with the longer prompt
    CK(launch_extend_commit(s, d_slots, d_fed, d_new, n, e->ctx_len, e->out_lens, e->finished, e->d_max_len));
    for (int i = 0; i < n; ++i) {
        RET(clear_lp_row(e, slots[i]));
        RET(stream_restart_row(e, slots[i]));                // extend_commit_kernel zeroed out_lens
    }
    RET(restart_automata(e, d_slots, n));
    // ---- the first tokens of the new turn: lm_head over the slots' last fed rows, the selection stage over a mask of the extended slots only
    RET(select_first_tokens(e, rows, e->ex_h, e->d_xn));
    CK(hipStreamSynchronize(s));
    mark_live(e, live.data(), n, false);
    for (int i = 0; top_n && i < n; ++i) e->sc_n[slots[i]] = fed[i];        // 1 + (fed - 1) entries
    guard.armed = false;
    return DOTS_OK;
}
}  // namespace

int dots_slots_extend(DotsEngine* e, const int32_t* slots, int n, const int32_t* ids, const int32_t* lens, const int32_t* keep_pending,
                      const int32_t* max_new_tokens) {
    if (!e) return DOTS_E_INVALID;
    if (!e->finalized) return e->fail(DOTS_E_STATE, "weights not finalized");
    if (!slots || !ids || !lens || !keep_pending || !max_new_tokens) return e->fail(DOTS_E_INVALID, "null argument");
    return extend_slots(e, "dots_slots_extend", slots, n, ids, lens, keep_pending, max_new_tokens, nullptr);
}

// Given tokens scored on live sequences: an extend that records, for every fed row but a slot's last, the logprob entry of
// the next fed token
int dots_slots_score(DotsEngine* e, const int32_t* slots, int n, const int32_t* ids, const int32_t* lens, const int32_t* keep_pending,
                     const int32_t* max_new_tokens, const int32_t* top_n) {
    if (!e) return DOTS_E_INVALID;
    if (!e->finalized) return e->fail(DOTS_E_STATE, "weights not finalized");
    if (!slots || !ids || !lens || !keep_pending || !max_new_tokens || !top_n) return e->fail(DOTS_E_INVALID, "null argument");
    return extend_slots(e, "dots_slots_score", slots, n, ids, lens, keep_pending, max_new_tokens, top_n);
}

// Entries [pos0, pos0 + n) of the slot's row of the score record, cut to the row's max_seq_len entries; *n_out = how many the last score
// of the slot recorded (the entries from there on are 0xFF: NaN / -1)
int dots_slot_scores(DotsEngine* e, int slot, int pos0, int n, float* tok_lp_host, int32_t* top_ids_host, float* top_lp_host, int32_t* n_out) {
    if (!e || !n_out || pos0 < 0 || n < 0 || (n > 0 && (!tok_lp_host || !top_ids_host || !top_lp_host)))
        return e ? e->fail(DOTS_E_INVALID, "bad slot_scores arguments") : DOTS_E_INVALID;
    if (!slot_occupied(e, slot)) return e->fail(DOTS_E_STATE, "slot %d is not occupied", slot);
    if (!e->sc_n[slot] || !e->sc_tok) return e->fail(DOTS_E_STATE, "slot %d has not been scored since it was filled (dots_slots_score)", slot);
    const int take = std::max(0, std::min(n, e->cfg.max_seq_len - pos0));
    *n_out = e->sc_n[slot] - 1;
    if (take < n) return e->fail(DOTS_E_INVALID, "slot_scores: entries [%d, %d) exceed max_seq_len %d", pos0, pos0 + n, e->cfg.max_seq_len);
    if (take <= 0) return DOTS_OK;
    CK(hipSetDevice(e->device));
    const size_t K = DOTS_MAX_TOP_LOGPROBS, o = (size_t)slot * e->cfg.max_seq_len + pos0;
    CK(hipMemcpyAsync(tok_lp_host, e->sc_tok + o, (size_t)take * 4, hipMemcpyDeviceToHost, e->stream));
    if (e->sc_ids && e->sc_top) {
        CK(hipMemcpyAsync(top_ids_host, e->sc_ids + o * K, (size_t)take * K * 4, hipMemcpyDeviceToHost, e->stream));
        CK(hipMemcpyAsync(top_lp_host, e->sc_top + o * K, (size_t)take * K * 4, hipMemcpyDeviceToHost, e->stream));
    } else {
        // no call has asked for a top list yet.  What the lists would hold: -1 / NaN beyond top_n = 0 as lp_final_entry writes them in
        // the recorded entries, 0xFF behind them
        const size_t rec = (size_t)std::max(0, std::min(take, e->sc_n[slot] - 1 - pos0));
        std::fill(top_ids_host, top_ids_host + rec * K, -1);
        std::fill(top_lp_host, top_lp_host + rec * K, __builtin_nanf(""));
        memset(top_ids_host + rec * K, 0xFF, (take - rec) * K * 4);
        memset(top_lp_host + rec * K, 0xFF, (take - rec) * K * 4);
    }
    CK(hipStreamSynchronize(e->stream));
    return DOTS_OK;
}

// Enter slot mode with every slot free and every KV page in the pool (whatever a static batch or an abandoned serving loop left behind).
int dots_slots_reset(DotsEngine* e) {
    if (!e) return DOTS_E_INVALID;
    if (!e->finalized) return e->fail(DOTS_E_STATE, "weights not finalized");
    CK(hipSetDevice(e->device));
    hipStream_t s = e->stream;
    if (e->pref_pending) {                               // a prefetched tower nobody took (an abandoned serving loop): drop it
        if (!e->pref_deferred) CK(hipStreamWaitEvent(s, e->ev_vis_ready, 0));
        e->pref_pending = e->pref_deferred = false;
    }
    RET(enter_slot_mode(e));
    if (e->pc) e->pc->release_all();                      // the leases of an abandoned serving loop; the cached blocks stay
    e->fresh_slots.clear();
    CK(hipMemsetAsync(e->out_lens, 0, e->cfg.max_batch * 4, s));
    CK(hipMemsetAsync(e->finished, 0, e->cfg.max_batch * 4, s));
    // no row carries any feature: the features' row tables (in RowFeature order; the own flags stand for the parameters), then the host record
    const struct { void* table; size_t row_bytes; } feature_tables[ROW_ALL_FEATURES] = {
        {e->d_row_own, 4}, {e->d_rules, sizeof(RowRules)}, {e->d_guides, sizeof(RowGuide)}, {e->d_ngram, sizeof(RowNgram)}, {e->d_stop, sizeof(RowStop)},
        {e->d_loop, sizeof(RowLoop)}};
    for (const auto& t : feature_tables)
        if (t.table) CK(hipMemsetAsync(t.table, 0, DOTS_MAX_BATCH * t.row_bytes, s));
    e->stage.reset();
    std::fill(e->row_guide, e->row_guide + DOTS_MAX_BATCH, 0);
    for (auto& g : e->guides) g.rows = 0;
    std::fill(e->row_stop, e->row_stop + DOTS_MAX_BATCH, 0);
    std::fill(e->row_stop_min, e->row_stop_min + DOTS_MAX_BATCH, 0);
    for (auto& a : e->stops) a.rows = 0;
    std::fill(e->row_loop, e->row_loop + DOTS_MAX_BATCH, DotsLoopRule{});
    if (e->d_row_lp) CK(hipMemsetAsync(e->d_row_lp, 0xFF, DOTS_MAX_BATCH * 4, s));
    std::fill(e->row_lp, e->row_lp + DOTS_MAX_BATCH, -1);
    e->n_lp = 0;
    RET(stream_reset(e));
    if (e->sp_ndraft) CK(hipMemsetAsync(e->sp_ndraft, 0, DOTS_MAX_BATCH * 4, s));
    if (e->sp_cls) CK(hipMemsetAsync(e->sp_cls, 0, DOTS_MAX_BATCH * 4, s));         // SPEC_ROW_ARGMAX: no row carries anything
    if (e->pr_stats) {                                                              // no slot holds a prediction
        for (int32_t* a : {e->pr_len, e->pr_cur, e->pr_at, e->pr_src, e->pr_seen}) CK(hipMemsetAsync(a, 0, DOTS_MAX_BATCH * 4, s));
        CK(hipMemsetAsync(e->pr_stats, 0, (size_t)DOTS_MAX_BATCH * 2 * sizeof(unsigned long long), s));
    }
    std::fill(e->row_pred, e->row_pred + DOTS_MAX_BATCH, 0);
    e->n_pred = 0;
    CK(hipStreamSynchronize(s));
    e->sel_dirty = true;
    return DOTS_OK;
}

// Shared-prefix attention: the plan of the next plain steps from the host record as it stands, uploaded in stream order.  A
// row's static pages are its full prompt pages: nobody writes them, and a beam group's device-side reordering never touches them.  A
// suspended row idles on the scratch page: it is not active here
static int share_replan(DotsEngine* e) {
    if (!e->d_share) {
        CK(e->alloc(&e->d_share, (size_t)SHARE_PLAN_WORDS));
        e->h_share.assign(SHARE_PLAN_WORDS, 0);
    }
    const int mb = e->cfg.max_batch;
    int32_t active[DOTS_MAX_BATCH], stat[DOTS_MAX_BATCH];
    uint64_t mask[DOTS_MAX_BATCH] = {0};
    for (int b = 0; b < mb; ++b) {
        active[b] = e->slot_active[b] && !e->parked[b].on;
        stat[b] = std::min(e->slot_prompt[b] / PAGE, (int)e->slot_pages[b].size());
    }
    int32_t* h = e->h_share.data();
    const int waves = decode_attn_waves();
    e->share_last = waves == 4 ? share_plan(active, e->hp_table.data(), e->max_pages, stat, mb, splits_for_ctx(e->cfg.max_seq_len), waves, e->max_pages,
                                            h + SHARE_ITEMS_OFF, h + SHARE_MEMBERS_OFF, mask)
                               : SharePlanCounts{0, 0, 0, 0};      // the shared kernel is the four-wave arithmetic
    h[0] = e->share_last.items;
    std::memcpy(h + SHARE_MASK_OFF, mask, sizeof(mask));
    CK(hipMemcpyAsync(e->d_share, h, (size_t)SHARE_PLAN_WORDS * 4, hipMemcpyHostToDevice, e->stream));
    e->share_cap = (int)round_up(e->share_last.items, SHARE_ITEM_QUANTUM);
    e->share_dirty = false;
    return DOTS_OK;
}

int dots_set_shared_prefix_attention(DotsEngine* e, int on) {
    if (!e) return DOTS_E_INVALID;
    e->share_on = on != 0;
    e->share_dirty = true;
    if (!e->share_on) { e->share_cap = 0; e->share_last = SharePlanCounts{0, 0, 0, 0}; }
    return DOTS_OK;
}

int dots_shared_prefix_info(DotsEngine* e, int64_t* out4) {
    if (!e || !out4) return e ? e->fail(DOTS_E_INVALID, "null argument") : DOTS_E_INVALID;
    const bool live = share_plan_now(e).cap > 0;
    out4[0] = live ? e->share_last.items : 0;
    out4[1] = live ? e->share_last.rows : 0;
    out4[2] = live ? e->share_last.pairs : 0;
    out4[3] = e->share_pages_saved;
    return DOTS_OK;
}

int dots_slots_decode(DotsEngine* e, int n_steps) {
    if (!e) return DOTS_E_INVALID;
    if (!e->slot_mode) return e->fail(DOTS_E_STATE, "no slot has been prefilled");
    if (n_steps < 1) return e->fail(DOTS_E_INVALID, "n_steps must be >= 1");
    CK(hipSetDevice(e->device));
    hipStream_t s = e->stream;
    int rows = 0;
    for (int b = 0; b < e->cfg.max_batch; ++b)
        if (e->slot_active[b]) rows = b + 1;
    if (!rows) return e->fail(DOTS_E_STATE, "every slot is free");
    RET(beam_before_decode(e, n_steps));                    // a refusal changes nothing
    e->fresh_slots.clear();                                 // the step overwrites the logits a fork selects from (dots_slots_fork)
    if (e->sel_dirty) {
        int32_t sel[DOTS_MAX_BATCH];
        // a group's rows are selected by its own kernels; a suspended row commits nothing
        for (int b = 0; b < DOTS_MAX_BATCH; ++b) sel[b] = e->slot_active[b] && !e->beam_of[b] && !e->parked[b].on;
        CK(hipMemcpyAsync(e->d_sel, sel, DOTS_MAX_BATCH * 4, hipMemcpyHostToDevice, s));
        e->sel_dirty = false;
        e->share_dirty = true;                              // whatever changes which rows run changes which rows share pages
    }
    if (e->share_on && e->share_dirty) RET(share_replan(e));
    // ---- paged KV: every running sequence gets the pages the next n_steps positions need, now.  Pool dry: the sequence keeps what it
    // has and its generation cap is lowered to what its pages hold — it finishes there with "length", like HF generate at the
    // context capacity (an admission policy that leaves head-room makes this rare: dots_ocr_amd/scheduler.py).
    // A speculating step may advance a row by spec_k + 1 positions and writes KV that far ahead: pages and the host's bound on the
    // context count n_steps x (k + 1) (dots_slots_poll brings the bound back to the row's true context)
    n_steps *= e->spec_k + 1;
    for (int b = 0; b < rows; ++b) {
        if (!slot_grows(e, b)) continue;
        int want = chunk_want(e, b, n_steps);
        bool changed = false;
        const int have = grow_pages(e, b, want, &changed);
        if (changed) CK(upload_table_row(e, b));
        if (have < want && e->spec_k) {
            // before a speculating row is capped, its bound becomes its true context: steps that accepted fewer than k drafts left it too high
            int32_t ctx = 0;
            CK(hipMemcpyAsync(&ctx, e->ctx_len + b, 4, hipMemcpyDeviceToHost, s));
            CK(hipStreamSynchronize(s));
            e->slot_ctx_ub[b] = std::min(e->slot_ctx_ub[b], (int)ctx);
            want = chunk_want(e, b, n_steps);
        }
        if (have < want) {
            // Positions [0, have) exist: the last step the row may take is the one at context have - 1, which leaves it with have + 1
            // tokens.  commit_token finishes a row when a step brings it to its cap — so a row that already sits AT context `have`
            // (the pool ran dry exactly on its page boundary) must be stopped here: its next step would write position
            // `have` through a block-table entry it does not own (the scratch page every idle row writes) and read it back.
            e->slot_limit[b] = have + 1;
            const int32_t cap = have + 1 - e->slot_prompt[b];               // generated tokens; >= the tokens generated so far
            static const int32_t one = 1;
            CK(hipMemcpyAsync(e->d_max_len + b, &cap, 4, hipMemcpyHostToDevice, s));
            if (have <= e->slot_ctx_ub[b]) CK(hipMemcpyAsync(e->finished + b, &one, 4, hipMemcpyHostToDevice, s));
            CK(hipStreamSynchronize(s));                                     // `cap` is a stack variable
            e->kv_capped += 1;
        }
        e->slot_ctx_ub[b] = chunk_want(e, b, n_steps);
    }
    n_steps /= e->spec_k + 1;
    const int n_splits = splits_for_ctx(e->cfg.max_seq_len);
    e->B = rows;
    const bool use_graph = !launch_switches().no_graph;
    // beside a prefetched vision tower (the next admission's: dots_vit_prefetch) the chunk is replayed on the decode partition, with the
    // half-chip launch plan when the rows allow it — exactly as dots_generate does
    hipStream_t cur = s;
    if (use_graph) { int r0 = pick_decode_stream(e, &cur); if (r0 != DOTS_OK) { e->B = 0; return r0; } }
    const int part = cur != s ? 1 : 0;
    hipGraphExec_t exec = nullptr;
    if (use_graph) {
        int r = step_graph(e, rows, n_splits, 0, &exec, part);
        if (r != DOTS_OK) { e->B = 0; return r; }
    }
    int r = DOTS_OK;
    for (int i = 0; i < n_steps && r == DOTS_OK; ++i) {
        if (exec) { if (hipGraphLaunch(exec, cur) != hipSuccess) r = e->fail(DOTS_E_HIP, "hipGraphLaunch failed"); }
        else r = decode_step_launches(e, n_splits);
    }
    if (r == DOTS_OK && e->ev_dec_end && hipEventRecord(e->ev_dec_end, cur) == hipSuccess) ++e->dec_end_seq;      // pick_tower_tail
    if (r == DOTS_OK) r = chain_streams(e, cur, s);
    if (r == DOTS_OK && share_plan_now(e).cap)
        e->share_pages_saved += (int64_t)n_steps * e->share_last.saved * decode_attn_waves() * e->cfg.num_kv_heads * e->cfg.num_layers;
    e->B = 0;
    e->stats.decode_steps += n_steps;
    return r;
}

int dots_slots_poll(DotsEngine* e, int32_t* finished, int32_t* out_lens) {
    if (!e || !finished || !out_lens) return e ? e->fail(DOTS_E_INVALID, "null argument") : DOTS_E_INVALID;
    CK(hipSetDevice(e->device));
    const int mb = e->cfg.max_batch;
    CK(hipMemcpyAsync(finished, e->finished, mb * 4, hipMemcpyDeviceToHost, e->stream));
    CK(hipMemcpyAsync(out_lens, e->out_lens, mb * 4, hipMemcpyDeviceToHost, e->stream));
    CK(hipStreamSynchronize(e->stream));
    poll_host_state(e, finished, out_lens);
    return DOTS_OK;
}

int dots_slot_read(DotsEngine* e, int slot, int32_t* out_ids, int capacity, int32_t* n_out) {
    if (!e || !out_ids || !n_out || capacity < 0) return e ? e->fail(DOTS_E_INVALID, "bad slot_read arguments") : DOTS_E_INVALID;
    if (!slot_occupied(e, slot)) return e->fail(DOTS_E_STATE, "slot %d is not occupied", slot);
    CK(hipSetDevice(e->device));
    int32_t n = 0;
    CK(hipMemcpyAsync(&n, e->out_lens + slot, 4, hipMemcpyDeviceToHost, e->stream));
    CK(hipStreamSynchronize(e->stream));
    *n_out = n;
    const int take = std::min<int>(n, capacity);
    if (take > 0) {
        CK(hipMemcpyAsync(out_ids, e->out_ids + (size_t)slot * e->cfg.max_seq_len, (size_t)take * 4, hipMemcpyDeviceToHost, e->stream));
        CK(hipStreamSynchronize(e->stream));
    }
    return DOTS_OK;
}

int dots_slot_logits(DotsEngine* e, int slot, float* out) {
    if (!e || !out) return e ? e->fail(DOTS_E_INVALID, "null argument") : DOTS_E_INVALID;
    if (!slot_occupied(e, slot)) return e->fail(DOTS_E_STATE, "slot %d is not occupied", slot);
    CK(hipSetDevice(e->device));
    CK(hipMemcpyAsync(out, e->d_logits + (size_t)slot * e->cfg.vocab_size, (size_t)e->cfg.vocab_size * 4, hipMemcpyDeviceToHost, e->stream));
    CK(hipStreamSynchronize(e->stream));
    return DOTS_OK;
}

int dots_slot_release(DotsEngine* e, int slot) {
    if (!e) return DOTS_E_INVALID;
    if (!slot_occupied(e, slot) && !(e->slot_mode && slot_filling(e, slot))) return e->fail(DOTS_E_STATE, "slot %d is not occupied", slot);
    CK(hipSetDevice(e->device));
    if (e->beam_of[slot]) return beam_release_group(e, slot);          // the slots of a beam group go together
    for (int f = 0; f < ROW_ALL_FEATURES; ++f) RET(clear_row_feature(e, slot, (RowFeature)f));
    RET(set_row_lp(e, slot, -1));
    RET(clear_row_prediction(e, slot));
    e->row_stream[slot] = 0;
    e->slot_active[slot] = 0;
    e->sel_dirty = true;
    CK(hipMemsetAsync(e->ctx_len + slot, 0, 4, e->stream));          // an idle row attends over one key only ...
    release_pages(e, slot);                                          // ... of the scratch page: its own pages go back to the pool
    CK(upload_table_row(e, slot));
    return DOTS_OK;
}

// ---------------------------------------------------------------------------------- suspend / resume
static size_t swap_unit_bytes(const DotsEngine* e) { return kv_page_bytes(e) * e->cfg.num_layers; }                          // one host page

// Moves n pages between the pool and the host space in chunks of KV_SWAP_CHUNK_PAGES through the staging buffer, in order on the engine's
// stream: pool page pool_pages[i] <-> host page host_pages[i] (ascending, so a chunk is usually ONE copy: one hipMemcpyAsync per run of
// consecutive host pages).  to_host: gather + copy out, else copy in + scatter.  The caller synchronises.
static int swap_move(DotsEngine* e, bool to_host, const std::vector<int32_t>& pool_pages, const std::vector<int32_t>& host_pages) {
    const int n = (int)pool_pages.size();
    if (!n) return DOTS_OK;
    hipStream_t s = e->stream;
    const size_t unit = swap_unit_bytes(e), page_bytes = kv_page_bytes(e);
    if (!e->swap_list) CK(e->alloc(&e->swap_list, (size_t)e->max_pages));
    if (!e->swap_stage) CK(e->alloc(&e->swap_stage, (size_t)KV_SWAP_CHUNK_PAGES * unit));
    e->swap_list_host = pool_pages;                          // outlives the asynchronous upload
    CK(hipMemcpyAsync(e->swap_list, e->swap_list_host.data(), (size_t)n * 4, hipMemcpyHostToDevice, s));
    for (int c0 = 0; c0 < n; c0 += KV_SWAP_CHUNK_PAGES) {
        const int cn = std::min(KV_SWAP_CHUNK_PAGES, n - c0);
        if (to_host) CK(launch_kv_gather_pages(s, e->pool, e->pool_layer_elems * 2, page_bytes, e->cfg.num_layers, e->swap_stage, e->swap_list + c0, cn));
        for (int i = 0; i < cn;) {
            int run = 1;
            while (i + run < cn && host_pages[c0 + i + run] == host_pages[c0 + i] + run) ++run;
            uint8_t *host = e->swap_host + (size_t)host_pages[c0 + i] * unit, *dev = e->swap_stage + (size_t)i * unit;
            if (to_host) CK(hipMemcpyAsync(host, dev, (size_t)run * unit, hipMemcpyDeviceToHost, s));
            else CK(hipMemcpyAsync(dev, host, (size_t)run * unit, hipMemcpyHostToDevice, s));
            i += run;
        }
        if (!to_host) CK(launch_kv_scatter_pages(s, e->pool, e->pool_layer_elems * 2, page_bytes, e->cfg.num_layers, e->swap_stage, e->swap_list + c0, cn));
    }
    return DOTS_OK;
}

int dots_kv_swap_reserve(DotsEngine* e, int pages) {
    if (!e) return DOTS_E_INVALID;
    if (pages < 0) return e->fail(DOTS_E_INVALID, "dots_kv_swap_reserve: pages must be >= 0, got %d", pages);
    if (e->n_parked) return e->fail(DOTS_E_STATE, "the host space cannot change while %d slot(s) are suspended", e->n_parked);
    if (pages == e->swap_total) return DOTS_OK;
    CK(hipSetDevice(e->device));
    CK(hipStreamSynchronize(e->stream));
    swap_free_host(e);
    if (pages) {
        void* p = nullptr;
        CK(hipHostMalloc(&p, (size_t)pages * swap_unit_bytes(e), hipHostMallocDefault));
        e->swap_host = static_cast<uint8_t*>(p);
        e->swap_total = e->swap_free = pages;
        e->swap_used.assign(pages, 0);
    }
    return DOTS_OK;
}

int dots_kv_swap_info(DotsEngine* e, int32_t* total_pages, int32_t* free_pages) {
    if (!e || !total_pages || !free_pages) return DOTS_E_INVALID;
    *total_pages = e->swap_total;
    *free_pages = e->swap_free;
    return DOTS_OK;
}

int dots_slot_suspend(DotsEngine* e, int slot) {
    if (!e) return DOTS_E_INVALID;
    if (!slot_occupied(e, slot)) return e->fail(DOTS_E_STATE, "slot %d is not occupied", slot);
    if (e->parked[slot].on) return e->fail(DOTS_E_STATE, "slot %d is already suspended", slot);
    if (e->beam_of[slot]) return e->fail(DOTS_E_STATE, "slot %d is a row of a beam group: a group cannot be suspended", slot);
    if (e->spec_k) return e->fail(DOTS_E_STATE, "a slot cannot be suspended while the engine speculates (dots_set_speculation)");
    CK(hipSetDevice(e->device));
    hipStream_t s = e->stream;
    // the row's scalars: an idle row sits at context 0, and whatever refills the batch meanwhile must find nothing of this row in them
    int32_t sc[3] = {0, 0, 0};
    CK(hipMemcpyAsync(&sc[0], e->cur_tokens + slot, 4, hipMemcpyDeviceToHost, s));
    CK(hipMemcpyAsync(&sc[1], e->ctx_len + slot, 4, hipMemcpyDeviceToHost, s));
    CK(hipMemcpyAsync(&sc[2], e->finished + slot, 4, hipMemcpyDeviceToHost, s));
    CK(hipStreamSynchronize(s));
    if (sc[2]) return e->fail(DOTS_E_STATE, "slot %d has finished: read and release it", slot);
    auto& mine = e->slot_pages[slot];
    const int ctx = sc[1], n_data = (ctx + 63) / 64;         // positions [0, ctx) are written: the token at ctx is the next step's input
    if (ctx < 1 || n_data > (int)mine.size()) return e->fail(DOTS_E_STATE, "slot %d: context %d is not covered by its %d pages", slot, ctx, (int)mine.size());
    // ---- what goes where: a page with other holders stays (nobody writes it: DESIGN §6.7), a page of the row alone is copied out if it
    // holds positions and simply returned if it was taken ahead of the context
    std::vector<int32_t> where(mine.size()), src, dst;
    for (int p = 0; p < (int)mine.size(); ++p) {
        if (e->page_refs[mine[p]] > 1) where[p] = mine[p];
        else if (p < n_data) { where[p] = -2; src.push_back(mine[p]); }
        else where[p] = -1;
    }
    while (!where.empty() && where.back() == -1) where.pop_back();
    if ((int)src.size() > e->swap_free)
        return e->fail(DOTS_E_CAPACITY, "host space exhausted: slot %d needs %d host pages, %d of %d are free (dots_kv_swap_reserve)", slot, (int)src.size(),
                       e->swap_free, e->swap_total);
    for (int h = 0; h < e->swap_total && dst.size() < src.size(); ++h)
        if (!e->swap_used[h]) dst.push_back(h);
    RET(swap_move(e, true, src, dst));
    CK(hipMemsetAsync(e->ctx_len + slot, 0, 4, s));          // idles like a released slot: one key of the scratch page
    CK(hipStreamSynchronize(s));
    // ---- the copies have landed: only now does anything change hands
    for (int32_t h : dst) e->swap_used[h] = 1;
    e->swap_free -= (int)dst.size();
    {
        size_t k = 0;
        for (auto& w : where)
            if (w == -2) w = -(dst[k++] + 2);
    }
    std::vector<int32_t> keep;
    for (auto it = mine.rbegin(); it != mine.rend(); ++it)
        if (e->page_refs[*it] == 1) { e->page_refs[*it] = 0; e->free_pages.push_back(*it); }
    for (int32_t pg : mine)
        if (e->page_refs[pg] > 1) keep.push_back(pg);
    mine = keep;                                              // the pages dots_slot_release still has to let go of
    std::fill(e->hp_table.begin() + (size_t)slot * e->max_pages, e->hp_table.begin() + (size_t)(slot + 1) * e->max_pages, e->n_pool_pages);
    CK(upload_table_row(e, slot));
    DotsEngine::Parked& pk = e->parked[slot];
    pk.on = true;
    pk.pages = where;
    pk.cur_token = sc[0]; pk.ctx = ctx; pk.finished = sc[2];
    e->n_parked += 1;
    e->slot_ctx_ub[slot] = ctx;
    e->sel_dirty = true;
    return DOTS_OK;
}

int dots_slot_resume(DotsEngine* e, int slot) {
    if (!e) return DOTS_E_INVALID;
    if (!slot_occupied(e, slot) || !e->parked[slot].on)
        return e->fail(DOTS_E_STATE, "slot %d is not suspended", slot);
    DotsEngine::Parked& pk = e->parked[slot];
    int need = 0;
    for (int32_t w : pk.pages) need += w < 0;
    ensure_free(e, need);
    if (need > (int)e->free_pages.size() || (int)pk.pages.size() > e->max_pages)
        return e->fail(DOTS_E_CAPACITY, "KV pool exhausted: slot %d needs %d pages of 64 tokens to resume, %d of %d are free", slot, need,
                       free_count(e), e->n_pool_pages);
    CK(hipSetDevice(e->device));
    hipStream_t s = e->stream;
    // fresh pages in free-list order, taken off the list only once the copies have landed
    std::vector<int32_t> row(pk.pages.size()), src, dst;
    for (size_t p = 0, k = 0; p < pk.pages.size(); ++p) {
        const int32_t w = pk.pages[p];
        if (w >= 0) { row[p] = w; continue; }
        row[p] = e->free_pages[e->free_pages.size() - 1 - k++];
        if (w <= -2) { src.push_back(-(w + 2)); dst.push_back(row[p]); }
    }
    RET(swap_move(e, false, dst, src));
    CK(hipMemcpyAsync(e->cur_tokens + slot, &pk.cur_token, 4, hipMemcpyHostToDevice, s));
    CK(hipMemcpyAsync(e->ctx_len + slot, &pk.ctx, 4, hipMemcpyHostToDevice, s));
    CK(hipMemcpyAsync(e->finished + slot, &pk.finished, 4, hipMemcpyHostToDevice, s));
    for (size_t p = 0; p < row.size(); ++p) e->hp_table[(size_t)slot * e->max_pages + p] = row[p];
    if (hipError_t r = upload_table_row(e, slot); r != hipSuccess || (r = hipStreamSynchronize(s)) != hipSuccess) {
        std::fill(e->hp_table.begin() + (size_t)slot * e->max_pages, e->hp_table.begin() + (size_t)(slot + 1) * e->max_pages, e->n_pool_pages);
        return e->fail(DOTS_E_HIP, "dots_slot_resume: %s", hipGetErrorString(r));
    }
    e->free_pages.resize(e->free_pages.size() - need);
    for (size_t p = 0; p < row.size(); ++p)
        if (pk.pages[p] < 0) e->page_refs[row[p]] = 1;
    e->slot_pages[slot] = row;
    drop_parked(e, slot);                                     // the host pages are free again
    e->slot_ctx_ub[slot] = pk.ctx;
    e->sel_dirty = true;
    return DOTS_OK;
}

int dots_slots_pages_short(DotsEngine* e, int n_steps, int32_t* pages) {
    if (!e || !pages) return e ? e->fail(DOTS_E_INVALID, "null argument") : DOTS_E_INVALID;
    if (!e->slot_mode) return e->fail(DOTS_E_STATE, "no slot has been prefilled");
    if (n_steps < 1) return e->fail(DOTS_E_INVALID, "n_steps must be >= 1");
    int64_t lack = 0;
    for (int b = 0; b < e->cfg.max_batch; ++b)
        if (slot_grows(e, b)) lack += chunk_pages_lacking(e, b, n_steps * (e->spec_k + 1));
    *pages = (int32_t)std::max<int64_t>(0, lack - (int64_t)free_count(e));
    return DOTS_OK;
}

int dots_kv_pool_info(DotsEngine* e, int32_t* total_pages, int32_t* free_pages) {
    if (!e || !total_pages || !free_pages) return DOTS_E_INVALID;
    *total_pages = e->n_pool_pages;
    *free_pages = (int32_t)free_count(e);
    return DOTS_OK;
}

int dots_set_kv_scales(DotsEngine* e, const float* scales_host) {
    if (!e || !scales_host) return e ? e->fail(DOTS_E_INVALID, "null argument") : DOTS_E_INVALID;
    const DotsConfig& c = e->cfg;
    const size_t n = (size_t)c.num_layers * c.num_kv_heads * 2;
    for (size_t i = 0; i < n; ++i)
        if (!std::isfinite(scales_host[i]) || !(scales_host[i] > 0.f))
            return e->fail(DOTS_E_INVALID, "kv scale %zu (layer %zu, kv head %zu, %s) is %g: must be finite and > 0", i, i / (2 * c.num_kv_heads),
                           (i / 2) % c.num_kv_heads, i % 2 ? "V" : "K", (double)scales_host[i]);
    // a cached token was quantised with the scales of its time: they are fixed while any sequence holds pages
    if (e->n_parked) return e->fail(DOTS_E_STATE, "KV scales cannot change while %d slot(s) are suspended: their KV is parked in host memory", e->n_parked);
    if ((int)e->free_pages.size() != e->n_pool_pages)
        return e->fail(DOTS_E_STATE, "KV scales cannot change while sequences hold KV pages (%d of %d in use): release them first (dots_slots_reset)",
                       e->n_pool_pages - free_count(e), e->n_pool_pages);
    CK(hipSetDevice(e->device));
    CK(hipMemcpyAsync(e->kv_scales, scales_host, n * 4, hipMemcpyHostToDevice, e->stream));
    CK(hipStreamSynchronize(e->stream));
    return DOTS_OK;
}

int dots_slot_capacity(DotsEngine* e, int slot, int32_t* pages_owned, int32_t* token_limit) {
    if (!e || !pages_owned || !token_limit) return DOTS_E_INVALID;
    if (!slot_occupied(e, slot)) return e->fail(DOTS_E_STATE, "slot %d is not occupied", slot);
    *pages_owned = (int32_t)e->slot_pages[slot].size();
    *token_limit = e->slot_limit[slot];
    return DOTS_OK;
}
}  // extern "C"
