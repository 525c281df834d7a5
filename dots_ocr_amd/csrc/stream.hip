// Streaming (dots_set_row_stream / dots_slots_drain): what every streaming row committed since the last drain, in one launch.
//
// A row's cursor stream_pos[row] is the number of its output tokens already delivered.  stream_drain_kernel is ONE workgroup:
//   phase 1  lane b of wave 0 owns row b (DOTS_MAX_BATCH = 64 = one wavefront): it reads finished / out_lens / the cursor, takes
//            count = min(out_len - cursor, DOTS_STREAM_ROW_CAP) when the row streams, a wave scan packs the rows in slot order (first[b];
//            lp_first[b] over the rows that also return logprobs), the lane writes its header entries and its advanced cursor — the only
//            reader of cursor b is lane b, before it writes it — and leaves (cursor, count, first, lp_first) in LDS;
//   barrier
//   phase 2  the workgroup's waves take rows round robin and copy out_ids[row][cursor, cursor + count) and the matching entries of
//            lp_tok / lp_ids / lp_top (contiguous per row: count and count x 20 words) behind first / lp_first.
// Everything is stored straight into mapped pinned host memory (StreamOut), so a drain is this launch and one stream synchronisation: a
// device staging buffer would need the packed size on the host before its copy could be sized — a second round trip — or a copy of the
// worst case (2.7 MB).  The launch is never part of a captured step.
#include "engine.h"

namespace {

constexpr int SD_THREADS = 512;

struct StreamOut {            // device addresses of the pinned block (engine.h: st_host)
    int32_t* head;            // [STREAM_HEAD]: finished, out_lens, first, count, lp_first [DOTS_MAX_BATCH] each, then n_tokens, n_lp
    int32_t* tokens;          // [DOTS_MAX_BATCH * DOTS_STREAM_ROW_CAP]
    float* tok_lp;            // [DOTS_MAX_BATCH * DOTS_STREAM_ROW_CAP]
    int32_t* top_ids;         // [..][DOTS_MAX_TOP_LOGPROBS]
    float* top_lp;            // [..][DOTS_MAX_TOP_LOGPROBS]
};
constexpr int STREAM_HEAD = 5 * DOTS_MAX_BATCH + 2;
constexpr size_t STREAM_POS = (size_t)DOTS_MAX_BATCH * DOTS_STREAM_ROW_CAP;
constexpr size_t STREAM_HEAD_PAD = 512;                              // int32 units: the payload starts 2 KiB in
constexpr size_t STREAM_WORDS = STREAM_HEAD_PAD + STREAM_POS * (2 + 2 * DOTS_MAX_TOP_LOGPROBS);
static_assert(STREAM_HEAD <= (int)STREAM_HEAD_PAD, "header does not fit");

DEVI int wave_scan_incl(int v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(v, o, 64);
        if (lane >= o) v += u;
    }
    return v;
}

__global__ __launch_bounds__(SD_THREADS) void stream_drain_kernel(const int32_t* __restrict__ finished, const int32_t* __restrict__ out_lens,
                                                                  const int32_t* __restrict__ out_ids, int out_stride, int rows,
                                                                  int32_t* __restrict__ stream_pos, uint64_t on_mask, uint64_t lp_mask,
                                                                  const float* __restrict__ lp_tok, const int32_t* __restrict__ lp_ids,
                                                                  const float* __restrict__ lp_top, StreamOut out) {
    __shared__ int32_t s_cur[DOTS_MAX_BATCH], s_cnt[DOTS_MAX_BATCH], s_first[DOTS_MAX_BATCH], s_lpf[DOTS_MAX_BATCH];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (wave == 0) {
        const int b = lane;
        const bool row = b < rows;
        const int fin = row ? finished[b] : 0;
        const int len = row ? min(max(out_lens[b], 0), out_stride) : 0;
        const int cur = row ? min(max(stream_pos[b], 0), len) : 0;
        const bool on = row && ((on_mask >> b) & 1), lp = on && ((lp_mask >> b) & 1);
        const int cnt = on ? min(len - cur, DOTS_STREAM_ROW_CAP) : 0;
        const int lcnt = lp ? cnt : 0;
        const int incl = wave_scan_incl(cnt, lane), lincl = wave_scan_incl(lcnt, lane);
        const int first = incl - cnt, lpf = lp ? lincl - lcnt : -1;
        out.head[b] = fin;
        out.head[DOTS_MAX_BATCH + b] = row ? out_lens[b] : 0;
        out.head[2 * DOTS_MAX_BATCH + b] = first;
        out.head[3 * DOTS_MAX_BATCH + b] = cnt;
        out.head[4 * DOTS_MAX_BATCH + b] = lpf;
        if (lane == 63) {
            out.head[5 * DOTS_MAX_BATCH] = incl;
            out.head[5 * DOTS_MAX_BATCH + 1] = lincl;
        }
        if (cnt) stream_pos[b] = cur + cnt;
        s_cur[b] = cur; s_cnt[b] = cnt; s_first[b] = first; s_lpf[b] = lpf;
    }
    __syncthreads();
    constexpr int K = DOTS_MAX_TOP_LOGPROBS;
    for (int b = wave; b < rows; b += SD_THREADS / 64) {
        const int cnt = s_cnt[b];
        if (!cnt) continue;
        const size_t src = (size_t)b * out_stride + s_cur[b];
        const int first = s_first[b], lpf = s_lpf[b];
        for (int i = lane; i < cnt; i += 64) out.tokens[first + i] = out_ids[src + i];
        if (lpf < 0) continue;
        for (int i = lane; i < cnt; i += 64) out.tok_lp[lpf + i] = lp_tok[src + i];
        for (int i = lane; i < cnt * K; i += 64) {
            out.top_ids[(size_t)lpf * K + i] = lp_ids[src * K + i];
            out.top_lp[(size_t)lpf * K + i] = lp_top[src * K + i];
        }
    }
}

// the cursor, the pinned block and its device addresses, by the first row switched on
int ensure_stream_state(DotsEngine* e) {
    if (e->stream_pos) return DOTS_OK;
    void* p = nullptr;
    CK(hipHostMalloc(&p, STREAM_WORDS * 4, hipHostMallocMapped | hipHostMallocCoherent));
    void* d = nullptr;
    if (hipHostGetDevicePointer(&d, p, 0) != hipSuccess) {
        hipHostFree(p);
        return e->fail(DOTS_E_HIP, "hipHostGetDevicePointer failed for the stream staging block");
    }
    memset(p, 0, STREAM_WORDS * 4);
    e->st_host = (int32_t*)p;
    e->st_dev = (int32_t*)d;
    CK(e->alloc(&e->stream_pos, DOTS_MAX_BATCH));
    return DOTS_OK;
}

StreamOut stream_out(int32_t* base) {
    int32_t* pay = base + STREAM_HEAD_PAD;
    return StreamOut{base, pay, (float*)(pay + STREAM_POS), pay + 2 * STREAM_POS, (float*)(pay + (2 + DOTS_MAX_TOP_LOGPROBS) * STREAM_POS)};
}

}  // namespace

namespace engine {

void stream_free_host(DotsEngine* e) {
    if (e->st_host) hipHostFree(e->st_host);
    e->st_host = e->st_dev = nullptr;
}

// a slot's output starts over (rows_go_live, extend_slots): so does its cursor
int stream_restart_row(DotsEngine* e, int row) {
    if (e->stream_pos) CK(hipMemsetAsync(e->stream_pos + row, 0, 4, e->stream));
    return DOTS_OK;
}

// dots_slots_reset: no row streams
int stream_reset(DotsEngine* e) {
    std::fill(e->row_stream, e->row_stream + DOTS_MAX_BATCH, 0);
    if (e->stream_pos) CK(hipMemsetAsync(e->stream_pos, 0, DOTS_MAX_BATCH * 4, e->stream));
    return DOTS_OK;
}

}  // namespace engine

using namespace engine;
extern "C" {

int dots_set_row_stream(DotsEngine* e, int row, int on) {
    if (!e) return DOTS_E_INVALID;
    if (row < 0 || row >= e->cfg.max_batch) return e->fail(DOTS_E_INVALID, "row %d out of range [0, %d)", row, e->cfg.max_batch);
    if (!on) { e->row_stream[row] = 0; return DOTS_OK; }
    if (beam_row(e, row)) return e->fail(DOTS_E_STATE, "slot %d is a row of a beam group: a group's outputs are reordered, it cannot stream", row);
    CK(hipSetDevice(e->device));
    RET(ensure_stream_state(e));
    if (!e->row_stream[row]) RET(stream_restart_row(e, row));
    e->row_stream[row] = 1;
    return DOTS_OK;
}

int dots_slots_drain(DotsEngine* e, int32_t* finished, int32_t* out_lens, int32_t* first, int32_t* count, int32_t* lp_first, int32_t* tokens,
                     int tokens_cap, float* tok_lp, int32_t* top_ids, float* top_lp, int lp_cap, int32_t* n_tokens, int32_t* n_lp) {
    if (!e || !finished || !out_lens || !first || !count || !lp_first || !n_tokens || !n_lp || tokens_cap < 0 || lp_cap < 0)
        return e ? e->fail(DOTS_E_INVALID, "bad slots_drain arguments") : DOTS_E_INVALID;
    const int mb = e->cfg.max_batch;
    // the rows that deliver: occupied (a suspended row too: what it held at the suspend), not filling, switched on
    uint64_t on_mask = 0, lp_mask = 0;
    for (int b = 0; b < mb; ++b) {
        if (!e->row_stream[b] || !slot_occupied(e, b) || slot_filling(e, b)) continue;
        on_mask |= 1ull << b;
        if (e->row_lp[b] >= 0 && e->lp_tok) lp_mask |= 1ull << b;
    }
    std::fill(first, first + mb, 0);
    std::fill(count, count + mb, 0);
    std::fill(lp_first, lp_first + mb, -1);
    *n_tokens = *n_lp = 0;
    if (!on_mask) return dots_slots_poll(e, finished, out_lens);
    // a row delivers at most DOTS_STREAM_ROW_CAP tokens: checked before the launch, which advances the cursors
    const int64_t need = (int64_t)__builtin_popcountll(on_mask) * DOTS_STREAM_ROW_CAP, need_lp = (int64_t)__builtin_popcountll(lp_mask) * DOTS_STREAM_ROW_CAP;
    if (tokens_cap < need || !tokens) return e->fail(DOTS_E_INVALID, "slots_drain: room for %d tokens, %lld may arrive", tokens_cap, (long long)need);
    if (need_lp && (lp_cap < need_lp || !tok_lp || !top_ids || !top_lp))
        return e->fail(DOTS_E_INVALID, "slots_drain: room for %d logprob entries, %lld may arrive", lp_cap, (long long)need_lp);
    CK(hipSetDevice(e->device));
    hipLaunchKernelGGL(stream_drain_kernel, dim3(1), dim3(SD_THREADS), 0, e->stream, e->finished, e->out_lens, e->out_ids, e->cfg.max_seq_len, mb,
                       e->stream_pos, on_mask, lp_mask, e->lp_tok, e->lp_ids, e->lp_top, stream_out(e->st_dev));
    CK(hipGetLastError());
    CK(hipStreamSynchronize(e->stream));
    const StreamOut h = stream_out(e->st_host);
    memcpy(finished, h.head, mb * 4);
    memcpy(out_lens, h.head + DOTS_MAX_BATCH, mb * 4);
    memcpy(first, h.head + 2 * DOTS_MAX_BATCH, mb * 4);
    memcpy(count, h.head + 3 * DOTS_MAX_BATCH, mb * 4);
    memcpy(lp_first, h.head + 4 * DOTS_MAX_BATCH, mb * 4);
    const int nt = h.head[5 * DOTS_MAX_BATCH], nl = h.head[5 * DOTS_MAX_BATCH + 1];
    if (nt < 0 || nt > need || nl < 0 || nl > need_lp) return e->fail(DOTS_E_HIP, "slots_drain: the kernel reported %d tokens, %d logprob entries", nt, nl);
    *n_tokens = nt;
    *n_lp = nl;
    constexpr size_t K = DOTS_MAX_TOP_LOGPROBS;
    if (nt) memcpy(tokens, h.tokens, (size_t)nt * 4);
    if (nl) {
        memcpy(tok_lp, h.tok_lp, (size_t)nl * 4);
        memcpy(top_ids, h.top_ids, (size_t)nl * K * 4);
        memcpy(top_lp, h.top_lp, (size_t)nl * K * 4);
    }
    poll_host_state(e, finished, out_lens);
    return DOTS_OK;
}

}  // extern "C"
