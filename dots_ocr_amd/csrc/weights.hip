// Weights of the dots.ocr engine: checkpoint tensors as loaded -> the packed (fp8 mode: quantised) matrices of ViT / prefill and their
// decode copies in MFMA fragment order, and the workspaces every engine allocates at creation.
#include "engine.h"

namespace {
__global__ void pack_w13_kernel(const bf16_t* __restrict__ gate, const bf16_t* __restrict__ up, bf16_t* __restrict__ out, int I, int K) {
    // out row r: group G = r/64; rows [0,32) of the group = gate[G*32 ..], rows [32,64) = up[G*32 ..]
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;      // 16-B chunk index
    const int cpr = K / 8;
    if (idx >= (int64_t)2 * I * cpr) return;
    const int r = (int)(idx / cpr), c = (int)(idx % cpr);
    const int G = r >> 6, wi = r & 63;
    const bf16_t* src = (wi < 32 ? gate + (size_t)(G * 32 + wi) * K : up + (size_t)(G * 32 + wi - 32) * K) + c * 8;
    *reinterpret_cast<u32x4*>(out + (size_t)r * K + c * 8) = *reinterpret_cast<const u32x4*>(src);
}

__global__ void pack_b13_kernel(const bf16_t* __restrict__ gate, const bf16_t* __restrict__ up, bf16_t* __restrict__ out, int I) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= 2 * I) return;
    const int G = r >> 6, wi = r & 63;
    out[r] = wi < 32 ? gate[G * 32 + wi] : up[G * 32 + wi - 32];
}

__global__ void convert_kernel(const void* __restrict__ src, int dtype, bf16_t* __restrict__ dst, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    if (dtype == DOTS_DTYPE_F32) dst[i] = f2bf(reinterpret_cast<const float*>(src)[i]);
    else if (dtype == DOTS_DTYPE_F16) dst[i] = f2bf(__half2float(reinterpret_cast<const __half*>(src)[i]));
    else dst[i] = reinterpret_cast<const bf16_t*>(src)[i];
}

// rows [n, K] -> [n, Kpad] zero padded
__global__ void pad_rows_kernel(const bf16_t* __restrict__ src, bf16_t* __restrict__ dst, int n, int K, int Kpad) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)n * Kpad) return;
    const int r = (int)(i / Kpad), c = (int)(i % Kpad);
    dst[i] = c < K ? src[(size_t)r * K + c] : (bf16_t)0;
}
}  // namespace

hipError_t launch_pack_w13(hipStream_t s, const bf16_t* gate, const bf16_t* up, bf16_t* out, int I, int K) {
    const int64_t n = (int64_t)2 * I * (K / 8);
    hipLaunchKernelGGL(pack_w13_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, gate, up, out, I, K);
    return hipGetLastError();
}
hipError_t launch_convert_to_bf16(hipStream_t s, const void* src, int dtype, bf16_t* dst, int64_t n) {
    hipLaunchKernelGGL(convert_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, src, dtype, dst, n);
    return hipGetLastError();
}

namespace engine {
namespace {
// ---------------------------------------------------------------------------------- weights
const Tensor* find(DotsEngine* e, const std::string& name) {
    auto it = e->raw.find(name);
    return it == e->raw.end() ? nullptr : &it->second;
}

int need(DotsEngine* e, const std::string& name, std::initializer_list<int64_t> shape, bf16_t** out) {
    const Tensor* t = find(e, name);
    if (!t) return e->fail(DOTS_E_STATE, "missing weight %s", name.c_str());
    if (t->shape != std::vector<int64_t>(shape)) return e->fail(DOTS_E_INVALID, "weight %s has unexpected shape", name.c_str());
    *out = t->p;
    return DOTS_OK;
}

int optional(DotsEngine* e, const std::string& name, std::initializer_list<int64_t> shape, bf16_t** out) {
    const Tensor* t = find(e, name);
    *out = nullptr;
    if (!t) return DOTS_OK;
    if (t->shape != std::vector<int64_t>(shape)) return e->fail(DOTS_E_INVALID, "weight %s has unexpected shape", name.c_str());
    *out = t->p;
    return DOTS_OK;
}

void drop(DotsEngine* e, const std::string& name) {
    auto it = e->raw.find(name);
    if (it == e->raw.end()) return;
    e->release(it->second.p);
    e->raw.erase(it);
}

// fp8 mode: W <- bf16(q) in place + a fresh scale array + the e4m3 bytes row-major; bf16 mode: *scale = *w8 = nullptr
int quantize(DotsEngine* e, bf16_t* W, float** scale, int64_t N, int K, uint8_t** w8 = nullptr) {
    *scale = nullptr;
    if (w8) *w8 = nullptr;
    if (!e->cfg.fp8_weights) return DOTS_OK;
    CK(e->alloc(scale, (size_t)N));
    CK(launch_quant_rows_fp8(e->stream, W, *scale, N, K));
    if (w8) {
        if (!gemm_fp8_supports((int)N, K)) return e->fail(DOTS_E_INVALID, "fp8_weights: a %lld x %d linear does not fit the fp8 GEMM (N %% 256, K %% 64)", (long long)N, K);
        CK(e->alloc(w8, (size_t)N * K));
        CK(launch_bf16q_to_fp8(e->stream, W, *w8, N * K));
    }
    return DOTS_OK;
}

// decode copy of a (quantised) row-major matrix: bf16 fragments, or e4m3 fragments in fp8 mode
int decode_copy(DotsEngine* e, const bf16_t* W, void** out, int64_t rows, int K, int rot_rows) {
    const size_t elems = (size_t)((rows + 15) / 16 * 16) * K;
    if (e->cfg.fp8_weights) {
        uint8_t* d = nullptr;
        CK(e->alloc(&d, elems));
        CK(launch_pack_frag_fp8(e->stream, W, d, rows, K, rot_rows));
        *out = d;
    } else {
        bf16_t* d = nullptr;
        CK(e->alloc(&d, elems));
        if (rot_rows) CK(launch_pack_frag_qkv(e->stream, W, d, e->cfg.num_heads, e->cfg.num_kv_heads, K));
        else CK(launch_pack_frag(e->stream, W, d, rows, K));
        *out = d;
    }
    return DOTS_OK;
}

int finalize_weights(DotsEngine* e) {
    const DotsConfig& c = e->cfg;
    hipStream_t s = e->stream;
    const int E = c.v_embed_dim, Iv = c.v_intermediate;
    // ---- vision
    {
        const std::string pre = "vision_tower.patch_embed.patchifier.";
        const Tensor* pw = find(e, pre + "proj.weight");
        if (!pw) return e->fail(DOTS_E_STATE, "missing weight %sproj.weight", pre.c_str());
        const int K = c.v_channels * c.v_patch * c.v_patch;
        if (pw->numel() != (int64_t)E * K) return e->fail(DOTS_E_INVALID, "patch embed weight has unexpected size");
        e->patch_k = K;
        e->patch_kpad = (int)round_up(K, 64);
        CK(e->alloc(&e->patch_w, (size_t)E * e->patch_kpad));
        const int64_t n = (int64_t)E * e->patch_kpad;
        hipLaunchKernelGGL(pad_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, pw->p, e->patch_w, E, K, e->patch_kpad);
        RET(optional(e, pre + "proj.bias", {E}, &e->patch_b));
        RET(need(e, pre + "norm.weight", {E}, &e->patch_norm));
    }
    e->vl.resize(c.v_layers);
    for (int i = 0; i < c.v_layers; ++i) {
        const std::string p = "vision_tower.blocks." + std::to_string(i) + ".";
        VLayer& L = e->vl[i];
        RET(need(e, p + "norm1.weight", {E}, &L.norm1));
        RET(need(e, p + "attn.qkv.weight", {3 * E, E}, &L.qkv_w));
        RET(optional(e, p + "attn.qkv.bias", {3 * E}, &L.qkv_b));
        RET(need(e, p + "attn.proj.weight", {E, E}, &L.proj_w));
        RET(optional(e, p + "attn.proj.bias", {E}, &L.proj_b));
        RET(need(e, p + "norm2.weight", {E}, &L.norm2));
        bf16_t *f1, *f3, *b1, *b3;
        RET(need(e, p + "mlp.fc1.weight", {Iv, E}, &f1));
        RET(need(e, p + "mlp.fc3.weight", {Iv, E}, &f3));
        RET(need(e, p + "mlp.fc2.weight", {E, Iv}, &L.w2));
        RET(optional(e, p + "mlp.fc1.bias", {Iv}, &b1));
        RET(optional(e, p + "mlp.fc3.bias", {Iv}, &b3));
        RET(optional(e, p + "mlp.fc2.bias", {E}, &L.b2));
        CK(e->alloc(&L.w13, (size_t)2 * Iv * E));
        CK(launch_pack_w13(s, f1, f3, L.w13, Iv, E));
        L.b13 = nullptr;
        if (b1 && b3) {
            CK(e->alloc(&L.b13, (size_t)2 * Iv));
            hipLaunchKernelGGL(pack_b13_kernel, dim3((2 * Iv + 255) / 256), dim3(256), 0, s, b1, b3, L.b13, Iv);
        }
        RET(quantize(e, L.qkv_w, &L.qkv_s, 3 * E, E, &L.qkv_8));
        RET(quantize(e, L.proj_w, &L.proj_s, E, E, &L.proj_8));
        RET(quantize(e, L.w13, &L.w13_s, 2 * Iv, E, &L.w13_8));          // packed row order: the scale index the SwiGLU epilogue uses
        RET(quantize(e, L.w2, &L.w2_s, E, Iv, &L.w2_8));
        CK(hipStreamSynchronize(s));
        drop(e, p + "mlp.fc1.weight");
        drop(e, p + "mlp.fc3.weight");
    }
    if (c.v_post_norm) RET(need(e, "vision_tower.post_trunk_norm.weight", {E}, &e->v_post_norm));
    const int Mg = E * c.v_merge * c.v_merge;
    RET(need(e, "vision_tower.merger.ln_q.weight", {E}, &e->m_ln_w));
    RET(need(e, "vision_tower.merger.ln_q.bias", {E}, &e->m_ln_b));
    RET(need(e, "vision_tower.merger.mlp.0.weight", {Mg, Mg}, &e->m0_w));
    RET(need(e, "vision_tower.merger.mlp.0.bias", {Mg}, &e->m0_b));
    RET(need(e, "vision_tower.merger.mlp.2.weight", {c.hidden_size, Mg}, &e->m2_w));
    RET(need(e, "vision_tower.merger.mlp.2.bias", {c.hidden_size}, &e->m2_b));
    RET(quantize(e, e->m0_w, &e->m0_s, Mg, Mg, &e->m0_8));
    RET(quantize(e, e->m2_w, &e->m2_s, c.hidden_size, Mg, &e->m2_8));

    // ---- language model
    const int H = c.hidden_size, I = c.intermediate_size, Nq = c.num_heads * 128, Nkv = c.num_kv_heads * 128;
    RET(need(e, "model.embed_tokens.weight", {c.vocab_size, H}, &e->embed));
    RET(need(e, "model.norm.weight", {H}, &e->final_norm));
    if (find(e, "lm_head.weight")) RET(need(e, "lm_head.weight", {c.vocab_size, H}, &e->lm_head));
    else e->lm_head = e->embed;                      // tie_word_embeddings
    if (c.fp8_weights) {                             // the embedding table stays bf16: quantise a copy of the (possibly tied) head
        bf16_t* tmp = nullptr;
        CK(hipMalloc(reinterpret_cast<void**>(&tmp), (size_t)c.vocab_size * H * 2));
        hipError_t r = hipMemcpyAsync(tmp, e->lm_head, (size_t)c.vocab_size * H * 2, hipMemcpyDeviceToDevice, s);
        int rc = r == hipSuccess ? quantize(e, tmp, &e->lm_head_s, c.vocab_size, H) : DOTS_E_HIP;
        if (rc == DOTS_OK) rc = decode_copy(e, tmp, &e->lm_head_d, c.vocab_size, H, 0);
        hipStreamSynchronize(s);
        hipFree(tmp);
        if (rc != DOTS_OK) return r == hipSuccess ? rc : e->fail(DOTS_E_HIP, "lm_head copy failed: %s", hipGetErrorString(r));
    } else {
        RET(decode_copy(e, e->lm_head, &e->lm_head_d, c.vocab_size, H, 0));
    }
    e->ll.resize(c.num_layers);
    for (int i = 0; i < c.num_layers; ++i) {
        const std::string p = "model.layers." + std::to_string(i) + ".";
        LLayer& L = e->ll[i];
        RET(need(e, p + "input_layernorm.weight", {H}, &L.ln1));
        RET(need(e, p + "post_attention_layernorm.weight", {H}, &L.ln2));
        bf16_t *qw, *kw, *vw, *qb, *kb, *vb, *gw, *uw;
        RET(need(e, p + "self_attn.q_proj.weight", {Nq, H}, &qw));
        RET(need(e, p + "self_attn.k_proj.weight", {Nkv, H}, &kw));
        RET(need(e, p + "self_attn.v_proj.weight", {Nkv, H}, &vw));
        RET(optional(e, p + "self_attn.q_proj.bias", {Nq}, &qb));
        RET(optional(e, p + "self_attn.k_proj.bias", {Nkv}, &kb));
        RET(optional(e, p + "self_attn.v_proj.bias", {Nkv}, &vb));
        RET(need(e, p + "self_attn.o_proj.weight", {H, Nq}, &L.o_w));
        RET(need(e, p + "mlp.gate_proj.weight", {I, H}, &gw));
        RET(need(e, p + "mlp.up_proj.weight", {I, H}, &uw));
        RET(need(e, p + "mlp.down_proj.weight", {H, I}, &L.down_w));
        CK(e->alloc(&L.qkv_w, (size_t)(Nq + 2 * Nkv) * H));
        CK(hipMemcpyAsync(L.qkv_w, qw, (size_t)Nq * H * 2, hipMemcpyDeviceToDevice, s));
        CK(hipMemcpyAsync(L.qkv_w + (size_t)Nq * H, kw, (size_t)Nkv * H * 2, hipMemcpyDeviceToDevice, s));
        CK(hipMemcpyAsync(L.qkv_w + (size_t)(Nq + Nkv) * H, vw, (size_t)Nkv * H * 2, hipMemcpyDeviceToDevice, s));
        L.qkv_b = nullptr;
        if (qb && kb && vb) {
            CK(e->alloc(&L.qkv_b, (size_t)(Nq + 2 * Nkv)));
            CK(hipMemcpyAsync(L.qkv_b, qb, (size_t)Nq * 2, hipMemcpyDeviceToDevice, s));
            CK(hipMemcpyAsync(L.qkv_b + Nq, kb, (size_t)Nkv * 2, hipMemcpyDeviceToDevice, s));
            CK(hipMemcpyAsync(L.qkv_b + Nq + Nkv, vb, (size_t)Nkv * 2, hipMemcpyDeviceToDevice, s));
        }
        CK(e->alloc(&L.w13, (size_t)2 * I * H));
        CK(launch_pack_w13(s, gw, uw, L.w13, I, H));
        RET(quantize(e, L.qkv_w, &L.qkv_s, Nq + 2 * Nkv, H, &L.qkv_8));
        RET(quantize(e, L.o_w, &L.o_s, H, Nq, &L.o_8));
        RET(quantize(e, L.w13, &L.w13_s, 2 * I, H, &L.w13_8));
        RET(quantize(e, L.down_w, &L.down_s, H, I, &L.down_8));
        // decode copies in MFMA fragment order (+3.1 GB of 288 GB, half of that in fp8 mode: every decode weight load is one contiguous chunk)
        RET(decode_copy(e, L.qkv_w, &L.qkv_wd, Nq + 2 * Nkv, H, Nq + Nkv));                   // q / k rows permuted: whole RoPE pairs per tile
        RET(decode_copy(e, L.o_w, &L.o_wd, H, Nq, 0));
        RET(decode_copy(e, L.w13, &L.w13_wd, 2 * I, H, 0));
        RET(decode_copy(e, L.down_w, &L.down_wd, H, I, 0));
        CK(hipStreamSynchronize(s));
        for (const char* n : {"self_attn.q_proj.weight", "self_attn.k_proj.weight", "self_attn.v_proj.weight",
                              "mlp.gate_proj.weight", "mlp.up_proj.weight"})
            drop(e, p + n);
    }
    // ---- rope frequency tables (same fp32 formula as the oracle / transformers)
    {
        std::vector<float> vf(32), lf(64);
        for (int i = 0; i < 32; ++i) vf[i] = 1.0f / powf(10000.0f, (float)(2 * i) / 64.0f);
        for (int i = 0; i < 64; ++i) lf[i] = 1.0f / powf(c.rope_theta, (float)(2 * i) / 128.0f);
        CK(e->alloc(&e->v_inv_freq, 32));
        CK(e->alloc(&e->lm_inv_freq, 64));
        CK(hipMemcpyAsync(e->v_inv_freq, vf.data(), 32 * 4, hipMemcpyHostToDevice, s));
        CK(hipMemcpyAsync(e->lm_inv_freq, lf.data(), 64 * 4, hipMemcpyHostToDevice, s));
        CK(hipStreamSynchronize(s));
    }
    e->finalized = true;
    return DOTS_OK;
}
}  // namespace

int alloc_workspaces(DotsEngine* e) {
    const DotsConfig& c = e->cfg;
    const int E = c.v_embed_dim, H = c.hidden_size, Nq = c.num_heads * 128, Nkv = c.num_kv_heads * 128;
    const int Mg = E * c.v_merge * c.v_merge;
    e->P = c.max_patches;
    e->Ppad = e->P + 64 * 256;                    // every image padded to a multiple of 64 keys
    const int kpad = (int)round_up(c.v_channels * c.v_patch * c.v_patch, 64);
    if (c.fp8_weights) {
        const size_t v_max = (size_t)e->P * std::max(E, c.v_intermediate);          // the merger's inputs are [P / g][E g]: P E bytes as well
        const size_t p_max = (size_t)c.max_prefill_tokens * std::max(H, std::max(Nq, c.intermediate_size));
        CK(e->alloc(&e->act_q, p_max));
        CK(e->alloc(&e->act_s, (size_t)c.max_prefill_tokens));
        CK(e->alloc(&e->act_q_v, v_max));
        CK(e->alloc(&e->act_s_v, (size_t)e->P));
    }
    CK(e->alloc(&e->v_xa, (size_t)e->P * kpad));
    CK(e->alloc(&e->v_x, (size_t)e->P * E));
    CK(e->alloc(&e->v_xn, (size_t)e->P * E));
    CK(e->alloc(&e->v_qkv, (size_t)e->P * 3 * E));
    CK(e->alloc(&e->v_q, (size_t)e->P * E));
    CK(e->alloc(&e->v_k, (size_t)(e->P + 64) * E));
    CK(e->alloc(&e->v_vt, (size_t)e->Ppad * E));
    CK(e->alloc(&e->v_att, (size_t)e->P * E));
    CK(e->alloc(&e->v_act, (size_t)e->P * c.v_intermediate));
    CK(e->alloc(&e->v_mh, (size_t)(e->P / 4 + 1) * Mg));
    CK(e->alloc(&e->vis, (size_t)(e->P / 4 + 1) * H));
    CK(e->alloc(&e->vis_pref, (size_t)(e->P / 4 + 1) * H));
    CK(e->alloc(&e->v_cs, (size_t)e->P * 64));
    CK(e->alloc(&e->v_pos, (size_t)e->P * 2));
    CK(e->alloc(&e->v_tiles, (size_t)(e->P / 64 + 256)));
    CK(e->alloc(&e->v_qblocks, (size_t)(e->P / 128 + 256) * c.v_heads));

    e->TP = c.max_prefill_tokens;
    e->TPpad = e->TP + 64 * c.max_batch;
    CK(e->alloc(&e->p_x, (size_t)e->TP * H));
    CK(e->alloc(&e->p_xn, (size_t)e->TP * H));
    CK(e->alloc(&e->p_qkv, (size_t)e->TP * (Nq + 2 * Nkv)));
    CK(e->alloc(&e->p_q, (size_t)e->TP * Nq));
    CK(e->alloc(&e->p_k, (size_t)(e->TP + 64) * Nkv));
    CK(e->alloc(&e->p_vt, (size_t)e->TPpad * Nkv));
    CK(e->alloc(&e->p_att, (size_t)e->TP * Nq));
    CK(e->alloc(&e->p_act, (size_t)e->TP * c.intermediate_size));
    CK(e->alloc(&e->p_cs, (size_t)e->TP * 64));
    CK(e->alloc(&e->p_pos, (size_t)e->TP));
    CK(e->alloc(&e->p_src, (size_t)e->TP));
    CK(e->alloc(&e->p_last, (size_t)DOTS_MAX_BATCH));
    CK(e->alloc(&e->p_tiles, (size_t)(e->TP / 64 + c.max_batch + 1)));
    CK(e->alloc(&e->p_qblocks, (size_t)(e->TP / 128 + c.max_batch + 1) * c.num_heads));

    e->max_pages = (c.max_seq_len + 63) / 64;
    // paged KV: a pool of 64-token pages shared by all sequence slots; a sequence reserves ceil((prompt + generation cap) / 64)
    // pages when it is prefilled and returns them when its slot is released (kv_pool_tokens = 0: room for max_batch sequences
    // of max_seq_len, i.e. no sequence can ever be refused for lack of pages)
    const int64_t pool_tokens = c.kv_pool_tokens > 0 ? c.kv_pool_tokens : (int64_t)c.max_batch * e->max_pages * 64;
    e->n_pool_pages = (int)((pool_tokens + 63) / 64);
    e->kv8 = c.kv_cache_dtype == 1;
    e->pool_layer_elems = (size_t)(e->n_pool_pages + 1) * c.num_kv_heads * 2 * 8192 / (e->kv8 ? 2 : 1);
    CK(e->alloc(&e->pool, e->pool_layer_elems * c.num_layers));
    const std::vector<float> kv_ones((size_t)c.num_layers * c.num_kv_heads * 2, 1.0f);      // lives until the stream is synchronised below
    CK(e->alloc(&e->kv_scales, kv_ones.size()));
    CK(hipMemcpyAsync(e->kv_scales, kv_ones.data(), kv_ones.size() * 4, hipMemcpyHostToDevice, e->stream));
    const int mb = (c.max_batch + 15) / 16 * 16;            // rows of the decode buffers: whole 16-row tiles
    CK(e->alloc(&e->block_table, (size_t)mb * e->max_pages));
    CK(e->alloc(&e->ctx_len, (size_t)mb));
    CK(e->alloc(&e->cur_tokens, (size_t)mb));
    CK(e->alloc(&e->out_ids, (size_t)mb * c.max_seq_len));
    CK(e->alloc(&e->out_lens, (size_t)mb));
    CK(e->alloc(&e->finished, (size_t)mb));
    CK(e->alloc(&e->eos_ids, (size_t)16));
    CK(e->alloc(&e->d_sel, (size_t)DOTS_MAX_BATCH));
    CK(e->alloc(&e->d_sel_new, (size_t)DOTS_MAX_BATCH));
    CK(e->alloc(&e->d_max_len, (size_t)DOTS_MAX_BATCH));
    CK(e->alloc(&e->p_dst, (size_t)DOTS_MAX_BATCH));
    CK(e->alloc(&e->fk_dev, (size_t)3 * DOTS_MAX_BATCH));
    CK(e->alloc(&e->am_idx, (size_t)mb * 64));
    CK(e->alloc(&e->am_val, (size_t)mb * 64));
    CK(e->alloc(&e->d_h, (size_t)mb * H));
    CK(e->alloc(&e->d_q, (size_t)mb * Nq));
    CK(e->alloc(&e->d_att, (size_t)mb * Nq));
    CK(e->alloc(&e->d_act, (size_t)mb * c.intermediate_size));
    CK(e->alloc(&e->d_xn, (size_t)DOTS_MAX_BATCH * H));
    CK(e->alloc(&e->d_part_h, (size_t)DEC_KSPLIT_PARTS * DOTS_MAX_BATCH * H));
    CK(e->alloc(&e->d_logits, (size_t)mb * c.vocab_size));
    CK(e->alloc(&e->d_part_o, (size_t)mb * c.num_heads * 64 * 128));
    CK(e->alloc(&e->d_part_ml, (size_t)mb * c.num_heads * 64 * 2));
    if (const char* fm = sw::read_now(sw::DECODE_PLAN)) {          // per engine (refused, not re-interpreted)
        const sw::DecodePlan plan = sw::parse_decode_plan(fm);
        if (!plan.ok) {
            fprintf(stderr, "dots.ocr: %s=%s ignored: must be 0 / 1 (partition plan on every step), + 2 (streaming attention) or + 4 (per-split attention)\n", sw::DECODE_PLAN, fm);
        } else {
            e->force_part = plan.force_part;
            e->attn_stream = plan.attn_stream;
        }
    }
    if (const char* v = sw::read_now(sw::TOWER_TAIL_LAYERS)) e->tail_fixed = sw::parse_tower_tail_layers(v, c.v_layers);      // per engine; dots_tower_tail
    // every slot starts free: its block-table row points at the scratch page (an idle row of the fixed-shape decode graph
    // keeps appending K/V at position 0 of whatever page its row names; it must never be a page a live sequence owns)
    e->hp_table.assign((size_t)mb * e->max_pages, e->n_pool_pages);
    e->slot_pages.assign(mb, {});
    e->free_pages.resize(e->n_pool_pages);
    e->page_refs.assign(e->n_pool_pages, 0);
    for (int p = 0; p < e->n_pool_pages; ++p) e->free_pages[p] = e->n_pool_pages - 1 - p;      // pop_back hands out page 0 first
    CK(hipMemcpyAsync(e->block_table, e->hp_table.data(), e->hp_table.size() * 4, hipMemcpyHostToDevice, e->stream));
    for (auto& ev : e->ev) CK(hipEventCreate(&ev));
    CK(hipStreamSynchronize(e->stream));
    return DOTS_OK;
}
}  // namespace engine

using namespace engine;
extern "C" {
int dots_load_weight(DotsEngine* e, const char* name, const void* data, int dtype, const int64_t* shape, int ndim) {
    if (!e || !name || !data || !shape || ndim < 1) return e ? e->fail(DOTS_E_INVALID, "null argument") : DOTS_E_INVALID;
    if (e->finalized) return e->fail(DOTS_E_STATE, "weights already finalized");
    CK(hipSetDevice(e->device));
    Tensor t;
    t.shape.assign(shape, shape + ndim);
    const int64_t n = t.numel();
    const size_t esz = dtype == DOTS_DTYPE_F32 ? 4 : 2;
    if (dtype != DOTS_DTYPE_BF16 && dtype != DOTS_DTYPE_F32 && dtype != DOTS_DTYPE_F16) return e->fail(DOTS_E_INVALID, "unsupported dtype %d", dtype);
    CK(e->alloc(&t.p, (size_t)n));
    if (dtype == DOTS_DTYPE_BF16) {
        CK(hipMemcpyAsync(t.p, data, n * 2, hipMemcpyHostToDevice, e->stream));
        CK(hipStreamSynchronize(e->stream));
    } else {
        void* tmp = nullptr;
        CK(hipMalloc(&tmp, n * esz));
        CK(hipMemcpyAsync(tmp, data, n * esz, hipMemcpyHostToDevice, e->stream));
        CK(launch_convert_to_bf16(e->stream, tmp, dtype, t.p, n));
        CK(hipStreamSynchronize(e->stream));
        hipFree(tmp);
    }
    drop(e, name);
    e->raw[name] = t;
    return DOTS_OK;
}

int dots_finalize_weights(DotsEngine* e) {
    if (!e) return DOTS_E_INVALID;
    if (e->finalized) return DOTS_OK;
    CK(hipSetDevice(e->device));
    return finalize_weights(e);
}
}  // extern "C"
