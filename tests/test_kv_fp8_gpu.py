"""The opt-in fp8 (OCP e4m3fn) paged KV cache (DotsConfig.kv_cache_dtype = 1; csrc/decode.hip header).

Numerics contract: one fp32 scale s per (layer, kv head, K|V); the cache stores e4m3fn(clamp(x / s, -448, 448)) (fp32 division, round to
nearest even) of exactly the bf16 value x the bf16 cache would hold, and reads back float(stored) * s.  Prefill attention runs on its bf16
buffers; every decode step reads the fp8 cache for all positions, its own token included.  So:

  1. the decode writer (dec_qkv at every batch path, bf16 and e4m3 weights) stores the torch quantisation of what the bf16 writer stores, bit
     for bit, saturating to +-448, and touches nothing else; q is the bf16 writer's q, bit for bit;
  2. the prefill writer likewise (static, packed multi-sequence and slot prefill; read back with Engine.read_kv);
  3. the attention kernel matches fp32 attention over the dequantised K / V within the bf16 attention test's tolerance;
  4. the whole model matches the oracle with a quantised-history KV cache within the bf16 engine's tolerance — and differs from the bf16 engine;
  5. a row's bits do not depend on its batch (1 / 8 / 33 / 64 rows), and slots (graph replay) equal static generate;
  6. the planted walk at the real dimensions decodes 32 / 32 with the fp8 cache;
  7. the scale rules: refused while pages are held; the same page count as a bf16 cache of the same kv_pool_tokens.
"""
import math

import numpy as np
import pytest
import torch

from oracle import model as om
from test_decode_kernels_gpu import K_IDX, V_IDX, close

pytestmark = pytest.mark.gpu

H, HQ, HKV = 1536, 12, 2
EPS, THETA = 1e-6, 1e6
NAN8 = 0x7F                       # an e4m3fn NaN: the saturating writers never produce it


def _kv8_byte(e):
    """element offset in a bf16 page -> byte offset in an fp8 page (decode_layout.h kv8_byte: chunk pairs interleaved per lane)"""
    return (e & ~1023) | (((e >> 3) & 63) << 4) | (((e >> 9) & 1) << 3) | (e & 7)


K8_IDX, V8_IDX = _kv8_byte(K_IDX), _kv8_byte(V_IDX)
assert sorted(K8_IDX.flatten().tolist()) == list(range(8192)) and sorted(V8_IDX.flatten().tolist()) == list(range(8192))


def quant(x, s):
    """the contract's stored value: raw e4m3fn bytes (uint8) of x (bf16 / fp32) with scale s (broadcastable fp32)"""
    return x.float().div(s).clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8)


def dequant(b, s):
    return b.view(torch.float8_e4m3fn).float() * s


def dev(x):
    return x.cuda().contiguous()


@pytest.fixture(scope="module")
def eng():
    from dots_ocr_amd.config import DotsConfig
    from dots_ocr_amd.engine import Engine
    e = Engine(DotsConfig.tiny(), max_batch=2, max_seq_len=256, max_patches=256, max_prefill_tokens=256, kv_cache_dtype="bf16")
    yield e
    e.close()


# ------------------------------------------------------------------------------------------------ 1. decode writer
@pytest.mark.parametrize("plan,B", [(0, b) for b in (1, 5, 8, 16, 17, 33, 64)] + [(1, 8), (1, 33)])      # plan 1: the partition plan's kernels
@pytest.mark.parametrize("fp8w", [False, True])
@pytest.mark.parametrize("unit", [True, False])
def test_dec_qkv_kv8_writer_is_the_quantised_bf16_writer(eng, plan, B, fp8w, unit):
    g = torch.Generator().manual_seed(300 + B + 7 * fp8w + 3 * unit + 11 * plan)
    h = (torch.randn(B, H, generator=g) * 2).bfloat16()
    ln_w = (1 + 0.1 * torch.randn(H, generator=g)).bfloat16()
    W = (torch.randn((HQ + 2 * HKV) * 128, H, generator=g) * 0.02).bfloat16()
    bias = (torch.randn((HQ + 2 * HKV) * 128, generator=g) * 0.1).bfloat16()
    positions = [(977 * i + 63 * (i % 3)) % 7000 for i in range(B)]
    max_pages = 128
    n_pages = B + 3
    perm = torch.randperm(n_pages, generator=g)[:B]
    table = torch.zeros(B, max_pages, dtype=torch.int32)
    for b in range(B):
        table[b, positions[b] >> 6] = int(perm[b])
    # per-head scales; the non-unit set makes K head 1 saturate (|k| ~ 0.8: 0.8 / 0.0015 > 448)
    scales = torch.ones(HKV, 2) if unit else torch.tensor([[0.013, 0.011], [0.0015, 0.02]])
    pool16 = dev(torch.full((n_pages, HKV, 2, 8192), 0x7F7F, dtype=torch.int16))
    pool8 = dev(torch.full((n_pages, HKV, 2, 8192), NAN8, dtype=torch.uint8))
    q16 = torch.zeros(B, HQ * 128, dtype=torch.bfloat16, device="cuda")
    q8 = torch.zeros_like(q16)
    hd, lnd, Wd_, bd, ctx_d, tab_d, sc_d = dev(h), dev(ln_w), dev(W), dev(bias), dev(torch.tensor(positions, dtype=torch.int32)), dev(table), dev(scales)
    torch.cuda.synchronize()
    eng.set_decode_plan(plan)
    try:
        eng.op_dec_qkv(hd.data_ptr(), lnd.data_ptr(), Wd_.data_ptr(), bd.data_ptr(), ctx_d.data_ptr(), tab_d.data_ptr(), max_pages,
                       pool16.data_ptr(), q16.data_ptr(), B, H, HQ, HKV, EPS, THETA, fp8=fp8w)
        eng.op_dec_qkv_kv8(hd.data_ptr(), lnd.data_ptr(), Wd_.data_ptr(), bd.data_ptr(), ctx_d.data_ptr(), tab_d.data_ptr(), max_pages,
                           pool8.data_ptr(), q8.data_ptr(), B, H, HQ, HKV, EPS, THETA, sc_d.data_ptr(), fp8=fp8w)
    finally:
        eng.set_decode_plan(0)
    assert torch.equal(q8.view(torch.int16).cpu(), q16.view(torch.int16).cpu()), "q differs from the bf16 writer's"
    got16, got8 = pool16.cpu(), pool8.cpu()
    touched = torch.zeros_like(got8, dtype=torch.bool)
    saturated = 0
    for b in range(B):
        pg, key = int(table[b, positions[b] >> 6]), positions[b] & 63
        for hk in range(HKV):
            for which, i16, i8 in ((0, K_IDX, K8_IDX), (1, V_IDX, V8_IDX)):
                x = got16[pg, hk, which][i16[key]].view(torch.bfloat16)
                want = quant(x, scales[hk, which])
                have = got8[pg, hk, which][i8[key]]
                assert torch.equal(have, want), f"row {b} head {hk} {'KV'[which]}: {int((have != want).sum())} of 128 bytes differ"
                touched[pg, hk, which][i8[key]] = True
                saturated += int(((have & 0x7F) == 0x7E).sum())
    assert (got8[~touched] == NAN8).all(), "the fp8 append wrote outside the new token's slots"
    assert not ((got8[touched] & 0x7F) == 0x7F).any(), "an fp8 slot holds NaN"
    if not unit:
        assert saturated > 0, "no value reached the saturation path"


# ------------------------------------------------------------------------------------------------ 2. prefill writer
def _prompts(cfg, lens, seed):
    rng = np.random.default_rng(seed)
    hi = min(cfg.vocab_size, cfg.image_token_id) - 1
    return [rng.integers(0, hi, n).astype(np.int32) for n in lens]


@pytest.fixture(scope="module")
def tiny_pair():
    from dots_ocr_amd.config import DotsConfig
    from dots_ocr_amd.engine import Engine
    from dots_ocr_amd.weights import random_state_dict
    cfg = DotsConfig.tiny(layers=3, v_layers=2, vocab=1024)
    sd = random_state_dict(cfg, seed=21)
    kw = dict(max_batch=64, max_seq_len=640, max_patches=1024, max_prefill_tokens=16384)
    e16 = Engine(cfg, kv_cache_dtype="bf16", **kw)
    e8 = Engine(cfg, kv_cache_dtype="fp8", **kw)
    e16.load_state_dict(sd)
    e8.load_state_dict(sd)
    rng = np.random.default_rng(4)
    scales = (0.5 + rng.random((cfg.num_hidden_layers, cfg.num_key_value_heads, 2))).astype(np.float32)
    e8.set_kv_scales(scales)
    yield cfg, sd, e16, e8, torch.from_numpy(scales)
    e16.close()
    e8.close()


def _check_prefill_kv(cfg, e16, e8, scales, rows_lens):
    for layer in range(cfg.num_hidden_layers):
        for row, n in rows_lens:
            for which, wi in (("k", 0), ("v", 1)):
                x = torch.from_numpy(e16.read_kv(layer, row, 0, n, which).view(np.int16)).view(torch.bfloat16)      # [Hkv, n, 128]
                want = quant(x, scales[layer, :, wi].view(-1, 1, 1))
                have = torch.from_numpy(e8.read_kv(layer, row, 0, n, which))
                assert torch.equal(have, want), f"layer {layer} row {row} {which}: {int((have != want).sum())} bytes differ"


def test_prefill_writer_static_packed_and_slots(tiny_pair):
    cfg, sd, e16, e8, scales = tiny_pair
    seqs = _prompts(cfg, [200, 70, 5, 64], seed=1)               # 200: four pages; 64: one full page
    ids, lens = np.concatenate(seqs), np.asarray([len(s) for s in seqs], np.int32)
    for e in (e16, e8):
        e.prefill(ids, lens)
    _check_prefill_kv(cfg, e16, e8, scales, list(enumerate(lens.tolist())))
    one = _prompts(cfg, [150], seed=2)[0]
    for e in (e16, e8):
        e.slots_reset()
        e.slots_prefill([5], one, [len(one)], [8])
    _check_prefill_kv(cfg, e16, e8, scales, [(5, len(one))])
    for e in (e16, e8):
        e.slots_reset()


# ------------------------------------------------------------------------------------------------ 3. attention kernel
@pytest.mark.parametrize("ctxs,max_seq_len", [
    ([1], 64),
    ([1, 63, 64, 65, 1000, 6000, 0, 127], 6224),
    ([(613 * i) % 6001 for i in range(62)] + [6000, 1000], 6224),
])
def test_decode_attention_kv8_matches_dequantised_oracle(eng, ctxs, max_seq_len):
    B = len(ctxs)
    g = torch.Generator().manual_seed(sum(ctxs) + B)
    max_pages = (max_seq_len + 63) // 64
    n_pages = [(c + 1 + 63) // 64 for c in ctxs]
    total = sum(n_pages)
    perm = torch.randperm(total + 2, generator=g)
    table = torch.zeros(B, max_pages, dtype=torch.int32)
    pool = torch.empty(total + 2, HKV, 2, 8192, dtype=torch.uint8)
    pool[:, :, :, 0::2] = 0x7E                                   # +448 / -448 wherever nothing is packed: keys past ctx must be masked
    pool[:, :, :, 1::2] = 0xFE
    scales = torch.tensor([[0.015, 0.011], [0.02, 0.03]])
    q = torch.randn(B, HQ, 128, generator=g).bfloat16()
    refs, off = [], 0
    for b, c in enumerate(ctxs):
        n = c + 1
        K8 = quant(torch.randn(n, HKV, 128, generator=g).bfloat16(), scales[:, 0].view(1, HKV, 1))
        V8 = quant(torch.randn(n, HKV, 128, generator=g).bfloat16(), scales[:, 1].view(1, HKV, 1))
        table[b, :n_pages[b]] = perm[off:off + n_pages[b]].to(torch.int32)
        off += n_pages[b]
        for p in range(n_pages[b]):
            m, pg = min(64, n - p * 64), int(table[b, p])
            for hk in range(HKV):
                pool[pg, hk, 0][K8_IDX[:m].reshape(-1)] = K8[p * 64:p * 64 + m, hk].reshape(-1)
                pool[pg, hk, 1][V8_IDX[:m].reshape(-1)] = V8[p * 64:p * 64 + m, hk].reshape(-1)
        Kf = dequant(K8, scales[:, 0].view(1, HKV, 1)).transpose(0, 1).repeat_interleave(HQ // HKV, 0)
        Vf = dequant(V8, scales[:, 1].view(1, HKV, 1)).transpose(0, 1).repeat_interleave(HQ // HKV, 0)
        refs.append(om._attention(q[b].float().unsqueeze(1), Kf, Vf, 1 / math.sqrt(128), False, False)[:, 0])
    qd, pd, cd, td, sd_ = dev(q.reshape(B, HQ * 128)), dev(pool), dev(torch.tensor(ctxs, dtype=torch.int32)), dev(table), dev(scales)
    outs = []
    try:
        for plan in (4, 2):                                      # 2 asks for the streaming kernel: an fp8 pool always runs the per-split one
            eng.set_decode_plan(plan)
            out = torch.zeros(B, HQ * 128, dtype=torch.bfloat16, device="cuda")
            torch.cuda.synchronize()
            eng.op_decode_attn_kv8(qd.data_ptr(), pd.data_ptr(), cd.data_ptr(), td.data_ptr(), max_pages, out.data_ptr(), B, HQ, HKV, max_seq_len,
                                   sd_.data_ptr())
            got = out.view(B, HQ, 128).float().cpu()
            for b in range(B):
                close(got[b], refs[b], rel=2 ** -6, abs_=4e-3, what=f"plan {plan} seq {b} ctx {ctxs[b]}")
            outs.append(out.cpu().view(torch.int16))
    finally:
        eng.set_decode_plan(0)
    assert torch.equal(outs[0], outs[1])


# ------------------------------------------------------------------------------------------------ 4. whole model
class QuantKVCache(om.KVCache):
    """The engine's view of its fp8 cache: the prefill pass attends over the raw (bf16) K / V, every single-token step over the dequantised
    history, its own token included."""

    def __init__(self, n_layers, scales):
        super().__init__(n_layers)
        self.scales = scales                                     # [layers, Hkv, 2]

    def append(self, i, k, v):
        K, V = super().append(i, k, v)
        if k.shape[1] > 1:
            return K, V
        s = self.scales[i]
        return dequant(quant(K, s[:, 0].view(-1, 1, 1)), s[:, 0].view(-1, 1, 1)), dequant(quant(V, s[:, 1].view(-1, 1, 1)), s[:, 1].view(-1, 1, 1))


def oracle_kv8_logits(sd, cfg, prompt, forced, scales):
    """bf16-emulated oracle over a quantised-history cache, teacher-forced: logits of the prefill and of len(forced) decode steps."""
    cache = QuantKVCache(cfg.num_hidden_layers, scales)
    emb_w = sd["model.embed_tokens.weight"].float()
    out = [om.lm_forward(sd, cfg, om._r(emb_w[torch.as_tensor(prompt, dtype=torch.long)], True), cache, True)[0]]
    for t in forced:
        out.append(om.lm_forward(sd, cfg, emb_w[torch.tensor([int(t)])], cache, True)[0])
    return out


def test_whole_model_logits_match_quantised_kv_oracle(tiny_pair):
    cfg, sd, e16, e8, scales = tiny_pair
    prompt = _prompts(cfg, [150], seed=3)[0]
    steps = 6
    logits = {}
    for name, e in (("bf16", e16), ("fp8", e8)):
        e.prefill(prompt, np.asarray([len(prompt)], np.int32))
        lg, tk = [e.get_logits()[0].copy()], [int(e.get_last_tokens()[0])]
        for _ in range(steps):
            e.decode_step()
            lg.append(e.get_logits()[0].copy())
            tk.append(int(e.get_last_tokens()[0]))
        logits[name] = (lg, tk)
    lg8, tk8 = logits["fp8"]
    ref = oracle_kv8_logits(sd, cfg, prompt, tk8[:steps], scales)
    for s, (a, r) in enumerate(zip(lg8, ref)):
        rng = float(r.max() - r.min())
        err = float((torch.from_numpy(a) - r).abs().max())
        print(f"step {s}: fp8-KV logit err vs quantised-KV oracle {err:.4f} (range {rng:.2f})")
        assert err < 0.03 * rng, f"step {s}: {err} vs range {rng}"
    assert np.array_equal(lg8[0], logits["bf16"][0][0]), "prefill logits must not see the fp8 cache"
    assert any(not np.array_equal(a, b) for a, b in zip(lg8[1:], logits["bf16"][0][1:])), "fp8-KV decode logits equal the bf16 engine's"


# ------------------------------------------------------------------------------------------------ 5. batch invariance, slots == static
def test_row_bits_do_not_depend_on_the_batch_and_slots_equal_static(tiny_pair):
    cfg, sd, e16, e8, scales = tiny_pair
    seqs = _prompts(cfg, [90 + (37 * i) % 200 for i in range(64)], seed=8)
    steps = 5

    def run(n):
        ids, lens = np.concatenate(seqs[:n]), np.asarray([len(s) for s in seqs[:n]], np.int32)
        e8.prefill(ids, lens)
        out = [e8.get_logits()[0].copy()]
        for _ in range(steps):
            e8.decode_step()
            out.append(e8.get_logits()[0].copy())
        return out

    alone = run(1)
    for n in (8, 33, 64):
        got = run(n)
        for s, (a, b) in enumerate(zip(alone, got)):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), f"row 0 in a batch of {n}: logits differ at step {s}"
    n_new = 12
    few = seqs[:5]
    static = [e8.generate(s, np.asarray([len(s)], np.int32), max_new_tokens=n_new)[0][0].tolist() for s in few]
    e8.slots_reset()
    e8.slots_prefill(list(range(len(few))), np.concatenate(few), [len(s) for s in few], [n_new] * len(few))
    e8.slots_decode(n_new)
    fin, lens = e8.slots_poll()
    assert (fin[:len(few)] == 1).all() and (lens[:len(few)] == n_new).all()
    for i in range(len(few)):
        assert e8.slot_read(i, n_new).tolist() == static[i], f"slot {i} != static generate"
    e8.slots_reset()


# ------------------------------------------------------------------------------------------------ 7. state rules
def test_kv_scales_state_rules_and_pool_pages():
    from dots_ocr_amd.config import DotsConfig
    from dots_ocr_amd.engine import DotsEngineError, Engine
    from dots_ocr_amd.weights import random_state_dict
    cfg = DotsConfig.tiny(layers=2, v_layers=2, vocab=1024)
    kw = dict(max_batch=4, max_seq_len=512, max_patches=256, max_prefill_tokens=1024, kv_pool_tokens=1000)
    e16, e8 = Engine(cfg, kv_cache_dtype="bf16", **kw), Engine(cfg, kv_cache_dtype="fp8", **kw)
    try:
        assert e16.kv_pool_info() == e8.kv_pool_info() == (16, 16)
        e8.load_state_dict(random_state_dict(cfg, seed=2))
        ones = np.ones((cfg.num_hidden_layers, cfg.num_key_value_heads, 2), np.float32)
        e8.set_kv_scales(ones * 0.5)
        for bad in (0.0, -1.0, np.inf, np.nan):
            with pytest.raises(DotsEngineError):
                e8.set_kv_scales(np.where(np.arange(ones.size).reshape(ones.shape) == 3, bad, ones).astype(np.float32))
        e8.slots_reset()
        ids = _prompts(cfg, [70], seed=1)[0]
        e8.slots_prefill([1], ids, [len(ids)], [4])
        assert e8.kv_pool_info()[1] < 16
        with pytest.raises(DotsEngineError):
            e8.set_kv_scales(ones)                               # pages are held
        e8.slot_release(1)
        e8.set_kv_scales(ones)
        e16.set_kv_scales(ones * 2)                              # accepted (unused) by a bf16 cache
    finally:
        e16.close()
        e8.close()


# ------------------------------------------------------------------------------------------------ 6. planted walk at the real dimensions
def test_planted_walk_with_fp8_kv_cache():
    import os

    from dots_ocr_amd.config import DotsConfig
    from dots_ocr_amd.engine import Engine
    from shared_weights import F32View, full_sd
    from test_planted_walk_gpu import N_STEPS, PROMPT, _decode_free_running, _rows, plant_walk
    cfg = DotsConfig()
    torch.set_num_threads(min(os.cpu_count() or 8, 64))
    sd = dict(full_sd(0))
    g = torch.Generator().manual_seed(11)
    prompt = torch.randint(1000, 100000, (PROMPT,), generator=g)
    walk = torch.randperm(100000, generator=g)[:N_STEPS] + 1000
    lm = dict(F32View(sd, skip_prefix="vision_tower."))
    planted, _ = plant_walk(lm, cfg, prompt, walk)
    head = sd["lm_head.weight"].clone()
    head[walk] = planted.to(head.dtype)
    sd["lm_head.weight"] = head
    lm["lm_head.weight"] = head.float()
    eng = Engine(cfg, max_batch=1, max_seq_len=PROMPT + N_STEPS + 64, max_patches=256, max_prefill_tokens=PROMPT + 64, kv_cache_dtype="fp8")
    try:
        eng.load_state_dict(sd)
        lg, tk = _decode_free_running(eng, prompt.numpy().astype(np.int32), N_STEPS)
    finally:
        eng.close()
    scales = torch.ones(cfg.num_hidden_layers, cfg.num_key_value_heads, 2)
    ref = oracle_kv8_logits(lm, cfg, prompt.numpy(), tk[:N_STEPS - 1], scales)
    rows = _rows(lg, tk, ref)
    worst = min(r["oracle_top2_margin"] / max(r["max_abs_logit_err"], 1e-9) for r in rows)
    print(f"fp8-KV planted walk: {sum(int(a == int(b)) for a, b in zip(tk, walk))} / {N_STEPS} tokens on the walk, min margin / error {worst:.1f}, "
          f"max logit error {max(r['max_abs_logit_err'] for r in rows):.4f}")
    assert tk == walk.tolist(), f"fp8-KV engine left the planted walk: {[(r['step'], r['engine_token'], r['oracle_argmax']) for r in rows if not r['token_equal']][:4]}"
    assert worst >= 4.0, worst
