"""The flash (prefill) and decode attention kernels on the probes of tests/attention_probes.py, AT THE SIZES THE BENCHMARK RUNS: indicator V
(every output element is the softmax mass of a class of keys), planted keys on both sides of every boundary the kernels have, poison
behind every sequence — compared element by element, relative, with a plain float64 softmax(q k^T) v.  test_attention_probes_cpu.py shows
that the tolerance comes from the reference (the emulated oracle lies inside a third of it) and that a dropped tile / page / key / split,
a causal mask off by one, a forgotten V^T group order, exchanged page-table entries and unmasked keys past ctx all lie >= 4 x outside it.

The existing bitwise tests (stream vs per-split, partition vs whole chip, fused qkv + rope, batch invariance) stay what they are; here every
decode plan is held to float64 on its own.
"""
import numpy as np
import pytest
import torch

import attention_probes as ap
from test_decode_kernels_gpu import K_IDX, V_IDX
from test_fullsize_gpu import _vt
from test_kv_fp8_gpu import K8_IDX, V8_IDX

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from dots_ocr_amd.config import DotsConfig
    from dots_ocr_amd.engine import Engine
    e = Engine(DotsConfig.tiny(), max_batch=2, max_seq_len=256, max_patches=256, max_prefill_tokens=256)
    yield e
    e.close()


def _poison(shape):
    return torch.full(shape, ap.POISON_BITS, dtype=torch.int16, device="cuda").view(torch.bfloat16)


# ------------------------------------------------------------------------------------------------ prefill
def _flash(eng, seqs, code, causal):
    """the packed batch as the engine lays it out: q / k head-major over the packed tokens (64 poisoned spare K rows behind the last head),
    V^T per sequence padded with zeros to a multiple of 64 keys; the work list is cut over the XCDs by dots_plan_flash_xcd's plan
    (dots_op_flash_attn builds it as the engine does).  -> one [n_i, Hq, 128] per sequence"""
    Hq, Hkv = seqs[0].Hq, seqs[0].Hkv
    lens = [s.n for s in seqs]
    T = sum(lens)
    qd = torch.cat([s.q for s in seqs]).cuda().permute(1, 0, 2).contiguous()
    kd = _poison((Hkv * T + 64, 128))
    kd[:Hkv * T] = torch.cat([s.k for s in seqs]).cuda().permute(1, 0, 2).reshape(Hkv * T, 128)
    vt = torch.cat([_vt(s.v_kernel(code).cuda()) for s in seqs], dim=2).contiguous()
    out = torch.zeros(T, Hq * 128, dtype=torch.bfloat16, device="cuda")
    cu = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    torch.cuda.synchronize()
    eng.op_flash_attn(qd.data_ptr(), kd.data_ptr(), vt.data_ptr(), out.data_ptr(), cu, Hq, Hkv, causal, ap.SCALE)
    eng.synchronize()
    return list(out.view(T, Hq, 128).split(lens))


def _check_prefill(outs, seqs, code, what):
    for out, s in zip(outs, seqs):
        got = out[s.rows].float().cpu()
        worst = ap.assert_close(got, s.reference(code), f"{what} {s.name} {code} code")
        print(f"{what} {s.name} {code}: {len(s.rows)} rows x {s.Hq} heads, worst error {worst:.3f} x the tolerance")


@pytest.mark.parametrize("name", list(ap.PREFILL_PROBES))
def test_flash_attn_bidirectional_probes_match_fp64(eng, name):
    seqs = ap.build("prefill", name)
    if len(seqs) > 1:                                       # the ragged batch: the plan the launch uses covers every work item exactly once
        from dots_ocr_amd.engine import plan_flash_xcd
        base, cnt, cost, n_items = plan_flash_xcd([s.n for s in seqs], seqs[0].Hq)
        assert int(cnt.sum()) == n_items and base.tolist() == [int(cnt[:x].sum()) for x in range(8)] and len(set(cnt.tolist())) > 1
    for code in ap.CODES:
        _check_prefill(_flash(eng, seqs, code, False), seqs, code, name)


def _rope_split(eng, s, code):
    """q, k, V^T of one sequence made by the engine's own split kernel (rope at position 0 is the identity): its V^T permutation and zero padding"""
    T, Hq, Hkv = s.n, s.Hq, s.Hkv
    qkv = torch.cat([s.q.reshape(T, -1), s.k.reshape(T, -1), s.v_kernel(code).reshape(T, -1)], 1).cuda().contiguous()
    qd = torch.zeros(Hq, T, 128, dtype=torch.bfloat16, device="cuda")
    kd = _poison((Hkv * (T + 64), 128))
    vtd = torch.full((Hkv, 128, (T + 63) // 64 * 64), 7.0, dtype=torch.bfloat16, device="cuda")
    cu = np.array([0, T], np.int32)
    torch.cuda.synchronize()
    eng.op_qkv_rope_split(qkv.data_ptr(), qd.data_ptr(), kd.data_ptr(), vtd.data_ptr(), cu, np.zeros(T, np.int32), Hq, Hkv, False, 1e6)
    eng.synchronize()
    assert torch.equal(qd.cpu(), s.q.permute(1, 0, 2)) and torch.equal(kd[:Hkv * T].view(Hkv, T, 128).cpu(), s.k.permute(1, 0, 2))
    return qd, kd, vtd


@pytest.mark.parametrize("name", list(ap.CAUSAL_PROBES))
def test_flash_attn_causal_gqa_probes_match_fp64(eng, name):
    (s,) = ap.build("causal", name)
    for code in ap.CODES:
        _check_prefill(_flash(eng, [s], code, True), [s], code, name)
    qd, kd, vtd = _rope_split(eng, s, "lane")               # and through the split kernel's own layouts
    out = torch.zeros(s.n, s.Hq * 128, dtype=torch.bfloat16, device="cuda")
    torch.cuda.synchronize()
    eng.op_flash_attn(qd.data_ptr(), kd.data_ptr(), vtd.data_ptr(), out.data_ptr(), np.array([0, s.n], np.int32), s.Hq, s.Hkv, True, ap.SCALE)
    eng.synchronize()
    _check_prefill([out.view(s.n, s.Hq, 128)], [s], "lane", name + " (split kernel's layouts)")


# ------------------------------------------------------------------------------------------------ decode
def _pack(pool, which, table_row, x, idx):
    """x [n, Hkv, 128] (2-byte or 1-byte raw elements) of one sequence -> slot `which` (0 K, 1 V) of its pages; slots past n stay as they are"""
    n, Hkv = x.shape[0], x.shape[1]
    full = n // 64
    if full:
        pg = table_row[:full].long().view(-1, 1, 1, 1)
        pool[pg, torch.arange(Hkv).view(1, -1, 1, 1), which, idx.view(1, 1, 64, 128)] = x[:full * 64].view(full, 64, Hkv, 128).permute(0, 2, 1, 3)
    m = n - full * 64
    if m:
        for h in range(Hkv):
            pool[int(table_row[full]), h, which][idx[:m].reshape(-1)] = x[full * 64:, h].reshape(-1)


def _decode_case(eng, name, scales, plans):
    ctxs, max_seq_len = ap.DECODE_PROBES[name]
    seqs = ap.build("decode", name, scales)
    B, Hq, Hkv = len(seqs), seqs[0].Hq, seqs[0].Hkv
    max_pages = (max_seq_len + 63) // 64
    n_pages = [s.tiles for s in seqs]
    total = sum(n_pages)
    g = torch.Generator().manual_seed(total)
    perm = torch.randperm(total + 2, generator=g)                              # page tables that are not the identity
    table = torch.zeros(B, max_pages, dtype=torch.int32)
    kv8 = scales is not None
    if kv8:
        pool = torch.empty(total + 2, Hkv, 2, 8192, dtype=torch.uint8)
        pool[..., 0::2] = 0x7E                                                 # +-448 wherever nothing is packed
        pool[..., 1::2] = 0xFE
        kidx, vidx, raw = K8_IDX, V8_IDX, torch.uint8
    else:
        pool = torch.full((total + 2, Hkv, 2, 8192), ap.POISON_BITS, dtype=torch.int16)
        kidx, vidx, raw = K_IDX, V_IDX, torch.int16
    off = 0
    for b, s in enumerate(seqs):
        table[b, :n_pages[b]] = perm[off:off + n_pages[b]].to(torch.int32)
        off += n_pages[b]
        _pack(pool, 0, table[b], (s.k8 if kv8 else s.k).view(raw), kidx)
    qd = torch.cat([s.q for s in seqs]).reshape(B, Hq * 128).cuda().contiguous()
    cd, td = torch.tensor(ctxs, dtype=torch.int32).cuda(), table.cuda()
    sd = ap.KV8_SCALES[scales].cuda().contiguous() if kv8 else None
    try:
        for code in ap.CODES:
            for b, s in enumerate(seqs):
                _pack(pool, 1, table[b], s.v_kernel(code).view(raw), vidx)
            ref = torch.cat([s.reference(code) for s in seqs])                  # [B, Hq, 128]
            pd = pool.cuda()
            for plan in plans:
                eng.set_decode_plan(plan)
                out = torch.zeros(B, Hq * 128, dtype=torch.bfloat16, device="cuda")
                torch.cuda.synchronize()
                if kv8:
                    eng.op_decode_attn_kv8(qd.data_ptr(), pd.data_ptr(), cd.data_ptr(), td.data_ptr(), max_pages, out.data_ptr(), B, Hq, Hkv, max_seq_len,
                                           sd.data_ptr())
                else:
                    eng.op_decode_attn(qd.data_ptr(), pd.data_ptr(), cd.data_ptr(), td.data_ptr(), max_pages, out.data_ptr(), B, Hq, Hkv, max_seq_len)
                eng.synchronize()
                worst = ap.assert_close(out.view(B, Hq, 128).float().cpu(), ref, f"{name} {scales or 'bf16'} plan {plan} {code} code")
                print(f"{name} {scales or 'bf16'} plan {plan} {code}: worst error {worst:.3f} x the tolerance")
    finally:
        eng.set_decode_plan(0)


@pytest.mark.parametrize("name", list(ap.DECODE_PROBES))
def test_decode_attention_probes_match_fp64_under_every_plan(eng, name):
    """plan 4 = the per-split kernel, 2 = streaming on the whole chip, 3 = streaming on the partition plan's workgroup count"""
    _decode_case(eng, name, None, (4, 2, 3))


@pytest.mark.parametrize("scales", list(ap.KV8_SCALES))
@pytest.mark.parametrize("name", list(ap.DECODE_PROBES))
def test_decode_attention_kv8_probes_match_fp64_of_the_dequantised_pool(eng, name, scales):
    _decode_case(eng, name, scales, (4, 2))
