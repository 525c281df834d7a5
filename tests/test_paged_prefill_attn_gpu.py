"""dots_op_flash_attn_paged (csrc/attn_paged.hip) on the probes of tests/chunk_probes.py: a block of new query rows behind a prefix that
lies in the sequence's own KV pages, bf16 and fp8 (e4m3) pool, held element by element to the float64 reference by
attention_probes.assert_close.  test_chunked_prefill_cpu.py shows without a GPU that the tolerance is the reference's own and that a causal
limit off by one, a dropped or exchanged page and an unmasked page tail lie far outside it.

Pages are scattered: the block table is a permutation with gaps, and every pool page no table names holds poison, as do the slots of the
last page behind the sequence.  The last tests are the kernel's exactness property: a row's bits do not depend on what shares its launch
or on where the rows were cut into launches.
"""
import pytest
import torch

import attention_probes as ap
import chunk_probes as cp
from test_attention_probes_gpu import _pack
from test_decode_kernels_gpu import K_IDX, V_IDX
from test_kv_fp8_gpu import K8_IDX, V8_IDX

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from dots_ocr_amd.config import DotsConfig
    from dots_ocr_amd.engine import Engine
    e = Engine(DotsConfig.tiny(), max_batch=2, max_seq_len=256, max_patches=256, max_prefill_tokens=256)
    yield e
    e.close()


class Pool:
    """the sequences' K and V in scattered pages of a poisoned pool; table row b = sequence b"""

    def __init__(self, seqs, code, scales):
        self.seqs, self.kv8 = seqs, scales is not None
        Hkv = seqs[0].Hkv
        tiles = [s.tiles for s in seqs]
        total = sum(tiles)
        self.max_pages = max(tiles) + 1
        perm = torch.randperm(2 * total + 3, generator=torch.Generator().manual_seed(total))
        table = torch.full((len(seqs), self.max_pages), 2 * total + 2, dtype=torch.int32)      # unused entries name a poisoned page
        if self.kv8:
            pool = torch.empty(2 * total + 3, Hkv, 2, 8192, dtype=torch.uint8)
            pool[..., 0::2] = 0x7E                                                 # +-448 wherever nothing is packed
            pool[..., 1::2] = 0xFE
            kidx, vidx, raw = K8_IDX, V8_IDX, torch.uint8
        else:
            pool = torch.full((2 * total + 3, Hkv, 2, 8192), ap.POISON_BITS, dtype=torch.int16)
            kidx, vidx, raw = K_IDX, V_IDX, torch.int16
        off = 0
        for b, s in enumerate(seqs):
            table[b, :tiles[b]] = perm[off:off + tiles[b]].to(torch.int32)
            off += tiles[b]
            _pack(pool, 0, table[b], (s.k8 if self.kv8 else s.k).view(raw), kidx)
            _pack(pool, 1, table[b], s.v_kernel(code).view(raw), vidx)
        self.pool, self.table = pool.cuda(), table.cuda()
        self.scales = scales[:Hkv].cuda().contiguous() if self.kv8 else None

    def run(self, eng, cuts):
        """one launch over cuts = [(sequence index, first new row, rows)]: -> [rows, Hq, 128] bf16 per cut"""
        s0 = self.seqs[0]
        q = torch.cat([self.seqs[b].q[lo:lo + m] for b, lo, m in cuts]).cuda().permute(1, 0, 2).contiguous()      # [Hq][T][128]
        T = q.shape[1]
        out = torch.zeros(T, s0.Hq * 128, dtype=torch.bfloat16, device="cuda")
        torch.cuda.synchronize()
        eng.op_flash_attn_paged(q.data_ptr(), self.pool.data_ptr(), self.table.data_ptr(), self.max_pages, len(self.seqs), out.data_ptr(),
                                [self.seqs[b].n - self.seqs[b].nq + lo for b, lo, m in cuts], [m for b, lo, m in cuts], s0.Hq, s0.Hkv, ap.SCALE,
                                kv_scales=None if self.scales is None else self.scales.data_ptr(), rows=[b for b, lo, m in cuts])
        eng.synchronize()
        return list(out.view(T, s0.Hq, 128).split([m for b, lo, m in cuts]))


def _check(out, seq, code, what):
    worst = ap.assert_close(out[seq.rows].float().cpu(), seq.reference(code), what)
    print(f"{what}: {len(seq.rows)} rows x {seq.Hq} heads, worst error {worst:.3f} x the tolerance")


POOLS = [None, "unit", "per_head"]


@pytest.mark.parametrize("scales", POOLS, ids=lambda s: s or "bf16")
@pytest.mark.parametrize("c,m", cp.SHAPES, ids=[f"{c}+{m}" for c, m in cp.SHAPES])
def test_paged_prefill_attention_probes_match_fp64(eng, c, m, scales):
    sc = None if scales is None else ap.KV8_SCALES[scales]
    seq = cp.suffix_probe(c, m, sc)
    for code in ap.CODES:
        (out,) = Pool([seq], code, sc).run(eng, [(0, 0, m)])
        _check(out, seq, code, f"{seq.name} {scales or 'bf16'} {code} code")


@pytest.mark.parametrize("scales", POOLS, ids=lambda s: s or "bf16")
def test_two_sequences_with_different_prefixes_share_one_launch(eng, scales):
    sc = None if scales is None else ap.KV8_SCALES[scales]
    seqs = [cp.suffix_probe(320, 64, sc), cp.suffix_probe(0, 65, sc), cp.suffix_probe(64, 1, sc)]
    for code in ap.CODES:
        outs = Pool(seqs, code, sc).run(eng, [(b, 0, s.nq) for b, s in enumerate(seqs)])
        for out, s in zip(outs, seqs):
            _check(out, s, code, f"packed {s.name} {scales or 'bf16'} {code} code")


@pytest.mark.parametrize("scales", POOLS, ids=lambda s: s or "bf16")
def test_a_row_does_not_depend_on_its_launch(eng, scales):
    """(128, 130) alone, packed behind another sequence, and fed as 64 + 66 rows in two launches: identical bits in every row"""
    sc = None if scales is None else ap.KV8_SCALES[scales]
    seq, other = cp.suffix_probe(128, 130, sc), cp.suffix_probe(192, 257, sc)
    pool = Pool([other, seq], "lane", sc)
    _, packed = pool.run(eng, [(0, 0, other.nq), (1, 0, 130)])
    (alone,) = pool.run(eng, [(1, 0, 130)])
    (first,) = pool.run(eng, [(1, 0, 64)])
    (second,) = pool.run(eng, [(1, 64, 66)])
    _check(alone, seq, "lane", f"{seq.name} {scales or 'bf16'} alone")
    assert torch.equal(alone, packed), "a row's bits depend on what is packed in front of it"
    assert torch.equal(alone, torch.cat([first, second])), "a row's bits depend on where the rows were cut into launches"
    (solo_pool_out,) = Pool([seq], "lane", sc).run(eng, [(0, 0, 130)])
    assert torch.equal(alone, solo_pool_out), "a row's bits depend on which physical pages hold its keys"


@pytest.mark.parametrize("scales", POOLS, ids=lambda s: s or "bf16")
def test_heads_per_wave_do_not_change_a_bit(eng, scales, monkeypatch):
    """three query heads of a kv head per wave (the launcher's choice) or one (DOTS_OCR_PAGED_ATTN_HEADS=1): the same bits either way"""
    sc = None if scales is None else ap.KV8_SCALES[scales]
    seqs = [cp.suffix_probe(192, 257, sc), cp.suffix_probe(0, 65, sc)]
    pool = Pool(seqs, "lane", sc)
    outs = {}
    for heads in ("1", "3"):
        monkeypatch.setenv("DOTS_OCR_PAGED_ATTN_HEADS", heads)
        outs[heads] = pool.run(eng, [(b, 0, s.nq) for b, s in enumerate(seqs)])
        for out, s in zip(outs[heads], seqs):
            _check(out, s, "lane", f"{s.name} {scales or 'bf16'} {heads} head(s) per wave")
    assert all(torch.equal(a, b) for a, b in zip(outs["1"], outs["3"]))


@pytest.mark.parametrize("heads", ["1", "3"])
@pytest.mark.parametrize("scales", [None, "per_head"], ids=lambda s: s or "bf16")
def test_the_model_heads_over_an_80_page_context(eng, scales, heads, monkeypatch):
    monkeypatch.setenv("DOTS_OCR_PAGED_ATTN_HEADS", heads)
    c, m = cp.BIG_SHAPE
    sc = None if scales is None else ap.KV8_SCALES[scales]
    seq = cp.suffix_probe(c, m, sc, Hq=12, Hkv=2)
    for code in ap.CODES:
        (out,) = Pool([seq], code, sc).run(eng, [(0, 0, m)])
        _check(out, seq, code, f"{seq.name} Hq 12 Hkv 2 {scales or 'bf16'} {code} code")


def test_an_unaligned_prefix_is_refused(eng):
    from dots_ocr_amd.engine import DotsEngineError, E_INVALID
    seq = cp.suffix_probe(64, 64)
    pool = Pool([seq], "lane", None)
    q = seq.q.cuda().permute(1, 0, 2).contiguous()
    out = torch.zeros(64, seq.Hq * 128, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(DotsEngineError) as ei:
        eng.op_flash_attn_paged(q.data_ptr(), pool.pool.data_ptr(), pool.table.data_ptr(), pool.max_pages, 1, out.data_ptr(), [63], [64], seq.Hq, seq.Hkv, ap.SCALE)
    assert ei.value.code == E_INVALID and "multiple of 64" in str(ei.value)
    with pytest.raises(DotsEngineError):                                           # more positions than the table row holds
        eng.op_flash_attn_paged(q.data_ptr(), pool.pool.data_ptr(), pool.table.data_ptr(), pool.max_pages, 1, out.data_ptr(), [pool.max_pages * 64], [64], seq.Hq, seq.Hkv, ap.SCALE)
