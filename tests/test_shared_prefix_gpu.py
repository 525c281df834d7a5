"""Shared-prefix decode attention on the GPU: with the switch on, the (rows, KV split) pairs whose four pages are the same
physical pages go through one workgroup that loads the pages once.  The contract is exact — the shared kernel writes the partials the
per-split kernel writes, bit for bit — so every comparison here is for equality: the op against dots_op_decode_attn over the same pool, and
an engine with the switch on against the same engine with it off, in tokens, logprob bits, beam parents and cumulative log-probabilities.
The plan's counters are held to arithmetic restated here, and at a prompt one token short of a shared split they must read zero."""
import numpy as np
import pytest
import torch

from dots_ocr_amd.config import DotsConfig
from dots_ocr_amd.engine import SamplingParams
from dots_ocr_amd.weights import random_state_dict

pytestmark = pytest.mark.gpu

LAYERS = 3
WAVES = 4                                   # pages of a KV split (the engine constant)


def _cfg():
    return DotsConfig.tiny(layers=LAYERS, v_layers=2, vocab=1024)


def _engine(**kw):
    from dots_ocr_amd.engine import Engine
    cfg = _cfg()
    args = dict(max_batch=8, max_seq_len=640, max_patches=256, max_prefill_tokens=4096)
    args.update(kw)
    e = Engine(cfg, **args)
    e.load_state_dict(random_state_dict(cfg, seed=11))
    return cfg, e


@pytest.fixture(scope="module")
def eng():
    cfg, e = _engine()
    yield cfg, e
    e.close()


@pytest.fixture(scope="module")
def eng8():
    cfg, e = _engine(kv_cache_dtype="fp8")
    yield cfg, e
    e.close()


def _prompt(cfg, L, seed=0):
    return np.random.default_rng(9000 + 13 * L + seed).integers(0, cfg.vocab_size - 8, L).astype(np.int32)


# ---------------------------------------------------------------------------------------------------- 1. the op, bitwise

def _splits(max_seq_len):
    return min(64, ((max_seq_len + 63) // 64 + WAVES - 1) // WAVES)


def _expected_pairs(table, ctxs, max_seq_len):
    """the planner's rule, restated: per split the rows whose context holds its four pages in full, classed by the page ids"""
    max_pages = table.shape[1]
    n_splits = _splits(max_seq_len)
    if n_splits * WAVES < max_pages:
        return 0
    pairs = 0
    for s in range(n_splits):
        classes = {}
        for b, c in enumerate(ctxs):
            if WAVES * (s + 1) <= c // 64:
                classes.setdefault(tuple(table[b, WAVES * s:WAVES * (s + 1)].tolist()), []).append(b)
        pairs += sum(len(v) for v in classes.values() if len(v) > 1)
    return pairs


def _op_case(e, groups, B, max_seq_len, kv8, seed, heads=(6, 1), shuffle_q=None):
    """groups: [(member rows, shared full pages, [context per member])]; every other row of the B is a loner with its own pages.
    -> (out of the shared op, out of the plain op, covered pairs, the test's own count), outs as int16 bits"""
    HQ, HKV = heads
    g = torch.Generator().manual_seed(seed)
    max_pages = (max_seq_len + 63) // 64
    ctxs = [int(x) for x in torch.randint(1, min(max_seq_len, 640) - 1, (B,), generator=g)]
    for rows, _, cs in groups:
        for r, c in zip(rows, cs):
            ctxs[r] = c
    n_pool = sum((c + 1 + 63) // 64 for c in ctxs) + 2
    perm = torch.randperm(n_pool, generator=g).to(torch.int32)
    table = torch.zeros(B, max_pages, dtype=torch.int32)
    off = 0
    for b, c in enumerate(ctxs):
        n = (c + 1 + 63) // 64
        table[b, :n] = perm[off:off + n]
        off += n
    for rows, shared, _ in groups:
        for r in rows[1:]:
            table[r, :shared] = table[rows[0], :shared]
    if kv8:
        pool = torch.randint(0, 256, (n_pool, HKV, 2, 8192), generator=g, dtype=torch.int32).to(torch.uint8)
        pool[(pool & 0x7F) == 0x7F] = 0x38                                      # e4m3fn has no inf; 0x7f / 0xff are its NaNs
        scales = (torch.rand(HKV, 2, generator=g) * 0.05 + 0.01).float().cuda()
    else:
        pool = torch.randn(n_pool, HKV, 2, 8192, generator=g).to(torch.bfloat16)
        scales = None
    q = torch.randn(B, HQ * 128, generator=g).to(torch.bfloat16)
    if shuffle_q is not None:
        q = q[shuffle_q]
    qd, pd, cd, td = q.cuda().contiguous(), pool.cuda().contiguous(), torch.tensor(ctxs, dtype=torch.int32).cuda(), table.cuda().contiguous()
    out_s = torch.zeros(B, HQ * 128, dtype=torch.bfloat16, device="cuda")
    out_p = torch.zeros_like(out_s)
    torch.cuda.synchronize()
    args = (qd.data_ptr(), pd.data_ptr(), cd.data_ptr(), td.data_ptr(), max_pages)
    pairs = e.op_decode_attn_shared(*args, out_s.data_ptr(), B, HQ, HKV, max_seq_len, None if scales is None else scales.data_ptr())
    if kv8:
        e.op_decode_attn_kv8(*args, out_p.data_ptr(), B, HQ, HKV, max_seq_len, scales.data_ptr())
    else:
        e.op_decode_attn(*args, out_p.data_ptr(), B, HQ, HKV, max_seq_len)
    assert torch.isfinite(out_p.float()).all()
    return out_s.cpu().view(torch.int16), out_p.cpu().view(torch.int16), pairs, _expected_pairs(table, ctxs, max_seq_len)


def _check(res, want_pairs=None):
    out_s, out_p, pairs, own = res
    assert pairs == own, (pairs, own)
    if want_pairs is not None:
        assert pairs == want_pairs, (pairs, want_pairs)
    assert torch.equal(out_s, out_p), f"{int((out_s != out_p).sum())} elements differ"


@pytest.mark.parametrize("kv8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("m", [2, 3, 5, 8])          # one pass, a half-empty pass, odd, four passes (two rows a pass at group 6)
def test_op_members_sweep(eng, kv8, m):
    _, e = eng
    rows = list(range(1, 1 + m))
    _check(_op_case(e, [(rows, 8, [520 + 7 * i for i in range(m)])], m + 2, 640, kv8, seed=100 + m), want_pairs=2 * m)


@pytest.mark.parametrize("kv8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("shared,n_shared_splits", [(3, 0), (4, 1), (5, 1), (7, 1), (8, 2), (9, 2)])
def test_op_shared_pages_sweep(eng, kv8, shared, n_shared_splits):
    _, e = eng
    _check(_op_case(e, [([0, 2, 3], shared, [600, 601, 602])], 4, 640, kv8, seed=200 + shared), want_pairs=3 * n_shared_splits)


@pytest.mark.parametrize("kv8", [False, True], ids=["bf16", "fp8"])
def test_op_two_groups_loners_and_ragged_contexts(eng, kv8):
    """two groups and loners in one batch; the second group's contexts differ by hundreds of tokens: its members agree on 8 pages but one
    of them holds only 4 in full, so it shares the first split alone"""
    _, e = eng
    groups = [([1, 5, 6], 4, [300, 310, 290]), ([0, 3, 7, 8], 8, [600, 256 + 30, 520, 575])]
    _check(_op_case(e, groups, 10, 640, kv8, seed=300), want_pairs=3 + 4 + 3)


@pytest.mark.parametrize("kv8", [False, True], ids=["bf16", "fp8"])
def test_op_rows_17_and_40_of_64(eng, kv8):
    _, e = eng
    _check(_op_case(e, [([17, 40], 4, [300, 333])], 64, 640, kv8, seed=400), want_pairs=2)


@pytest.mark.parametrize("heads", [(12, 2), (16, 1), (4, 1), (5, 1), (8, 1)], ids=lambda h: f"{h[0]}q{h[1]}kv")
def test_op_other_gqa_groups(eng, heads):
    """two kv heads; a group above 8 (one row a pass); 4, 5 and 8 heads a group (four, three and two rows a pass, 15 live columns at 5)"""
    _, e = eng
    _check(_op_case(e, [([0, 1, 2, 4, 5], 4, [300, 301, 302, 303, 304])], 6, 640, False, seed=500 + heads[0], heads=heads), want_pairs=5)


def test_op_above_16k_shares_nothing(eng):
    """max_seq_len 16448: 257 pages a row against 64 splits of 4 — the plan is empty, the op launches the plain kernels"""
    _, e = eng
    _check(_op_case(e, [([0, 1, 2], 8, [520, 530, 540])], 3, 16448, False, seed=600), want_pairs=0)


def test_op_rows_are_not_interchangeable(eng):
    """the members' q permuted: every member's output changes, so equality above cannot come from rows that compute the same thing"""
    _, e = eng
    groups = [([0, 1, 2, 3], 8, [600, 600, 600, 600])]
    a = _op_case(e, groups, 4, 640, False, seed=700)
    b = _op_case(e, groups, 4, 640, False, seed=700, shuffle_q=[1, 2, 3, 0])
    _check(a, want_pairs=8)
    _check(b, want_pairs=8)
    for r in range(4):
        assert not torch.equal(a[0][r], b[0][r])


# ---------------------------------------------------------------------------------------------------- engine helpers

SLOTS = [1, 4, 2, 6]                 # parent, then three children
CHUNK = 16


def _sampled(i):
    return SamplingParams(temperature=1.0, top_p=0.95, seed=5200 + i)


def _start(e, on):
    e.set_sampling(0.0, 1.0, 0)
    e.slots_reset()
    e.set_eos([])
    e.set_shared_prefix_attention(on)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _read(e, slots, n):
    out = []
    for s in slots:
        tok, ids, top = e.row_logprobs(s, n)
        out.append((e.slot_read(s, n).tolist(), _bits(tok).tolist(), ids.tolist(), _bits(top).tolist()))
    return out


def _saved_per_step(members, shared_splits):
    """KV pages one step does not read: (members - 1) x 4 pages x kv heads x layers per shared split"""
    return (members - 1) * WAVES * 1 * LAYERS * shared_splits


def _fork_run(cfg, e, L, on, chunks=3):
    """a prompt of L tokens, three sampled children with logprobs beside the parent, chunks x 16 steps -> (rows read, info after each chunk)"""
    _start(e, on)
    base = e.shared_prefix_info()["pages_not_read"]
    for i, s in enumerate(SLOTS):
        e.set_row_sampling(s, _sampled(i))
        e.set_row_logprobs(s, 5)
    e.slots_prefill(SLOTS[:1], _prompt(cfg, L), [L], [chunks * CHUNK + 1])
    e.slots_fork(SLOTS[0], SLOTS[1:])
    infos = []
    for _ in range(chunks):
        e.slots_decode(CHUNK)
        info = e.shared_prefix_info()
        info["pages_not_read"] -= base
        infos.append(info)
    got = _read(e, SLOTS, chunks * CHUNK + 1)
    e.slots_reset()
    e.set_shared_prefix_attention(False)
    return got, infos


def _check_fork(cfg, e, L):
    want, off_infos = _fork_run(cfg, e, L, False)
    got, infos = _fork_run(cfg, e, L, True)
    assert len({tuple(r[0]) for r in want}) >= 3                     # the children really differ
    assert got == want
    shared_splits = (L // 64) // WAVES
    for k, info in enumerate(infos):
        assert info["pages_not_read"] == (k + 1) * CHUNK * _saved_per_step(4, shared_splits), (L, k, info)
        assert (info["items"], info["rows"], info["pairs"]) == ((shared_splits, 4, 4 * shared_splits) if shared_splits else (0, 0, 0)), (L, info)
    assert all(i == {"items": 0, "rows": 0, "pairs": 0, "pages_not_read": 0} for i in off_infos)
    return infos


# ---------------------------------------------------------------------------------------------------- 2. forks

@pytest.mark.parametrize("L", [255, 256, 257, 300, 520])
def test_forked_rows_equal_the_switch_off_run(eng, L):
    cfg, e = eng
    infos = _check_fork(cfg, e, L)
    assert (infos[-1]["pages_not_read"] > 0) == (L >= 256)


# ---------------------------------------------------------------------------------------------------- 3. membership changes between chunks

def _membership_run(cfg, e, on):
    _start(e, on)
    e.kv_swap_reserve(16)
    base = e.shared_prefix_info()["pages_not_read"]
    for i, s in enumerate(SLOTS):
        e.set_row_sampling(s, _sampled(i))
        e.set_row_logprobs(s, 5)
    L, n_new = 300, 6 * CHUNK + 1
    e.slots_prefill(SLOTS[:1], _prompt(cfg, L), [L], [n_new])
    e.slots_fork(SLOTS[0], SLOTS[1:])
    reads, infos = [], []

    def chunk(live):
        e.slots_decode(CHUNK)
        info = e.shared_prefix_info()
        info["pages_not_read"] -= base
        infos.append(info)
        fin, lens = e.slots_poll()
        reads.append([(s, e.slot_read(s, int(lens[s])).tolist(), _bits(e.row_logprobs(s, int(lens[s]))[0]).tolist()) for s in live])

    chunk(SLOTS)                                     # 4 members
    e.slot_release(4)
    chunk([1, 2, 6])                                 # 3
    e.slot_suspend(2)
    chunk([1, 6])                                    # 2
    e.slot_resume(2)
    chunk([1, 2, 6])                                 # 3 again
    e.set_row_sampling(4, None)
    e.set_row_logprobs(4, 5)
    e.slots_prefill([4], _prompt(cfg, 270, seed=9), [270], [n_new])      # an unrelated request in the freed slot: its own pages
    chunk([1, 2, 4, 6])                              # still 3
    e.slots_reset()
    e.kv_swap_reserve(0)
    e.set_shared_prefix_attention(False)
    return reads, infos


def test_membership_changes_between_chunks(eng):
    cfg, e = eng
    want, _ = _membership_run(cfg, e, False)
    got, infos = _membership_run(cfg, e, True)
    assert got == want
    members = [4, 3, 2, 3, 3]
    total = 0
    for info, m in zip(infos, members):
        total += CHUNK * _saved_per_step(m, 1)
        assert (info["items"], info["rows"], info["pairs"], info["pages_not_read"]) == (1, m, m, total), (info, m)


# ---------------------------------------------------------------------------------------------------- 4. the other sharing paths

def _beam_run(cfg, e, on):
    _start(e, on)
    slots, n_new = [1, 4, 2, 6], 2 * CHUNK + 1
    e.slots_prefill(slots[:1], _prompt(cfg, 300, seed=2), [300], [n_new])
    e.slots_beam(slots[0], slots[1:])
    cums = []
    for _ in range(2):
        e.slots_decode(CHUNK)
        cums.append(_bits(e.beam_read(slots[0])["cum"]).tolist())
    tr = e.beam_read(slots[0])
    info = e.shared_prefix_info()
    e.slots_reset()
    e.set_shared_prefix_attention(False)
    return (tr["tokens"].tolist(), tr["parents"].tolist(), cums), info


def test_beam_group_equals_the_switch_off_run(eng):
    cfg, e = eng
    want, _ = _beam_run(cfg, e, False)
    got, info = _beam_run(cfg, e, True)
    assert got == want
    assert len({tuple(t) for t in want[0]}) >= 2 and any(p != list(range(4)) for p in np.array(want[1]).T.tolist())      # beams differ and move
    assert (info["items"], info["rows"], info["pairs"]) == (1, 4, 4)


def _fanout_run(cfg, e, on):
    """several prompts over one page: the shared 300-token prefix is prefilled once, forked, and every row extended with its own prompt"""
    _start(e, on)
    slots, n_new = [0, 3, 5], 2 * CHUNK + 1
    for s in slots:
        e.set_row_logprobs(s, 5)
    e.slots_prefill(slots[:1], _prompt(cfg, 300, seed=3), [300], [4])
    e.slots_fork(slots[0], slots[1:])
    e.slots_extend(slots, [_prompt(cfg, 9 + 4 * i, seed=20 + i).tolist() for i in range(3)], keep_pending=False, max_new_tokens=n_new)
    for _ in range(2):
        e.slots_decode(CHUNK)
    got = _read(e, slots, n_new)
    info = e.shared_prefix_info()
    e.slots_reset()
    e.set_shared_prefix_attention(False)
    return got, info


def test_prompts_fan_out_equals_the_switch_off_run(eng):
    cfg, e = eng
    want, _ = _fanout_run(cfg, e, False)
    got, info = _fanout_run(cfg, e, True)
    assert got == want and len({tuple(r[0]) for r in want}) == 3
    assert (info["items"], info["rows"], info["pairs"]) == (1, 3, 3)


def _cache_hits_run(cfg, e, on):
    """two live requests over one 320-token prompt through the prefix cache: the second and the third start behind the first one's pages"""
    _start(e, on)
    e.prefix_cache_enable(False)
    e.prefix_cache_enable(True)
    ids, n_new = _prompt(cfg, 320, seed=4), 2 * CHUNK + 1
    hits = []
    for i, s in enumerate((2, 5, 7)):
        e.set_row_sampling(s, _sampled(i))
        e.set_row_logprobs(s, 5)
        lease, hit, _ = e.prefix_cache_lookup(ids, None)
        hits.append(hit)
        e.slots_prefill_begin_cached([s], ids, [320], [n_new], [lease], [None])
        while e.slots_prefill_advance(128) > 0:
            pass
    for _ in range(2):
        e.slots_decode(CHUNK)
    got = _read(e, (2, 5, 7), n_new)
    info = e.shared_prefix_info()
    e.slots_reset()
    e.prefix_cache_enable(False)
    e.set_shared_prefix_attention(False)
    return got, info, hits


def test_concurrent_prefix_cache_hits_equal_the_switch_off_run(eng):
    cfg, e = eng
    want, _, hits = _cache_hits_run(cfg, e, False)
    got, info, _ = _cache_hits_run(cfg, e, True)
    assert hits[0] == 0 and hits[1] >= 256 and hits[2] >= 256               # pages shared without any fork
    assert got == want and len({tuple(r[0]) for r in want}) == 3
    assert (info["items"], info["rows"], info["pairs"]) == (1, 3, 3)


# ---------------------------------------------------------------------------------------------------- 5. the fp8 pool

def test_forked_rows_on_the_fp8_pool(eng8):
    cfg, e = eng8
    infos = _check_fork(cfg, e, 300)
    assert infos[-1]["pages_not_read"] > 0


# ---------------------------------------------------------------------------------------------------- 6. switch on, nobody shares

def _independent_run(cfg, e, on):
    _start(e, on)
    slots, n_new = list(range(8)), 2 * CHUNK + 1
    lens = [260 + 3 * i for i in range(8)]
    e.slots_prefill(slots, np.concatenate([_prompt(cfg, n, seed=30 + i) for i, n in enumerate(lens)]), lens, [n_new] * 8)
    for _ in range(2):
        e.slots_decode(CHUNK)
    got = [e.slot_read(s, n_new).tolist() for s in slots]
    info = e.shared_prefix_info()
    e.slots_reset()
    e.set_shared_prefix_attention(False)
    return got, info


def test_independent_prompts_share_nothing(eng):
    cfg, e = eng
    base = e.shared_prefix_info()["pages_not_read"]
    want, _ = _independent_run(cfg, e, False)
    got, info = _independent_run(cfg, e, True)
    assert got == want
    assert info == {"items": 0, "rows": 0, "pairs": 0, "pages_not_read": base}
