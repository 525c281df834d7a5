"""Parallel sampling on the GPU: Engine.slots_fork turns free slots into copies of a freshly prefilled sequence over shared,
reference-counted KV pages.  The contract is exact: a forked row generates, bit for bit, what an independent prefill of the same prompt
into the same slot under the same row parameters generates — tokens and logprobs — so every comparison here is for equality, and the
sampled sequences are checked to differ from each other so that equality cannot hold vacuously."""
import numpy as np
import pytest
import torch

from dots_ocr_amd import guided as G
from dots_ocr_amd.config import DotsConfig
from dots_ocr_amd.engine import DotsEngineError, NgramRule, SamplingParams
from dots_ocr_amd.weights import random_state_dict

pytestmark = pytest.mark.gpu

SEED = 4100
N_NEW = 80
SLOTS = [1, 4, 2, 6]                 # parent, then the three children: neither ascending nor adjacent


def _cfg():
    return DotsConfig.tiny(layers=3, v_layers=3, vocab=1024)


def _engine(**kw):
    from dots_ocr_amd.engine import Engine
    cfg = _cfg()
    args = dict(max_batch=8, max_seq_len=640, max_patches=4096, max_prefill_tokens=2048)
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
def small():
    """12 pages: the LIFO free list hands a freed page straight out again"""
    cfg, e = _engine(kv_pool_tokens=12 * 64)
    yield cfg, e
    e.close()


def _prompt(cfg, L, seed=0):
    return np.random.default_rng(7000 + 13 * L + seed).integers(0, cfg.vocab_size - 8, L).astype(np.int32)


def _image_prompt(cfg, L):
    """the smallest grid the tiny tower takes: 1 x 4 x 4 patches = 4 merged rows"""
    g = torch.Generator().manual_seed(L)
    pv = torch.randn(16, cfg.vision.patch_dim, generator=g).numpy()
    grid = np.array([[1, 4, 4]], np.int64)
    ids = _prompt(cfg, L)
    ids[3:7] = cfg.image_token_id
    return ids, pv, grid


def _sampled(i):
    return SamplingParams(temperature=1.0, top_p=0.95, seed=SEED + i)


def _set_row(e, s, sp=None, lp=None, ngram=None, guide=None):
    if sp is not None:
        e.set_row_sampling(s, sp)
    if lp is not None:
        e.set_row_logprobs(s, lp)
    if ngram is not None:
        e.set_row_ngram(s, ngram)
    if guide is not None:
        e.set_row_guide(s, guide)


def _start(e):
    e.set_sampling(0.0, 1.0, 0)
    e.slots_reset()
    e.set_eos([])


def _finish(e, slots, n_new, lp=False, chunk=16, done=0):
    while done < n_new - 1:
        e.slots_decode(chunk)
        done += chunk
    fin, lens = e.slots_poll()
    assert all(fin[s] == 1 and lens[s] == n_new for s in slots), (fin, lens)
    toks = [e.slot_read(s, n_new).tolist() for s in slots]
    lps = [e.row_logprobs(s, n_new) for s in slots] if lp else None
    return toks, lps


def _forked(e, ids, slots, rows, n_new=N_NEW, lp=False, image=None):
    """rows[i] = keyword arguments of _set_row for slots[i]; slots[0] is prefilled, the others forked from it"""
    _start(e)
    for s, r in zip(slots, rows):
        _set_row(e, s, **r)
    if image is not None:
        e.vit_forward(*image)
    e.slots_prefill(slots[:1], ids, [len(ids)], [n_new])
    e.slots_fork(slots[0], slots[1:])
    return _finish(e, slots, n_new, lp)


def _independent(e, ids, slots, rows, n_new=N_NEW, lp=False, image=None):
    """the same prompt prefilled once per slot, as independent sequences of one group"""
    _start(e)
    for s, r in zip(slots, rows):
        _set_row(e, s, **r)
    n = len(slots)
    if image is not None:
        e.vit_forward(np.concatenate([image[0]] * n), np.concatenate([image[1]] * n))
    e.slots_prefill(slots, np.concatenate([ids] * n), [len(ids)] * n, [n_new] * n)
    return _finish(e, slots, n_new, lp)


_REF = {}


def _reference(eng, L):
    """tokens and logprobs of the four independent sampled sequences of the length-L prompt (computed once, never changed)"""
    cfg, e = eng
    if L not in _REF:
        rows = [dict(sp=_sampled(i), lp=5) for i in range(4)]
        _REF[L] = _independent(e, _prompt(cfg, L), SLOTS, rows, lp=True)
    return _REF[L]


def _same_lp(a, b):
    return all(x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))


def _distinct(toks):
    return len({tuple(t) for t in toks})


# ---------------------------------------------------------------------------------------------------- 1. a forked row is an independent request

@pytest.mark.parametrize("L", [64, 65, 127, 130])
def test_forked_rows_equal_independent_requests(eng, L):
    cfg, e = eng
    want_t, want_lp = _reference(eng, L)
    rows = [dict(sp=_sampled(i), lp=5) for i in range(4)]
    got_t, got_lp = _forked(e, _prompt(cfg, L), SLOTS, rows, lp=True)
    assert _distinct(want_t) >= 3                                      # seeds s .. s + 3 really give different readings
    assert got_t == want_t
    for g, w in zip(got_lp, want_lp):
        assert _same_lp(g, w)
    e.slots_reset()
    assert e.kv_pool_info()[1] == e.kv_pool_info()[0]


def test_forked_rows_with_image_tokens_run_the_tower_once(eng):
    cfg, e = eng
    ids, pv, grid = _image_prompt(cfg, 70)
    rows = [dict(sp=_sampled(i), lp=5) for i in range(4)]
    want_t, want_lp = _independent(e, ids, SLOTS, rows, lp=True, image=(pv, grid))
    got_t, got_lp = _forked(e, ids, SLOTS, rows, lp=True, image=(pv, grid))         # one vit_forward of one image
    assert _distinct(want_t) >= 3
    assert got_t == want_t
    for g, w in zip(got_lp, want_lp):
        assert _same_lp(g, w)


# ---------------------------------------------------------------------------------------------------- 2. a child's prompt KV is the parent's

def _check_prompt_kv(cfg, e, L):
    _start(e)
    ids = _prompt(cfg, L)
    e.slots_prefill([1], ids, [L], [8])
    e.slots_fork(1, [4, 2, 6])
    e.slots_decode(3)                                                  # every row has appended its own keys behind the prompt
    for layer in range(cfg.num_hidden_layers):
        for which in ("k", "v"):
            parent = e.read_kv(layer, 1, 0, L, which)
            assert parent.any()
            for child in (4, 2, 6):
                assert np.array_equal(e.read_kv(layer, child, 0, L, which), parent), (layer, which, child)
    e.slots_reset()


@pytest.mark.parametrize("L", [64, 65, 127, 130])
def test_child_prompt_kv_is_the_parents_bf16(eng, L):
    cfg, e = eng
    _check_prompt_kv(cfg, e, L)


def test_child_prompt_kv_is_the_parents_fp8():
    cfg, e = _engine(kv_cache_dtype="fp8")
    try:
        for L in (65, 127):
            _check_prompt_kv(cfg, e, L)
    finally:
        e.close()


# ---------------------------------------------------------------------------------------------------- 3. reference counts

def test_reference_counts_survive_the_parents_release(eng, small):
    cfg, e = small
    L = 130
    want_t, _ = _reference(eng, L)
    _start(e)
    total, free0 = e.kv_pool_info()
    assert (total, free0) == (12, 12)
    for i, s in enumerate(SLOTS):
        _set_row(e, s, sp=_sampled(i), lp=5)
    e.slots_prefill(SLOTS[:1], _prompt(cfg, L), [L], [N_NEW])
    parent_pages = e.slot_capacity(SLOTS[0])[0]
    admit_pages = (L + 64 + 63) // 64
    assert parent_pages == admit_pages
    e.slots_fork(SLOTS[0], SLOTS[1:])
    assert e.kv_pool_info()[1] == total - parent_pages - 3 * (admit_pages - L // 64)
    e.slots_decode(5)
    e.slot_release(SLOTS[0])
    assert e.kv_pool_info()[1] == total - 2 - 3 * (admit_pages - L // 64)          # the two shared pages stay: the children hold them
    other = _prompt(cfg, 100, seed=5)
    e.slots_prefill(SLOTS[:1], other, [len(other)], [20])                           # takes the pages the parent just returned
    got_t, _ = _finish(e, SLOTS[1:], N_NEW, done=5)
    assert got_t == want_t[1:]
    for s in SLOTS:
        e.slot_release(s)
    assert e.kv_pool_info() == (total, total)
    e.slots_reset()
    assert e.kv_pool_info() == (total, total)


# ---------------------------------------------------------------------------------------------------- 4. refusals change nothing

def test_refusals_change_nothing(small):
    cfg, e = small
    L, cap = 130, 40
    ids, big, mid = _prompt(cfg, L), _prompt(cfg, 100, seed=3), _prompt(cfg, 70, seed=4)
    _start(e)
    e.slots_prefill([0], ids, [L], [cap])
    want, _ = _finish(e, [0], cap)                                                  # the unforked run

    _start(e)
    # the source holds ceil(170 / 64) = 3 pages, the others 3 and 2: 4 of 12 are free, and a child needs 3 - 130 // 64 = 1 of its own
    e.slots_prefill([0, 5, 7], np.concatenate([ids, big, mid]), [L, len(big), len(mid)], [cap, 64, 20])
    pool = e.kv_pool_info()
    assert pool == (12, 4)

    def refused(dst, code):
        with pytest.raises(DotsEngineError, match=rf"\({code}\)"):
            e.slots_fork(0, dst)
        assert e.kv_pool_info() == pool
        fin, _ = e.slots_poll()
        assert [int(fin[s]) for s in range(8)] == [0, -1, -1, -1, -1, 0, -1, 0]

    refused([1, 5], -3)                       # an occupied destination
    refused([1, 0], -1)                       # the source itself
    refused([1, 2, 1], -1)                    # a destination given twice
    refused([1, 8], -1)                       # out of range
    refused([1, 2, 3, 4, 6], -4)              # five children, four pages: the pool is one page short
    e.slots_decode(1)
    refused([1], -3)                          # the source has taken a decode step
    got, _ = _finish(e, [0], cap, done=1)
    assert got == want
    e.slots_reset()
    assert e.kv_pool_info() == (12, 12)


# ---------------------------------------------------------------------------------------------------- 5. row state follows the child

def _token_bytes(V):
    toks = [bytes([i]) for i in range(256)] + [bytes([97 + i % 3, 32 if i % 5 == 0 else 97 + (i // 3) % 3]) for i in range(256, V)]
    return G.TokenBytes(toks, range(V - 8, V))


@pytest.mark.parametrize("first", ["parent", "child"])
def test_row_state_follows_the_child(first):
    """penalties (counts and prompt-presence bits), an n-gram rule and a guide on a forked row; the penalty state of the engine is first
    allocated by the parent's parameters (before the prefill) or by the child's (after it, before the fork)"""
    cfg, e = _engine()
    try:
        e.set_token_bytes(_token_bytes(cfg.vocab_size))
        h = e.create_guide(G.compile_regex(r"[a-c ]*"))
        L, n_new = 65, 48
        ids = _prompt(cfg, L)
        ids[:20] = np.arange(97, 117)                  # the prompt holds what the guide allows: the presence bits matter
        pen = SamplingParams(temperature=0.8, top_p=0.95, seed=31, repetition_penalty=1.3, frequency_penalty=0.5)
        child = dict(sp=pen, ngram=NgramRule(3), guide=h, lp=3)
        parent = dict(sp=pen) if first == "parent" else dict(sp=SamplingParams(temperature=0.8, seed=30))
        _start(e)
        _set_row(e, 0, **parent)
        e.slots_prefill([0], ids, [L], [n_new])
        _set_row(e, 3, **child)                        # set, then fork
        e.slots_fork(0, [3])
        got_t, got_lp = _finish(e, [0, 3], n_new, lp=True)
        state = e.row_guide_state(3)
        want_t, want_lp = _independent(e, ids, [0, 3], [parent, child], n_new, lp=True)
        assert got_t == want_t and _same_lp(got_lp[1], want_lp[1])
        assert state == e.row_guide_state(3)
        plain_t, _ = _independent(e, ids, [0, 3], [parent, dict(sp=SamplingParams(temperature=0.8, top_p=0.95, seed=31))], n_new)
        assert plain_t[1] != got_t[1]                  # the settings decide the child's tokens
        e.slots_reset()
        e.destroy_guide(h)
    finally:
        e.close()


# ---------------------------------------------------------------------------------------------------- 6. under speculation

def test_fork_under_speculation(eng):
    cfg, e = eng
    L, n_new = 127, 64
    ids = np.tile(_prompt(cfg, 16), 8)[:L]             # a repetitive prompt: the output repeats too, drafts get accepted
    _start(e)
    e.slots_prefill([0], ids, [L], [n_new])
    want, _ = _finish(e, [0], n_new)
    e.slots_reset()
    e.set_speculation(3)
    try:
        assert e.usable_slots == 2
        e.set_eos([])
        e.slots_prefill([0], ids, [L], [n_new])
        pool = e.kv_pool_info()
        with pytest.raises(DotsEngineError, match=r"\(-4\)"):
            e.slots_fork(0, [2])                       # outside the usable slots
        assert e.kv_pool_info() == pool
        e.slots_fork(0, [1])
        assert e.spec_stats(1) == {"steps": 0, "drafted": 0, "accepted": 0}
        got, _ = _finish(e, [0, 1], n_new)
        assert got == [want[0], want[0]]
    finally:
        e.slots_reset()
        e.set_speculation(0)


# ---------------------------------------------------------------------------------------------------- 7. through the scheduler

def test_parallel_sampling_through_the_scheduler(eng):
    from dots_ocr_amd.scheduler import ContinuousBatcher, Request
    cfg, e = eng
    e.set_sampling(0.0, 1.0, 0)
    ids, pv, grid = _image_prompt(cfg, 70)
    other = _prompt(cfg, 40, seed=9)
    sp = SamplingParams(temperature=1.0, top_p=0.95, seed=SEED)
    alone = []
    for i in range(3):
        spi = SamplingParams(temperature=1.0, top_p=0.95, seed=SEED + i)
        r = Request(ids, pv, grid, 40, sampling=spi, logprobs=2)
        alone.append((ContinuousBatcher(e, chunk=8).run([r])[0].tolist(), r.logprobs_out))
    other_alone = ContinuousBatcher(e, chunk=8).run([Request(other, max_new_tokens=30)])[0].tolist()
    cb = ContinuousBatcher(e, chunk=8)
    first, second = Request(ids, pv, grid, 40, sampling=sp, logprobs=2, n=3), Request(other, max_new_tokens=30)
    out = cb.run([first, second])
    assert cb.admissions == 1                                          # one prefill for the whole group
    assert [o.tolist() for o in first.outputs] == [a for a, _ in alone]
    assert _distinct([a for a, _ in alone]) == 3
    assert out[0].tolist() == alone[0][0] and out[1].tolist() == other_alone
    for got, (_, want) in zip(first.logprobs_out, alone):
        assert _same_lp(got, want)
    assert e.kv_pool_info()[1] == e.kv_pool_info()[0]
