"""Beam search on the GPU: Engine.slots_beam makes a group of B beams over shared KV pages whose selection and
mid-generation fork run inside the captured decode steps.  The contract is exact: a beam row's logits are bitwise those of an ordinary
row teacher-forced along the same prefix, so the oracle is the host model (dots_ocr_amd.beam.beam_search_host) fed with the engine's own
unbeamed logprobs of every prefix that was ever live — a prefix the host model asks for that the group never held is itself the failure.
Parents, tokens, the bits of cum (after every decode chunk) and the completed records must be equal."""
import numpy as np
import pytest
import torch

from dots_ocr_amd.beam import backtrace, beam_search_host
from dots_ocr_amd.config import DotsConfig
from dots_ocr_amd.engine import DotsEngineError, LogitRules, SamplingParams
from dots_ocr_amd.weights import random_state_dict

pytestmark = pytest.mark.gpu

FILLER = 1                                   # the token a forced path ends with when only its distribution is wanted


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
def eng8():
    cfg, e = _engine(kv_cache_dtype="fp8")
    yield cfg, e
    e.close()


def _prompt(cfg, L, seed=0):
    return np.random.default_rng(9000 + 13 * L + seed).integers(0, cfg.vocab_size - 8, L).astype(np.int32)


def _image_prompt(cfg, L):
    """the smallest grid the tiny tower takes: 1 x 4 x 4 patches = 4 merged rows"""
    g = torch.Generator().manual_seed(L)
    pv = torch.randn(16, cfg.vision.patch_dim, generator=g).numpy()
    grid = np.array([[1, 4, 4]], np.int64)
    ids = _prompt(cfg, L)
    ids[3:7] = cfg.image_token_id
    return ids, (pv, grid)


def _start(e, eos=()):
    e.set_sampling(0.0, 1.0, 0)
    e.slots_reset()
    e.set_eos(list(eos))


def run_group(e, ids, slots, n_new, chunk=16, image=None, eos=(), release=True, before=None):
    """the group's trace after n_new steps (the first selection and n_new - 1 decode steps), with cum read after every chunk:
    trace["cum_at"] = {steps done: float32 [B]}"""
    _start(e, eos)
    if image is not None:
        e.vit_forward(*image)
    e.slots_prefill(slots[:1], ids, [len(ids)], [n_new])
    e.slots_beam(slots[0], slots[1:])
    cum_at = {}
    tr = e.beam_read(slots[0])
    cum_at[tr["steps"]] = tr["cum"]
    done = 1
    while done < n_new:
        e.slots_decode(chunk)
        done += chunk
        tr = e.beam_read(slots[0])
        cum_at[tr["steps"]] = tr["cum"]
    fin, lens = e.slots_poll()
    assert all(fin[s] == 1 for s in slots), (fin, lens)
    tr["cum_at"] = cum_at
    if release:
        e.slot_release(slots[-1])
    return tr


def live_prefixes(tr):
    """every prefix of generated tokens a live beam ever held, the empty one included"""
    out = {()}
    for t in range(tr["steps"]):
        for j in range(tr["B"]):
            if tr["parents"][j, t] >= 0:
                out.add(tuple(backtrace(tr["parents"], tr["tokens"], t, j)))
    return out


def forced_table(e, ids, prefixes, n_new, image=None, slots=None):
    """{prefix: (top_ids [16], top_lp float32 [16])}: the unbeamed logprobs of the next token after every prefix, from ordinary slots
    forced along the root-to-leaf paths by an allowed list of one id, eight paths at a time"""
    pre = {p for p in prefixes if len(p) < n_new}                # the distribution after a full-length prefix is never asked for
    leaves = sorted(p for p in pre if not any(q[:len(p)] == p and len(q) == len(p) + 1 for q in pre))
    table = {}
    slots = list(range(e.max_batch)) if slots is None else slots
    for at in range(0, len(leaves), len(slots)):
        paths = [list(p) + [FILLER] for p in leaves[at:at + len(slots)]]
        use = slots[:len(paths)]
        _start(e)
        for s, p in zip(use, paths):
            e.set_row_logit_rules(s, LogitRules(allowed=[p[0]]))
            e.set_row_logprobs(s, 16)
        if image is not None:
            e.vit_forward(np.concatenate([image[0]] * len(use)), np.concatenate([image[1]] * len(use)))
        e.slots_prefill(use, np.concatenate([ids] * len(use)), [len(ids)] * len(use), [len(p) for p in paths])
        for k in range(1, max(len(p) for p in paths)):
            for s, p in zip(use, paths):
                if k < len(p):
                    e.set_row_logit_rules(s, LogitRules(allowed=[p[k]]))
            e.slots_decode(1)
        for s, p in zip(use, paths):
            assert e.slot_read(s, len(p)).tolist() == p
            _, top_ids, top_lp = e.row_logprobs(s, len(p))
            for k in range(len(p)):
                key = tuple(p[:k])
                if key in table:                                     # a shared prefix: the same bits from whichever path
                    assert np.array_equal(table[key][0], top_ids[k, :16]) and np.array_equal(table[key][1].view(np.uint32), top_lp[k, :16].view(np.uint32))
                table[key] = (top_ids[k, :16].copy(), top_lp[k, :16].copy())
    return table


def oracle(e, ids, tr, n_new, eos=(), image=None):
    table = forced_table(e, ids, live_prefixes(tr), n_new, image=image)
    B = tr["B"]

    def top_fn(prefix):
        assert prefix in table, f"the host model asks for prefix {prefix}, which the group never held"
        return table[prefix][0][:2 * B], table[prefix][1][:2 * B]
    return beam_search_host(top_fn, B, n_new, eos)


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def assert_same(tr, completed, host, n_new):
    assert tr["steps"] == host["tokens"].shape[1]
    assert np.array_equal(tr["parents"], host["parents"])
    assert np.array_equal(tr["tokens"], host["tokens"])
    for steps, cum in tr["cum_at"].items():
        assert np.array_equal(bits(cum), bits(host["cum"][steps - 1])), steps
    assert len(tr["completed"]) == len(completed)
    for a, b in zip(tr["completed"], completed):
        assert a[:3] == b[:3] and bits(a[3]) == bits(b[3]), (a, b)


def check(e, ids, slots, n_new, chunk=16, image=None, eos=()):
    tr = run_group(e, ids, slots, n_new, chunk=chunk, image=image, eos=eos)
    completed, host = oracle(e, ids, tr, n_new, eos=eos, image=image)
    assert_same(tr, completed, host, n_new)
    return tr


_LONG = {}


def _long(eng_, name):
    """the L = 63, B = 3, 70-step group in slots [5, 0, 7] and its oracle (computed once per engine, never changed)"""
    cfg, e = eng_
    if name not in _LONG:
        ids = _prompt(cfg, 63)
        tr = run_group(e, ids, [5, 0, 7], 70)
        _LONG[name] = (tr,) + oracle(e, ids, tr, 70)
    return _LONG[name]


# ---------------------------------------------------------------------------------------------------- 1. the group is the host model
def test_long_group_crosses_two_pages_and_shares_a_frozen_one(eng):
    """L = 63: the tail page holds prompt tokens at the fork; positions 64 and 128 are page boundaries; page 1 is generated whole, frozen
    and shared by pointer"""
    tr, completed, host = _long(eng, "bf16")
    assert_same(tr, completed, host, 70)


def test_the_long_case_exercises_the_reorder(eng):
    """at least one step has a beam with two children and a beam with none: otherwise no page is ever forked mid-generation"""
    tr, _, _ = _long(eng, "bf16")
    forks = 0
    for t in range(1, tr["steps"]):
        kids = np.bincount(tr["parents"][:, t][tr["parents"][:, t] >= 0], minlength=tr["B"])
        forks += int(kids.max() >= 2 and kids.min() == 0)
    assert forks >= 1
    assert any(tr["parents"][j, t] not in (j, -1) for t in range(1, tr["steps"]) for j in range(tr["B"]))


def test_long_group_fp8_kv(eng8):
    tr, completed, host = _long(eng8, "fp8")
    assert_same(tr, completed, host, 70)


def test_chunks_of_one_and_sixteen_agree(eng):
    cfg, e = eng
    tr16, _, host = _long(eng, "bf16")
    tr1 = run_group(e, _prompt(cfg, 63), [5, 0, 7], 70, chunk=1)
    assert np.array_equal(tr1["parents"], tr16["parents"]) and np.array_equal(tr1["tokens"], tr16["tokens"])
    assert len(tr1["cum_at"]) == 70
    for steps, cum in tr1["cum_at"].items():                         # cum after every single step
        assert np.array_equal(bits(cum), bits(host["cum"][steps - 1])), steps


def test_no_tail_at_the_fork(eng):
    cfg, e = eng
    check(e, _prompt(cfg, 64), [2, 3], 6)


def test_group_fills_the_engine_with_an_image_prompt(eng):
    cfg, e = eng
    ids, image = _image_prompt(cfg, 70)
    check(e, ids, [0, 1, 2, 3, 4, 5, 6, 7], 6, image=image)


def test_other_slot_order(eng):
    cfg, e = eng
    check(e, _prompt(cfg, 63, seed=1), [7, 3, 1, 4], 20)


def test_eos_completes_hypotheses_at_rank_zero_and_beyond_b(eng):
    cfg, e = eng
    ids, B, n_new = _prompt(cfg, 63, seed=2), 4, 12
    root = forced_table(e, ids, {()}, n_new)[()]
    eos = [int(root[0][0]), int(root[0][B + 1])]                     # the root's best id and one of rank B + 1
    tr = check(e, ids, [1, 2, 3, 4], n_new, eos=eos)
    first = [r for r in tr["completed"] if r[0] == 0]
    assert [(r[1], r[2]) for r in first] == [(0, eos[0]), (0, eos[1])]
    assert all(t not in eos for t in tr["tokens"].ravel())


# ---------------------------------------------------------------------------------------------------- 2. beside other rows
def _solo(e, ids, slot, n_new, sp=None):
    _start(e)
    if sp is not None:
        e.set_row_sampling(slot, sp)
    e.slots_prefill([slot], ids, [len(ids)], [n_new])
    for _ in range(0, n_new - 1, 16):
        e.slots_decode(16)
    return e.slot_read(slot, n_new).tolist()


def test_rows_beside_a_group_generate_their_solo_tokens(eng):
    cfg, e = eng
    n_new = 40
    a, b = _prompt(cfg, 50, seed=3), _prompt(cfg, 81, seed=4)
    sp = SamplingParams(temperature=1.0, top_p=0.95, seed=77)
    want_a, want_b = _solo(e, a, 1, n_new), _solo(e, b, 6, n_new, sp)
    tr, _, _ = _long(eng, "bf16")
    _start(e)
    e.set_row_sampling(6, sp)
    e.slots_prefill([1, 6], np.concatenate([a, b]), [len(a), len(b)], [n_new, n_new])
    e.slots_prefill([5], _prompt(cfg, 63), [63], [70])
    e.slots_beam(5, [0, 7])
    for _ in range(0, 70, 16):
        e.slots_decode(16)
    assert e.slot_read(1, n_new).tolist() == want_a
    assert e.slot_read(6, n_new).tolist() == want_b
    got = e.beam_read(0)
    assert np.array_equal(got["tokens"], tr["tokens"]) and np.array_equal(got["parents"], tr["parents"])
    assert np.array_equal(bits(got["cum"]), bits(tr["cum"]))


# ---------------------------------------------------------------------------------------------------- 3. pages
def test_release_of_one_slot_frees_the_group_and_the_pool_is_whole(eng):
    cfg, e = eng
    _start(e)
    total, free = e.kv_pool_info()
    assert free == total
    e.slots_prefill([2], _prompt(cfg, 130), [130], [70])
    e.slots_beam(2, [4, 0])
    # two shared prompt pages; every beam owns ceil(200 / 64) - 2 = 2 pages and a spare
    assert e.kv_pool_info()[1] == total - 2 - 3 * 3
    e.slots_decode(16)
    e.slot_release(4)
    fin, _ = e.slots_poll()
    assert all(fin[s] == -1 for s in (0, 2, 4))
    assert e.kv_pool_info() == (total, total)
    with pytest.raises(DotsEngineError):
        e.beam_read(2)


def test_a_pool_a_few_pages_short_refuses_the_group():
    cfg, e = _engine(kv_pool_tokens=11 * 64)
    try:
        _start(e)
        ids = _prompt(cfg, 63)
        e.slots_prefill([0], ids, [63], [70])                        # 2 pages; the group needs 3 x (3 + 1) = 12
        free = e.kv_pool_info()[1]
        with pytest.raises(DotsEngineError, match=r"\(-4\)"):
            e.slots_beam(0, [1, 2])
        assert e.kv_pool_info()[1] == free
        fin, lens = e.slots_poll()
        assert fin[0] == 0 and lens[0] == 1 and fin[1] == fin[2] == -1
        e.slots_prefill([1], ids, [63], [70])                        # an ordinary prefill still works, and so does the refused source
        e.slots_decode(16)
        assert e.slot_read(0, 17).tolist() == e.slot_read(1, 17).tolist()
    finally:
        e.close()


# ---------------------------------------------------------------------------------------------------- 4. refusals
def test_preconditions_are_refused_with_the_state_unchanged(eng):
    cfg, e = eng
    ids = _prompt(cfg, 63)
    _start(e)
    e.slots_prefill([0, 3], np.concatenate([ids, ids]), [63, 63], [20, 20])
    free = e.kv_pool_info()[1]
    for dst, code in (([3], -3), ([0], -1), ([1, 1], -1), ([8], -1), ([], -1), ([1, 2, 4, 5, 6, 7, 3, 1], -1)):
        with pytest.raises(DotsEngineError, match=rf"\({code}\)"):
            e.slots_beam(0, dst)
    e.set_row_logprobs(1, 4)
    with pytest.raises(DotsEngineError, match=r"\(-1\)"):
        e.slots_beam(0, [1, 2])
    e.set_row_logprobs(1, None)
    e.set_row_sampling(2, SamplingParams(temperature=0.0, top_k=5))
    with pytest.raises(DotsEngineError, match=r"\(-1\)"):
        e.slots_beam(0, [1, 2])
    e.set_row_sampling(2, None)
    assert e.kv_pool_info()[1] == free
    e.slots_beam(0, [1, 2])
    for call in (lambda: e.set_row_sampling(1, SamplingParams(temperature=1.0)), lambda: e.set_row_logprobs(0, 3),
                 lambda: e.set_row_logit_rules(2, LogitRules(allowed=[5]))):
        with pytest.raises(DotsEngineError, match=r"\(-1\)"):
            call()
    with pytest.raises(DotsEngineError, match=r"\(-3\)"):
        e.slots_fork(0, [4])                                         # the source of a group is no plain sequence any more
    e.slots_decode(1)
    with pytest.raises(DotsEngineError, match=r"\(-3\)"):
        e.slots_beam(3, [4, 5])                                      # a decode step has run
    assert e.beam_info(1)[:2] == (3, 2)


def test_a_speculating_engine_refuses_a_group(eng):
    cfg, e = eng
    _start(e)
    e.set_speculation(1)
    try:
        e.slots_prefill([0], _prompt(cfg, 63), [63], [20])
        with pytest.raises(DotsEngineError, match=r"\(-3\)"):
            e.slots_beam(0, [1])
    finally:
        e.slots_reset()
        e.set_speculation(0)
