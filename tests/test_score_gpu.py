"""Scoring given tokens on a live sequence on the GPU: Engine.slots_score is slots_extend with a record — for every fed
token but the first, the entry the logprob stage would have written had the row before it selected that token.

The contract is exact.  The run that exists without the feature scores one token per decode step: a greedy row whose logit rules allow
one id is teacher-forced with logprobs on (tests/test_extend_gpu.py::_forced), and entry j - 1 of a score equals position j of that row's
row_logprobs in every bit, top lists included.  A random suffix is not the arg max, so the scored values are checked to differ from the
top entry: a stage that took the selected token would not pass.  One test holds the entries to the CPU oracle's log-softmax."""
import ctypes

import numpy as np
import pytest
import torch

from dots_ocr_amd.config import DotsConfig
from dots_ocr_amd.engine import DotsEngineError, LogitRules, SamplingParams
from dots_ocr_amd.weights import random_state_dict

pytestmark = pytest.mark.gpu

N_GEN = 24
K = 20


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


@pytest.fixture(scope="module")
def small():
    cfg, e = _engine(kv_pool_tokens=12 * 64)
    yield cfg, e
    e.close()


def _prompt(cfg, L, seed=0):
    return np.random.default_rng(7000 + 13 * L + seed).integers(0, cfg.vocab_size - 8, L).astype(np.int32)


def _suffix(cfg, n, seed=0):
    return [int(t) for t in np.random.default_rng(9100 + 7 * n + seed).integers(0, cfg.vocab_size - 8, n)]


def _image_prompt(cfg, L):
    """the smallest grid the tiny tower takes: 1 x 4 x 4 patches = 4 merged rows"""
    g = torch.Generator().manual_seed(L)
    pv = torch.randn(16, cfg.vision.patch_dim, generator=g).numpy()
    grid = np.array([[1, 4, 4]], np.int64)
    ids = _prompt(cfg, L)
    ids[3:7] = cfg.image_token_id
    return ids, pv, grid


def _start(e):
    e.set_sampling(0.0, 1.0, 0)
    e.slots_reset()
    e.set_eos([])


def _same_lp(a, b):
    return all(x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))


def _blank(lp):
    """every bit of the entries is set: nothing was recorded there"""
    return all(bool((x.view(np.uint32) == 0xFFFFFFFF).all()) for x in lp)


def _forced_lp(e, s, P, E, top_n, image=None, head=0):
    """The reference that exists without the feature: P prefilled into slot s with logprobs at top_n, its first token forced to E[0],
    E[1:] forced one decode step each.  Returns row_logprobs of positions [1 + head, len(E)): position j is the entry of E[j]."""
    _start(e)
    e.set_row_logprobs(s, top_n)
    e.set_row_logit_rules(s, LogitRules(allowed=(int(E[0]),)))
    if image is not None:
        e.vit_forward(*image)
    e.slots_prefill([s], P, [len(P)], [len(E) + 1])
    for t in E[1:]:
        e.set_row_logit_rules(s, LogitRules(allowed=(int(t),)))
        e.slots_decode(1)
    assert e.slot_read(s, len(E)).tolist() == [int(t) for t in E]      # the forcing held
    lp = e.row_logprobs(s, len(E))
    e.set_row_logit_rules(s, None)
    return tuple(x[1 + head:] for x in lp)


def _scored(e, s, P, E, top_n, image=None):
    _start(e)
    if image is not None:
        e.vit_forward(*image)
    e.slots_prefill([s], P, [len(P)], [4])
    (got,) = e.slots_score([s], [E], top_n=top_n, max_new_tokens=N_GEN)
    return got


def _check_targets_are_given(lp, top_n):
    tok, ids, top = lp
    assert len(set(tok.view(np.uint32).tolist())) > 1                   # not one value throughout
    if top_n > 0:
        assert (tok != top[:, 0]).any()                                # the given token, not the arg max, is what is scored


def _check_score_equals_forcing(e, s, P, E, top_n, image=None):
    want = _forced_lp(e, s, P, E, top_n, image=image)
    got = _scored(e, s, P, E, top_n, image=image)
    assert got[0].shape == (len(E) - 1,) and got[1].shape == (len(E) - 1, K) and got[2].shape == (len(E) - 1, K)
    assert _same_lp(got, want)
    if len(E) > 2:
        _check_targets_are_given(got, top_n)
    if len(E) > 1:
        assert not np.isnan(got[0]).any()
        assert (got[1][:, :top_n] >= 0).all() and (got[1][:, top_n:] == -1).all() and np.isnan(got[2][:, top_n:]).all()
    # the record stays readable, and nothing lies behind its last entry
    again = e.slot_scores(s)
    assert _same_lp(again, got)
    assert _blank(e.slot_scores(s, n=3, pos0=len(E) - 1))
    e.slots_reset()
    assert e.kv_pool_info()[1] == e.kv_pool_info()[0]


# ---------------------------------------------------------------------------------------------------- 1. a score is sequential forcing

_CASES = [(LP, LE, 5) for LP in (61, 64) for LE in (1, 2, 8, 9, 10, 67)] + [(LP, 9, t) for LP in (61, 64) for t in (0, 20)]


@pytest.mark.parametrize("LP,LE,top_n", _CASES)
def test_score_equals_sequential_forcing(eng, LP, LE, top_n):
    """LE = 9: row 7's target sits in the next chunk; 8: the last row of a full chunk records nothing; 61 + 7 crosses a page inside a
    chunk; 67 is nine chunks; 1 records nothing at all"""
    cfg, e = eng
    _check_score_equals_forcing(e, 2, _prompt(cfg, LP), _suffix(cfg, LE, seed=3), top_n)


# ---------------------------------------------------------------------------------------------------- 2. on the fp8 KV cache

def test_score_on_an_fp8_cache(eng8):
    cfg, e = eng8
    _check_score_equals_forcing(e, 2, _prompt(cfg, 61), _suffix(cfg, 9, seed=2), 5)


# ---------------------------------------------------------------------------------------------------- 3. behind a generated answer

def test_keep_pending_scores_behind_an_answer(eng):
    cfg, e = eng
    s, P, E2 = 5, _prompt(cfg, 61, seed=3), _suffix(cfg, 9, seed=3)
    _start(e)
    e.slots_prefill([s], P, [len(P)], [6])
    e.slots_decode(5)
    fin, lens = e.slots_poll()
    assert fin[s] == 1 and lens[s] == 6
    A = e.slot_read(s, 6).tolist()                                     # its last token is pending: selected, its K/V not written
    (got,) = e.slots_score([s], [E2], top_n=5, keep_pending=True, max_new_tokens=4)
    assert got[0].shape == (len(E2),)                                  # F = [pending] + ids: entry 0 is lp(ids[0] | ..., pending)
    want = _forced_lp(e, s, P, A + E2, 5, head=len(A) - 1)
    assert _same_lp(got, want)
    _check_targets_are_given(got, 5)
    # without the pending token the first target has another row before it
    _start(e)
    e.slots_prefill([s], P, [len(P)], [6])
    e.slots_decode(5)
    (drop,) = e.slots_score([s], [E2], top_n=5, keep_pending=False, max_new_tokens=4)
    assert drop[0].shape == (len(E2) - 1,) and not _same_lp(drop, tuple(x[1:] for x in got))
    e.slots_reset()


# ---------------------------------------------------------------------------------------------------- 4. chunks above 32 rows

def test_score_in_chunks_above_32_rows():
    cfg, e = _engine(max_batch=64)
    try:
        P, E = _prompt(cfg, 61, seed=4), _suffix(cfg, 70, seed=4)     # a 64-row chunk and a 6-row chunk
        _check_score_equals_forcing(e, 3, P, E, 5)
    finally:
        e.close()


# ---------------------------------------------------------------------------------------------------- 5. packed slots are independent

def test_packed_slots_are_independent(eng):
    cfg, e = eng
    slots = [1, 4, 6]
    prompts = [_prompt(cfg, L, seed=4) for L in (61, 64, 70)]
    # fed lengths 3, 4 and 5: 12 rows in chunks of 8 + 4.  Slots 1 and 4 end inside the first chunk; slot 6 has row 7 in the first chunk
    # (its target is in the next one) and rows 8 .. 11 in the second
    sufs = [_suffix(cfg, n, seed=4) for n in (3, 4, 5)]
    tops = [5, 0, 20]
    _start(e)
    e.slots_prefill(slots, np.concatenate(prompts), [len(p) for p in prompts], [4] * 3)
    packed = e.slots_score(slots, sufs, top_n=tops, max_new_tokens=N_GEN)
    for s, suf, got in zip(slots, sufs, packed):
        assert got[0].shape == (len(suf) - 1,)
        assert _blank(e.slot_scores(s, n=4, pos0=len(suf) - 1))        # nothing of a neighbour's landed behind the last entry
    for s, p, suf, t, got in zip(slots, prompts, sufs, tops, packed):
        alone = _scored(e, s, p, suf, t)
        assert _same_lp(got, alone)
        assert _same_lp(got, _forced_lp(e, s, p, suf, t))
    assert len({tuple(g[0].view(np.uint32).tolist()) for g in packed}) == 3
    # ---- the same over a fork of one prefix
    fslots = [1, 4, 2]
    prefix = _prompt(cfg, 70, seed=6)                                  # 70 % 64 != 0: every child gets a copy of the tail page
    _start(e)
    free0 = e.kv_pool_info()[1]
    e.slots_prefill(fslots[:1], prefix, [len(prefix)], [4])
    e.slots_fork(fslots[0], fslots[1:])
    forked = e.slots_score(fslots, sufs, top_n=5, max_new_tokens=1)
    for s in fslots:
        e.slot_release(s)
    assert e.kv_pool_info()[1] == free0
    for s, suf, got in zip(fslots, sufs, forked):
        assert got[0].shape == (len(suf) - 1,)
        assert _same_lp(got, _scored(e, s, prefix, suf, 5))
    e.slots_reset()


# ---------------------------------------------------------------------------------------------------- 6. a score is an extend

def test_a_score_is_an_extend(eng):
    cfg, e = eng
    s, P, E = 2, _prompt(cfg, 61, seed=5), _suffix(cfg, 9, seed=3)

    def run(score):
        _start(e)
        e.set_row_logprobs(s, 5)
        e.slots_prefill([s], P, [len(P)], [4])
        if score:
            e.slots_score([s], [E], top_n=3, max_new_tokens=N_GEN)
        else:
            e.slots_extend([s], [E], max_new_tokens=N_GEN)
        pool0 = e.kv_pool_info()
        assert e.slots_poll()[1][s] == 1                               # the first token of the new turn is selected
        e.slots_decode(N_GEN - 1)
        fin, lens = e.slots_poll()
        assert fin[s] == 1 and lens[s] == N_GEN
        return e.slot_read(s, N_GEN).tolist(), e.row_logprobs(s, N_GEN), pool0, e.kv_pool_info()

    st, sl, sp0, sp1 = run(True)
    et, el, ep0, ep1 = run(False)
    assert st == et and _same_lp(sl, el) and (sp0, sp1) == (ep0, ep1)
    assert len(set(st)) > 1
    e.slots_reset()


# ---------------------------------------------------------------------------------------------------- 7. bystanders

def test_a_score_leaves_other_slots_alone(eng):
    cfg, e = eng
    Q, P, E = _prompt(cfg, 50, seed=5), _prompt(cfg, 61, seed=6), _suffix(cfg, 9, seed=6)
    n_by = 3 + N_GEN
    by = 5            # above the scored slot: the call's own first-token lm_head runs over rows [0, 3] of the engine's logits, as an extend's
    _start(e)
    e.slots_prefill([by], Q, [len(Q)], [n_by])
    e.slots_decode(n_by - 1)
    want = e.slot_read(by, n_by).tolist()
    _start(e)
    e.slots_prefill([by], Q, [len(Q)], [n_by])
    e.slots_prefill([3], P, [len(P)], [4])
    e.slots_decode(3)
    before = e.slot_logits(by).view(np.uint32).copy()
    assert len(set(before.tolist())) > 1
    e.slots_score([3], [E], top_n=5, max_new_tokens=4)                 # a chunk of 8 rows and one of 1
    assert np.array_equal(e.slot_logits(by).view(np.uint32), before)   # the fed rows' logits went to a scratch of the call's own
    e.slots_decode(n_by - 4)
    fin, lens = e.slots_poll()
    assert fin[by] == 1 and lens[by] == n_by
    assert e.slot_read(by, n_by).tolist() == want
    e.slots_reset()


# ---------------------------------------------------------------------------------------------------- 8. against the oracle

def test_scores_match_the_oracle(eng):
    """Bound: 2 x 0.03 x the oracle's logit range at the position.  tests/test_model_gpu.py::test_prefill_and_decode_logits_match_oracle
    holds every decode-step logit to max |error| < 0.03 x range; lp = l[tok] - lse, |d lse| <= max |d l|, so |d lp| <= 2 x max |d l|."""
    from oracle import model as om
    cfg, e = eng
    sd = random_state_dict(cfg, seed=11)
    ids, pv, grid = _image_prompt(cfg, 61)
    E = _suffix(cfg, 9, seed=9)
    got = _scored(e, 2, ids, E, 5, image=(pv, grid))
    worst = 0.0
    for j in range(len(E) - 1):
        full = torch.cat([torch.from_numpy(ids).long(), torch.tensor(E[:j + 1])])
        _, lg = om.generate(sd, cfg, full, torch.from_numpy(pv), torch.from_numpy(grid), 1, emulate_bf16=True, return_logits=True)
        l = lg[0].double()
        want = float(torch.log_softmax(l, -1)[E[j + 1]])
        rng = float(l.max() - l.min())
        err = abs(float(got[0][j]) - want)
        worst = max(worst, err / rng)
        assert err <= 2 * 0.03 * rng, (j, err, rng)
    print(f"scored entries vs the emulated oracle's log-softmax: worst |error| {100 * worst:.3f} % of the logit range (bound 6 %)")
    e.slots_reset()


# ---------------------------------------------------------------------------------------------------- 9. refusals change nothing

def _read_tokens(e, s, n):
    fin, lens = e.slots_poll()
    assert fin[s] == 1 and lens[s] == n, (fin, lens)
    return e.slot_read(s, n).tolist()


def test_refusals_change_nothing(small):
    cfg, e = small
    P, big = _prompt(cfg, 61, seed=8), _prompt(cfg, 600, seed=8)
    cap = 40
    _start(e)
    e.slots_prefill([0], P, [len(P)], [cap])
    e.slots_decode(cap - 1)
    want = _read_tokens(e, 0, cap)
    E = _suffix(cfg, 5, seed=8)

    _start(e)
    e.kv_swap_reserve(12)
    # slot 0: 2 pages (61 + 40 tokens); slot 5: 10 pages (600 + 40): the pool of 12 is full
    e.slots_prefill([0, 5], np.concatenate([P, big]), [len(P), len(big)], [cap, 40])
    pool = e.kv_pool_info()
    assert pool == (12, 0)

    def refused(code, slots, ids_list, **kw):
        with pytest.raises(DotsEngineError, match=rf"\({code}\)"):
            e.slots_score(slots, ids_list, **kw)
        assert e.kv_pool_info() == pool

    with pytest.raises(DotsEngineError, match=r"\(-3\)"):
        e.slot_scores(0)                                               # never scored
    with pytest.raises(DotsEngineError, match=r"\(-3\)"):
        e.slot_scores(1)                                               # a free slot
    refused(-3, [1], [E])                                              # a free slot
    refused(-1, [0, 0], [E, E])                                        # listed twice
    refused(-1, [0], [[]])                                             # nothing to feed
    refused(-1, [8], [E])                                              # out of range
    refused(-1, [0], [[cfg.image_token_id]])                           # vision rows enter at the prefill only
    refused(-1, [0], [E], top_n=21)                                    # top_n out of range
    refused(-1, [0], [E], top_n=-1)
    refused(-4, [0], [E], max_new_tokens=640)                          # beyond max_seq_len
    refused(-4, [0], [_suffix(cfg, 44, seed=8)], max_new_tokens=24)    # one page short, off a page boundary
    refused(-4, [0], [_suffix(cfg, 67, seed=8)], max_new_tokens=1)     # ... and on one
    e.set_row_sampling(0, SamplingParams(temperature=0.0, repetition_penalty=1.2))
    refused(-3, [0], [E])                                              # a row that carries a penalty
    e.set_row_sampling(0, None)
    e.slots_decode(2)
    e.slot_suspend(5)
    pool = e.kv_pool_info()
    refused(-3, [5], [E])                                              # a suspended slot
    e.slot_release(5)
    pool = e.kv_pool_info()
    with pytest.raises(DotsEngineError, match=r"\(-3\)"):
        e.slot_scores(0)                                               # no refusal left a record
    e.slots_decode(cap - 3)
    assert _read_tokens(e, 0, cap) == want                             # the slot decoded exactly what it would have
    e.slots_reset()

    # ---- a filling slot
    _start(e)
    e.slots_prefill_begin([2], P, [len(P)], [8])
    pool = e.kv_pool_info()
    refused(-3, [2], [E])
    e.slots_reset()

    # ---- a row of a beam group
    _start(e)
    e.slots_prefill([0], P, [len(P)], [8])
    e.slots_beam(0, [1])
    pool = e.kv_pool_info()
    refused(-3, [0], [E])
    refused(-3, [1], [E])
    e.slots_reset()

    # ---- a speculating engine
    e.set_speculation(1)
    try:
        e.set_eos([])
        e.slots_prefill([0], P, [len(P)], [8])
        pool = e.kv_pool_info()
        refused(-3, [0], [E])
    finally:
        e.slots_reset()
        e.set_speculation(0)

    # ---- a static batch
    e.prefill(P, np.asarray([len(P)], np.int32))
    pool = e.kv_pool_info()
    refused(-3, [0], [E])
    e.slots_reset()
    assert e.kv_pool_info() == (12, 12)

    # ---- a record ends with the sequence it belongs to: an extend, a prefill into the slot after a release
    _start(e)
    e.slots_prefill([0], P, [len(P)], [4])
    e.slots_score([0], [E], max_new_tokens=4)
    assert e.slot_scores(0)[0].shape == (len(E) - 1,)
    e.slots_extend([0], [E], max_new_tokens=4)
    with pytest.raises(DotsEngineError, match=r"\(-3\)"):
        e.slot_scores(0)
    e.slots_score([0], [E[:1]], max_new_tokens=4)
    assert e.slot_scores(0)[0].shape == (0,)                           # scored, with no entry
    e.slot_release(0)
    e.slots_prefill([0], P, [len(P)], [4])
    with pytest.raises(DotsEngineError, match=r"\(-3\)"):
        e.slot_scores(0)
    e.slots_reset()


# ---------------------------------------------------------------------------------------------------- 10. nothing left pending

def test_score_leaves_no_pending_hip_error_behind():
    from dots_ocr_amd.engine import Engine
    cfg = DotsConfig.tiny(layers=2, v_layers=2, vocab=1024)
    e = Engine(cfg, max_batch=4, max_seq_len=512, max_patches=2048, max_prefill_tokens=1024)
    e.load_state_dict(random_state_dict(cfg, seed=4))
    loaded = [ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64" in ln]
    assert loaded, "no HIP runtime mapped?"
    hip = ctypes.CDLL(loaded[0])
    hip.hipGetLastError()                                                    # start clean
    _start(e)
    P = _prompt(cfg, 61)
    e.slots_prefill([1], P, [len(P)], [4])
    e.slots_fork(1, [3])
    a, b = e.slots_score([1, 3], [_suffix(cfg, 9), _suffix(cfg, 2)], top_n=[0, 7], max_new_tokens=6)
    assert a[0].shape == (8,) and b[0].shape == (1,) and not np.isnan(a[0]).any() and not np.isnan(b[0]).any()
    e.slots_decode(5)
    assert e.slots_poll()[1].tolist() == [0, 6, 0, 6]
    with pytest.raises(DotsEngineError):
        e.slots_score([0], [[1]])
    e.stats()
    assert hip.hipGetLastError() == 0, "a HIP error was left pending after a score"
    y = torch.ones(8, device="cuda") * 2
    torch.cuda.synchronize()
    assert float(y.sum()) == 16.0
    e.close()


# ---------------------------------------------------------------------------------------------------- 11. through the scheduler and modeling

def _lone_score(e, ids, image, cand, top_n):
    """the prefix prefilled alone into slot 0 and scored with one candidate"""
    return _scored(e, 0, ids, cand, top_n, image=image)


def test_score_through_the_scheduler(eng):
    from dots_ocr_amd.scheduler import ContinuousBatcher, Request
    cfg, e = eng
    ids, pv, grid = _image_prompt(cfg, 70)
    cands = [_suffix(cfg, n, seed=10) for n in (3, 9, 5)]
    want = [_lone_score(e, ids, (pv, grid), c, 2) for c in cands]
    other = _prompt(cfg, 40, seed=9)
    _start(e)
    e.slots_prefill([0], other, [len(other)], [30])
    e.slots_decode(29)
    other_alone = e.slot_read(0, 30).tolist()
    e.slots_reset()
    for m in (1, 3):
        cb = ContinuousBatcher(e, chunk=8)
        first, second = Request(ids, pv, grid, score=cands[:m], score_top_logprobs=2), Request(other, max_new_tokens=30)
        out = cb.run([first, second])
        assert cb.admissions == 1                                      # one tower and one prefill for the m candidates
        assert len(first.scores_out) == m and [o.tolist() for o in first.outputs] == [[]] * m
        for got, w in zip(first.scores_out, want):
            assert _same_lp(got, w)
        assert out[0].tolist() == [] and out[1].tolist() == other_alone        # the generating request beside it is undisturbed
        assert not cb.running and e.kv_pool_info()[1] == e.kv_pool_info()[0]   # no slot is held afterwards
        assert (e.slots_poll()[0] < 0).all()
    assert len({tuple(w[0].view(np.uint32).tolist()) for w in want}) == 3


def test_model_score():
    from dots_ocr_amd.modeling import DotsOcrHipForCausalLM
    cfg = _cfg()
    model = DotsOcrHipForCausalLM(cfg, random_state_dict(cfg, seed=11), device=0, max_batch=4, max_seq_len=640, max_patches=4096)
    try:
        e = model.engine
        ids, pv, grid = _image_prompt(cfg, 70)
        cands = [_suffix(cfg, n, seed=11) for n in (4, 9)]
        want = [_lone_score(e, ids, (pv, grid), c, 3) for c in cands]
        got = model.score(torch.from_numpy(ids).long()[None], torch.from_numpy(pv), torch.from_numpy(grid), candidates=cands, top_logprobs=3)
        assert len(got) == 2 and all(_same_lp(g, w) for g, w in zip(got, want))
        assert not _same_lp(got[0], tuple(x[:3] for x in got[1]))
        with pytest.raises(ValueError):
            model.score(torch.from_numpy(ids).long()[None], torch.from_numpy(pv), torch.from_numpy(grid), candidates=[[1]] * 9)
    finally:
        model.engine.close()


def test_top_lists_read_before_any_call_asked_for_one():
    """an engine whose every score so far had top_n = 0 holds no top lists: the read returns what they would hold, in the bits of a forced
    row with top_n = 0"""
    cfg, e = _engine(max_batch=4)
    try:
        P, E = _prompt(cfg, 61, seed=12), _suffix(cfg, 6, seed=12)
        got = _scored(e, 1, P, E, 0)
        assert _blank(e.slot_scores(1, n=2, pos0=len(E) - 1))
        assert _blank(tuple(x[len(E) - 1:] for x in e.slot_scores(1, n=len(E) + 1)))
        assert _same_lp(got, _forced_lp(e, 1, P, E, 0))
        assert (got[1] == -1).all() and np.isnan(got[2]).all() and not np.isnan(got[0]).any()
    finally:
        e.close()
