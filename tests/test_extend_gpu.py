"""Extending a live sequence on the GPU: Engine.slots_extend feeds more prompt tokens behind the KV cache a slot holds.

The contract is exact: an extend leaves, bit for bit, the state that feeding the same tokens one decode step at a time leaves.  That
sequential run exists without the feature — a greedy row whose logit rules allow exactly one id is teacher-forced — so the comparisons
here are for equality of tokens and of logprob bits against it, and every continuation is checked not to be constant and to differ from
the un-extended one, so that equality cannot hold vacuously.  One test holds the first logits after an extend to the CPU oracle at the
bound tests/test_model_gpu.py::test_prefill_and_decode_logits_match_oracle applies to decode-step logits on this configuration."""
import ctypes

import numpy as np
import pytest
import torch

from dots_ocr_amd import guided as G
from dots_ocr_amd.config import DotsConfig
from dots_ocr_amd.engine import DotsEngineError, LogitRules, SamplingParams
from dots_ocr_amd.weights import random_state_dict

pytestmark = pytest.mark.gpu

N_GEN = 24


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


def _read(e, s, n=None):
    """tokens and logprobs of the finished slot s; n: the length it must have (None: whatever it ended at)"""
    fin, lens = e.slots_poll()
    assert fin[s] == 1 and (n is None or lens[s] == n), (s, fin, lens)
    n = int(lens[s])
    return e.slot_read(s, n).tolist(), e.row_logprobs(s, n)


def _same_lp(a, b):
    return all(x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))


def _forced(e, s, P, E, n_gen=N_GEN, image=None, before_last=None, eos=None):
    """The sequential reference: P prefilled into slot s with its first token forced to E[0] (a greedy row that may select one id only),
    E[1:] forced one single decode step each, then n_gen free tokens.  before_last(e) runs before the step that selects the first free
    token.  eos: EOS ids of the run (the free tokens may then end early).  Returns (the free tokens, their logprobs)."""
    _start(e)
    if eos is not None:
        e.set_eos(list(eos))
    e.set_row_logprobs(s, 5)
    e.set_row_logit_rules(s, LogitRules(allowed=(int(E[0]),)))
    if image is not None:
        e.vit_forward(*image)
    e.slots_prefill([s], P, [len(P)], [len(E) + n_gen])
    for t in E[1:]:
        e.set_row_logit_rules(s, LogitRules(allowed=(int(t),)))
        e.slots_decode(1)
    e.set_row_logit_rules(s, None)
    if before_last is not None:
        before_last(e)
    for _ in range(n_gen):
        e.slots_decode(1)
    toks, lps = _read(e, s, len(E) + n_gen if eos is None else None)
    assert toks[:len(E)] == [int(t) for t in E]                       # the forcing held
    return toks[len(E):], tuple(x[len(E):] for x in lps)


def _extended(e, s, P, E, n_gen=N_GEN, image=None, prefill_cap=4):
    _start(e)
    e.set_row_logprobs(s, 5)
    if image is not None:
        e.vit_forward(*image)
    e.slots_prefill([s], P, [len(P)], [prefill_cap])
    e.slots_extend([s], [E], keep_pending=False, max_new_tokens=n_gen)
    assert e.slots_poll()[1][s] == 1                                   # the first token of the new turn is selected
    e.slots_decode(n_gen - 1)
    return _read(e, s, n_gen)


def _plain(e, s, P, n_gen=N_GEN, image=None):
    _start(e)
    if image is not None:
        e.vit_forward(*image)
    e.slots_prefill([s], P, [len(P)], [n_gen])
    e.slots_decode(n_gen - 1)
    return e.slot_read(s, n_gen).tolist()


def _check_extend_equals_forcing(cfg, e, s, P, E, image=None):
    want_t, want_lp = _forced(e, s, P, E, image=image)
    got_t, got_lp = _extended(e, s, P, E, image=image)
    assert got_t == want_t
    assert _same_lp(got_lp, want_lp)
    assert len(set(got_t)) > 1                                         # not a constant continuation
    assert got_t != _plain(e, s, P, image=image)                       # and the suffix decides it
    e.slots_reset()
    assert e.kv_pool_info()[1] == e.kv_pool_info()[0]


# ---------------------------------------------------------------------------------------------------- 1. an extend is sequential teacher forcing

@pytest.mark.parametrize("LE", [1, 2, 7, 8, 9, 67])
@pytest.mark.parametrize("LP", [61, 64])
def test_extend_equals_sequential_forcing(eng, LP, LE):
    """8 and 9 cross the max_batch = 8 chunk boundary, 61 + 7 crosses a page boundary inside one chunk, 67 spans nine chunks and a page, 64
    starts on a page boundary"""
    cfg, e = eng
    # suffix seed 3: the tiny random model falls into a constant continuation behind some suffixes, which would show nothing
    _check_extend_equals_forcing(cfg, e, 2, _prompt(cfg, LP), _suffix(cfg, LE, seed=3))


def test_extend_behind_an_image_prompt(eng):
    cfg, e = eng
    ids, pv, grid = _image_prompt(cfg, 61)
    _check_extend_equals_forcing(cfg, e, 3, ids, _suffix(cfg, 9, seed=1), image=(pv, grid))


@pytest.mark.parametrize("LP,LE", [(61, 9), (64, 67)])
def test_extend_on_an_fp8_cache(eng8, LP, LE):
    cfg, e = eng8
    _check_extend_equals_forcing(cfg, e, 2, _prompt(cfg, LP), _suffix(cfg, LE, seed=2))


# ---------------------------------------------------------------------------------------------------- 2. a next turn behind a finished answer

@pytest.mark.parametrize("end", ["cap", "eos"])
def test_keep_pending_after_a_finished_turn(eng, end):
    cfg, e = eng
    s, P, E2 = 5, _prompt(cfg, 61, seed=3), _suffix(cfg, 9, seed=3)
    first = _plain(e, s, P, n_gen=10)
    _start(e)
    e.set_row_logprobs(s, 5)
    n_a = 10
    if end == "eos":
        n_a = 1 + next(i for i in range(1, 10) if first[i] not in first[:i])      # the answer ends at its first new token: that is the EOS
        e.set_eos([first[n_a - 1]])
    e.slots_prefill([s], P, [len(P)], [10])
    e.slots_decode(12)                         # the finished row idles for a few steps: its input token keeps moving, its output does not
    A, _ = _read(e, s, n_a)
    assert A == first[:n_a]
    e.set_eos([])
    e.slots_extend([s], [E2], keep_pending=True, max_new_tokens=N_GEN)
    e.slots_decode(N_GEN - 1)
    got_t, got_lp = _read(e, s, N_GEN)
    want_t, want_lp = _forced(e, s, P, A + E2)
    assert got_t == want_t and _same_lp(got_lp, want_lp)
    assert len(set(got_t)) > 1
    # dropping the pending token instead is a different sequence
    drop_t, _ = _forced(e, s, P, A[:-1] + E2)
    assert drop_t != got_t


# ---------------------------------------------------------------------------------------------------- 3. packed extends are row-independent

def _three(cfg):
    slots = [1, 4, 6]
    prompts = [_prompt(cfg, L, seed=4) for L in (61, 64, 70)]
    sufs = [_suffix(cfg, n, seed=4) for n in (5, 9, 3)]                # 17 rows: three chunks, slot 4's tokens straddle the first two
    return slots, prompts, sufs


def test_packed_extends_are_row_independent(eng):
    cfg, e = eng
    slots, prompts, sufs = _three(cfg)
    Q = _prompt(cfg, 50, seed=5)
    n_by = 3 + N_GEN
    want_by = _plain(e, 0, Q, n_gen=n_by)

    def run(which, mode, bystander):
        _start(e)
        for s in which:
            e.set_row_logprobs(s, 5)
        if bystander:
            e.slots_prefill([0], Q, [len(Q)], [n_by])
            e.slots_decode(3)
        idx = [slots.index(s) for s in which]
        e.slots_prefill(which, np.concatenate([prompts[i] for i in idx]), [len(prompts[i]) for i in idx], [4] * len(idx))
        if mode == "packed":
            e.slots_extend(which, [sufs[i] for i in idx], max_new_tokens=N_GEN)
        else:
            for i in idx:
                e.slots_extend([slots[i]], [sufs[i]], max_new_tokens=N_GEN)
        e.slots_decode(N_GEN - 1)
        out = [_read(e, s, N_GEN) for s in which]
        by = e.slot_read(0, n_by).tolist() if bystander else None
        return out, by

    packed, by = run(slots, "packed", True)
    assert by == want_by                                               # the running bystander generates what it generates with no extend at all
    single, _ = run(slots, "single", False)
    for (pt, pl), (st, sl) in zip(packed, single):
        assert pt == st and _same_lp(pl, sl)
    for i, s in enumerate(slots):
        (at, al), = run([s], "packed", False)[0]
        assert at == packed[i][0] and _same_lp(al, packed[i][1])
        want_t, want_lp = _forced(e, s, prompts[i], sufs[i])
        assert at == want_t and _same_lp(al, want_lp)
    assert len({tuple(t) for t, _ in packed}) == 3
    e.slots_reset()


# ---------------------------------------------------------------------------------------------------- 4. fan-out over a fork

def test_fan_out_over_a_fork(eng):
    cfg, e = eng
    slots = [1, 4, 2, 6]
    prefix = _prompt(cfg, 70, seed=6)                                  # 70 % 64 != 0: every child gets a copy of the tail page
    sufs = [_suffix(cfg, n, seed=6) for n in (3, 8, 11, 1)]
    _start(e)
    free0 = e.kv_pool_info()[1]
    for s in slots:
        e.set_row_logprobs(s, 5)
    e.slots_prefill(slots[:1], prefix, [len(prefix)], [4])
    e.slots_fork(slots[0], slots[1:])
    e.slots_extend(slots, sufs, keep_pending=False, max_new_tokens=N_GEN)
    e.slots_decode(N_GEN - 1)
    got = [_read(e, s, N_GEN) for s in slots]
    for s in slots:
        e.slot_release(s)
    assert e.kv_pool_info()[1] == free0
    for s, suf, (gt, gl) in zip(slots, sufs, got):                     # the parent included: its shared pages were not written
        wt, wl = _extended(e, s, prefix, suf)
        assert gt == wt and _same_lp(gl, wl)
    assert len({tuple(t) for t, _ in got}) == 4
    # a parent extended while its children keep running on the shared pages
    _start(e)
    e.slots_prefill([1], prefix, [len(prefix)], [N_GEN])
    e.slots_fork(1, [4])
    e.slots_extend([1], [sufs[1]], max_new_tokens=N_GEN)
    e.slots_decode(N_GEN - 1)
    assert e.slot_read(1, N_GEN).tolist() == got[1][0]
    assert e.slot_read(4, N_GEN).tolist() == _plain(e, 4, prefix)
    e.slots_reset()


# ---------------------------------------------------------------------------------------------------- 5. features restart at the extend

def _token_list(V):
    return [bytes([i]) for i in range(256)] + [bytes([97 + i % 3, 32 if i % 5 == 0 else 97 + (i // 3) % 3]) for i in range(256, V)]


def test_features_restart_at_the_extend():
    cfg, e = _engine()
    try:
        V = cfg.vocab_size
        toks = _token_list(V)
        e.set_token_bytes(G.TokenBytes(toks, range(V - 8, V)))
        P, E = _prompt(cfg, 61, seed=7), _suffix(cfg, 9, seed=7)

        # ---- a guide: the reference takes it (at its root) before the step that selects the first free token
        choices = ["abcabcab", "bcabcc a", "cabbac"]
        h = e.create_guide(G.compile_choice(choices))
        eos = [V - 1]
        _start(e)
        e.set_eos(eos)
        e.set_row_logprobs(2, 5)
        e.set_row_guide(2, h)
        e.slots_prefill([2], P, [len(P)], [8])
        e.slots_decode(2)                                              # the automaton is in the middle of a choice (or through it)
        n1 = int(e.slots_poll()[1][2])
        head = e.slot_read(2, n1).tolist()[:-1]                        # the last token is pending: the extend drops it
        e.slots_extend([2], [E], max_new_tokens=N_GEN)
        e.slots_decode(N_GEN - 1)
        got_t, got_lp = _read(e, 2)
        assert got_t[-1] == V - 1 and b"".join(toks[t] for t in got_t[:-1]).decode() in choices      # one whole choice, from the root
        want_t, want_lp = _forced(e, 2, P, head + E, before_last=lambda e_: e_.set_row_guide(2, h), eos=eos)
        assert got_t == want_t and _same_lp(got_lp, want_lp)
        assert got_t != _forced(e, 2, P, head + E, eos=eos)[0][:len(got_t)]      # the guide decides the tokens
        e.slots_reset()
        e.destroy_guide(h)

        # ---- stop strings: the row ends at the right token of the NEW output, and the hit indexes the new output
        free_t, _ = _extended(e, 2, P, E)                              # no first turn here: the prefill's token is dropped at once
        text = b"".join(toks[t] for t in free_t)
        ends = np.cumsum([len(toks[t]) for t in free_t])
        j = next(i for i in range(3, N_GEN - 1) if free_t[i] >= 256 and free_t[i + 1] >= 256)      # two tokens of two ASCII bytes each
        stop = (toks[free_t[j]] + toks[free_t[j + 1]]).decode("ascii")
        at = text.find(stop.encode("ascii")) + len(stop)               # first occurrence, wherever it is
        k = int(np.searchsorted(ends, at))                             # the token that completes it
        hs = e.create_stop([stop])
        _start(e)
        e.set_row_stop(2, hs)
        e.slots_prefill([2], P, [len(P)], [4])                         # the automaton has walked the prefill's token
        e.slots_extend([2], [E], max_new_tokens=N_GEN)
        e.slots_decode(N_GEN - 1)
        fin, lens = e.slots_poll()
        assert fin[2] == 1 and lens[2] == k + 1
        assert e.slot_read(2, N_GEN).tolist() == free_t[:k + 1]
        hit = e.row_stop_hit(2)
        assert hit is not None and hit[0] == k and hit[3] == 0
        e.slots_reset()

        # ---- a seeded sampled row: the same tokens in two slots, other tokens for another seed
        def sampled(slot, seed):
            _start(e)
            e.set_row_sampling(slot, SamplingParams(temperature=1.0, top_p=0.95, seed=seed))
            e.slots_prefill([slot], P, [len(P)], [8])
            e.slots_decode(3)
            e.slots_extend([slot], [E], max_new_tokens=N_GEN)
            e.slots_decode(N_GEN - 1)
            fin, lens = e.slots_poll()
            assert fin[slot] == 1 and lens[slot] == N_GEN
            return e.slot_read(slot, N_GEN).tolist()

        a, b, c = sampled(1, 77), sampled(6, 77), sampled(1, 78)
        assert a == b and a != c and a != free_t
        e.slots_reset()
    finally:
        e.close()


# ---------------------------------------------------------------------------------------------------- 6. refusals change nothing

def test_refusals_change_nothing(small):
    cfg, e = small
    P, big = _prompt(cfg, 61, seed=8), _prompt(cfg, 600, seed=8)
    cap = 40
    want = _plain(e, 0, P, n_gen=cap)
    E = _suffix(cfg, 5, seed=8)

    _start(e)
    e.kv_swap_reserve(12)
    # slot 0: 2 pages (61 + 40 tokens); slot 5: 10 pages (600 + 40): the pool of 12 is full
    e.slots_prefill([0, 5], np.concatenate([P, big]), [len(P), len(big)], [cap, 40])
    pool = e.kv_pool_info()
    assert pool == (12, 0)

    def refused(code, slots, ids_list, **kw):
        with pytest.raises(DotsEngineError, match=rf"\({code}\)"):
            e.slots_extend(slots, ids_list, **kw)
        assert e.kv_pool_info() == pool

    refused(-3, [1], [E])                                              # a free slot
    refused(-1, [0, 0], [E, E])                                        # listed twice
    refused(-1, [0], [[]])                                             # nothing to feed
    refused(-1, [8], [E])                                              # out of range
    refused(-1, [0], [[cfg.image_token_id]])                           # vision rows enter at the prefill only
    refused(-4, [0], [E], max_new_tokens=640)                          # beyond max_seq_len
    # one page short, off a page boundary: 61 + 44 = 105 tokens + 24 ahead = 129 -> 3 pages, the slot holds 2, none is free
    refused(-4, [0], [_suffix(cfg, 44, seed=8)], max_new_tokens=24)
    # ... and on one: 61 + 67 = 128 tokens + 1 ahead -> 3 pages
    refused(-4, [0], [_suffix(cfg, 67, seed=8)], max_new_tokens=1)
    e.set_row_sampling(0, SamplingParams(temperature=0.0, repetition_penalty=1.2))
    refused(-3, [0], [E])                                              # a row that carries a penalty
    e.set_row_sampling(0, None)
    e.slots_decode(2)
    e.slot_suspend(5)
    pool = e.kv_pool_info()
    refused(-3, [5], [E])                                              # a suspended slot
    e.slot_release(5)
    pool = e.kv_pool_info()
    e.slots_decode(cap - 3)
    assert _read_tokens(e, 0, cap) == want                             # the slot decoded exactly what it would have
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

    # ---- the pool exactly sufficient: 61 + 66 = 127 tokens + 1 ahead = 128 -> 2 pages, with no page free
    _start(e)
    e.slots_prefill([0, 5], np.concatenate([P, big]), [len(P), len(big)], [cap, 40])
    assert e.kv_pool_info() == (12, 0)
    e.slots_extend([0], [_suffix(cfg, 66, seed=8)], max_new_tokens=1)
    assert e.kv_pool_info() == (12, 0) and e.slots_poll()[0][0] == 1
    e.slots_reset()


def _read_tokens(e, s, n):
    fin, lens = e.slots_poll()
    assert fin[s] == 1 and lens[s] == n, (fin, lens)
    return e.slot_read(s, n).tolist()


# ---------------------------------------------------------------------------------------------------- several prompts per page

def _lone(e, ids, image, suf, sp=None, lp=None, n_gen=N_GEN):
    """the prefix prefilled alone into slot 0 and extended by one suffix"""
    _start(e)
    if sp is not None:
        e.set_row_sampling(0, sp)
    if lp is not None:
        e.set_row_logprobs(0, lp)
    e.vit_forward(*image)
    e.slots_prefill([0], ids, [len(ids)], [4])
    e.slots_extend([0], [suf], max_new_tokens=n_gen)
    e.slots_decode(n_gen - 1)
    fin, lens = e.slots_poll()
    assert fin[0] == 1 and lens[0] == n_gen
    return e.slot_read(0, n_gen).tolist(), (e.row_logprobs(0, n_gen) if lp is not None else None)


def test_suffixes_through_the_scheduler(eng):
    import dataclasses
    from dots_ocr_amd.scheduler import ContinuousBatcher, Request
    cfg, e = eng
    ids, pv, grid = _image_prompt(cfg, 70)
    sufs = [_suffix(cfg, n, seed=10) for n in (3, 9, 5)]
    sp = SamplingParams(temperature=1.0, top_p=0.95, seed=500)
    want = [_lone(e, ids, (pv, grid), suf, dataclasses.replace(sp, seed=500 + i), lp=2) for i, suf in enumerate(sufs)]
    other = _prompt(cfg, 40, seed=9)
    other_alone = _plain(e, 0, other, n_gen=30)
    e.slots_reset()
    cb = ContinuousBatcher(e, chunk=8)
    first, second = Request(ids, pv, grid, N_GEN, sampling=sp, logprobs=2, suffixes=sufs), Request(other, max_new_tokens=30)
    out = cb.run([first, second])
    assert cb.admissions == 1                                          # one tower and one prefill for the three prompts
    assert [o.tolist() for o in first.outputs] == [t for t, _ in want]
    assert len({tuple(t) for t, _ in want}) == 3
    for got, (_, w) in zip(first.logprobs_out, want):
        assert _same_lp(got, w)
    assert out[0].tolist() == want[0][0] and out[1].tolist() == other_alone
    assert first.kv_truncated_each == [False] * 3
    assert e.kv_pool_info()[1] == e.kv_pool_info()[0]


def test_generate_with_prompt_suffixes():
    from dots_ocr_amd.modeling import DotsOcrHipForCausalLM
    cfg = _cfg()
    model = DotsOcrHipForCausalLM(cfg, random_state_dict(cfg, seed=11), device=0, max_batch=4, max_seq_len=640, max_patches=4096)
    try:
        e = model.engine
        ids, pv, grid = _image_prompt(cfg, 70)
        sufs = [_suffix(cfg, n, seed=11) for n in (4, 9)]
        want = [_lone(e, ids, (pv, grid), suf)[0] for suf in sufs]
        out = model.generate(input_ids=torch.from_numpy(ids).long()[None], pixel_values=torch.from_numpy(pv), image_grid_thw=torch.from_numpy(grid),
                             max_new_tokens=N_GEN, eos_token_id=[], prompt_suffixes=sufs)
        assert out.shape == (2, len(ids) + N_GEN)
        assert out[:, :len(ids)].tolist() == [ids.tolist()] * 2 and out[:, len(ids):].tolist() == want
        assert want[0] != want[1]
        for kw in (dict(num_return_sequences=2), dict(num_beams=2), dict(repetition_penalty=1.2), dict(speculative_ngram=2), dict(continuous=False)):
            with pytest.raises(ValueError, match="prompt_suffixes"):
                model.generate(input_ids=torch.from_numpy(ids).long()[None], pixel_values=torch.from_numpy(pv), image_grid_thw=torch.from_numpy(grid),
                               max_new_tokens=4, prompt_suffixes=sufs, **kw)
    finally:
        model.engine.close()


# ---------------------------------------------------------------------------------------------------- against the oracle

def test_first_logits_after_an_extend_match_the_oracle(eng):
    """the bound of tests/test_model_gpu.py::test_prefill_and_decode_logits_match_oracle for decode-step logits: max |error| below 3 % of
    the oracle's logit range, against the bf16-emulated oracle's logits for prefix + suffix"""
    from oracle import model as om
    cfg, e = eng
    sd = random_state_dict(cfg, seed=11)
    ids, pv, grid = _image_prompt(cfg, 61)
    E = _suffix(cfg, 9, seed=9)
    _start(e)
    e.vit_forward(pv, grid)
    e.slots_prefill([2], ids, [len(ids)], [4])
    e.slots_extend([2], [E], max_new_tokens=4)
    got = torch.from_numpy(e.slot_logits(2))
    first = int(e.slot_read(2, 1)[0])
    full = torch.cat([torch.from_numpy(ids).long(), torch.tensor(E)])
    toks, lg = om.generate(sd, cfg, full, torch.from_numpy(pv), torch.from_numpy(grid), 1, emulate_bf16=True, return_logits=True)
    rng = (lg[0].max() - lg[0].min()).item()
    err = (got - lg[0]).abs().max().item()
    print(f"first logits after an extend: err vs emu {err:.4f} (range {rng:.2f})")
    assert err < 0.03 * rng
    top2 = torch.topk(lg[0], 2).values
    if (top2[0] - top2[1]).item() > 4 * err:
        assert first == toks[0]
    e.slots_reset()


# ---------------------------------------------------------------------------------------------------- 7. nothing left pending

def test_extend_leaves_no_pending_hip_error_behind():
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
    e.slots_extend([1, 3], [_suffix(cfg, 9), _suffix(cfg, 2)], max_new_tokens=6)
    e.slots_decode(5)
    assert e.slots_poll()[1].tolist() == [0, 6, 0, 6]
    with pytest.raises(DotsEngineError):
        e.slots_extend([0], [[1]])
    e.stats()
    assert hip.hipGetLastError() == 0, "a HIP error was left pending after an extend"
    y = torch.ones(8, device="cuda") * 2
    torch.cuda.synchronize()
    assert float(y.sum()) == 16.0
    e.close()
