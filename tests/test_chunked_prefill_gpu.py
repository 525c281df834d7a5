"""Chunked prefill on the GPU: Engine.slots_prefill_begin / slots_prefill_advance fill a prompt in passes over its own KV
pages.

The claim is exact: what a position computes does not depend on where the cuts fall.  So most comparisons here are for equality of bits —
logits, KV pages, tokens, logprobs — between fills with different chunks, between a fill that shared its engine with decode steps and one
that did not, and between an engine whose workspace holds the prompt and one whose workspace does not.  Against the one-shot prefill only
layer 0's K / V are bitwise (later layers pass through a different attention kernel); the first logits are held to the CPU oracle at the
bounds tests/test_model_gpu.py::test_prefill_and_decode_logits_match_oracle applies, and under the fp8 cache to the quantised-cache oracle
of tests/test_kv_fp8_gpu.py fed the prompt position by position — a chunked fill reads every earlier position quantised, its own pass
included, which the one-shot prefill does not (two different valid evaluations).
"""
import numpy as np
import pytest
import torch

from dots_ocr_amd import guided as G
from dots_ocr_amd.config import DotsConfig
from dots_ocr_amd.engine import DotsEngineError, E_CAPACITY, E_INVALID, E_STATE, LogitRules, SamplingParams
from dots_ocr_amd.weights import random_state_dict
from oracle import model as om
from test_kv_fp8_gpu import QuantKVCache

pytestmark = pytest.mark.gpu

N_GEN = 9                     # the first token and the next 8
L_IMAGE, L_TEXT = 233, 261    # len % 64 != 0 and > 192: three full cuts and a ragged tail at chunk 64
WHOLE = 320                   # a chunk that holds either prompt
DTYPES = ["bf16", "fp8"]


def _cfg():
    return DotsConfig.tiny()


_SD = {}


def _sd():
    if "sd" not in _SD:
        _SD["sd"] = random_state_dict(_cfg(), seed=11)
    return _SD["sd"]


def _scales(cfg):
    return (0.5 + np.random.default_rng(4).random((cfg.num_hidden_layers, cfg.num_key_value_heads, 2))).astype(np.float32)


def _engine(dtype="bf16", **kw):
    from dots_ocr_amd.engine import Engine
    cfg = _cfg()
    args = dict(max_batch=8, max_seq_len=640, max_patches=1024, max_prefill_tokens=2048, kv_cache_dtype=dtype)
    args.update(kw)
    e = Engine(cfg, **args)
    e.load_state_dict(_sd())
    if dtype == "fp8":
        e.set_kv_scales(_scales(cfg))
    return e


@pytest.fixture(scope="module")
def engines():
    es = {d: _engine(d) for d in DTYPES}
    yield es
    for e in es.values():
        e.close()


def _text(cfg, L, seed=0):
    return np.random.default_rng(7000 + 13 * L + seed).integers(0, cfg.vocab_size - 8, L).astype(np.int32)


def _image(cfg, L):
    """the smallest grid the tiny tower takes: 1 x 4 x 4 patches = 4 merged rows"""
    pv = torch.randn(16, cfg.vision.patch_dim, generator=torch.Generator().manual_seed(L)).numpy()
    ids = _text(cfg, L)
    ids[3:7] = cfg.image_token_id
    return ids, (pv, np.array([[1, 4, 4]], np.int64))


def _prompt(cfg, kind):
    # text seed 1: the tiny random model falls into a constant continuation behind some prompts, which would show nothing
    return _image(cfg, L_IMAGE) if kind == "image" else (_text(cfg, L_TEXT, seed=1), None)


def _start(e):
    e.set_sampling(0.0, 1.0, 0)
    e.slots_reset()
    e.set_eos([])


def _fill(e, s, ids, chunk, image=None, max_new=N_GEN):
    if image is not None:
        e.vit_forward(*image)
    e.slots_prefill_chunked([s], ids, [len(ids)], [max_new], chunk)


def _kv(e, s, L):
    return [e.read_kv(layer, s, 0, L, w) for layer in range(e.cfg.num_hidden_layers) for w in ("k", "v")]


def _bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _state(e, s, L, n_gen=N_GEN):
    """everything the claim covers, of slot s just filled with an L-token prompt: logits, K / V of every layer over every position, then
    n_gen tokens (the first included) and their logprobs"""
    st = dict(logits=e.slot_logits(s), kv=_kv(e, s, L))
    e.slots_decode(n_gen - 1)
    fin, lens = e.slots_poll()
    assert fin[s] == 1 and lens[s] == n_gen
    st["tokens"] = e.slot_read(s, n_gen).tolist()
    st["lp"] = e.row_logprobs(s, n_gen)
    return st


def _assert_same_state(a, b, what):
    assert _same(a["logits"], b["logits"]), f"{what}: the first logits differ"
    assert a["tokens"][0] == b["tokens"][0], f"{what}: the first token differs"
    for i, (x, y) in enumerate(zip(a["kv"], b["kv"])):
        assert _same(x, y), f"{what}: layer {i // 2} {'KV'[i % 2]} differs at positions {sorted(set(np.nonzero(x != y)[1].tolist()))[:8]}"
    assert a["tokens"] == b["tokens"], f"{what}: the generated tokens differ"
    assert all(_same(x, y) for x, y in zip(a["lp"], b["lp"])), f"{what}: the logprobs differ"


def _filled_state(e, kind, chunk, s=2):
    ids, image = _prompt(e.cfg, kind)
    _start(e)
    e.set_row_logprobs(s, 5)
    _fill(e, s, ids, chunk, image)
    return _state(e, s, len(ids))


_REF = {}


def _ref(engines, dtype, kind):
    """the fill whose chunk holds the whole prompt: computed once per (cache, prompt), shared, never changed"""
    if (dtype, kind) not in _REF:
        _REF[dtype, kind] = _filled_state(engines[dtype], kind, WHOLE)
    return _REF[dtype, kind]


# ---------------------------------------------------------------------------------------------------- 1. cut invariance, bitwise

@pytest.mark.parametrize("chunk", [64, 128, 192])
@pytest.mark.parametrize("kind", ["image", "text"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_the_cuts_do_not_change_a_bit(engines, dtype, kind, chunk):
    want = _ref(engines, dtype, kind)
    got = _filled_state(engines[dtype], kind, chunk)
    _assert_same_state(got, want, f"{dtype} {kind} chunk {chunk}")
    assert len(set(want["tokens"])) > 1                                  # not a constant continuation


# ---------------------------------------------------------------------------------------------------- 2. layer 0 against the one-shot prefill

@pytest.mark.parametrize("kind", ["image", "text"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_layer_0_pages_equal_the_one_shot_prefill(engines, dtype, kind):
    """layer 0's K / V do not pass through attention: a wrong page index, rope position or tile offset shows here"""
    e = engines[dtype]
    ids, image = _prompt(e.cfg, kind)
    _start(e)
    if image is not None:
        e.vit_forward(*image)
    e.slots_prefill([2], ids, [len(ids)], [N_GEN])
    one_shot = _kv(e, 2, len(ids))[:2]
    for chunk in (64, 192):
        _start(e)
        _fill(e, 5, ids, chunk, image)
        for got, want, w in zip(_kv(e, 5, len(ids))[:2], one_shot, "KV"):
            assert _same(got, want), f"{dtype} {kind} chunk {chunk}: layer 0 {w} differs from the one-shot prefill"


# ---------------------------------------------------------------------------------------------------- 3. against the oracle

def _embeds(cfg, ids, image):
    sd = _sd()
    vis = None
    if image is not None:
        vis = om.vision_tower(sd, cfg, torch.from_numpy(image[0]), torch.from_numpy(image[1]), emulate_bf16=True)
    return om._r(om.build_embeds(sd, cfg, torch.from_numpy(ids).long(), vis), True)


@pytest.mark.parametrize("kind", ["image", "text"])
def test_first_logits_match_the_oracle(engines, kind):
    cfg = _cfg()
    ids, image = _prompt(cfg, kind)
    got = _ref(engines, "bf16", kind)
    pv, grid = (torch.from_numpy(image[0]), torch.from_numpy(image[1])) if image is not None else (None, None)
    toks, lg = om.generate(_sd(), cfg, torch.from_numpy(ids).long(), pv, grid, 1, emulate_bf16=True, return_logits=True)
    _, lg32 = om.generate(_sd(), cfg, torch.from_numpy(ids).long(), pv, grid, 1, emulate_bf16=False, return_logits=True)
    logits = torch.from_numpy(got["logits"])
    rng = (lg[0].max() - lg[0].min()).item()
    err, err32 = (logits - lg[0]).abs().max().item(), (logits - lg32[0]).abs().max().item()
    print(f"{kind}: first logits after a chunked fill: err vs emu {err:.4f} vs fp32 {err32:.4f} (range {rng:.2f})")
    assert err < 0.03 * rng and err32 < 0.06 * rng
    top2 = torch.topk(lg[0], 2).values
    if (top2[0] - top2[1]).item() > 4 * err:
        assert got["tokens"][0] == toks[0]


@pytest.mark.parametrize("kind", ["image", "text"])
def test_first_logits_match_the_quantised_cache_oracle_fed_position_by_position(engines, kind):
    """under the fp8 cache a chunked fill reads every earlier position quantised, its own pass included: the reference is the oracle whose
    cache quantises its history, fed one position at a time"""
    cfg = _cfg()
    ids, image = _prompt(cfg, kind)
    got = _ref(engines, "fp8", kind)
    emb = _embeds(cfg, ids, image)
    cache = QuantKVCache(cfg.num_hidden_layers, torch.from_numpy(_scales(cfg)))
    with torch.no_grad():
        for t in range(len(ids)):
            ref = om.lm_forward(_sd(), cfg, emb[t:t + 1], cache, True)[0]
    logits = torch.from_numpy(got["logits"])
    rng, err = float(ref.max() - ref.min()), float((logits - ref).abs().max())
    print(f"{kind}: fp8-KV first logits after a chunked fill: err vs the quantised-cache oracle {err:.4f} (range {rng:.2f})")
    assert err < 0.03 * rng
    top2 = torch.topk(ref, 2).values
    if float(top2[0] - top2[1]) > 4 * err:
        assert got["tokens"][0] == int(torch.argmax(ref))
    # the one-shot prefill attends over unquantised K / V: a different valid evaluation, so the two fills are not bit-equal here
    e = engines["fp8"]
    _start(e)
    if image is not None:
        e.vit_forward(*image)
    e.slots_prefill([2], ids, [len(ids)], [N_GEN])
    assert not _same(e.slot_logits(2), got["logits"])


# ---------------------------------------------------------------------------------------------------- 4. beyond the workspace

@pytest.mark.parametrize("dtype", DTYPES)
def test_a_prompt_longer_than_the_workspace(engines, dtype):
    cfg = _cfg()
    ids = _text(cfg, 300, seed=4)
    big = engines[dtype]
    _start(big)
    big.set_row_logprobs(2, 5)
    _fill(big, 2, ids, WHOLE)
    want = _state(big, 2, len(ids))
    small = _engine(dtype, max_prefill_tokens=128)
    try:
        _start(small)
        with pytest.raises(DotsEngineError) as ei:
            small.slots_prefill([2], ids, [len(ids)], [N_GEN])                # unchanged: the one-shot prefill is bounded by the workspace
        assert ei.value.code == E_CAPACITY and small.kv_pool_info()[0] == small.kv_pool_info()[1]
        with pytest.raises(DotsEngineError) as ei:
            small.slots_prefill_advance(192)                                 # a pass is bounded by it too
        assert ei.value.code == E_INVALID
        small.set_row_logprobs(2, 5)
        _fill(small, 2, ids, 128)
        _assert_same_state(_state(small, 2, len(ids)), want, f"{dtype}: a 128-token workspace")
    finally:
        small.close()


# ---------------------------------------------------------------------------------------------------- 5. interleaving is exact

def _bystanders(e, fill=None):
    """slots 0-2 decode 4 steps at a time; fill(e, round) runs before each chunk.  -> their tokens and logprobs"""
    cfg = e.cfg
    others = [_text(cfg, 70 + 9 * i, seed=20 + i) for i in range(3)]
    _start(e)
    for s in range(3):
        e.set_row_logprobs(s, 5)
    e.slots_prefill([0, 1, 2], np.concatenate(others), [len(o) for o in others], [41] * 3)
    for r in range(10):
        if fill is not None:
            fill(e, r)
        e.slots_decode(4)
    fin, lens = e.slots_poll()
    assert all(fin[s] == 1 and lens[s] == 41 for s in range(3))
    return [(e.slot_read(s, 41).tolist(), e.row_logprobs(s, 41)) for s in range(3)]


@pytest.mark.parametrize("kind", ["image", "text"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_fill_between_decode_chunks_disturbs_nothing(engines, dtype, kind):
    e = engines[dtype]
    want_fill = _ref(engines, dtype, kind)
    ids, image = _prompt(e.cfg, kind)
    undisturbed = _bystanders(e)
    seen = {}

    def fill(e, r):
        if r == 0:
            e.set_row_logprobs(3, 5)
            if image is not None:
                e.vit_forward(*image)
            e.slots_prefill_begin([3], ids, [len(ids)], [N_GEN])
            assert e.slots_poll()[0][3] == 3
        if "left" not in seen or seen["left"] > 0:
            seen["left"] = e.slots_prefill_advance(64)
            if seen["left"] == 0:                                          # just completed: before any step runs over it
                seen["logits"], seen["kv"] = e.slot_logits(3), _kv(e, 3, len(ids))

    got = _bystanders(e, fill)
    for s, ((t0, lp0), (t1, lp1)) in enumerate(zip(undisturbed, got)):
        assert t0 == t1 and all(_same(x, y) for x, y in zip(lp0, lp1)), f"bystander {s} was disturbed by the fill"
    fin, lens = e.slots_poll()
    assert fin[3] == 1 and lens[3] == N_GEN
    mine = dict(logits=seen["logits"], kv=seen["kv"], tokens=e.slot_read(3, N_GEN).tolist(), lp=e.row_logprobs(3, N_GEN))
    _assert_same_state(mine, want_fill, f"{dtype} {kind}: a fill interleaved with decode chunks")


@pytest.mark.parametrize("dtype", DTYPES)
def test_two_prompts_filling_at_once(engines, dtype):
    e = engines[dtype]
    cfg = e.cfg
    (ids_a, image), ids_b = _image(cfg, L_IMAGE), _prompt(cfg, "text")[0]
    _start(e)
    for s in (1, 4):
        e.set_row_logprobs(s, 5)
    e.vit_forward(*image)
    e.slots_prefill_begin([4], ids_a, [len(ids_a)], [N_GEN])
    assert e.slots_prefill_advance(128) == L_IMAGE - 128
    e.slots_prefill_begin([1], ids_b, [len(ids_b)], [N_GEN])               # joins while the first is half filled
    left, done_at, passes = None, {}, 0
    while left != 0:
        left = e.slots_prefill_advance(128)
        passes += 1
        fin = e.slots_poll()[0]
        for s in (4, 1):
            if fin[s] == 0 and s not in done_at:
                done_at[s] = passes
                done_at[s, "logits"], done_at[s, "kv"] = e.slot_logits(s), _kv(e, s, L_IMAGE if s == 4 else L_TEXT)
    assert done_at[4] < done_at[1]                                         # the older fill finishes passes earlier
    e.slots_decode(N_GEN - 1)
    for s, kind in ((4, "image"), (1, "text")):
        mine = dict(logits=done_at[s, "logits"], kv=done_at[s, "kv"], tokens=e.slot_read(s, N_GEN).tolist(), lp=e.row_logprobs(s, N_GEN))
        _assert_same_state(mine, _ref(engines, dtype, kind), f"{dtype}: {kind} prompt filled beside another")


# ---------------------------------------------------------------------------------------------------- 6. the end state is a prefilled slot's

def _token_bytes(V):
    toks = [bytes([i]) for i in range(256)] + [bytes([97 + i % 3, 32 if i % 5 == 0 else 97 + (i // 3) % 3]) for i in range(256, V)]
    return G.TokenBytes(toks, range(V - 8, V))


def _read_all(e, slots):
    fin, lens = e.slots_poll()
    return [(int(fin[s]), e.slot_read(s, int(lens[s])).tolist(), e.row_logprobs(s, int(lens[s]))) for s in slots]


def _same_runs(a, b):
    return len(a) == len(b) and all(x[0] == y[0] and x[1] == y[1] and all(_same(p, q) for p, q in zip(x[2], y[2])) for x, y in zip(a, b))


def _after_fork(e, chunk):
    ids, image = _image(e.cfg, L_IMAGE)
    pens = [SamplingParams(temperature=0.8, top_p=0.95, seed=31 + i, repetition_penalty=1.3, frequency_penalty=0.5) for i in range(3)]
    _start(e)
    for s in range(3):
        e.set_row_sampling(s, pens[s])
        e.set_row_logprobs(s, 3)
    _fill(e, 0, ids, chunk, image, max_new=24)
    e.slots_fork(0, [1, 2])
    e.slots_decode(23)
    forked = _read_all(e, [0, 1, 2])
    # children equal independent requests (tests/test_fork_gpu.py's statement): the same prompt filled into each slot under its own settings
    alone = []
    for s in range(3):
        _start(e)
        e.set_row_sampling(s, pens[s])
        e.set_row_logprobs(s, 3)
        _fill(e, s, ids, chunk, image, max_new=24)
        e.slots_decode(23)
        alone += _read_all(e, [s])
    assert _same_runs(forked, alone), "a child of a chunked fill is not the independent request"
    assert len({tuple(r[1]) for r in forked}) == 3
    return forked


def _after_extend(e, chunk):
    ids, image = _image(e.cfg, L_IMAGE)
    E = [int(t) for t in _text(e.cfg, 9, seed=3)]
    _start(e)
    e.set_row_logprobs(2, 5)
    _fill(e, 2, ids, chunk, image, max_new=4)
    e.slots_extend([2], [E], keep_pending=False, max_new_tokens=12)
    e.slots_decode(11)
    return _read_all(e, [2])


def _after_suspend(e, chunk):
    ids, image = _image(e.cfg, L_IMAGE)
    e.kv_swap_reserve(8)
    _start(e)
    e.set_row_logprobs(2, 5)
    _fill(e, 2, ids, chunk, image, max_new=12)
    e.slots_decode(3)
    e.slot_suspend(2)
    assert e.slots_poll()[0][2] == 2
    e.slot_resume(2)
    e.slots_decode(8)
    out = _read_all(e, [2])
    e.slots_reset()
    e.kv_swap_reserve(0)
    return out


def _after_row_features(e, chunk):
    """a guide, stop strings, logit rules and a repetition penalty set BEFORE begin: set, then fill"""
    cfg = e.cfg
    ids, image = _image(cfg, L_IMAGE)
    ids = ids.copy()
    ids[20:40] = np.arange(97, 117)                                        # the prompt holds what the guide allows: the presence bits matter
    if e.token_bytes is None:
        e.set_token_bytes(_token_bytes(cfg.vocab_size))
    h = e.create_guide(G.compile_regex(r"[a-c ]*"))
    _start(e)
    e.set_row_guide(2, h)
    e.set_row_stop(2, e.create_stop(["cab", "bb a"]), 2)
    e.set_row_logit_rules(2, LogitRules(bias={97: -1.5, 98: 0.75}, min_tokens=3))
    e.set_row_sampling(2, SamplingParams(temperature=0.7, seed=5, repetition_penalty=1.4, presence_penalty=0.3))
    e.set_row_logprobs(2, 3)
    _fill(e, 2, ids, chunk, image, max_new=20)
    e.slots_decode(19)
    out = _read_all(e, [2]) + [e.row_stop_hit(2), e.row_guide_state(2)]
    e.slots_reset()
    e.destroy_guide(h)
    return out


@pytest.mark.parametrize("what", ["fork", "extend", "suspend", "row_features"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_the_end_state_is_that_of_a_prefill(engines, dtype, what):
    e = engines[dtype]
    run = {"fork": _after_fork, "extend": _after_extend, "suspend": _after_suspend, "row_features": _after_row_features}[what]
    cut, whole = run(e, 64), run(e, WHOLE)
    if what == "row_features":
        assert cut[1:] == whole[1:], "stop hit or guide state differ"
        cut, whole = cut[:1], whole[:1]
    assert _same_runs(cut, whole), f"{dtype} {what}: behind a fill cut at 64 it differs from behind an uncut fill"
    assert all(len(r[1]) >= 1 for r in cut)


# ---------------------------------------------------------------------------------------------------- 7. refusals

def test_what_a_filling_slot_refuses(engines):
    e = engines["bf16"]
    cfg = e.cfg
    ids, other = _text(cfg, L_TEXT), _text(cfg, 50, seed=2)
    _start(e)
    pool0 = e.kv_pool_info()
    e.slots_prefill_begin([3], ids, [len(ids)], [8])
    assert e.slots_prefill_advance(64) == L_TEXT - 64
    pool1 = e.kv_pool_info()
    assert pool1[1] == pool0[1] - (L_TEXT + 8 + 63) // 64                  # a filling slot's pages count as used
    e.slots_prefill([0], other, [len(other)], [8])                         # a one-shot prefill of another slot between two passes
    pool2 = e.kv_pool_info()

    def state():
        return e.kv_pool_info(), e.slots_poll()[0].tolist(), e.slots_poll()[1].tolist()

    before = state()
    assert before[1][3] == 3 and before[1][0] == 0
    refused = [
        lambda: e.slot_suspend(3),
        lambda: e.slots_extend([3], [[5, 6]], max_new_tokens=4),
        lambda: e.slots_fork(3, [4]),
        lambda: e.slots_fork(0, [3]),                                      # as a destination too
        lambda: e.slots_beam(3, [4]),
        lambda: e.slots_beam(0, [3]),
        lambda: e.slot_read(3, 4),
        lambda: e.slot_logits(3),
        lambda: e.slots_prefill([3], other, [len(other)], [8]),
        lambda: e.slots_prefill_begin([3], other, [len(other)], [8]),
    ]
    for i, call in enumerate(refused):
        with pytest.raises(DotsEngineError) as ei:
            call()
        assert ei.value.code == E_STATE, (i, str(ei.value))
        assert i not in (3, 5, 8, 9) or "filling" in str(ei.value), (i, str(ei.value))
        assert state() == before, f"refusal {i} changed something"
    for bad in (0, 63, 100, 4096):                                         # not a positive multiple of 64, or above max_prefill_tokens
        with pytest.raises(DotsEngineError) as ei:
            e.slots_prefill_advance(bad)
        assert ei.value.code == E_INVALID and state() == before
    # the bystander decodes on while slot 3 fills; a release while filling returns the pages
    e.slots_decode(2)
    e.slot_release(3)
    assert e.kv_pool_info() == (pool0[0], pool0[1] - (pool1[1] - pool2[1])) and e.slots_poll()[0][3] == -1
    assert e.slots_prefill_advance(64) == 0                                # nothing is filling: a no-op
    e.slots_prefill_begin([3], ids, [len(ids)], [8])
    e.slots_reset()                                                        # drops every fill
    assert e.kv_pool_info() == pool0 and e.slots_poll()[0][3] == -1 and e.slots_prefill_advance(64) == 0


def test_the_pool_bounds_a_begin_all_or_nothing():
    e = _engine("bf16", kv_pool_tokens=8 * 64)
    try:
        cfg = e.cfg
        _start(e)
        e.slots_prefill_begin([0], _text(cfg, L_TEXT), [L_TEXT], [8])      # 5 of 8 pages
        pool = e.kv_pool_info()
        two = [_text(cfg, 60, seed=1), _text(cfg, 150, seed=2)]            # 2 + 3 pages: the first alone would fit
        with pytest.raises(DotsEngineError) as ei:
            e.slots_prefill_begin([1, 2], np.concatenate(two), [60, 150], [8, 8])
        assert ei.value.code == E_CAPACITY and e.kv_pool_info() == pool and e.slots_poll()[0].tolist()[:3] == [3, -1, -1]
        while e.slots_prefill_advance(128):
            pass
        assert e.slots_poll()[0][0] == 0 and e.slots_poll()[1][0] == 1
    finally:
        e.close()


def test_begin_is_refused_on_a_speculating_engine(engines):
    e = engines["bf16"]
    ids = _text(e.cfg, 100)
    _start(e)
    e.set_speculation(3)
    try:
        with pytest.raises(DotsEngineError, match="speculat") as ei:
            e.slots_prefill_begin([0], ids, [len(ids)], [8])
        assert ei.value.code == E_STATE and e.kv_pool_info()[0] == e.kv_pool_info()[1]
    finally:
        e.slots_reset()
        e.set_speculation(0)
    e.slots_prefill_begin([0], ids, [len(ids)], [8])
    with pytest.raises(DotsEngineError) as ei:                             # and speculation cannot be switched on over a fill
        e.set_speculation(3)
    assert ei.value.code == E_STATE
    e.slots_reset()


# ---------------------------------------------------------------------------------------------------- 8. through the scheduler and the server

def test_six_requests_through_three_slots(engines):
    """request by request the tokens of Engine.slots_prefill_chunked plus greedy decode run alone"""
    from dots_ocr_amd.scheduler import ContinuousBatcher, Request
    e = _engine("bf16", max_batch=3)
    try:
        cfg = e.cfg
        prompts = [_image(cfg, 90), (_text(cfg, 150, seed=1), None), (_text(cfg, 61, seed=2), None), _image(cfg, 200), (_text(cfg, 129, seed=3), None),
                   (_text(cfg, 64, seed=4), None)]
        caps = [10, 7, 12, 9, 6, 11]
        alone = []
        for (ids, image), cap in zip(prompts, caps):
            _start(e)
            _fill(e, 1, ids, 64, image, max_new=cap)
            if cap > 1:
                e.slots_decode(cap - 1)
            alone.append(e.slot_read(1, cap).tolist())
        reqs = [Request(ids, None if image is None else image[0], None if image is None else image[1], cap) for (ids, image), cap in zip(prompts, caps)]
        cb = ContinuousBatcher(e, eos_ids=(), chunk=4, prefill_chunk=64)
        outs = cb.run(reqs)
        assert [o.tolist() for o in outs] == alone
        assert cb.fill_passes >= sum(-(-len(ids) // 64) for ids, _ in prompts) - 2 and e.kv_pool_info()[0] == e.kv_pool_info()[1]
        assert len({tuple(a) for a in alone}) == len(alone)
    finally:
        e.close()


def test_the_server_and_generate_with_chunked_prefill():
    import threading
    from fastapi.testclient import TestClient
    from dots_ocr_amd.image_utils import PILimage_to_base64
    from dots_ocr_amd.modeling import DotsOcrHipForCausalLM
    from dots_ocr_amd.processing import DotsOcrProcessor
    from dots_ocr_amd.server import create_app
    from dots_ocr_amd.synthetic import synth_page
    cfg = DotsConfig.tiny()
    model = DotsOcrHipForCausalLM(cfg, _sd(), device=0, max_batch=3, max_seq_len=1024, max_patches=4096)
    try:
        proc = DotsOcrProcessor(cfg, engine=model.engine)
        prompt = "Extract the text content from this image."
        pages = [synth_page(i, (224, 252 + 28 * (i % 3))) for i in range(4)]
        n_new = 10

        def direct(page, chunk):
            messages = [{"role": "user", "content": [{"type": "image", "image": page}, {"type": "text", "text": prompt}]}]
            text = proc.apply_chat_template(messages, tokenize=False, add_generation_prompt=True)
            inputs = proc(text=[text], images=[page], padding=True, return_tensors="pt").to("cuda")
            assert inputs.input_ids.shape[1] > 64                          # more than one pass
            out = model.generate(**inputs, max_new_tokens=n_new, prefill_chunk=chunk)
            return proc.batch_decode([out[0, inputs.input_ids.shape[1]:]], skip_special_tokens=True)[0]
        want = [direct(p, 64) for p in pages]
        assert want == [direct(p, 512) for p in pages]                     # generate(prefill_chunk=): the tokens do not depend on it
        app = create_app(model, proc, model_name="model", max_batch=3, max_wait_ms=20, prefill_chunk=64)
        got = [None] * len(pages)
        with TestClient(app) as c:
            def go(i):
                body = {"model": "model", "messages": [{"role": "user", "content": [
                    {"type": "image_url", "image_url": {"url": PILimage_to_base64(pages[i])}},
                    {"type": "text", "text": f"<|img|><|imgpad|><|endofimg|>{prompt}"}]}],
                    "max_completion_tokens": n_new, "temperature": 0.0, "top_p": 1.0}
                r = c.post("/v1/chat/completions", json=body)
                got[i] = (r.status_code, r.json())
            th = [threading.Thread(target=go, args=(i,)) for i in range(len(pages))]
            [t.start() for t in th]
            [t.join() for t in th]
        for i, (code, d) in enumerate(got):
            assert code == 200, d
            assert d["choices"][0]["message"]["content"] == want[i], f"request {i}: the chunking server's text differs from model.generate"
    finally:
        model.engine.close()


# ---------------------------------------------------------------------------------------------------- 9. nothing moves when off

RECORDED = ("slots_reset", "set_eos", "vit_forward", "slots_prefill", "slots_prefill_begin", "slots_prefill_advance", "slots_fork", "slots_extend",
            "slots_decode", "slot_release")


class Recorder:
    """forwards everything to the engine and writes down the calls that change its state"""

    def __init__(self, engine):
        self._e, self.calls = engine, []

    def __getattr__(self, name):
        attr = getattr(self._e, name)
        if name not in RECORDED:
            return attr

        def call(*a, **kw):
            if name == "slots_prefill":
                brief = (tuple(int(s) for s in a[0]), tuple(int(n) for n in a[2]), tuple(int(c) for c in a[3]))
            else:
                brief = tuple(tuple(int(v) for v in x) if isinstance(x, (list, tuple, np.ndarray)) else x for x in a)
            self.calls.append((name,) + brief)
            return attr(*a, **kw)
        return call


def test_nothing_moves_when_off(engines):
    """a ContinuousBatcher without prefill_chunk makes the engine calls it made on the commit before the feature: the list was recorded
    there (the scheduler of that commit over this scenario; with no EOS every request runs to its cap, so the calls follow from the caps)"""
    from dots_ocr_amd.scheduler import ContinuousBatcher, Request
    e = engines["bf16"]
    e.set_sampling(0.0, 1.0, 0)
    caps = [5, 12, 3, 9, 7, 12, 4, 8, 6, 10, 5, 7]
    reqs = [Request(_text(e.cfg, 70 + 9 * i, seed=i), max_new_tokens=c) for i, c in enumerate(caps)]
    rec = Recorder(e)
    outs = ContinuousBatcher(rec, eos_ids=(), chunk=4).run(reqs)
    assert [len(o) for o in outs] == caps
    assert rec.calls == [
        ("set_eos", ()), ("slots_reset",),
        ("slots_prefill", (0, 1, 2, 3, 4, 5, 6, 7), (70, 79, 88, 97, 106, 115, 124, 133), (5, 12, 3, 9, 7, 12, 4, 8)),
        ("slots_decode", 4), ("slot_release", 0), ("slot_release", 2), ("slot_release", 6),
        ("slots_prefill", (0, 2, 6), (142, 151, 160), (6, 10, 5)),
        ("slots_decode", 4), ("slot_release", 3), ("slot_release", 4), ("slot_release", 6), ("slot_release", 7),
        ("slots_prefill", (3,), (169,), (7,)),
        ("slots_decode", 4), ("slot_release", 0), ("slot_release", 1), ("slot_release", 5),
        ("slots_decode", 4), ("slot_release", 2), ("slot_release", 3)]
