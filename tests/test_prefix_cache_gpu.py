"""Prefix caching over the chunked prefill on the GPU: Engine.prefix_cache_lookup / slots_prefill_begin_cached start a fill
behind full prompt pages another sequence filled.

The contract is exact: a hit equals the COLD chunked fill of the same prompt — on an engine that has no cache — in every bit of the first
logits, of every layer's K / V over every position, and of N_GEN tokens and their logprobs.  Every comparison below is for equality.
"""
import numpy as np
import pytest
import torch

from dots_ocr_amd.engine import DotsEngineError, E_INVALID, E_STATE, SamplingParams
from test_chunked_prefill_gpu import (DTYPES, N_GEN, WHOLE, Recorder, _assert_same_state, _engine, _kv, _read_all, _same, _same_runs, _start,
                                      _state, _text)

pytestmark = pytest.mark.gpu

KEY_A, KEY_B = bytes([7, 0] + list(range(1, 15))), bytes([7, 0] + list(range(101, 115)))      # digests hold zero bytes: the keys differ behind one
L_A = 233                     # three full pages and a ragged tail: 192 positions can hit


@pytest.fixture(scope="module")
def engines():
    """per cache dtype: `cold`, the reference engine without the cache, and `hot`, the same engine with it"""
    es = {(d, w): _engine(d) for d in DTYPES for w in ("cold", "hot")}
    yield es
    for e in es.values():
        e.close()


def _pixels(n_patches, seed, cfg):
    return torch.randn(n_patches, cfg.vision.patch_dim, generator=torch.Generator().manual_seed(seed)).numpy()


def _prompt(cfg, L, seed=0, pads=(3, 7), grid=(1, 4, 4), pix_seed=5):
    """an L-token prompt whose image's pads stand at [pads[0], pads[1]): grid 1 x 4 x 4 = 4 merged rows, 1 x 8 x 8 = 16"""
    assert grid[0] * grid[1] * grid[2] // 4 == pads[1] - pads[0]
    ids = _text(cfg, L, seed=seed)
    ids[pads[0]:pads[1]] = cfg.image_token_id
    return ids, (_pixels(grid[0] * grid[1] * grid[2], pix_seed, cfg), np.array([grid], np.int64))


def _tail(cfg, ids, keep, L=None, seed=77):
    """the first `keep` ids, then another tail"""
    L = len(ids) if L is None else L
    out = _text(cfg, L, seed=seed)
    out[:keep] = ids[:keep]
    assert keep < min(L, len(ids)) and out[keep] != ids[keep]
    return out


_COLD = {}


def _cold(engines, dtype, ids, image, n_gen=N_GEN, s=2):
    """the reference, once per (cache dtype, prompt, pixels): a cold chunked fill on the engine without the cache"""
    k = (dtype, ids.tobytes(), None if image is None else image[0].tobytes(), n_gen, s)
    if k not in _COLD:
        e = engines[dtype, "cold"]
        _start(e)
        e.set_row_logprobs(s, 5)
        if image is not None:
            e.vit_forward(*image)
        e.slots_prefill_chunked([s], ids, [len(ids)], [n_gen], WHOLE)
        _COLD[k] = _state(e, s, len(ids), n_gen)
    return _COLD[k]


def _hot(engines, dtype):
    """the caching engine, empty: no slot, no block"""
    e = engines[dtype, "hot"]
    _start(e)
    e.prefix_cache_enable(False)
    e.prefix_cache_enable(True)
    return e


def _fill(e, s, ids, key, image, chunk=64, max_new=N_GEN, expect=None, lease=None):
    """a fill through the cache; image None: the tower cannot run.  -> (hit_tokens, needs_tower)"""
    if lease is None:
        lease, hit, tower = e.prefix_cache_lookup(ids, key)
    else:
        lease, hit, tower = lease
    if expect is not None:
        assert (hit, tower) == expect, f"lookup gave hit {hit}, needs_tower {tower}"
    if tower:
        e.vit_forward(*image)
    e.slots_prefill_begin_cached([s], ids, [len(ids)], [max_new], [lease], [key])
    while e.slots_prefill_advance(chunk) > 0:
        pass
    return hit, tower


def _seed(e, ids, key, image, s=2):
    """a sequence fills the prompt and is released: its full pages stay"""
    _fill(e, s, ids, key, image)
    e.slot_release(s)


# ---------------------------------------------------------------------------------------------------- 1. a hit behind a released sequence

@pytest.mark.parametrize("chunk", [64, WHOLE])
@pytest.mark.parametrize("dtype", DTYPES)
def test_hit_behind_a_released_sequence(engines, dtype, chunk):
    e = _hot(engines, dtype)
    cfg = e.cfg
    a, image = _prompt(cfg, L_A)
    a2 = _tail(cfg, a, 200)
    _seed(e, a, KEY_A, image)
    assert e.prefix_cache_info()["resident"] == 3
    e.set_row_logprobs(5, 5)
    _fill(e, 5, a2, KEY_A, None, chunk, expect=(192, False))                 # no image given: no vit_forward call
    got = _state(e, 5, len(a2))
    _assert_same_state(got, _cold(engines, dtype, a2, image), f"{dtype} chunk {chunk}: a hit of 192 positions")
    assert len(set(got["tokens"])) > 1
    info = e.prefix_cache_info()
    assert info["lookups"] == 2 and info["hit_tokens"] == 192


# ---------------------------------------------------------------------------------------------------- 2. tail rows

@pytest.mark.parametrize("dtype", DTYPES)
def test_image_rows_behind_the_hit_come_from_the_retained_tail(engines, dtype):
    e = _hot(engines, dtype)
    cfg = e.cfg
    a, image = _prompt(cfg, L_A, pads=(60, 76), grid=(1, 8, 8))
    a2 = _tail(cfg, a, 100)
    _seed(e, a, KEY_A, image)
    e.set_row_logprobs(5, 5)
    _fill(e, 5, a2, KEY_A, None, expect=(64, False))                         # positions 64 .. 75 are embedded from the retained rows
    _assert_same_state(_state(e, 5, len(a2)), _cold(engines, dtype, a2, image), f"{dtype}: tail rows")


# ---------------------------------------------------------------------------------------------------- 3. exact repeat, then L = 256

@pytest.mark.parametrize("dtype", DTYPES)
def test_exact_repeat_and_a_prompt_of_whole_pages(engines, dtype):
    e = _hot(engines, dtype)
    cfg = e.cfg
    for L in (L_A, 256):
        ids, image = _prompt(cfg, L, seed=L)
        _seed(e, ids, KEY_A if L == L_A else KEY_B, image)
        e.set_row_logprobs(5, 5)
        _fill(e, 5, ids, KEY_A if L == L_A else KEY_B, None, expect=(192, False))          # at 256 too: one position is always computed
        _assert_same_state(_state(e, 5, L), _cold(engines, dtype, ids, image), f"{dtype}: exact repeat at L = {L}")
        e.slot_release(5)
    assert e.prefix_cache_info()["resident"] == 3 + 4


# ---------------------------------------------------------------------------------------------------- 4. the key decides

@pytest.mark.parametrize("dtype", DTYPES)
def test_the_key_decides(engines, dtype):
    e = _hot(engines, dtype)
    cfg = e.cfg
    a, image = _prompt(cfg, L_A)
    other = (_pixels(16, 6, cfg), image[1])
    _seed(e, a, KEY_A, image)
    e.set_row_logprobs(5, 5)
    _fill(e, 5, a, KEY_B, other, expect=(0, True))                           # the same ids, other pixels under another key: a miss
    want = _cold(engines, dtype, a, other)
    _assert_same_state(_state(e, 5, L_A), want, f"{dtype}: other pixels under another key")
    assert not _same(want["logits"], _cold(engines, dtype, a, image)["logits"])          # the pixels do matter
    e.slot_release(5)
    before = e.prefix_cache_info()
    assert before["inserted"] == 6
    e.set_row_logprobs(5, 5)
    _fill(e, 5, a, None, other, expect=(0, True))                            # no key: the prompt bypasses the cache
    _assert_same_state(_state(e, 5, L_A), want, f"{dtype}: no key")
    assert e.prefix_cache_info() == before                                   # neither looked up nor inserted


# ---------------------------------------------------------------------------------------------------- 5. a live source

@pytest.mark.parametrize("dtype", DTYPES)
def test_a_hit_on_the_pages_of_a_sequence_still_decoding(engines, dtype):
    e = _hot(engines, dtype)
    cfg = e.cfg
    a, image = _prompt(cfg, L_A)
    a2 = _tail(cfg, a, 200)
    n_a = 13                                                                 # A: its first token, 4 before the hit and 8 beside it
    for s in (2, 5):
        e.set_row_logprobs(s, 5)
    _fill(e, 2, a, KEY_A, image, max_new=n_a)
    e.slots_decode(4)
    pages = _kv(e, 2, 192)
    _fill(e, 5, a2, KEY_A, None, expect=(192, False))
    first = dict(logits=e.slot_logits(5), kv=_kv(e, 5, len(a2)))
    e.slots_decode(8)
    fin, lens = e.slots_poll()
    assert (fin[2], lens[2], fin[5], lens[5]) == (1, n_a, 1, N_GEN)
    want_a, want_a2 = _cold(engines, dtype, a, image, n_gen=n_a), _cold(engines, dtype, a2, image)
    assert e.slot_read(2, n_a).tolist() == want_a["tokens"] and all(_same(x, y) for x, y in zip(e.row_logprobs(2, n_a), want_a["lp"]))
    got = dict(first, tokens=e.slot_read(5, N_GEN).tolist(), lp=e.row_logprobs(5, N_GEN))
    _assert_same_state(got, want_a2, f"{dtype}: a hit beside its live source")
    assert all(_same(x, y) for x, y in zip(_kv(e, 2, 192), pages)), "the source's shared pages changed"


# ---------------------------------------------------------------------------------------------------- 6. eviction

def _pool_is_consistent(e, held):
    """free (which counts evictable pages) + the pages slots hold = the pool"""
    total, free = e.kv_pool_info()
    info = e.prefix_cache_info()
    assert free == total - held and 0 <= info["evictable"] <= free, (total, free, held, info)
    return info


@pytest.mark.parametrize("dtype", DTYPES)
def test_eviction_makes_room_and_spares_what_is_held(engines, dtype):
    e = _engine(dtype, kv_pool_tokens=16 * 64)
    try:
        cfg = e.cfg
        _start(e)
        e.prefix_cache_enable(True)
        live = _text(cfg, L_A, seed=40)
        _fill(e, 0, live, None, None, max_new=20)                            # a live sequence: 4 pages, 3 of them cached too
        e.slots_decode(2)
        live_kv = _kv(e, 0, L_A)
        olds = [_text(cfg, L_A, seed=41 + i) for i in range(3)]
        for p in olds:
            _seed(e, p, None, None)
            _pool_is_consistent(e, 4)
        info = _pool_is_consistent(e, 4)
        assert (info["resident"], info["evictable"], info["evicted"]) == (12, 9, 0)          # 3 pages are on the free list
        big = _text(cfg, 500, seed=50)
        _fill(e, 1, big, None, None, expect=(0, False))                      # 8 pages: 5 cached pages have to go
        info = _pool_is_consistent(e, 12)
        assert info["evicted"] == 5 and info["evictable"] == 4
        assert all(_same(x, y) for x, y in zip(_kv(e, 0, L_A), live_kv)), "a page of the live sequence was evicted"
        e.slot_release(1)
        _pool_is_consistent(e, 4)
        e.set_row_logprobs(2, 5)
        _fill(e, 2, olds[0], None, None, expect=(0, False))                  # the oldest went first: a miss now
        _assert_same_state(_state(e, 2, L_A), _cold(engines, dtype, olds[0], None), f"{dtype}: the evicted prompt, filled again")
        assert all(_same(x, y) for x, y in zip(_kv(e, 0, L_A), live_kv))
        e.slots_decode(4)                                                    # the live sequence decodes on over its cached pages
        assert e.slots_poll()[1][0] == 1 + 2 + N_GEN - 1 + 4
    finally:
        e.close()


# ---------------------------------------------------------------------------------------------------- 7. the lease holds

@pytest.mark.parametrize("dtype", DTYPES)
def test_a_lease_keeps_its_pages_under_pressure(engines, dtype):
    e = _engine(dtype, kv_pool_tokens=12 * 64)
    try:
        cfg = e.cfg
        _start(e)
        e.prefix_cache_enable(True)
        a, image = _prompt(cfg, L_A)
        a2 = _tail(cfg, a, 200)
        _seed(e, a, KEY_A, image)
        lease = e.prefix_cache_lookup(a2, KEY_A)
        assert lease[1:] == (192, False) and lease[0] > 0
        for seed in (60, 61):
            _seed(e, _text(cfg, 300, seed=seed), None, None)                 # 4 cached pages each
        assert e.prefix_cache_info()["resident"] == 11 and e.prefix_cache_info()["evictable"] == 8
        _fill(e, 0, _text(cfg, 560, seed=62), None, None, max_new=8)         # 9 pages: the free one and everything evictable
        info = e.prefix_cache_info()
        assert info["evicted"] == 8 and info["evictable"] == 0 and e.kv_pool_info()[1] == 0
        e.slot_release(0)
        e.set_row_logprobs(5, 5)
        _fill(e, 5, a2, KEY_A, None, lease=lease)                            # the leased pages are still there
        _assert_same_state(_state(e, 5, len(a2)), _cold(engines, dtype, a2, image), f"{dtype}: a begin with a lease taken before the pressure")
        e.slot_release(5)
        with pytest.raises(DotsEngineError) as ei:
            e.prefix_cache_release(lease[0])                                 # consumed by the begin
        assert ei.value.code == E_INVALID
        evictable = e.prefix_cache_info()["evictable"]
        again = e.prefix_cache_lookup(a2, KEY_A)
        assert again[1:] == (192, False) and e.prefix_cache_info()["evictable"] == evictable - 3
        e.prefix_cache_release(again[0])
        assert e.prefix_cache_info()["evictable"] == evictable               # a released lease makes the pages evictable again
    finally:
        e.close()


# ---------------------------------------------------------------------------------------------------- 8. neighbours

@pytest.mark.parametrize("dtype", DTYPES)
def test_a_fork_of_a_hit_filled_slot(engines, dtype):
    e = _hot(engines, dtype)
    cfg = e.cfg
    a, image = _prompt(cfg, L_A)
    a2 = _tail(cfg, a, 200)
    pens = [SamplingParams(temperature=0.8, top_p=0.95, seed=31 + i, repetition_penalty=1.3, frequency_penalty=0.5) for i in range(3)]
    _seed(e, a, KEY_A, image, s=6)
    for s in range(3):
        e.set_row_sampling(s, pens[s])
        e.set_row_logprobs(s, 3)
    _fill(e, 0, a2, KEY_A, None, max_new=24, expect=(192, False))
    e.slots_fork(0, [1, 2])
    e.slots_decode(23)
    forked = _read_all(e, [0, 1, 2])
    c = engines[dtype, "cold"]
    alone = []
    for s in range(3):                                                       # independent requests: the prompt filled cold into each slot under its settings
        _start(c)
        c.set_row_sampling(s, pens[s])
        c.set_row_logprobs(s, 3)
        c.vit_forward(*image)
        c.slots_prefill_chunked([s], a2, [len(a2)], [24], 64)
        c.slots_decode(23)
        alone += _read_all(c, [s])
    _start(c)                                                                # no row keeps its parameters
    _start(e)
    assert _same_runs(forked, alone), f"{dtype}: a child of a hit-filled slot is not the independent request"
    assert len({tuple(r[1]) for r in forked}) == 3


@pytest.mark.parametrize("dtype", DTYPES)
def test_suspend_and_resume_over_cached_pages(engines, dtype):
    e = _hot(engines, dtype)
    cfg = e.cfg
    a, image = _prompt(cfg, L_A)
    a2 = _tail(cfg, a, 200)
    _seed(e, a, KEY_A, image, s=6)
    e.kv_swap_reserve(8)
    try:
        e.set_row_logprobs(2, 5)
        _fill(e, 2, a2, KEY_A, None, max_new=12, expect=(192, False))
        e.slots_decode(3)
        resident = e.prefix_cache_info()["resident"]
        host_free = e.kv_swap_info()[1]
        e.slot_suspend(2)
        assert e.slots_poll()[0][2] == 2
        assert e.kv_swap_info()[1] == host_free - 1                          # only the ragged page of its own is parked: the cached pages stay
        assert e.prefix_cache_info()["resident"] == resident and e.prefix_cache_info()["evictable"] == 0
        e.slot_resume(2)
        e.slots_decode(8)
        got = _read_all(e, [2])
    finally:
        e.slots_reset()
        e.kv_swap_reserve(0)
    want = _cold(engines, dtype, a2, image, n_gen=12)
    assert got[0][0] == 1 and got[0][1] == want["tokens"] and all(_same(x, y) for x, y in zip(got[0][2], want["lp"]))


def test_release_of_a_filling_leased_slot_and_switching_off(engines):
    e = _hot(engines, "bf16")
    cfg = e.cfg
    a, image = _prompt(cfg, L_A)
    a2 = _tail(cfg, a, 200)
    total, free0 = e.kv_pool_info()
    assert total == free0
    _seed(e, a, KEY_A, image)
    assert e.kv_pool_info() == (total, total)                                # cached pages count as free
    lease, hit, tower = e.prefix_cache_lookup(a2, KEY_A)
    assert e.kv_pool_info()[1] == total - 3                                  # leased pages do not
    e.slots_prefill_begin_cached([4], a2, [len(a2)], [N_GEN], [lease], [KEY_A])
    assert e.slots_poll()[0][4] == 3 and e.kv_pool_info()[1] == total - 4    # three shared pages and one of its own
    with pytest.raises(DotsEngineError) as ei:
        e.prefix_cache_enable(False)                                         # not while anything fills
    assert ei.value.code == E_STATE
    e.slot_release(4)
    info = e.prefix_cache_info()
    assert e.kv_pool_info() == (total, total) and info["resident"] == 3 and info["evictable"] == 3
    other = e.prefix_cache_lookup(a2, KEY_A)
    with pytest.raises(DotsEngineError) as ei:                               # a lease is for the prompt it was taken for
        e.slots_prefill_begin_cached([4], _text(cfg, L_A, seed=9), [L_A], [N_GEN], [other[0]], [None])
    assert ei.value.code == E_INVALID and e.kv_pool_info()[1] == total - 3
    e.prefix_cache_release(other[0])                                         # a refused begin leaves the lease held
    assert e.kv_pool_info() == (total, total)
    with pytest.raises(DotsEngineError) as ei:
        e.set_speculation(3)                                                 # not beside the cache
    assert ei.value.code == E_STATE
    e.prefix_cache_enable(False)
    assert e.kv_pool_info() == (total, total)
    with pytest.raises(DotsEngineError) as ei:
        e.prefix_cache_info()
    assert ei.value.code == E_STATE
    e.vit_forward(*image)
    e.slots_prefill_chunked([0], a, [L_A], [N_GEN], 64)                      # the plain entry point, as ever
    e.slots_reset()
    assert e.kv_pool_info() == (total, total)
    e.prefix_cache_enable(True)                                              # as _hot leaves it


# ---------------------------------------------------------------------------------------------------- 9. nothing moves when off

CACHE_CALLS = ("prefix_cache_enable", "prefix_cache_lookup", "prefix_cache_release", "slots_prefill_begin_cached", "prefix_cache_info")


class CacheRecorder(Recorder):
    def __getattr__(self, name):
        if name in CACHE_CALLS:
            self.calls.append((name,))
        return super().__getattr__(name)


def test_nothing_moves_when_off(engines):
    """a chunking ContinuousBatcher without prefix_caching makes the engine calls it made on the commit before the feature: the list was
    recorded there (that commit's scheduler over this scenario; with no EOS every request runs to its cap, so the calls follow from the
    caps), and none of the cache's entry points is among them"""
    from dots_ocr_amd.scheduler import ContinuousBatcher, Request
    e = engines["bf16", "cold"]
    e.set_sampling(0.0, 1.0, 0)
    caps = [5, 12, 3, 9, 7, 12]
    reqs = [Request(_text(e.cfg, 70 + 29 * i, seed=i), max_new_tokens=c) for i, c in enumerate(caps)]
    rec = CacheRecorder(e)
    outs = ContinuousBatcher(rec, eos_ids=(), chunk=4, prefill_chunk=128).run(reqs)
    assert [len(o) for o in outs] == caps
    calls = [c[:2] + c[3:] if c[0] == "slots_prefill_begin" else c for c in rec.calls]          # (slots, lens, caps): without the token ids
    A, D = ("slots_prefill_advance", 128), ("slots_decode", 4)
    assert calls == [
        ("set_eos", ()), ("slots_reset",),
        ("slots_prefill_begin", (0, 1, 2, 3, 4, 5), (70, 99, 128, 157, 186, 215), (5, 12, 3, 9, 7, 12)),
        A, D, ("slot_release", 0), A, D, A, D, ("slot_release", 2), A, D, ("slot_release", 1), A, D, A, D, ("slot_release", 3),
        A, D, ("slot_release", 4), A, D, D, D, ("slot_release", 5)]


# ---------------------------------------------------------------------------------------------------- 10. through generate and the server

def test_generate_and_the_server_with_prefix_caching():
    """a page read again — by generate with the caller's key, by the server under another prompt — hits, and reads what an uncached run reads"""
    from fastapi.testclient import TestClient
    from dots_ocr_amd.config import DotsConfig
    from dots_ocr_amd.image_utils import PILimage_to_base64
    from dots_ocr_amd.modeling import DotsOcrHipForCausalLM
    from dots_ocr_amd.parser import DotsOCRParser
    from dots_ocr_amd.processing import DotsOcrProcessor
    from dots_ocr_amd.server import create_app
    from dots_ocr_amd.synthetic import synth_page
    from dots_ocr_amd.weights import random_state_dict
    cfg = DotsConfig.tiny()
    model = DotsOcrHipForCausalLM(cfg, random_state_dict(cfg, seed=11), device=0, max_batch=3, max_seq_len=1024, max_patches=4096)
    try:
        proc = DotsOcrProcessor(cfg, engine=model.engine)
        page, n_new = synth_page(0, (280, 336)), 10
        prompts = ["Extract the text content from this image.", "Extract the text content from this image, then say so."]

        def direct(prompt, **kw):
            messages = [{"role": "user", "content": [{"type": "image", "image": page}, {"type": "text", "text": prompt}]}]
            text = proc.apply_chat_template(messages, tokenize=False, add_generation_prompt=True)
            inputs = proc(text=[text], images=[page], padding=True, return_tensors="pt").to("cuda")
            assert inputs.input_ids.shape[1] > 128
            out = model.generate(**inputs, max_new_tokens=n_new, prefill_chunk=64, **kw)
            return proc.batch_decode([out[0, inputs.input_ids.shape[1]:]], skip_special_tokens=True)[0]
        want = [direct(p) for p in prompts]
        key = DotsOCRParser._image_key(page)
        assert len(key) == 16 and key != DotsOCRParser._image_key(synth_page(1, (280, 336)))
        got = [direct(p, enable_prefix_caching=True, image_keys=[key]) for p in prompts + prompts]
        assert got == want + want
        info = model.engine.prefix_cache_info()
        assert info["lookups"] == 4 and info["hit_tokens"] >= 3 * 64          # every call after the first began behind the image's pages
        model.engine.slots_reset()
        model.engine.prefix_cache_enable(False)
        app = create_app(model, proc, model_name="model", max_batch=3, max_wait_ms=20, prefill_chunk=64, prefix_caching=True)
        usage = []
        with TestClient(app) as c:
            for p in prompts + prompts[:1]:
                body = {"model": "model", "messages": [{"role": "user", "content": [
                    {"type": "image_url", "image_url": {"url": PILimage_to_base64(page)}},
                    {"type": "text", "text": f"<|img|><|imgpad|><|endofimg|>{p}"}]}],
                    "max_completion_tokens": n_new, "temperature": 0.0, "top_p": 1.0}
                r = c.post("/v1/chat/completions", json=body)
                assert r.status_code == 200, r.text
                assert r.json()["choices"][0]["message"]["content"] == want[prompts.index(p)]
                usage.append(r.json()["usage"])
        cached = [u["prompt_tokens_details"]["cached_tokens"] for u in usage]
        assert cached[0] == 0 and cached[1] >= 64 and cached[2] == 64 * ((usage[2]["prompt_tokens"] - 1) // 64)
    finally:
        model.engine.close()
