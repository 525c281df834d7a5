"""Prefix caching without a GPU.

1. The block index (csrc/prefix_cache.h) driven by tests/prefix_cache_model.cpp, a stand-alone program built here with the host compiler —
   once plainly and once with -fsanitize=address,undefined (it has its own main: nothing is preloaded).
2. The scheduler's policy over a fake engine with a prefix cache: hits skip the tower and count no patches, a mixed group packs only the
   misses' pixels, every failure path gives its leases back, and with prefix_caching off the calls are the parent's.
3. The constructor's and the server's refusals, the server's image key and `cached_tokens` in the usage object.
4. The C ABI exports the entry points.
"""
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from dots_ocr_amd.scheduler import ContinuousBatcher, Request
from test_chunked_prefill_cpu import ChunkEngine, _steps

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "dots_ocr_amd" / "csrc"
IMG = 7                                                                      # the fake's image token
KEY_A, KEY_B = bytes(range(16)), bytes(range(16, 32))


# ---------------------------------------------------------------------------------------------------- 1. the block index

@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitized"])
def test_block_index_model(tmp_path, flags):
    cxx = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    assert cxx, "no C++ compiler (c++, g++ or clang++) on PATH"
    exe = tmp_path / "prefix_cache_model"
    p = subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", *flags, f"-I{CSRC}", str(ROOT / "tests" / "prefix_cache_model.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert int(re.search(r"(\d+) checks", p.stdout).group(1)) > 2000, p.stdout


def test_the_index_is_host_code():
    """no HIP, no engine type: it compiles and is tested on a CPU"""
    src = (CSRC / "prefix_cache.h").read_text()
    code = "\n".join(ln.split("//")[0] for ln in src.splitlines())
    assert "hip" not in code.lower() and "DotsEngine" not in code and '#include "' not in code


# ---------------------------------------------------------------------------------------------------- 2. the scheduler

class CacheEngine(ChunkEngine):
    """ChunkEngine + the prefix cache's surface.  A block is (the ids up to its end, the key if a pad lies in it or before it); blocks enter
    when the pass that completed them ran; a lookup's lease is remembered until a begin consumes it or a release returns it.  The fake
    keeps no tail rows: the tower is needed whenever a pad lies at or behind the hit.  fail_begin: the next begin raises."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.cache_on, self.blocks, self.leases, self.next_lease, self.fail_begin = False, set(), {}, 0, False
        self.cached = {}                                                     # filling slot -> (ids, key) of a fill that inserts
        self.image_token = IMG

    def prefix_cache_enable(self, on=True):
        assert not self.slots and not self.fills
        self.cache_on = bool(on)
        if not on:
            self.blocks.clear()
        self.log.append(("cache", bool(on)))

    def _block(self, ids, key, b):
        pads = np.nonzero(ids[:64 * (b + 1)] == self.image_token)[0]
        return (tuple(int(t) for t in ids[:64 * (b + 1)]), key if len(pads) else None)

    def prefix_cache_lookup(self, ids, key=None):
        assert self.cache_on
        ids = np.asarray(ids)
        pads = np.nonzero(ids == self.image_token)[0]
        if len(pads) and key is None:
            return 0, 0, True                                                # bypass
        hit = 0
        while hit < (len(ids) - 1) // 64 and self._block(ids, key, hit) in self.blocks:
            hit += 1
        tower = bool(len(pads)) and int(pads[-1]) >= 64 * hit
        lease = 0
        if hit:
            self.next_lease += 1
            lease = self.next_lease
            self.leases[lease] = (hit, tuple(int(t) for t in ids))
        self.log.append(("lookup", lease, 64 * hit, tower))
        return lease, 64 * hit, tower

    def prefix_cache_release(self, lease):
        del self.leases[lease]                                               # KeyError: released twice, or never held
        self.log.append(("unlease", lease))

    def slots_prefill_begin_cached(self, slots, ids, lens, caps, leases, keys):
        assert self.cache_on and len(slots) == len(leases) == len(keys)
        if self.fail_begin:
            self.fail_begin = False
            raise RuntimeError("begin failed")
        off, hits = 0, []
        for n, lease in zip(lens, leases):
            hit = 0
            if lease:
                hit, want = self.leases[lease]
                assert want == tuple(int(t) for t in ids[off:off + n]), "a lease is for the prompt it was taken for"
            hits.append(hit)
            off += n
        need = [self._need(n, c) - h for n, c, h in zip(lens, caps, hits)]
        if sum(need) > self.free:
            raise RuntimeError("KV pool exhausted")
        off = 0
        for s, n, c, p, h, lease, key in zip(slots, lens, caps, need, hits, leases, keys):
            assert 0 <= s < self.max_batch and s not in self.slots and s not in self.fills
            self.order += 1
            prompt = np.asarray(ids[off:off + n]).copy()
            self.fills[s] = dict(prompt=prompt, cap=int(c), cursor=64 * h, pages=p, order=self.order)
            self.cached[s] = (prompt, key)
            self.free -= p
            self.leases.pop(lease, None)
            off += n
        self.log.append(("begin_cached", tuple(slots), tuple(64 * h for h in hits)))

    def slots_prefill_advance(self, n):
        before = {s: f["cursor"] for s, f in self.fills.items()}
        prompts = {s: f["prompt"] for s, f in self.fills.items()}
        left = super().slots_prefill_advance(n)
        for s, c0 in before.items():
            c1 = self.fills[s]["cursor"] if s in self.fills else len(prompts[s])
            if s in self.cached and not (len(np.nonzero(prompts[s] == self.image_token)[0]) and self.cached[s][1] is None):
                for b in range(c0 // 64, c1 // 64):
                    self.blocks.add(self._block(prompts[s], self.cached[s][1], b))
            if s not in self.fills:
                self.cached.pop(s, None)
        return left


def _engine(pool_pages=40, **kw):
    args = dict(max_batch=4, max_patches=100, max_prefill_tokens=128, max_seq_len=640)
    args.update(kw)
    return CacheEngine(lambda prompt: [1 + int(prompt[0]) % 7] * 1000, pool_pages, **args)


def _req(L=200, cap=6, first=0, image=None, key=None, tail=3, **kw):
    """image: (first pad, grid h, grid w) — h * w / 4 pads from there; tail: the id the prompt is filled with from position 150 on"""
    ids = np.full(L, 3, np.int32)
    ids[0] = first
    ids[150:] = tail
    pv = grid = None
    if image is not None:
        p0, h, w = image
        ids[p0:p0 + h * w // 4] = IMG
        pv, grid = np.zeros((h * w, 4), np.float32), np.array([[1, h, w]], np.int64)
    return Request(ids, pv, grid, max_new_tokens=cap, image_key=key, **kw)


def _batcher(e, **kw):
    args = dict(chunk=4, prefill_chunk=64, headroom_pages=0, prefix_caching=True)
    args.update(kw)
    return ContinuousBatcher(e, **args)


def _events(steps, *kinds):
    return [ev for st in steps for ev in st if ev[0] in kinds]


def test_a_hit_skips_the_tower_and_counts_no_patches():
    e = _engine(max_patches=64)                                              # ONE 8 x 8 image fits the tower's workspace
    cb = _batcher(e)
    first = cb.submit(_req(image=(5, 8, 8), key=KEY_A, first=1))
    done, steps = _steps(cb, e)
    assert done[first] == [2] * 6 and _events(steps, "vit") == [("vit", 64, 64)] and cb.prefix_hits == 0
    # the same page under two other prompts, together: neither sends pixels, so both fit one group although two towers would not
    a, b = cb.submit(_req(image=(5, 8, 8), key=KEY_A, first=1, tail=4)), cb.submit(_req(image=(5, 8, 8), key=KEY_A, first=1, tail=5))
    done, steps = _steps(cb, e)
    assert done[a] == done[b] == [2] * 6
    assert _events(steps, "vit", "prefetch") == []
    assert _events(steps, "begin_cached") == [("begin_cached", (0, 1), (128, 128))]
    assert cb.prefix_hits == 2 and cb.prefix_hit_tokens == 256
    assert e.leases == {} and e.kv_pool_info() == (40, 40)


def test_a_mixed_group_packs_only_the_misses_pixels():
    e = _engine()
    cb = _batcher(e)
    cb.submit(_req(image=(5, 4, 4), key=KEY_A, first=1))
    _steps(cb, e)
    hit, miss, text = _req(image=(5, 4, 4), key=KEY_A, first=1, tail=4), _req(image=(5, 4, 8), key=KEY_B, first=2), _req(first=1, tail=9)
    ids = [cb.submit(r) for r in (hit, miss, text)]
    done, steps = _steps(cb, e)
    assert sorted(done) == sorted(ids)
    assert _events(steps, "vit") == [("vit", 32, 32)]                        # the 4 x 8 image alone
    assert _events(steps, "begin_cached") == [("begin_cached", (0, 1, 2), (128, 0, 0))]
    assert (hit.cached_tokens, miss.cached_tokens, text.cached_tokens) == (128, 0, 0)
    # other pixels under another key miss although the ids are equal; an image without a key is not even looked up
    other, bare = _req(image=(5, 4, 4), key=KEY_B, first=1), _req(image=(5, 4, 4), key=None, first=1)
    for r in (other, bare):
        cb.submit(r)
    _, steps = _steps(cb, e)
    assert [ev[1:] for ev in _events(steps, "lookup")] == [(0, 0, True)] and len(_events(steps, "vit")) == 1
    assert other.cached_tokens == bare.cached_tokens == 0


def test_leases_are_released_on_every_failure_path():
    # 1. the begin fails: the group returns to the queue, its leases to the engine
    e = _engine()
    cb = _batcher(e)
    cb.submit(_req(first=1))
    _steps(cb, e)
    r = cb.submit(_req(first=1, tail=4))
    e.fail_begin = True
    with pytest.raises(RuntimeError, match="begin failed"):
        cb.step()
    assert e.leases == {} and cb._leases == {} and [rid for rid, _ in cb.pending] == [r]
    done, _ = _steps(cb, e)                                                  # the retry looks up again and hits
    assert done[r] == [2] * 6 and cb.prefix_hits == 1 and e.leases == {}
    # 2. the pool cannot take the request yet: it waits without a lease
    e = _engine(pool_pages=9)
    cb = _batcher(e)
    cb.submit(_req(first=1, cap=200))
    cb.step()                                                                # 200 + 64 positions: 5 pages; its first page is filled and cached
    waiting = cb.submit(_req(L=400, first=1, cap=200))                       # 8 pages less what it hits: not beside it
    for _ in range(3):
        cb.step()
        assert [rid for rid, _ in cb.pending] == [waiting] and e.leases == {} and cb._leases == {}
    looked = [ev for ev in e.log if ev[0] == "lookup" and ev[1]]
    assert len(looked) == 3 and [ev[1] for ev in e.log if ev[0] == "unlease"] == [ev[1] for ev in looked]      # taken, and given back, step by step
    # 3. the engine refuses a request's own parameters: rejected alone, its lease returned
    e = _engine()

    def refuse_logprobs(slot, top_n):
        if top_n is not None:
            raise ValueError("no logprobs here")
    e.set_row_logprobs = refuse_logprobs
    cb = _batcher(e)
    cb.submit(_req(first=1))
    _steps(cb, e)
    bad, good = _req(first=1, tail=4, logprobs=3), _req(first=1, tail=5)
    cb.submit(bad), cb.submit(good)
    out = cb.step()
    assert [r is bad for _, r, _ in out] == [True] and bad.error is not None
    assert e.leases == {} and cb._leases == {}
    _steps(cb, e)
    assert good.cached_tokens == 128 and e.leases == {}
    # 4. the look-ahead: a hit that needs no tower is not prefetched and keeps no lease while it waits for the ordinary admission
    e = _engine()
    cb = _batcher(e, prefetch=2)
    cb.submit(_req(image=(5, 4, 4), key=KEY_A, first=1))
    _steps(cb, e)
    for i in range(4):
        cb.submit(_req(L=70, first=2 + i, cap=12))                           # every slot is taken ...
    hit = _req(image=(5, 4, 4), key=KEY_A, first=1, tail=4)
    again = cb.submit(hit)                                                   # ... so the look-ahead meets the hit at the head of the queue
    done, steps = {}, []
    while not cb.idle:
        mark = len(e.log)
        for rid, _, toks in cb.step():
            done[rid] = toks.tolist()
        steps.append(e.log[mark:])
        assert e.leases == {} and cb._leases == {}                           # between steps nothing is pinned for it
    assert done[again] == [2] * 6 and _events(steps, "prefetch", "vit", "take") == [] and hit.cached_tokens == 128
    assert len([ev for ev in _events(steps, "lookup") if ev[1]]) >= 2        # the look-ahead asked, then the admission


def test_constructor_refusals():
    with pytest.raises(ValueError, match="prefill_chunk"):
        ContinuousBatcher(_engine(), prefix_caching=True)
    with pytest.raises(ValueError, match="prefix_cache_lookup"):
        ContinuousBatcher(ChunkEngine(lambda p: [1] * 10, 12, max_prefill_tokens=128), prefill_chunk=64, prefix_caching=True)
    spec = _engine()
    spec.spec_k = 2
    with pytest.raises(ValueError, match="speculating"):
        ContinuousBatcher(spec, prefill_chunk=64, prefix_caching=True)
    from dots_ocr_amd.parser import DotsOCRParser
    with pytest.raises(ValueError, match="prefill_chunk"):
        DotsOCRParser(enable_prefix_caching=True)                            # the callers' switches ask for the same
    assert DotsOCRParser(prefill_chunk=64, enable_prefix_caching=True)._chunk_kw() == {"prefill_chunk": 64, "prefix_caching": True}
    assert DotsOCRParser(prefill_chunk=64)._chunk_kw() == {"prefill_chunk": 64} and DotsOCRParser()._chunk_kw() == {}
    e = _engine()
    assert not ContinuousBatcher(e, prefill_chunk=64, prefix_caching=False).prefix_caching and ("cache", True) not in e.log
    assert ContinuousBatcher(e, prefill_chunk=64, prefix_caching=True).prefix_caching and e.log[-1] == ("cache", True)


def test_nothing_moves_when_off():
    """prefix_caching=None: the engine's log is the one the parent commit's scheduler left over this scenario (recorded there), and none of
    the cache's calls is in it"""
    e = _engine(max_prefill_tokens=512)
    cb = ContinuousBatcher(e, chunk=4, headroom_pages=0, prefill_chunk=128, prefix_caching=None)
    reqs = [_req(60, 6, first=1), _req(300, 11, first=2, image=(5, 4, 4), key=KEY_A), _req(100, 3, first=3), _req(90, 7, first=4), _req(70, 5, first=5)]
    ids = [cb.submit(r) for r in reqs]
    done, steps = _steps(cb, e)
    assert done == {i: [2 + k] * r.max_new_tokens for k, (i, r) in enumerate(zip(ids, reqs))}
    assert [ev for st in steps for ev in st] == PARENT_LOG
    assert not hasattr(reqs[0], "cached_tokens") and cb.prefix_hits == 0


PARENT_LOG = [("vit", 16, 16), ("begin", (0, 1, 2, 3)), ("advance", 128, ((0, 60), (1, 64))), ("decode", 4, (0,)), ("advance", 128, ((1, 128),)),
              ("decode", 4, (0,)), ("begin", (0,)), ("advance", 128, ((1, 108),)), ("decode", 4, (1,)), ("advance", 128, ((2, 100),)),
              ("decode", 4, (1, 2)), ("advance", 128, ((3, 90),)), ("decode", 4, (1, 3)), ("advance", 128, ((0, 70),)), ("decode", 4, (0, 3))]


# ---------------------------------------------------------------------------------------------------- 3. the server

def test_server_flag_validation():
    from dots_ocr_amd.server import build_arg_parser, chunked_prefill_args, main, prefix_caching_args
    ap_ = build_arg_parser()
    assert prefix_caching_args(ap_.parse_args([])) is False                  # the default: today's behaviour
    assert prefix_caching_args(ap_.parse_args(["--enable-chunked-prefill"])) is False
    assert prefix_caching_args(ap_.parse_args(["--enable-chunked-prefill", "--enable-prefix-caching"])) is True
    with pytest.raises(ValueError, match="--enable-chunked-prefill"):
        prefix_caching_args(ap_.parse_args(["--enable-prefix-caching"]))
    for with_ in ("--static-batching", ["--speculative-ngram", "2"]):       # and so with static batching and speculation
        argv = ["--enable-prefix-caching", "--enable-chunked-prefill"] + ([with_] if isinstance(with_, str) else with_)
        with pytest.raises(ValueError):
            chunked_prefill_args(ap_.parse_args(argv))
        with pytest.raises(SystemExit):                                      # refused at server start, before anything is loaded
            main(argv)
    with pytest.raises(SystemExit):
        main(["--enable-prefix-caching"])


def test_cached_tokens_and_the_image_key_through_the_server():
    import base64
    import io
    from fastapi.testclient import TestClient
    from dots_ocr_amd.config import DotsConfig
    from dots_ocr_amd.processing import DotsOcrProcessor
    from dots_ocr_amd.server import ContinuousWorker, _image_source, create_app
    from dots_ocr_amd.synthetic import synth_page
    from test_server_cpu import _payload
    cfg = DotsConfig.tiny()
    proc = DotsOcrProcessor(cfg)

    class Model:
        config = cfg

    model = Model()
    model.engine = CacheEngine(lambda prompt: proc.tokenizer.encode("ok") + [cfg.eos_token_ids[0]], 400, max_batch=3, max_patches=4096,
                               max_prefill_tokens=4096, max_seq_len=2048)
    with pytest.raises(ValueError, match="prefill_chunk"):
        create_app(model, proc, model_name="model", max_batch=3, prefix_caching=True)
    with pytest.raises(ValueError, match="continuous"):
        create_app(model, proc, model_name="model", max_batch=3, continuous=False, prefill_chunk=64, prefix_caching=True)
    model.engine.image_token = cfg.image_token_id
    app = create_app(model, proc, model_name="model", max_batch=3, prefill_chunk=64, prefix_caching=True, look_ahead=0)
    with TestClient(app) as c:
        assert isinstance(app.state.worker, ContinuousWorker) and app.state.worker._chunk_kw() == {"prefill_chunk": 64, "prefix_caching": True}
        page = synth_page(0, (224, 168))
        usage = []
        for _ in range(2):                                               # the same page posted twice
            r = c.post("/v1/chat/completions", json=_payload(page))
            assert r.status_code == 200, r.text
            assert r.json()["choices"][0]["message"]["content"] == "ok"
            usage.append(r.json()["usage"])
        r = c.post("/v1/chat/completions", json=_payload(synth_page(1, (224, 168))))      # another page of the same size: other bytes, another key
        usage.append(r.json()["usage"])
    assert usage[0]["prompt_tokens_details"] == {"cached_tokens": 0}
    hit = usage[1]["prompt_tokens_details"]["cached_tokens"]
    assert hit == 64 * ((usage[1]["prompt_tokens"] - 1) // 64) > 0
    assert usage[2]["prompt_tokens"] == usage[0]["prompt_tokens"] and usage[2]["prompt_tokens_details"]["cached_tokens"] < hit
    assert len([ev for ev in model.engine.log if ev[0] == "vit"]) == 2   # the repeat ran no tower
    # off: no field, no key, nothing new handed to the batcher
    app = create_app(model, proc, model_name="model", max_batch=3, prefill_chunk=64)
    assert app.state.worker._chunk_kw() == {"prefill_chunk": 64}
    with TestClient(app) as c:
        r = c.post("/v1/chat/completions", json=_payload(page))
        assert r.status_code == 200 and "prompt_tokens_details" not in r.json()["usage"]
    # the key is taken over what was received inline; a URL names bytes that may change behind it
    buf = io.BytesIO()
    synth_page(0, (56, 56)).save(buf, format="PNG")
    url = "data:image/png;base64," + base64.b64encode(buf.getvalue()).decode()
    msg = lambda u: [{"role": "user", "content": [{"type": "image_url", "image_url": {"url": u}}, {"type": "text", "text": "x"}]}]
    assert _image_source(msg(url)) == url.encode() and _image_source(msg("https://example.invalid/a.png")) is None
    assert _image_source([{"role": "user", "content": "no image"}]) is None


# ---------------------------------------------------------------------------------------------------- 4. the C ABI

def test_the_library_exports_the_entry_points():
    from dots_ocr_amd import _lib, build, engine
    build.build(verbose=False)
    lib = _lib.load()
    header = (ROOT / "include" / "dots_ocr_hip.h").read_text()
    for sym in ("dots_prefix_cache_enable", "dots_prefix_cache_lookup", "dots_prefix_cache_release", "dots_slots_prefill_begin_cached",
                "dots_prefix_cache_info"):
        assert hasattr(lib, sym) and sym in engine.EXPORTED_SYMBOLS and re.search(r"^int " + sym + r"\(", header, re.M), sym
    for method in ("prefix_cache_enable", "prefix_cache_lookup", "prefix_cache_release", "slots_prefill_begin_cached", "prefix_cache_info"):
        assert callable(getattr(engine.Engine, method))
