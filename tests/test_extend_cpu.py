"""Several prompts over one page without a GPU: the scheduler's Request(suffixes=...) over a fake paged engine that forks
and extends, the server's `prompts` field, the parser's parse_image_regions, the Python binding's packing and the C-ABI symbol."""
import ctypes as C
import json
import re
import types
from pathlib import Path

import numpy as np
import pytest

from dots_ocr_amd.config import DotsConfig
from dots_ocr_amd.engine import SamplingParams
from fakes import FakePagedEngine

ROOT = Path(__file__).resolve().parent.parent
EOS = 9


class ExtendEngine(FakePagedEngine):
    """FakePagedEngine + per-row parameters + slots_fork / slots_extend as the engine defines them.  A fork child shares the source's
    floor(L / 64) full prompt pages; an extend appends ids behind the slot's prompt, grows the slot to the admission reserve of the longer
    prompt and restarts its output.  `script` may read self.cur / self.rows: the slot it is asked about."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.rows, self.cur, self.fresh, self.groups, self.spec_k = {}, None, set(), {}, 0

    def set_row_sampling(self, row, params):
        if params is None:
            self.rows.pop(row, None)
        else:
            self.rows[row] = params

    def _admit(self, prompt, cap):
        return (min(prompt + min(cap, 64), self.max_seq_len) + 63) // 64

    def _restart(self, s):
        st = self.slots[s]
        self.cur = s
        st.update(plan=list(self.script(st["prompt"])), out=[], done=False)
        self._advance(st)

    def slots_reset(self):
        super().slots_reset()
        self.fresh, self.groups = set(), {}

    def slots_prefill(self, slots, ids, lens, caps):
        super().slots_prefill(slots, ids, lens, caps)
        for s in slots:
            self._restart(s)
        self.fresh = set(slots)

    def slots_decode(self, n):
        self.fresh = set()
        super().slots_decode(n)

    def slots_fork(self, src, dst):
        assert src in self.fresh and src in self.slots, "only a freshly prefilled sequence can be forked"
        assert len(set(dst)) == len(dst) and all(0 <= d < self.max_batch and d not in self.slots for d in dst)
        p = self.slots[src]
        L, shared = len(p["prompt"]), len(p["prompt"]) // 64
        own = self._admit(L, p["limit"] - L) - shared
        if own * len(dst) > self.free:
            raise RuntimeError("KV pool exhausted")
        key = p.setdefault("group", ("group", src, len(self.log)))
        self.groups[key] = self.groups.get(key, 1) + len(dst)
        for d in dst:
            self.slots[d] = dict(prompt=p["prompt"].copy(), cap=p["limit"] - L, pages=shared + own, limit=p["limit"], ctx=L, group=key, shared=shared)
            self.free -= own
            self._restart(d)
        p["shared"] = shared
        self.log.append(("fork", src, tuple(dst)))

    def slots_extend(self, slots, ids_list, keep_pending=False, max_new_tokens=1):
        assert not keep_pending
        assert len(set(slots)) == len(slots) == len(ids_list) and all(s in self.slots for s in slots) and all(len(x) >= 1 for x in ids_list)
        lacking = [max(0, self._admit(len(self.slots[s]["prompt"]) + len(x), max_new_tokens) - self.slots[s]["pages"]) for s, x in zip(slots, ids_list)]
        if sum(lacking) > self.free:
            raise RuntimeError("KV pool exhausted")
        for s, x, more in zip(slots, ids_list, lacking):
            st = self.slots[s]
            st["prompt"] = np.concatenate([st["prompt"], np.asarray(x, st["prompt"].dtype)])
            st.update(pages=st["pages"] + more, cap=int(max_new_tokens), limit=len(st["prompt"]) + int(max_new_tokens), ctx=len(st["prompt"]))
            self.free -= more
            self._restart(s)
        self.fresh = set()
        self.log.append(("extend", tuple(slots), tuple(len(x) for x in ids_list), tuple(self.rows.get(s) for s in slots)))

    def slot_release(self, s):
        st = self.slots[s]
        key = st.get("group")
        if key is not None:
            self.groups[key] -= 1
            if self.groups[key] > 0:
                self.free -= st["shared"]            # other rows still hold the shared pages: they stay out of the pool
        self.rows.pop(s, None)
        super().slot_release(s)


def _seq(prompt, seed):
    """what a sequence generates: its prompt's last id and length and its seed, 2 + seed % 3 times, then the EOS"""
    return [int(prompt[-1]) * 1000 + len(prompt) * 10 + seed] * (2 + seed % 3) + [EOS]


def _engine(pool_pages=64, max_batch=8, cls=ExtendEngine, **kw):
    box = []

    def script(prompt):
        sp = getattr(box[0], "rows", {}).get(getattr(box[0], "cur", None))
        return _seq(prompt, 0 if sp is None else sp.seed)
    e = cls(script, pool_pages, max_batch=max_batch, max_prefill_tokens=1024, max_seq_len=1024, **kw)
    box.append(e)
    return e


def _req(first, L=70, cap=40, **kw):
    from dots_ocr_amd.scheduler import Request
    return Request(np.full(L, first, np.int32), max_new_tokens=cap, **kw)


# ---------------------------------------------------------------------------------------------------- scheduler

def test_suffixes_take_one_prefill_one_fork_one_extend_before_any_decode():
    from dots_ocr_amd.scheduler import ContinuousBatcher
    eng = _engine()
    sufs = [[11, 12, 13], [21], [31, 32, 33, 34, 35]]
    sp = SamplingParams(temperature=1.0, seed=4)
    r = _req(7, sampling=sp, suffixes=sufs)
    r.pixel_values, r.grid_thw = np.zeros((16, 4), np.float32), np.array([[1, 4, 4]], np.int64)
    other = _req(5, L=10)
    cb = ContinuousBatcher(eng, eos_ids=(EOS,), chunk=2)
    outs = cb.run([r, other])
    kinds = [ev[0] for ev in eng.log]
    first_decode = kinds.index("decode")
    assert kinds[:first_decode] == ["vit", "prefill", "fork", "extend"]                   # one of each, in that order, before any step
    assert kinds.count("vit") == 1 and kinds.count("fork") == 1 and kinds.count("extend") == 1
    assert eng.log[1] == ("prefill", (0, 3))                                               # the request's kids take slots 1 and 2
    assert eng.log[2] == ("fork", 0, (1, 2))
    ext = eng.log[3]
    assert ext[1] == (0, 1, 2) and ext[2] == (3, 1, 5)
    assert [p.seed for p in ext[3]] == [4, 5, 6]                                           # seed + i per sequence, as with n
    # outputs in suffix order: each spells ITS suffix's last id, the extended length and its seed
    assert [o.tolist() for o in r.outputs] == [_seq([13] * 73, 4), _seq([21] * 71, 5), _seq([35] * 75, 6)]
    assert outs[0].tolist() == r.outputs[0].tolist() and outs[1].tolist() == _seq([5] * 10, 0)
    assert r.kv_truncated_each == [False] * 3 and cb.admissions == 1
    assert eng.kv_pool_info() == (64, 64) and not eng.slots


def test_page_accounting_includes_the_suffixes():
    from dots_ocr_amd.scheduler import ContinuousBatcher
    # prefix 70 (one full page shared), cap 40: suffixes of 3 / 20 / 60 tokens end at 73 / 90 / 130 -> 2 / 3 / 3 pages, less 2 shared ones
    sufs = [[1] * 3, [2] * 20, [3] * 60]
    eng = _engine(pool_pages=6)
    cb = ContinuousBatcher(eng, eos_ids=(EOS,), chunk=2)
    r = _req(7, suffixes=sufs)
    cb.submit(r)
    assert cb._group_pages(r) == 2 + 3 + 3 - 2 == 6
    assert cb._worst_pages(r) == (113 + 63) // 64 + (130 + 63) // 64 + (170 + 63) // 64 - 2 == 6
    plain = _req(7)
    plain.input_ids = np.asarray(plain.input_ids, np.int32)
    assert cb._group_pages(plain) == 2                                                     # what the prefix alone would take
    cb.step()
    assert ("extend", (0, 1, 2), (3, 20, 60), (None, None, None)) in eng.log
    assert eng.kv_pool_info()[1] == 0 or not eng.slots                                     # all six pages were in use right after the admission
    while not cb.idle:
        cb.step()
    assert eng.kv_pool_info() == (6, 6)
    # a pool one page short of that never admits it
    eng5 = _engine(pool_pages=5)
    with pytest.raises(ValueError, match="KV pages"):
        ContinuousBatcher(eng5, eos_ids=(EOS,)).submit(_req(7, suffixes=sufs))
    # the cap leaves room for the longest suffix
    long = _req(7, L=900, cap=500, suffixes=[[1] * 100, [2]])
    ContinuousBatcher(_engine(), eos_ids=(EOS,)).submit(long)
    assert long.max_new_tokens == 1024 - 900 - 100


def test_suffix_refusals_are_raised_at_submit():
    from dots_ocr_amd.scheduler import ContinuousBatcher, RequestRejected
    eng = _engine()
    cb = ContinuousBatcher(eng, eos_ids=(EOS,))
    two = [[1], [2]]
    for kw, what in ((dict(suffixes=two, n=2), "n > 1"), (dict(suffixes=two, num_beams=2), "num_beams"),
                     (dict(suffixes=two, sampling=SamplingParams(repetition_penalty=1.2)), "penalty"),
                     (dict(suffixes=two, sampling=SamplingParams(presence_penalty=0.5)), "penalty"),
                     (dict(suffixes=[[1], []]), "empty"), (dict(suffixes=[[1]]), "2 .. 8"), (dict(suffixes=[[1]] * 9), "2 .. 8")):
        with pytest.raises(RequestRejected, match=what):
            cb.submit(_req(7, **kw))
    assert not cb.pending and not eng.log
    eng.spec_k = 2
    with pytest.raises(RequestRejected, match="speculates"):
        ContinuousBatcher(eng, eos_ids=(EOS,)).submit(_req(7, suffixes=two))
    eng.spec_k = 0
    static = _engine(cls=FakePagedEngine)                                                  # no slots_fork / slots_extend: static batching
    with pytest.raises(RequestRejected, match="static batching"):
        ContinuousBatcher(static, eos_ids=(EOS,)).submit(_req(7, suffixes=two))
    eng.cfg = types.SimpleNamespace(vocab_size=4000)
    with pytest.raises(RequestRejected, match="outside"):
        ContinuousBatcher(eng, eos_ids=(EOS,)).submit(_req(7, suffixes=[[1], [4000]]))
    cb.submit(_req(7, suffixes=two))                                                       # and the plain one goes in
    assert len(cb.pending) == 1


def test_common_prefix_split_never_leaves_an_empty_suffix():
    from dots_ocr_amd.scheduler import split_common_prefix
    assert split_common_prefix([[1, 2, 3, 4], [1, 2, 5]]) == ([1, 2], [[3, 4], [5]])
    assert split_common_prefix([[1, 2, 3], [1, 2, 3, 4, 5]]) == ([1, 2], [[3], [3, 4, 5]])       # one is a prefix of the other
    assert split_common_prefix([[1, 2, 3], [1, 2, 3]]) == ([1, 2], [[3], [3]])
    assert split_common_prefix([[7], [8, 9]]) == ([], [[7], [8, 9]])
    with pytest.raises(ValueError):
        split_common_prefix([[1], []])


# ---------------------------------------------------------------------------------------------------- binding and C ABI

def test_engine_slots_extend_packs_its_lists():
    from dots_ocr_amd import engine
    calls = []

    def fake(h, slots, n, ids, lens, keep, cap):
        tot = sum(lens[i] for i in range(n))
        calls.append(([slots[i] for i in range(n)], [ids[i] for i in range(tot)], [lens[i] for i in range(n)], [keep[i] for i in range(n)],
                      [cap[i] for i in range(n)]))
        return 0
    e = engine.Engine.__new__(engine.Engine)
    e.lib, e.h = types.SimpleNamespace(dots_slots_extend=fake), None
    e.slots_extend([4, 1], [[7, 8, 9], [5]], keep_pending=False, max_new_tokens=24)
    e.slots_extend([2, 0, 6], [[1], [2, 3], [4]], keep_pending=[True, False, True], max_new_tokens=[3, 4, 5])
    assert calls[0] == ([4, 1], [7, 8, 9, 5], [3, 1], [0, 0], [24, 24])
    assert calls[1] == ([2, 0, 6], [1, 2, 3, 4], [1, 2, 1], [1, 0, 1], [3, 4, 5])


def test_extend_symbols_are_exported_and_declared():
    from dots_ocr_amd import _lib, engine
    lib = _lib.load()
    engine._set_signatures(lib) if hasattr(engine, "_set_signatures") else None
    header = (ROOT / "include" / "dots_ocr_hip.h").read_text()
    for sym in ("dots_slots_extend", "dots_slot_logits"):
        assert sym in engine.EXPORTED_SYMBOLS and hasattr(lib, sym)
        assert re.search(rf"^int {sym}\(DotsEngine\* e,", header, re.M)
    assert "READ THE EARLIER OUTPUT FIRST" in header and "A fork comes before an extend" in header
    i32p = C.POINTER(C.c_int32)
    lib.dots_slots_extend.restype = C.c_int32
    lib.dots_slots_extend.argtypes = [C.c_void_p, i32p, C.c_int32, i32p, i32p, i32p, i32p]
    one = (C.c_int32 * 1)(0)
    assert lib.dots_slots_extend(None, one, 1, one, one, one, one) == -1                   # no engine: refused before anything is touched
    kernels = (ROOT / "dots_ocr_amd" / "csrc" / "kernels.h").read_text()
    src = (ROOT / "dots_ocr_amd" / "csrc" / "extend.hip").read_text()
    for k in ("extend_expand_kernel", "extend_commit_kernel"):
        assert k in src
    assert "launch_extend_expand" in kernels and "launch_extend_commit" in kernels


# ---------------------------------------------------------------------------------------------------- server

fastapi = pytest.importorskip("fastapi")


class _SlotModel:
    """a model object whose engine forks and extends: every sequence answers with the text of its own prompt"""

    def __init__(self, proc, cfg, cls=ExtendEngine):
        self.config = cfg

        def script(prompt):
            return [int(t) for t in prompt if t != cfg.image_token_id][-40:] + [cfg.eos_token_ids[0]]
        self.engine = cls(script, 4096, max_batch=8, max_patches=4096, max_prefill_tokens=4096, max_seq_len=2048)


def _payload(page, **kw):
    from dots_ocr_amd.image_utils import PILimage_to_base64
    body = {"model": "model", "messages": [{"role": "user", "content": [
        {"type": "image_url", "image_url": {"url": PILimage_to_base64(page)}},
        {"type": "text", "text": "<|img|><|imgpad|><|endofimg|>ignored when prompts are given"}]}],
        "max_completion_tokens": 128, "temperature": 0}
    body.update(kw)
    return body


def test_server_prompts_field():
    from fastapi.testclient import TestClient
    from dots_ocr_amd.processing import DotsOcrProcessor
    from dots_ocr_amd.server import create_app
    from dots_ocr_amd.synthetic import synth_page
    cfg = DotsConfig.tiny()
    proc = DotsOcrProcessor(cfg)
    model = _SlotModel(proc, cfg)
    page = synth_page(0, (140, 84))
    n_img = (84 // 14) * (140 // 14) // 4
    base = "Extract text from the given bounding box on the image (format: [x1, y1, x2, y2]).\nBounding Box:\n"
    prompts = [base + "[10, 20, 30, 40]", base + "[10, 20, 300, 400]", base + "[10, 20, 30, 40]", base + "[10, 20, 30"]
    with TestClient(create_app(model, proc, model_name="model", max_batch=8)) as c:
        r = c.post("/v1/chat/completions", json=_payload(page, prompts=prompts))
        assert r.status_code == 200, r.text
        d = r.json()
        assert [ch["index"] for ch in d["choices"]] == [0, 1, 2, 3]
        for ch, p in zip(d["choices"], prompts):                                           # choice i answers prompts[i]
            assert ch["message"]["content"].rstrip().endswith(p[-12:]) and ch["finish_reason"] == "stop"
        eng = model.engine
        kinds = [ev[0] for ev in eng.log if ev[0] in ("vit", "prefetch", "prefill", "fork", "extend")]
        assert kinds.count("prefill") == 1 and kinds.count("fork") == 1 and kinds.count("extend") == 1
        assert kinds.count("vit") + kinds.count("prefetch") == 1                           # the page went through the tower once
        ext = [ev for ev in eng.log if ev[0] == "extend"][0]
        assert all(n >= 1 for n in ext[2])                                                 # no empty suffix, although prompts[3] is a prefix of prompts[0]
        # usage: the prefix once plus every suffix
        ids = [proc(text=[proc.apply_chat_template([{"role": "user", "content": [{"type": "image", "image": page}, {"type": "text", "text": p}]}],
                                                   tokenize=False, add_generation_prompt=True)], images=[page])["input_ids"][0].tolist() for p in prompts]
        from dots_ocr_amd.scheduler import split_common_prefix
        prefix, sufs = split_common_prefix(ids)
        assert prefix.count(cfg.image_token_id) == n_img and tuple(len(s) for s in sufs) == ext[2]
        assert d["usage"]["prompt_tokens"] == len(prefix) + sum(len(s) for s in sufs)
        assert d["usage"]["completion_tokens"] == sum(len(s[-40:]) + 1 for s in ([t for t in i if t != cfg.image_token_id] for i in ids))
        # every conflicting field is a 400 that names it
        for kw, what in ((dict(n=2), "n"), (dict(use_beam_search=True, beam_width=2), "use_beam_search"),
                         (dict(repetition_penalty=1.3), "repetition_penalty"), (dict(presence_penalty=0.4), "presence_penalty"),
                         (dict(frequency_penalty=0.4), "frequency_penalty")):
            bad = c.post("/v1/chat/completions", json=_payload(page, prompts=prompts, **kw))
            assert bad.status_code == 400 and what in bad.json()["detail"], (kw, bad.text)
        for value in (["only one"], "a string", [""] * 2, ["x"] * 9):
            assert c.post("/v1/chat/completions", json=_payload(page, prompts=value)).status_code == 400
        no_image = {"messages": [{"role": "user", "content": "hi"}], "prompts": prompts[:2]}
        assert c.post("/v1/chat/completions", json=no_image).status_code == 400
        eng.spec_k = 2
        bad = c.post("/v1/chat/completions", json=_payload(page, prompts=prompts))
        assert bad.status_code == 400 and "--speculative-ngram" in bad.json()["detail"]
        eng.spec_k = 0
    with TestClient(create_app(model, proc, model_name="model", max_batch=8, continuous=False)) as c:
        bad = c.post("/v1/chat/completions", json=_payload(page, prompts=prompts))
        assert bad.status_code == 400 and "--static-batching" in bad.json()["detail"]


# ---------------------------------------------------------------------------------------------------- parser

def test_parse_image_regions_issues_one_request(tmp_path, monkeypatch):
    import dots_ocr.model.inference as inf
    from dots_ocr_amd.parser import DotsOCRParser
    from dots_ocr_amd.synthetic import synth_page
    page_path = tmp_path / "page.png"
    synth_page(0, (280, 168)).save(page_path)
    calls, singles = [], []

    def many(image, prompts, **kw):
        calls.append((image.size, list(prompts), kw))
        return [f"text of {p.splitlines()[-1]}" for p in prompts]

    def single(image, prompt, **kw):
        singles.append(prompt)
        return f"text of {prompt.splitlines()[-1]}"
    monkeypatch.setattr(inf, "inference_prompts_with_vllm", many)
    monkeypatch.setattr(inf, "inference_with_vllm", single)
    parser = DotsOCRParser(output_dir=str(tmp_path / "out"), stop=["\n\n"])
    boxes = [[10, 10, 100, 60], [20, 70, 200, 120], [5, 5, 50, 50]]
    (tmp_path / "ref").mkdir()
    results = parser.parse_image_regions(str(page_path), boxes)
    assert len(calls) == 1 and not singles                                                 # one request for the three boxes
    size, prompts, kw = calls[0]
    assert len(prompts) == 3 and len(set(prompts)) == 3 and kw["extra_body"] == {"stop": ["\n\n"]}
    assert len(results) == 3
    for i, (res, box) in enumerate(zip(results, boxes)):
        want = parser.parse_image(str(page_path), f"ref_{i}", "prompt_grounding_ocr", str(tmp_path / "ref"), bbox=box)[0]
        assert set(res) == set(want) and res["file_path"] == want["file_path"]
        assert (res["input_height"], res["input_width"], res["page_no"]) == (want["input_height"], want["input_width"], want["page_no"])
        assert json.loads(Path(res["layout_info_path"]).read_text()) == f"text of {prompts[i].splitlines()[-1]}"       # box i got answer i
        for key in ("md_content_path", "layout_info_path"):                               # the same files as the per-box call writes
            assert Path(res[key]).read_text() == Path(want[key]).read_text()
    assert singles == prompts                                                              # the per-box path sends exactly these prompts, one each
    # nine boxes: one request of eight and a lone ordinary one
    calls.clear(), singles.clear()
    assert len(parser.parse_image_regions(str(page_path), [[1, 1, 20 + i, 20] for i in range(9)])) == 9
    assert [len(c[1]) for c in calls] == [8] and len(singles) == 1
