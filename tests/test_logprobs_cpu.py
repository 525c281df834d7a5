"""Per-token logprobs above the kernels, on CPU: the server's `logprobs` / `top_logprobs` fields and the OpenAI
`logprobs` object, the scheduler's set_row_logprobs / row_logprobs calls around a slot's life, and token_bytes of the tokenizers."""
import threading
import time

import numpy as np
import pytest

from dots_ocr_amd.config import DotsConfig
from dots_ocr_amd.row_features import rows_holding

K = 20


def _lp_engine(base):
    """a slot engine with the logprob calls: scripted values, and a log of the order of the calls"""
    class LpEngine(base):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            self.lp, self.lp_calls, self.prefill_lp, self.events = {}, [], [], []

        def set_row_logprobs(self, row, top_n):
            self.lp_calls.append((row, top_n))
            if top_n is None:
                self.lp.pop(row, None)
            else:
                self.lp[row] = top_n

        def slots_prefill(self, slots, ids, lens, caps):
            off = 0
            for s, n in zip(slots, lens):
                self.prefill_lp.append((s, int(ids[off]), self.lp.get(s)))
                off += n
            super().slots_prefill(slots, ids, lens, caps)

        def row_logprobs(self, s, n, pos0=0):
            """position i of slot s: token logprob -(i + 1) / 8, alternatives ids 65 + k with logprob -k / 4 (k < top_n), then -1 / NaN"""
            assert s in self.slots
            self.events.append(("row_logprobs", s))
            m = max(0, min(n, len(self.slots[s]["out"]) - pos0))
            top_n = self.lp.get(s, -1)
            tok = np.array([-(pos0 + i + 1) / 8 for i in range(m)], np.float32)
            ids = np.full((m, K), -1, np.int32)
            top = np.full((m, K), np.nan, np.float32)
            for k in range(max(0, top_n)):
                ids[:, k] = 65 + k
                top[:, k] = -k / 4
            return tok, ids, top

        def slot_release(self, s):           # the engine switches the row off with the slot (dots_slot_release)
            self.events.append(("release", s))
            self.lp.pop(s, None)
            super().slot_release(s)
    return LpEngine


# ---------------------------------------------------------------------------------------------------- scheduler

def test_scheduler_sets_the_flag_before_the_prefill_and_reads_before_release():
    from fakes import FakeSlotEngine
    from dots_ocr_amd.scheduler import ContinuousBatcher, Request
    eng = _lp_engine(FakeSlotEngine)(lambda prompt: [5] * (3 + int(prompt[0]) % 3), max_batch=2, max_prefill_tokens=64)
    asks = [3, None, 0, None, 20, None]
    reqs = [Request(np.array([10 + i, 1, 2], np.int32), max_new_tokens=4 + i, logprobs=a) for i, a in enumerate(asks)]
    outs = ContinuousBatcher(eng, chunk=2).run(reqs)
    assert len(outs) == len(reqs) and len(eng.prefill_lp) == len(reqs)
    for slot, first, flag in eng.prefill_lp:
        assert flag == asks[first - 10], (slot, first)
    for r, toks in zip(reqs, outs):
        if r.logprobs is None:
            assert not hasattr(r, "logprobs_out")
            continue
        tok, ids, top = r.logprobs_out
        assert tok.shape == (len(toks),) and ids.shape == top.shape == (len(toks), K)
        assert (ids[:, :r.logprobs] >= 0).all() and (ids[:, r.logprobs:] == -1).all()
    reads = [i for i, ev in enumerate(eng.events) if ev[0] == "row_logprobs"]
    assert len(reads) == sum(a is not None for a in asks)
    for i in reads:                                          # each read comes before that slot's release
        assert eng.events[i + 1] == ("release", eng.events[i][1])


def test_scheduler_clears_the_flag_on_reuse_without_logprobs():
    from fakes import FakeSlotEngine
    from dots_ocr_amd.scheduler import ContinuousBatcher, Request
    eng = _lp_engine(FakeSlotEngine)(lambda prompt: [5] * 6, max_batch=1, max_prefill_tokens=64)
    eng.slot_release = FakeSlotEngine.slot_release.__get__(eng)          # an engine that keeps the flag until told otherwise
    ContinuousBatcher(eng, chunk=2).run([Request(np.array([1, 2], np.int32), max_new_tokens=3, logprobs=5),
                                         Request(np.array([3, 4], np.int32), max_new_tokens=3)])
    assert eng.lp_calls == [(0, 5), (0, None)]
    assert [p[2] for p in eng.prefill_lp] == [5, None]


def test_scheduler_clears_the_flag_when_the_prefill_fails():
    from fakes import FakeSlotEngine
    from dots_ocr_amd.scheduler import ContinuousBatcher, Request
    eng = _lp_engine(FakeSlotEngine)(lambda prompt: [5] * 4, max_batch=2, max_prefill_tokens=64)

    def fail(*a):
        raise RuntimeError("KV pool exhausted")
    eng.slots_prefill = fail
    cb = ContinuousBatcher(eng, chunk=2)
    cb.submit(Request(np.array([1, 2], np.int32), max_new_tokens=3, logprobs=2))
    with pytest.raises(RuntimeError):
        cb.step()
    assert eng.lp == {} and rows_holding(cb._rows, "logprobs") == []
    assert eng.lp_calls == [(0, 2), (0, None)]


def test_scheduler_without_logprobs_makes_no_logprob_calls():
    from fakes import FakeSlotEngine
    from dots_ocr_amd.scheduler import ContinuousBatcher, Request
    eng = _lp_engine(FakeSlotEngine)(lambda prompt: [5] * 4, max_batch=2, max_prefill_tokens=64)
    ContinuousBatcher(eng, chunk=2).run([Request(np.array([1 + i, 2], np.int32), max_new_tokens=3) for i in range(4)])
    assert eng.lp_calls == [] and not any(ev[0] == "row_logprobs" for ev in eng.events)


# ---------------------------------------------------------------------------------------------------- server

class _Model:
    def __init__(self, cfg, proc, logprobs=True):
        from fakes import FakeSlotEngine

        class Eng(FakeSlotEngine):
            def slots_decode(self, n):
                time.sleep(0.002)
                super().slots_decode(n)
        script = lambda prompt: proc.tokenizer.encode("ok é") + [cfg.eos_token_ids[0]]        # noqa: E731
        self.config = cfg
        self.engine = (_lp_engine(Eng) if logprobs else Eng)(script, max_batch=2, max_patches=4096, max_prefill_tokens=4096,
                                                               max_seq_len=2048)


def _payload(**kw):
    body = {"model": "model", "messages": [{"role": "user", "content": "Read this."}], "max_completion_tokens": 32}
    body.update(kw)
    return body


def _app(logprobs=True, continuous=True):
    pytest.importorskip("fastapi")
    from dots_ocr_amd.processing import DotsOcrProcessor
    from dots_ocr_amd.server import create_app
    cfg = DotsConfig.tiny()
    proc = DotsOcrProcessor(cfg)
    return cfg, proc, create_app(_Model(cfg, proc, logprobs), proc, model_name="model", max_batch=2, continuous=continuous)


def test_server_rejects_bad_logprob_fields():
    from fastapi.testclient import TestClient
    _, _, app = _app()
    with TestClient(app) as c:
        for bad in (dict(top_logprobs=2), dict(logprobs=False, top_logprobs=2), dict(logprobs=True, top_logprobs=21),
                    dict(logprobs=True, top_logprobs=-1), dict(logprobs=True, top_logprobs=1.5), dict(logprobs=True, top_logprobs=True),
                    dict(logprobs=1), dict(logprobs="yes")):
            r = c.post("/v1/chat/completions", json=_payload(**bad))
            assert r.status_code == 400, (bad, r.text)


def test_server_refuses_logprobs_where_the_engine_cannot_return_them():
    from fastapi.testclient import TestClient
    _, _, app = _app(continuous=False)                       # static batches through model.generate
    with TestClient(app) as c:
        r = c.post("/v1/chat/completions", json=_payload(logprobs=True))
        assert r.status_code == 400 and "logprobs" in r.text
    _, _, app = _app(logprobs=False)                         # slots, but an engine without set_row_logprobs
    with TestClient(app) as c:
        assert c.post("/v1/chat/completions", json=_payload(logprobs=True, top_logprobs=1)).status_code == 400
        assert c.post("/v1/chat/completions", json=_payload()).status_code == 200


def test_server_returns_the_openai_logprobs_object():
    from fastapi.testclient import TestClient
    cfg, proc, app = _app()
    tk = proc.tokenizer
    with TestClient(app) as c:
        res = {}

        def go(key, body):
            res[key] = c.post("/v1/chat/completions", json=_payload(**body))
        asks = {"top3": dict(logprobs=True, top_logprobs=3), "top0": dict(logprobs=True), "none": dict(), "off": dict(logprobs=False)}
        th = [threading.Thread(target=go, args=(k, b)) for k, b in asks.items()]
        [t.start() for t in th]
        [t.join() for t in th]
        for key in ("top3", "top0"):
            r = res[key]
            assert r.status_code == 200, r.text
            d = r.json()
            ch = d["choices"][0]
            content = ch["logprobs"]["content"]
            ids = tk.encode("ok é") + [cfg.eos_token_ids[0]]
            assert len(content) == d["usage"]["completion_tokens"] == len(ids)          # the final EOS id included
            assert ch["finish_reason"] == "stop"
            for n, (e, t) in enumerate(zip(content, ids)):
                assert e["token"] == tk.decode([t], skip_special_tokens=False)
                assert e["bytes"] == list(tk.token_bytes(t))
                assert e["logprob"] == pytest.approx(-(n + 1) / 8)
                want = asks[key].get("top_logprobs", 0)
                assert len(e["top_logprobs"]) == want
                for k, alt in enumerate(e["top_logprobs"]):
                    assert alt == {"token": tk.decode([65 + k], skip_special_tokens=False), "logprob": pytest.approx(-k / 4),
                                   "bytes": [65 + k]}
        for key in ("none", "off"):                          # not asked: no logprobs key at all
            r = res[key]
            assert r.status_code == 200
            assert "logprobs" not in r.json()["choices"][0]
            assert set(r.json()["choices"][0]) == {"index", "message", "finish_reason"}


# ---------------------------------------------------------------------------------------------------- token bytes

def test_synthetic_tokenizer_token_bytes():
    from dots_ocr_amd.processing import IMG_PAD, SyntheticByteTokenizer
    cfg = DotsConfig.tiny()
    tk = SyntheticByteTokenizer(cfg)
    assert tk.token_bytes(65) == b"A" and tk.token_bytes(0xC3) == b"\xc3" and tk.token_bytes(0) == b"\x00"
    assert tk.token_bytes(cfg.image_token_id) == IMG_PAD.encode()
    assert tk.token_bytes(cfg.eos_token_ids[0]) == b"<|endoftext|>"
    assert b"".join(tk.token_bytes(t) for t in tk.encode("naïve ü")) == "naïve ü".encode()


def test_byte_level_inverse_on_hand_written_tokens():
    from dots_ocr_amd.processing import BYTE_TO_UNICODE, UNICODE_TO_BYTE, byte_level_token_bytes
    assert len(BYTE_TO_UNICODE) == 256 and sorted(UNICODE_TO_BYTE.values()) == list(range(256))
    assert byte_level_token_bytes("Ġthe") == b" the"            # U+0120 = the space byte
    assert byte_level_token_bytes("ĊĊ") == b"\n\n"              # U+010A = newline
    assert byte_level_token_bytes("Ã©") == "é".encode()          # the two UTF-8 bytes of é
    assert byte_level_token_bytes("ä½ł") == "你".encode()
    assert byte_level_token_bytes("ðŁĺ") == b"\xf0\x9f\x98"     # a partial UTF-8 sequence stays raw bytes
    assert byte_level_token_bytes("abc") == b"abc"


def test_hf_tokenizer_token_bytes(tmp_path):
    pytest.importorskip("tokenizers")
    import json
    from dots_ocr_amd.processing import HFJsonTokenizer
    vocab = {"a": 0, "b": 1, "Ġ": 2, "Ġa": 3, "Ã©": 4}
    tj = {"version": "1.0", "truncation": None, "padding": None,
          "added_tokens": [{"id": 5, "content": "<|endoftext|>", "single_word": False, "lstrip": False, "rstrip": False,
                            "normalized": False, "special": True}],
          "normalizer": None, "pre_tokenizer": {"type": "ByteLevel", "add_prefix_space": False, "trim_offsets": True, "use_regex": True},
          "post_processor": None, "decoder": {"type": "ByteLevel", "add_prefix_space": True, "trim_offsets": True, "use_regex": True},
          "model": {"type": "BPE", "dropout": None, "unk_token": None, "continuing_subword_prefix": None, "end_of_word_suffix": None,
                    "fuse_unk": False, "byte_fallback": False, "vocab": vocab, "merges": ["Ġ a"]}}
    (tmp_path / "tokenizer.json").write_text(json.dumps(tj), encoding="utf-8")
    tk = HFJsonTokenizer(tmp_path, DotsConfig.tiny())
    assert tk.token_bytes(3) == b" a" and tk.token_bytes(0) == b"a"
    assert tk.token_bytes(4) == "é".encode()
    assert tk.token_bytes(5) == b"<|endoftext|>"
