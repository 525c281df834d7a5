"""OpenAI-compatible `/v1/chat/completions` endpoint on top of the HIP engine.

The reference's DEFAULT backend is an HTTP client of a vLLM server (dots_ocr/model/inference.py:7-48, used by
`DotsOCRParser(use_hf=False)`, demo/demo_vllm*.py and the Gradio/Streamlit apps): it POSTs one user message holding an
`image_url` data URL (base64 PNG, image_utils.py:67-71) and a text part "<|img|><|imgpad|><|endofimg|>{prompt}", with
`max_completion_tokens`, `temperature`, `top_p` (inference.py:28-43), and reads `choices[0].message.content`.  This module
serves exactly that wire format from the MI355X engine, so those callers work unchanged when pointed at it:

    python -m dots_ocr_amd.server --model-path ./weights/DotsOCR --port 8000

Concurrent requests (the reference client uses a ThreadPool of up to 64, parser.py:286-290) share the engine the way they
share a vLLM server: `ContinuousWorker` admits a request into a free sequence slot as soon as one exists and refills slots
as pages finish (dots_ocr_amd/scheduler.py).  On an engine with per-row selection (Engine.set_row_sampling) every request
carries its own sampling parameters on its slot and one running set serves them all; on an engine without it, requests with
other parameters wait for the running set to drain, and a request that asks for top_k or a penalty is refused (400).
`logprobs` / `top_logprobs` return the OpenAI `choices[0].logprobs` object (raw-logit log-probabilities, Engine.set_row_logprobs); they
need continuous batching on an engine that has them, else 400.
`logit_bias`, `allowed_token_ids`, `min_tokens`, `stop_token_ids` and `ignore_eos` travel as the request's LogitRules on its slot
(Engine.set_row_logit_rules); a worker that cannot honour them (static batching, an engine without the call) answers 400.
`no_repeat_ngram_size`, `no_repeat_ngram_window` and `no_repeat_ngram_whitelist` (token ids) travel as the request's NgramRule on its slot
(Engine.set_row_ngram): the row never completes an n-gram its own output already holds, inside the last `window` generated
tokens when one is given, whitelisted ids excepted.  The prompt is not part of the history (vLLM's convention).  Bad values, and a worker
that cannot honour the fields (static batching, an engine without the call), answer 400.
`BatchingWorker` (static batches through `model.generate`) remains for model objects without engine slots.
"""
from __future__ import annotations

import argparse
import math
import queue
import threading
import time
import uuid
from collections import OrderedDict
from concurrent.futures import Future
from typing import List, Optional

from .image_utils import fetch_image
from .scheduler import RequestRejected
from .processing import ASSISTANT, END_USER, IMG_END, IMG_PAD, IMG_START, USER


class _Job:
    __slots__ = ("image", "text", "max_tokens", "temperature", "top_p", "top_k", "repetition_penalty", "frequency_penalty",
                 "presence_penalty", "seed", "logprobs", "rules", "guide", "ngram", "n", "future")

    def __init__(self, image, text, max_tokens, temperature, top_p, top_k=0, repetition_penalty=1.0, frequency_penalty=0.0,
                 presence_penalty=0.0, seed=None, logprobs=None):
        self.image, self.text, self.max_tokens, self.temperature, self.top_p = image, text, max_tokens, temperature, top_p
        self.top_k, self.repetition_penalty = top_k, repetition_penalty
        self.frequency_penalty, self.presence_penalty, self.seed = frequency_penalty, presence_penalty, seed
        self.logprobs = logprobs                    # top_logprobs (0..20) when the request asked for logprobs, else None
        self.rules = None                           # engine.LogitRules when the request carries logit rules, else None
        self.guide = None                           # guided.Guide when the request carries a guided decoding field, else None
        self.ngram = None                           # engine.NgramRule when the request carries no_repeat_ngram_size, else None
        self.n = 1                                  # sequences to return (parallel sampling)
        self.future: Future = Future()

    @property
    def extended(self) -> bool:
        """asks for a selection knob beyond (temperature, top_p, seed)"""
        return self.top_k > 0 or self.repetition_penalty != 1.0 or self.frequency_penalty != 0.0 or self.presence_penalty != 0.0


class BatchingWorker:
    """Single consumer thread (the engine handle is not thread-safe): groups queued jobs by sampling parameters."""

    def __init__(self, model, processor, max_batch: int = 8, max_wait_ms: float = 5.0, seed: int = 0):
        self.model, self.processor = model, processor
        self.max_batch, self.max_wait = max_batch, max_wait_ms / 1e3
        self.q: "queue.Queue[_Job]" = queue.Queue()
        self.seed = seed
        self.batches: List[int] = []            # sizes of the executed batches (observability / tests)
        self._stop = False
        self.thread = threading.Thread(target=self._run, name="dots-ocr-batcher", daemon=True)
        self.thread.start()

    def submit(self, job: _Job) -> Future:
        self.q.put(job)
        return job.future

    def close(self):
        self._stop = True
        self.q.put(None)
        self.thread.join(timeout=5)

    def _run(self):
        pending: List[_Job] = []
        while not self._stop:
            if not pending:
                job = self.q.get()
                if job is None:
                    return
                pending.append(job)
            deadline = time.monotonic() + self.max_wait
            while len(pending) < 4 * self.max_batch:
                try:
                    job = self.q.get(timeout=max(0.0, deadline - time.monotonic()))
                except queue.Empty:
                    break
                if job is None:
                    self._stop = True
                    break
                pending.append(job)
            key = self._group_key(pending[0])
            batch = [j for j in pending if self._group_key(j) == key][: self.max_batch]
            pending = [j for j in pending if j not in batch]
            self._execute(batch)

    @staticmethod
    def _group_key(j: _Job):
        return (j.max_tokens, j.temperature, j.top_p, j.top_k, j.repetition_penalty, j.frequency_penalty, j.presence_penalty, j.seed)

    def _execute(self, batch: List[_Job]):
        try:
            images = [j.image for j in batch if j.image is not None]
            inputs = self.processor(text=[j.text for j in batch], images=images or None, padding=True, return_tensors="pt")
            j0 = batch[0]
            self.seed += 1
            extra = {}
            if j0.extended:                                          # only then: generate() keeps today's path otherwise
                extra = dict(top_k=j0.top_k, repetition_penalty=j0.repetition_penalty, frequency_penalty=j0.frequency_penalty,
                             presence_penalty=j0.presence_penalty)
            out = self.model.generate(**inputs, max_new_tokens=j0.max_tokens, do_sample=j0.temperature > 0,
                                      temperature=j0.temperature, top_p=j0.top_p, seed=self.seed if j0.seed is None else j0.seed, **extra)
            new = [o[len(i):] for i, o in zip(inputs.input_ids, out)]
            texts = self.processor.batch_decode(new, skip_special_tokens=True, clean_up_tokenization_spaces=False)
            pad = self.processor.tokenizer.pad_token_id
            eos = set(getattr(self.model, "config", None).eos_token_ids) if getattr(self.model, "config", None) else set()
            self.batches.append(len(batch))
            for j, t, ids, inp in zip(batch, texts, new, inputs.input_ids):
                toks = [int(x) for x in ids.tolist()]
                while toks and toks[-1] == pad and pad not in eos:
                    toks.pop()
                n_new = len(toks)
                hit_eos = any(x in eos for x in toks)
                j.future.set_result({"text": t, "prompt_tokens": int((inp != pad).sum()) if pad not in eos else int(len(inp)),
                                     "completion_tokens": n_new, "finish_reason": "stop" if hit_eos else "length"})
        except Exception as e:                      # surface the failure to every waiting request
            for j in batch:
                if not j.future.done():
                    j.future.set_exception(e)


class ContinuousWorker(BatchingWorker):
    """Continuous batching over the engine's sequence slots; same submit()/close() surface as BatchingWorker.
    `batches` records the number of occupied slots after every admission."""

    def __init__(self, model, processor, max_batch: int = 8, max_wait_ms: float = 5.0, seed: int = 0, chunk: int = 16,
                 look_ahead: Optional[int] = None):
        self.chunk = chunk
        # scheduler look-ahead (ContinuousBatcher(prefetch=k)): the towers of the next k queued requests run on the CU-masked side stream
        # beside the occupied slots.  Measured on A4 pages of mixed output length (tools/serve_bench.py, profiles/r04_serve_bench_a4_*.json):
        # 8 slots 3.26 -> 3.50 pages/s with k = 2, 16 slots 4.13 -> 4.36 with k = 8; identical tokens.  0 switches it off.
        self.look_ahead = (2 if max_batch <= 8 else min(8, max_batch // 2)) if look_ahead is None else max(0, int(look_ahead))
        # guided decoding: the vocabulary's bytes go to the engine once, here; compiled guides are kept as engine handles in a
        # small LRU keyed by pattern (_guide_handle), a handle is evicted only when no request in flight uses it
        self._guides: "OrderedDict[str, int]" = OrderedDict()
        self._guide_users: dict = {}
        engine = getattr(model, "engine", None)
        if engine is not None and hasattr(engine, "set_token_bytes") and getattr(engine, "token_bytes", None) is None \
                and hasattr(processor, "guide_token_bytes"):
            engine.set_token_bytes(processor.guide_token_bytes())
        super().__init__(model, processor, max_batch=max_batch, max_wait_ms=max_wait_ms, seed=seed)

    @staticmethod
    def _key(j: _Job):
        return (j.temperature, j.top_p)

    @property
    def per_row(self) -> bool:
        """the engine selects tokens with per-row parameters: one running set serves every request"""
        return hasattr(self.model.engine, "set_row_sampling")

    def _row_params(self, job: _Job):
        """the request's SamplingParams on its slot (None: a plain greedy request, the engine-wide greedy path)"""
        from .engine import SamplingParams
        if job.temperature <= 0 and not job.extended:
            return None
        seed = job.seed
        if seed is None:                             # n sequences run under seed .. seed + n - 1: they take n values of the counter
            seed = self.seed + 1
            self.seed += job.n
        return SamplingParams(temperature=job.temperature, top_p=job.top_p, top_k=job.top_k, repetition_penalty=job.repetition_penalty,
                              frequency_penalty=job.frequency_penalty, presence_penalty=job.presence_penalty, seed=seed)

    @property
    def has_logprobs(self) -> bool:
        """the engine returns per-token log-probabilities (Engine.set_row_logprobs)"""
        return hasattr(self.model.engine, "set_row_logprobs")

    @property
    def has_rules(self) -> bool:
        """the engine takes per-request logit rules (Engine.set_row_logit_rules)"""
        return hasattr(self.model.engine, "set_row_logit_rules")

    @property
    def has_ngram(self) -> bool:
        """the engine takes per-request n-gram rules (Engine.set_row_ngram)"""
        return hasattr(self.model.engine, "set_row_ngram")

    GUIDE_CACHE = 16                                 # compiled guides kept on the engine

    @property
    def has_guides(self) -> bool:
        """the engine takes guides and knows its vocabulary's bytes (Engine.set_row_guide / set_token_bytes)"""
        return hasattr(self.model.engine, "set_row_guide") and getattr(self.model.engine, "token_bytes", None) is not None

    def _guide_handle(self, job: _Job) -> Optional[int]:
        """the engine handle of the job's guide, compiled guides cached per pattern (worker thread only)"""
        if job.guide is None:
            return None
        key = job.guide.pattern
        h = self._guides.get(key)
        if h is None:
            for old in [k for k in self._guides if not self._guide_users.get(self._guides[k])][:max(0, len(self._guides) + 1 - self.GUIDE_CACHE)]:
                self.model.engine.destroy_guide(self._guides.pop(old))       # no request in flight uses it, so no row holds it
            h = self._guides[key] = self.model.engine.create_guide(job.guide)
        self._guides.move_to_end(key)
        self._guide_users[h] = self._guide_users.get(h, 0) + 1
        return h

    def _guide_done(self, req):
        h = getattr(req, "guide", None)
        if h is not None and self._guide_users.get(h, 0) > 0:
            self._guide_users[h] -= 1

    def _finish(self, job: _Job, prompt_tokens: int, toks, kv_truncated: bool = False, logprobs=None):
        job.future.set_result(self._result(job, prompt_tokens, toks, kv_truncated, logprobs))

    def _finish_group(self, job: _Job, prompt_tokens: int, req):
        """a request with n > 1: one result per sequence, in index order; the prompt is counted once"""
        lps = getattr(req, "logprobs_out", None) or [None] * job.n
        each = [self._result(job, prompt_tokens, t, k, l) for t, k, l in zip(req.outputs, req.kv_truncated_each, lps)]
        job.future.set_result({"prompt_tokens": prompt_tokens, "completion_tokens": sum(r["completion_tokens"] for r in each), "choices": each})

    def _result(self, job: _Job, prompt_tokens: int, toks, kv_truncated: bool = False, logprobs=None):
        eos = set(self.model.config.eos_token_ids)
        if job.guide is not None:                    # a guided row ends at an EOS id whether or not ignore_eos is set
            eos = eos | (set(job.rules.stop) if job.rules is not None else set())
        elif job.rules is not None:                    # the request's own stop ids end it as an EOS does; ignore_eos takes the EOS ids out
            eos = (set() if job.rules.ignore_eos else eos) | set(job.rules.stop)
        toks = [int(t) for t in toks]
        text = self.processor.batch_decode([toks], skip_special_tokens=True, clean_up_tokenization_spaces=False)[0]
        # "kv_pool_exhausted": the engine ended the sequence at what its KV pages hold (vLLM would preempt and recompute; here the
        # caller sees that the output is short for a reason other than max_tokens and can resubmit)
        reason = "stop" if toks and toks[-1] in eos else ("kv_pool_exhausted" if kv_truncated else "length")
        res = {"text": text, "prompt_tokens": prompt_tokens, "completion_tokens": len(toks), "finish_reason": reason}
        if job.logprobs is not None:
            res["logprobs"] = _logprobs_object(self.processor, toks, logprobs, job.logprobs)
        return res

    def _run(self):
        from collections import deque
        from .scheduler import ContinuousBatcher, Request
        engine = self.model.engine
        per_row = self.per_row
        keyf = (lambda j: None) if per_row else self._key             # per-row parameters: one running set, no drains
        waiting: "deque[_Job]" = deque()
        cb, key = None, None
        while True:
            busy = cb is not None and not cb.idle
            if not busy and not waiting:
                job = self.q.get()                                   # nothing to do: block
                if job is None:
                    return
                waiting.append(job)
            while True:                                              # take whatever else has arrived
                try:
                    job = self.q.get_nowait()
                except queue.Empty:
                    break
                if job is None:
                    self._stop = True
                    break
                waiting.append(job)
            if self._stop and not busy and not waiting:
                return
            try:
                if not busy and waiting and (cb is None or key != keyf(waiting[0])):
                    key = keyf(waiting[0])                           # switch sampling parameters between drained sets only
                    if per_row:
                        engine.set_sampling(0.0, 1.0, 0)             # plain greedy requests; every other request brings its own
                    else:
                        self.seed += 1
                        engine.set_sampling(key[0], key[1], self.seed)
                    cb = ContinuousBatcher(engine, eos_ids=self.model.config.eos_token_ids, chunk=self.chunk, prefetch=self.look_ahead)
                # admit the FIFO prefix that shares the running parameters; a different request at the head makes the set drain
                admitted = 0
                while waiting and keyf(waiting[0]) == key and len(cb.pending) < 2 * cb.n_slots:
                    job = waiting.popleft()
                    try:
                        inputs = self.processor(text=[job.text], images=[job.image] if job.image is not None else None,
                                                padding=True, return_tensors="pt")
                        ids = inputs["input_ids"][0].numpy()
                        req = Request(ids, inputs.get("pixel_values"), None if "image_grid_thw" not in inputs
                                      else inputs["image_grid_thw"].numpy(), job.max_tokens, tag=job,
                                      sampling=self._row_params(job) if per_row else None, logprobs=job.logprobs, rules=job.rules,
                                      guide=self._guide_handle(job), ngram=job.ngram, n=job.n)
                        try:
                            cb.submit(req)
                        except Exception:
                            self._guide_done(req)
                            raise
                        admitted += 1
                    except Exception as e:                           # a bad request fails alone
                        job.future.set_exception(e)
                if cb is not None and not cb.idle:
                    for _, req, toks in cb.step():
                        self._guide_done(req)
                        if getattr(req, "error", None) is not None:      # refused at admission: this request alone
                            req.tag.future.set_exception(req.error)
                            continue
                        if req.n > 1:
                            self._finish_group(req.tag, int(req.input_ids.shape[0]), req)
                            continue
                        self._finish(req.tag, int(req.input_ids.shape[0]), toks, getattr(req, "kv_truncated", False),
                                     getattr(req, "logprobs_out", None))
                    if admitted:
                        self.batches.append(len(cb.running))
            except Exception as e:                                   # engine failure: fail everything in flight, start clean
                if cb is not None:
                    for _, req in list(cb.running.values()) + list(cb.pending) + list(cb._ahead):
                        if not req.tag.future.done():
                            req.tag.future.set_exception(e)
                cb, key = None, None
                self._guide_users.clear()                            # the next ContinuousBatcher resets the slots: no row holds a guide


def _load_request_image(url: str, allow_remote: bool, allow_local: bool):
    """Image of a chat request.  Default: `data:image/...;base64,` URLs only — all the reference client sends
    (model/inference.py:20-33).  http(s) URLs and local paths are opt-in server flags: the server listens on 0.0.0.0, so
    resolving client-supplied locations would let a remote caller read local files or reach internal services (SSRF)."""
    if not isinstance(url, str):
        raise ValueError("image_url must be a string")
    if url.startswith("data:image"):
        return fetch_image(url)
    if url.startswith(("http://", "https://")):
        if not allow_remote:
            raise ValueError("remote image URLs are disabled (start the server with --allow-remote-images)")
        import requests
        from io import BytesIO
        from PIL import Image
        resp = requests.get(url, timeout=(3.0, 10.0), stream=True)
        resp.raise_for_status()
        data = resp.raw.read(64 * 1024 * 1024 + 1, decode_content=True)
        if len(data) > 64 * 1024 * 1024:
            raise ValueError("remote image larger than 64 MiB")
        return fetch_image(Image.open(BytesIO(data)))
    if not allow_local:
        raise ValueError("local image paths are disabled (start the server with --allow-local-images)")
    return fetch_image(url)


def _parse_messages(messages, processor=None, allow_remote: bool = False, allow_local: bool = False):
    """OpenAI chat messages -> (PIL image or None, chat-template text).  The text is rendered by the processor's chat
    template (the checkpoint's own Jinja template when it ships one).  The reference client writes the image placeholder
    tokens into its text part itself (model/inference.py:33); a client that sends them and an image part gets ONE image."""
    image, conv = None, []
    for m in messages:
        role, content = m.get("role", "user"), m.get("content")
        if isinstance(content, str):
            conv.append({"role": role, "content": [{"type": "text", "text": content}]})
            continue
        items = []
        for c in content or []:
            if c.get("type") == "image_url":
                url = c["image_url"]["url"] if isinstance(c["image_url"], dict) else c["image_url"]
                if image is not None:                  # one page per request, like the reference client (model/inference.py:23-43)
                    raise ValueError("exactly one image per request is supported")
                image = _load_request_image(url, allow_remote, allow_local)
                items.append({"type": "image", "image": "request"})
            elif c.get("type") == "text":
                items.append({"type": "text", "text": c["text"]})
        conv.append({"role": role, "content": items})
    for m in conv:                                    # placeholders already written into THIS message's text: drop its image item
        if any(IMG_PAD in it.get("text", "") for it in m["content"]):
            m["content"] = [it for it in m["content"] if it.get("type") != "image"]
    if processor is not None:
        return image, processor.apply_chat_template(conv, tokenize=False, add_generation_prompt=True)
    out = []                                          # no processor (unit tests): the stand-in template
    for m in conv:
        body = "".join(IMG_START + IMG_PAD + IMG_END if it.get("type") == "image" else it.get("text", "") for it in m["content"])
        out.append(body if m["role"] == "system" else (USER + body + END_USER if m["role"] == "user" else ASSISTANT + body))
    return image, "".join(out) + ASSISTANT


def _selection_fields(req: dict) -> dict:
    """top_k (vLLM: -1 or 0 = off), repetition_penalty, frequency_penalty, presence_penalty, seed of a request, validated
    (ValueError / TypeError on a value out of range) and normalised the way SamplingParams does it."""
    def num(name, default, cast=float):
        v = req.get(name)
        if v is None:
            return default
        if isinstance(v, bool) or not isinstance(v, (int, float)):
            raise TypeError(f"{name} must be a number")
        if cast is int and float(v) != int(v):
            raise ValueError(f"{name} must be an integer")
        return cast(v)
    from .engine import SamplingParams
    out = dict(top_k=min(max(0, num("top_k", 0, int)), SamplingParams.TOP_K_MAX), repetition_penalty=num("repetition_penalty", 1.0),
               frequency_penalty=num("frequency_penalty", 0.0), presence_penalty=num("presence_penalty", 0.0), seed=num("seed", None, int))
    if not (out["repetition_penalty"] > 0 and out["repetition_penalty"] != float("inf")):
        raise ValueError("repetition_penalty must be finite and > 0")
    for name in ("frequency_penalty", "presence_penalty"):
        if not -2.0 <= out[name] <= 2.0:
            raise ValueError(f"{name} must be in [-2, 2]")
    if out["seed"] is not None:
        out["seed"] &= 2 ** 64 - 1
    return out


def _logprob_fields(req: dict) -> Optional[int]:
    """`logprobs` (bool) and `top_logprobs` (0..20, only with logprobs: true) of a request -> the top_n to return, or None when the
    request does not ask for logprobs.  ValueError / TypeError on a bad value."""
    from .engine import MAX_TOP_LOGPROBS
    lp, top = req.get("logprobs"), req.get("top_logprobs")
    if lp is not None and not isinstance(lp, bool):
        raise TypeError("logprobs must be a boolean")
    if top is not None:
        if isinstance(top, bool) or not isinstance(top, int):
            raise TypeError("top_logprobs must be an integer")
        if not lp:
            raise ValueError("top_logprobs needs logprobs: true")
        if not 0 <= top <= MAX_TOP_LOGPROBS:
            raise ValueError(f"top_logprobs must be in [0, {MAX_TOP_LOGPROBS}]")
    return (top or 0) if lp else None


GUIDE_FIELDS = ("guided_regex", "guided_choice", "guided_json", "guided_layout", "guided_whitespace_pattern", "response_format")


def _guide_fields(req: dict, min_tokens: int = 0):
    """`guided_regex`, `guided_choice`, `guided_json` (object or JSON string) with `guided_whitespace_pattern` (vLLM),
    `response_format: {"type": "json_schema", "json_schema": {"schema": ...}}` (OpenAI) and this server's `guided_layout: true`
    (guided.layout_schema) -> the compiled guided.Guide, or None when the request carries none.  At most one of them; a compile error, a
    recursive format ({"type": "json_object"}) and a `min_tokens` above the guide's shortest match raise ValueError (a 400).  The
    min_tokens test is a cheap sufficient one in bytes: a match shorter than min_tokens bytes could end before min_tokens tokens, where
    the EOS is still forbidden and nothing else is allowed; a longer shortest match cannot."""
    from .guided import compile_request
    rf = req.get("response_format")
    schema = None
    if rf is not None:
        if not isinstance(rf, dict):
            raise ValueError("response_format must be an object")
        kind = rf.get("type")
        if kind == "json_object":
            raise ValueError("response_format json_object: free-form JSON is recursive; give a schema")
        if kind == "json_schema":
            js = rf.get("json_schema")
            if not isinstance(js, dict) or not isinstance(js.get("schema"), dict):
                raise ValueError("response_format json_schema needs json_schema.schema")
            schema = js["schema"]
        elif kind not in (None, "text"):
            raise ValueError(f"unsupported response_format type {kind!r}")
    gj = req.get("guided_json")
    if gj is not None and schema is not None:
        raise ValueError("at most one of the guided decoding fields may be given, got guided_json, response_format")
    if gj is not None and not isinstance(gj, (dict, str)):
        raise ValueError("guided_json must be a schema object or a JSON string")
    layout = req.get("guided_layout")
    if layout is not None and not isinstance(layout, bool):
        raise ValueError("guided_layout must be true or false")
    guide = compile_request(req.get("guided_regex"), req.get("guided_choice"), gj if gj is not None else schema, bool(layout),
                            whitespace=req.get("guided_whitespace_pattern"))
    if guide is not None and min_tokens > guide.min_length:
        raise ValueError(f"min_tokens={min_tokens} exceeds the guide's shortest match ({guide.min_length} bytes): the row could be left "
                         "with nothing to select")
    return guide


RULE_FIELDS = ("logit_bias", "allowed_token_ids", "min_tokens", "stop_token_ids", "ignore_eos")


def _rule_fields(req: dict, vocab_size: Optional[int], max_tokens: int, eos_ids=None):
    """`logit_bias` (OpenAI: {"id": value in [-100, 100]}), `allowed_token_ids`, `min_tokens`, `stop_token_ids`, `ignore_eos` (vLLM) of a
    request -> engine.LogitRules, or None when the request uses none of them.  ValueError / TypeError on a bad value."""
    if all(req.get(k) is None for k in RULE_FIELDS):
        return None
    from .engine import LogitRules

    def id_list(name):
        v = req.get(name)
        if v is None:
            return None
        if not isinstance(v, list) or any(isinstance(t, bool) or not isinstance(t, int) for t in v):
            raise TypeError(f"{name} must be a list of integer token ids")
        return v
    bias = {}
    lb = req.get("logit_bias")
    if lb is not None:
        if not isinstance(lb, dict):
            raise TypeError("logit_bias must be an object of token id -> bias")
        for k, v in lb.items():
            try:
                t = int(k)
            except (TypeError, ValueError):
                raise ValueError(f"logit_bias key {k!r} is not a token id")
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not -100.0 <= float(v) <= 100.0:
                raise ValueError(f"logit_bias[{k!r}] must be a number in [-100, 100]")
            if t in bias:
                raise ValueError(f"logit_bias names token {t} twice")
            bias[t] = float(v)
    mt = req.get("min_tokens")
    if mt is not None and (isinstance(mt, bool) or not isinstance(mt, int) or mt < 0):
        raise TypeError("min_tokens must be an integer >= 0")
    if mt is not None and mt > max_tokens:
        raise ValueError(f"min_tokens ({mt}) exceeds max_tokens ({max_tokens})")
    ie = req.get("ignore_eos")
    if ie is not None and not isinstance(ie, bool):
        raise TypeError("ignore_eos must be a boolean")
    rules = LogitRules(bias=bias, allowed=id_list("allowed_token_ids"), min_tokens=mt or 0, stop=tuple(id_list("stop_token_ids") or ()),
                       ignore_eos=bool(ie), vocab_size=vocab_size, eos_ids=eos_ids)
    return None if rules.empty else rules


NGRAM_FIELDS = ("no_repeat_ngram_size", "no_repeat_ngram_window", "no_repeat_ngram_whitelist")


def _ngram_fields(req: dict, vocab_size: Optional[int], max_seq_len: Optional[int] = None):
    """`no_repeat_ngram_size` (HF's name; 0 or absent = off), `no_repeat_ngram_window` (0 or absent = the whole output) and
    `no_repeat_ngram_whitelist` (token ids) of a request -> engine.NgramRule, or None when the request asks for none.  ValueError /
    TypeError on a bad value."""
    if all(req.get(k) is None for k in NGRAM_FIELDS):
        return None
    from .engine import NgramRule
    n, w, wl = (req.get(k) for k in NGRAM_FIELDS)
    for name, v in (("no_repeat_ngram_size", n), ("no_repeat_ngram_window", w)):
        if v is not None and (isinstance(v, bool) or not isinstance(v, int) or v < 0):
            raise TypeError(f"{name} must be an integer >= 0")
    if wl is not None and (not isinstance(wl, list) or any(isinstance(t, bool) or not isinstance(t, int) for t in wl)):
        raise TypeError("no_repeat_ngram_whitelist must be a list of integer token ids")
    if not n:
        if w or wl:
            raise ValueError("no_repeat_ngram_window and no_repeat_ngram_whitelist need no_repeat_ngram_size >= 1")
        return None
    return NgramRule(n, w or 0, tuple(wl or ()), vocab_size=vocab_size, max_seq_len=max_seq_len)


def _logprobs_object(processor, toks, logprobs, top_n: int) -> dict:
    """The OpenAI `choices[i].logprobs` object: one entry per generated id (the final EOS included), each with `top_n` alternatives.
    logprobs = (tok_lp [n], top_ids [n, 20], top_lp [n, 20]) as Engine.row_logprobs returns them."""
    tok_lp, top_ids, top_lp = logprobs

    def entry(t, v):
        v = float(v)
        return {"token": processor.tokenizer.decode([int(t)], skip_special_tokens=False), "logprob": v if math.isfinite(v) else -9999.0,
                "bytes": list(processor.token_bytes(int(t)))}
    content = []
    for n, t in enumerate(toks):
        e = entry(t, tok_lp[n])
        e["top_logprobs"] = [entry(top_ids[n][k], top_lp[n][k]) for k in range(top_n)]
        content.append(e)
    return {"content": content}


def create_app(model, processor, model_name: str = "model", max_batch: int = 8, max_wait_ms: float = 5.0, continuous: Optional[bool] = None,
               allow_remote_images: bool = False, allow_local_images: bool = False, look_ahead: Optional[int] = None):
    from fastapi import FastAPI, HTTPException
    from fastapi.concurrency import run_in_threadpool

    app = FastAPI(title="dots.ocr MI355X engine")
    if continuous is None:
        continuous = hasattr(model, "engine")
    worker = (ContinuousWorker(model, processor, max_batch=max_batch, max_wait_ms=max_wait_ms, look_ahead=look_ahead) if continuous
              else BatchingWorker(model, processor, max_batch=max_batch, max_wait_ms=max_wait_ms))
    app.state.worker = worker

    @app.get("/health")
    def health():
        return {"status": "ok"}

    @app.get("/v1/models")
    def models():
        return {"object": "list", "data": [{"id": model_name, "object": "model", "owned_by": "dots_ocr_amd"}]}

    @app.post("/v1/chat/completions")
    async def chat(req: dict):
        if req.get("stream"):
            raise HTTPException(400, "streaming is not supported")
        messages = req.get("messages")
        if not messages:
            raise HTTPException(400, "messages is required")
        try:            # decoding (and, when enabled, fetching) an image must not stall the event loop
            image, text = await run_in_threadpool(_parse_messages, messages, processor, allow_remote_images, allow_local_images)
        except Exception as e:
            raise HTTPException(400, f"bad message content: {e}")
        max_tokens = int(req.get("max_completion_tokens") or req.get("max_tokens") or 16384)
        temperature = float(req.get("temperature", 1.0) if req.get("temperature") is not None else 1.0)
        top_p = float(req.get("top_p", 1.0) if req.get("top_p") is not None else 1.0)
        try:
            job = _Job(image, text, max_tokens, max(0.0, temperature), min(max(top_p, 1e-6), 1.0), **_selection_fields(req))
            from .engine import SamplingParams       # the values exactly as the engine will be given them (fp32, int32)
            SamplingParams(temperature=job.temperature, top_p=job.top_p, top_k=job.top_k, repetition_penalty=job.repetition_penalty,
                           frequency_penalty=job.frequency_penalty, presence_penalty=job.presence_penalty, seed=job.seed or 0)
        except (TypeError, ValueError) as e:
            raise HTTPException(400, f"bad sampling parameters: {e}")
        if job.extended and isinstance(worker, ContinuousWorker) and not worker.per_row:
            raise HTTPException(400, "top_k, repetition_penalty, frequency_penalty and presence_penalty need an engine with per-row selection")
        try:
            job.logprobs = _logprob_fields(req)
        except (TypeError, ValueError) as e:
            raise HTTPException(400, f"bad logprobs parameters: {e}")
        if job.logprobs is not None and not (isinstance(worker, ContinuousWorker) and worker.has_logprobs):
            raise HTTPException(400, "logprobs need continuous batching on an engine that returns log-probabilities (Engine.set_row_logprobs)")
        try:
            mcfg = getattr(model, "config", None)     # the EOS ids the request will run under: never-selectable rules are a 400 here
            job.rules = _rule_fields(req, getattr(mcfg, "vocab_size", None), max_tokens, getattr(mcfg, "eos_token_ids", None))
        except (TypeError, ValueError) as e:
            raise HTTPException(400, f"bad logit rules: {e}")
        if job.rules is not None and not (isinstance(worker, ContinuousWorker) and worker.has_rules):
            raise HTTPException(400, "logit_bias, allowed_token_ids, min_tokens, stop_token_ids and ignore_eos need continuous batching on an "
                                     "engine with per-row logit rules (Engine.set_row_logit_rules)")
        try:
            job.ngram = _ngram_fields(req, getattr(mcfg, "vocab_size", None), getattr(getattr(model, "engine", None), "max_seq_len", None))
        except (TypeError, ValueError) as e:
            raise HTTPException(400, f"bad n-gram rule: {e}")
        if job.ngram is not None and not (isinstance(worker, ContinuousWorker) and worker.has_ngram):
            raise HTTPException(400, "no_repeat_ngram_size, no_repeat_ngram_window and no_repeat_ngram_whitelist need continuous batching on an "
                                     "engine with per-row n-gram rules (Engine.set_row_ngram)")
        if any(req.get(k) is not None for k in GUIDE_FIELDS):
            try:                                     # compiling a large schema takes a while: off the event loop
                job.guide = await run_in_threadpool(_guide_fields, req, job.rules.min_tokens if job.rules is not None else 0)
            except (TypeError, ValueError) as e:
                raise HTTPException(400, f"bad guided decoding parameters: {e}")
            if job.guide is not None and not (isinstance(worker, ContinuousWorker) and worker.has_guides):
                raise HTTPException(400, "guided_regex, guided_choice, guided_json, guided_layout and a json_schema response_format need "
                                         "continuous batching on an engine with guides (Engine.set_row_guide) that knows its token bytes")
        n = req.get("n")
        if n is not None:                            # parallel sampling: n sequences of one page from one tower and one prefill
            if isinstance(n, bool) or not isinstance(n, int) or n < 1:
                raise HTTPException(400, "n must be an integer >= 1")
            if n > 1 and not (isinstance(worker, ContinuousWorker) and hasattr(model.engine, "slots_fork")):
                raise HTTPException(400, "n > 1 needs continuous batching on an engine that forks a prefilled sequence (Engine.slots_fork)")
            slots = int(getattr(getattr(model, "engine", None), "usable_slots", max_batch))
            if n > slots:
                raise HTTPException(400, f"n = {n} exceeds the {slots} sequences this server runs at a time")
            job.n = n
        fut = worker.submit(job)
        try:
            res = await run_in_threadpool(fut.result)
        except RequestRejected as e:                 # the engine refused this request's own parameters: its fault alone
            raise HTTPException(400, f"request refused: {e}")
        except Exception as e:
            raise HTTPException(500, f"generation failed: {e}")
        choices = []
        for index, r in enumerate(res["choices"] if job.n > 1 else [res]):
            choice = {"index": index, "message": {"role": "assistant", "content": r["text"]}, "finish_reason": r["finish_reason"]}
            if job.logprobs is not None:             # only when asked: other responses stay exactly as they were
                choice["logprobs"] = r["logprobs"]
            choices.append(choice)
        return {
            "id": "chatcmpl-" + uuid.uuid4().hex, "object": "chat.completion", "created": int(time.time()),
            "model": req.get("model", model_name),
            "choices": choices,
            "usage": {"prompt_tokens": res["prompt_tokens"], "completion_tokens": res["completion_tokens"],
                      "total_tokens": res["prompt_tokens"] + res["completion_tokens"]},
        }

    @app.on_event("shutdown")
    def _shutdown():
        worker.close()

    return app


def build_arg_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description="OpenAI-compatible server for the dots.ocr MI355X engine")
    ap.add_argument("--model-path", default="./weights/DotsOCR")
    ap.add_argument("--random-weights", action="store_true", help="seeded random weights (no checkpoint): plumbing tests only")
    ap.add_argument("--host", default="0.0.0.0")
    ap.add_argument("--port", type=int, default=8000)
    ap.add_argument("--served-model-name", default="model")
    ap.add_argument("--max-batch", type=int, default=8)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--fp8-weights", action="store_true", help="quantise the linears to e4m3 (per-output-channel scale) at load time")
    ap.add_argument("--kv-cache-dtype", choices=["bf16", "fp8"], default=None,
                    help="paged KV cache element type (vLLM's flag): fp8 = e4m3fn with per-(layer, kv head) scales (the checkpoint's "
                         "self_attn.k_scale / v_scale, else 1.0); default $DOTS_OCR_KV_CACHE_DTYPE or bf16")
    ap.add_argument("--static-batching", action="store_true", help="static batches through model.generate instead of continuous batching")
    ap.add_argument("--look-ahead", type=int, default=None,
                    help="continuous batching: vision towers of the next N queued requests run on a CU partition beside the decoding slots "
                         "(default 2 up to 8 slots, min(8, slots / 2) above; 0 = off)")
    ap.add_argument("--allow-remote-images", action="store_true", help="let requests name http(s) image URLs (off: data: URLs only)")
    ap.add_argument("--allow-local-images", action="store_true", help="let requests name image paths on the server's file system")
    ap.add_argument("--speculative-ngram", type=int, default=0, metavar="K",
                    help="n-gram speculative decoding (vLLM's speculative_config method \"ngram\"): greedy requests verify up to K drafted tokens "
                         "per decode step, exactly the same tokens; the server then runs max_batch // (K + 1) requests at a time.  Sampled or "
                         "rule-carrying requests run unspeculated.  0 = off (default)")
    ap.add_argument("--prompt-lookup-min", type=int, default=2, metavar="N", help="shortest n-gram the drafter looks up (with --speculative-ngram)")
    ap.add_argument("--prompt-lookup-max", type=int, default=4, metavar="N", help="longest n-gram the drafter looks up (with --speculative-ngram)")
    return ap


def speculation_args(a) -> Optional[tuple]:
    """(k, min_n, max_n) of the parsed flags, or None when speculation is off.  ValueError on values the engine would refuse."""
    from .engine import MAX_NGRAM_SIZE, MAX_SPEC_DRAFTS, spec_usable_slots
    k = int(a.speculative_ngram)
    if k == 0:
        return None
    if not 1 <= k <= MAX_SPEC_DRAFTS:
        raise ValueError(f"--speculative-ngram must be in [0, {MAX_SPEC_DRAFTS}], got {k}")
    lo, hi = int(a.prompt_lookup_min), int(a.prompt_lookup_max)
    if not 1 <= lo <= hi <= MAX_NGRAM_SIZE:
        raise ValueError(f"need 1 <= --prompt-lookup-min <= --prompt-lookup-max <= {MAX_NGRAM_SIZE}, got {lo} and {hi}")
    if a.static_batching:
        raise ValueError("--speculative-ngram needs continuous batching: it cannot be combined with --static-batching")
    if spec_usable_slots(a.max_batch, k) < 1:
        raise ValueError(f"--speculative-ngram {k} needs --max-batch >= {k + 1}: a request takes {k + 1} rows of a decode step")
    return k, lo, hi


def main(argv: Optional[List[str]] = None):
    ap = build_arg_parser()
    a = ap.parse_args(argv)
    try:
        spec = speculation_args(a)
    except ValueError as e:
        ap.error(str(e))
    import uvicorn
    from .modeling import DotsOcrHipForCausalLM
    from .processing import DotsOcrProcessor
    if a.random_weights:
        model = DotsOcrHipForCausalLM.from_random(device=a.device, max_batch=a.max_batch, fp8_weights=a.fp8_weights, kv_cache_dtype=a.kv_cache_dtype)
        proc = DotsOcrProcessor(model.config, engine=model.engine)
    else:
        model = DotsOcrHipForCausalLM.from_pretrained(a.model_path, device=a.device, max_batch=a.max_batch, fp8_weights=a.fp8_weights,
                                                      kv_cache_dtype=a.kv_cache_dtype)
        proc = DotsOcrProcessor.from_pretrained(a.model_path, engine=model.engine)
    if spec is not None:                             # server-wide, before any slot is occupied; /health and the requests are unchanged
        model.engine.set_speculation(*spec)
    uvicorn.run(create_app(model, proc, a.served_model_name, a.max_batch, continuous=not a.static_batching,
                           allow_remote_images=a.allow_remote_images, allow_local_images=a.allow_local_images, look_ahead=a.look_ahead),
                host=a.host, port=a.port)


if __name__ == "__main__":
    main()
