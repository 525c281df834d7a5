"""``DotsOCRParser`` on the MI355X engine.

Same constructor keywords, methods, on-disk outputs and result dicts as the reference class
(dots_ocr/parser.py:17-322); the difference is what sits behind ``_inference_with_hf``: instead of
HF ``AutoModelForCausalLM`` + flash-attn on CUDA (parser.py:62-117) the model object is
``DotsOcrHipForCausalLM`` (hand-written gfx950 kernels behind a C ABI) and the processor is
``DotsOcrProcessor``.  ``use_hf=True`` therefore selects the HIP engine.  PDF parsing feeds ALL pages
of a document to the engine at once (the reference forces one page at a time, parser.py:279-282): with the
real engine as a pipeline — host threads prepare pages ahead of the GPU, the continuous batcher keeps the
sequence slots full, finished pages are post-processed (layout clean-up, drawing, markdown, file writes:
parser.py:171-262) on host threads while the GPU decodes the others.
The vLLM HTTP client path (use_hf=False, model/inference.py) talks to an external server and is kept
for API compatibility only.
"""
from __future__ import annotations

import json
import os
from typing import List, Optional

from .consts import MAX_PIXELS, MIN_PIXELS, image_extensions
from .format_transformer import layoutjson2md
from .image_utils import fetch_image, get_image_by_fitz_doc, smart_resize
from .layout_utils import draw_layout_on_image, post_process_output, pre_process_bboxes
from .prompts import dict_promptmode_to_prompt

_LAYOUT_MODES = ("prompt_layout_all_en", "prompt_layout_only_en", "prompt_grounding_ocr")


class PageText(str):
    """A page's response with what the loop guard found in it: repetition = {"period", "span"} when the page was ended
    because its output cycled (the text then keeps one copy of the cycle), else None."""
    repetition = None


class DotsOCRParser:
    """parse image or pdf file"""

    def __init__(self, protocol="http", ip="localhost", port=8000, model_name="model", temperature=0.1, top_p=1.0,
                 max_completion_tokens=16384, num_thread=64, dpi=200, output_dir="./output", min_pixels=None,
                 max_pixels=None, use_hf=False, model_path="./weights/DotsOCR", model=None, processor=None,
                 hf_max_new_tokens=24000, guided=False, no_repeat_ngram_size=None, no_repeat_ngram_window=None,
                 no_repeat_ngram_whitelist=None, speculative_ngram=None, prompt_lookup_min=2, prompt_lookup_max=4, stop=None,
                 speculative_rows=None, num_beams=None, length_penalty=1.0, speculative_guided=False, speculative_shaped=None,
                 prefill_chunk=None, enable_prefix_caching=False, speculative_logprobs=False, loop_guard=None, shared_prefix_attention=False,
                 prediction=None):
        self.dpi = dpi
        # predicted outputs, opt-in: a text the pages' output is expected to resemble — a string for every page, or a
        # callable (page_index, image) -> str | None.  The in-process model generates with it (generate(prediction_ids=): with
        # speculative_ngram the engine drafts from it, the tokens are those of a run without it); the server request carries OpenAI's
        # `prediction` field.  With the default None the request and the call are exactly what they were
        if prediction is not None and not (isinstance(prediction, str) or callable(prediction)):
            raise ValueError("prediction must be a string or a callable (page_index, image) -> str | None")
        if prediction is not None and num_beams and int(num_beams) != 1:
            raise ValueError("num_beams cannot be combined with prediction")
        self.prediction = prediction
        # shared-prefix attention, opt-in: the in-process model's rows that share prompt KV pages (beams, the prompts of one
        # page, prefix-cache hits) read each shared KV split once per decode step; the same tokens.  A server shares by its own
        # --shared-prefix-attention flag: requests carry nothing.  Accepted and inert with speculative_ngram
        self.shared_prefix_attention = bool(shared_prefix_attention)
        # loop guard, opt-in: True (loop_guard.LoopRule's defaults), a LoopRule or a dict of its fields.  The server request
        # carries `loop_guard`; the in-process model generates with it, the page's ids are cut back to one copy of the cycle
        # (loop_guard.trimmed) and its result carries "repetition".  With the default None the request and the call are exactly what they were.
        from .loop_guard import as_rule
        self.loop_guard = as_rule(loop_guard)
        if self.loop_guard is not None and num_beams and int(num_beams) != 1:
            raise ValueError("num_beams cannot be combined with loop_guard")
        # prefix caching, opt-in over prefill_chunk: the in-process model keeps the full KV pages of the pages it has read and
        # starts a page it meets again — with another prompt, or in a retry — behind them, keyed on the decoded image's bytes and size.  A
        # server caches by its own --enable-prefix-caching flag: requests carry nothing.
        self.enable_prefix_caching = bool(enable_prefix_caching)
        if self.enable_prefix_caching and prefill_chunk is None:
            raise ValueError("enable_prefix_caching needs prefill_chunk")
        # chunked prefill, opt-in: the in-process model fills every page's prompt in passes of prefill_chunk positions
        # between which the pages already running keep decoding (same tokens).  A server chunks by its own --enable-chunked-prefill flag, as
        # vLLM does: requests carry nothing.
        self.prefill_chunk = None if prefill_chunk is None else int(prefill_chunk)
        if self.prefill_chunk is not None and speculative_ngram:
            raise ValueError("prefill_chunk cannot be combined with speculative_ngram")
        # beam search, opt-in: every page is decoded by a group of num_beams beams and its best hypothesis returned (the
        # server request carries use_beam_search with temperature 0, the in-process model generates with num_beams).  It combines with
        # none of the other selection settings: they are refused, not dropped.
        self.num_beams = None if not num_beams or int(num_beams) == 1 else int(num_beams)
        self.length_penalty = float(length_penalty)
        if self.num_beams is not None and (guided or no_repeat_ngram_size or speculative_ngram or stop is not None):
            raise ValueError("num_beams cannot be combined with guided, no_repeat_ngram_size, speculative_ngram or stop")
        # stop strings, opt-in: the server request carries `stop`, the in-process model generates with stop_strings and the
        # text is cut where the match starts.  With the default None the request and the call are exactly what they were.
        self.stop = None
        if stop is not None:
            from .stop_strings import check_stop_strings
            self.stop = list(check_stop_strings(stop))
        # n-gram speculative decoding, opt-in: the in-process model generates with it (same tokens, fewer decode steps).  A
        # server speculates by its own --speculative-ngram flag, as vLLM does: requests carry nothing.
        self.speculative_ngram = None if not speculative_ngram else int(speculative_ngram)
        self.prompt_lookup_min, self.prompt_lookup_max = int(prompt_lookup_min), int(prompt_lookup_max)
        # which sequences beside the plain greedy ones speculate (generate(speculative_rows=): "sampled", "stop", a tuple, "all"); None =
        # greedy only.  A server decides by its own --speculative-rows flag.
        from .engine import spec_rows_flags
        if spec_rows_flags(speculative_rows) and not self.speculative_ngram:
            raise ValueError("speculative_rows needs speculative_ngram")
        self.speculative_rows = speculative_rows
        # may guided sequences verify drafts (generate(speculative_guided=), Engine.set_speculation_guided).  A server decides by its own
        # --speculative-guided flag.
        if speculative_guided and not self.speculative_ngram:
            raise ValueError("speculative_guided needs speculative_ngram")
        self.speculative_guided = bool(speculative_guided)
        # may sequences that return logprobs verify drafts (generate(speculative_logprobs=), Engine.set_speculation_logprobs).  A server
        # decides by its own --speculative-logprobs flag.
        if speculative_logprobs and not self.speculative_ngram:
            raise ValueError("speculative_logprobs needs speculative_ngram")
        self.speculative_logprobs = bool(speculative_logprobs)
        # which sequences whose logits are shaped verify drafts (generate(speculative_shaped=): "ngram", "rules", "penalties", a comma list,
        # a tuple, "all"; Engine.set_speculation_shaped); None = none.  A server decides by its own --speculative-shaped flag.
        from .engine import spec_shaped_flags
        if spec_shaped_flags(speculative_shaped) and not self.speculative_ngram:
            raise ValueError("speculative_shaped needs speculative_ngram")
        self.speculative_shaped = speculative_shaped if spec_shaped_flags(speculative_shaped) else None
        # no-repeat n-gram blocking, opt-in: the server request carries the three fields, the in-process model generates
        # with them.  With the default None the request and the call are exactly what they were.
        self.no_repeat_ngram_size = no_repeat_ngram_size
        self.no_repeat_ngram_window = no_repeat_ngram_window
        self.no_repeat_ngram_whitelist = None if no_repeat_ngram_whitelist is None else [int(t) for t in no_repeat_ngram_whitelist]
        # guided: opt-in guided decoding for the two layout prompt modes: the server request carries guided_layout, the
        # in-process model generates under guided.layout_schema().  Off by default: the output is then exactly what it was.
        self.guided = bool(guided)
        self.protocol, self.ip, self.port, self.model_name = protocol, ip, port, model_name
        self.temperature, self.top_p, self.max_completion_tokens = temperature, top_p, max_completion_tokens
        self.num_thread = num_thread
        self.output_dir = output_dir
        self.min_pixels, self.max_pixels = min_pixels, max_pixels
        self.model_path = model_path
        self.hf_max_new_tokens = hf_max_new_tokens
        self.use_hf = use_hf or model is not None
        if model is not None:                       # injected engine (tests, random-weight smoke runs)
            self.model, self.processor = model, processor
            from .processing import process_vision_info
            self.process_vision_info = process_vision_info
        elif self.use_hf:
            self._load_hf_model()
            print("use hf model, num_thread will be set to 1")
        else:
            print(f"use vllm model, num_thread will be set to {self.num_thread}")
        assert self.min_pixels is None or self.min_pixels >= MIN_PIXELS
        assert self.max_pixels is None or self.max_pixels <= MAX_PIXELS

    # ------------------------------------------------------------------ backend (the drop-in boundary)
    def _load_hf_model(self):
        from .modeling import DotsOcrHipForCausalLM
        from .processing import DotsOcrProcessor, process_vision_info
        self.model = DotsOcrHipForCausalLM.from_pretrained(self.model_path)
        self.processor = DotsOcrProcessor.from_pretrained(self.model_path, engine=self.model.engine)   # GPU image preprocessing
        self.process_vision_info = process_vision_info

    def _build_inputs(self, images, prompts):
        texts, flat = [], []
        for image, prompt in zip(images, prompts):
            messages = [{"role": "user", "content": [{"type": "image", "image": image}, {"type": "text", "text": prompt}]}]
            texts.append(self.processor.apply_chat_template(messages, tokenize=False, add_generation_prompt=True))
            imgs, _ = self.process_vision_info(messages)
            flat.extend(imgs)
        return self.processor(text=texts, images=flat, videos=None, padding=True, return_tensors="pt")

    def _guided_layout(self, prompts) -> bool:
        """guided decoding applies: the switch is on and every prompt is one of the layout modes' (their output is the layout array)"""
        layout = {dict_promptmode_to_prompt[m] for m in ("prompt_layout_all_en", "prompt_layout_only_en")}
        return self.guided and all(p in layout for p in prompts)

    def _loop_field(self) -> dict:
        """the server request's `loop_guard` field, when the guard is on.  The server ends the page at the firing token and says so on the
        choice; the helpers of the server path hand back the text alone, so such a page is neither cut back nor marked here"""
        if self.loop_guard is None:
            return {}
        import dataclasses
        return {"loop_guard": dataclasses.asdict(self.loop_guard)}

    def _prediction_text(self, page_index: int, image) -> Optional[str]:
        """the prediction of one page as text, or None"""
        if self.prediction is None:
            return None
        text = self.prediction(page_index, image) if callable(self.prediction) else self.prediction
        if text is not None and not isinstance(text, str):
            raise ValueError(f"the prediction of page {page_index} must be a string or None, got {type(text).__name__}")
        return text or None

    def _prediction_ids(self, page_index: int, image) -> Optional[list]:
        """... tokenised with the processor's tokenizer, without special tokens, and cut to what a sequence can hold"""
        text = self._prediction_text(page_index, image)
        if text is None:
            return None
        ids = [int(t) for t in self.processor.tokenizer.encode(text)]
        return ids[:int(getattr(self.model, "max_seq_len", len(ids)))] or None

    def _ngram_fields(self) -> dict:
        """the no_repeat_ngram_* settings that are set, under the names generate() and the server share"""
        return {k: v for k, v in (("no_repeat_ngram_size", self.no_repeat_ngram_size), ("no_repeat_ngram_window", self.no_repeat_ngram_window),
                                  ("no_repeat_ngram_whitelist", self.no_repeat_ngram_whitelist)) if v is not None}

    def _inference_batch_with_hf(self, images, prompts, page0: int = 0) -> List[str]:
        inputs = self._build_inputs(images, prompts)
        kw = self._ngram_fields()
        if self.prediction is not None:              # page0: the page index of images[0]
            kw["prediction_ids"] = [self._prediction_ids(page0 + i, im) for i, im in enumerate(images)]
        if self.speculative_ngram:
            kw.update(speculative_ngram=self.speculative_ngram, prompt_lookup_min=self.prompt_lookup_min, prompt_lookup_max=self.prompt_lookup_max)
            if self.speculative_rows is not None:
                kw["speculative_rows"] = self.speculative_rows
            if self.speculative_guided:
                kw["speculative_guided"] = True
            if self.speculative_logprobs:
                kw["speculative_logprobs"] = True
            if self.speculative_shaped is not None:
                kw["speculative_shaped"] = self.speculative_shaped
        if self._guided_layout(prompts):
            from .guided import layout_schema
            if getattr(self.model.engine, "token_bytes", None) is None:
                self.model.engine.set_token_bytes(self.processor.guide_token_bytes())
            kw["guided_json"] = layout_schema()
        if self.stop:
            if getattr(self.model.engine, "token_bytes", None) is None:
                self.model.engine.set_token_bytes(self.processor.guide_token_bytes())
            kw["stop_strings"] = self.stop
        if self.loop_guard is not None:
            kw["loop_guard"] = self.loop_guard
        if self.num_beams:
            kw.update(num_beams=self.num_beams, length_penalty=self.length_penalty, do_sample=False)
        if self.prefill_chunk is not None:
            kw["prefill_chunk"] = self.prefill_chunk
        if self.enable_prefix_caching:
            kw.update(enable_prefix_caching=True, image_keys=[self._image_key(im) for im in images])
        if self.shared_prefix_attention:
            kw["shared_prefix_attention"] = True
        generated = self.model.generate(**inputs, max_new_tokens=self.hf_max_new_tokens, **kw)
        trimmed, loops = self._cut_loops([out[len(inp):] for inp, out in zip(inputs.input_ids, generated)])
        texts = self.processor.batch_decode(trimmed, skip_special_tokens=True, clean_up_tokenization_spaces=False)
        return self._mark_loops(self._cut_at_stops(trimmed, texts), loops)

    @staticmethod
    def _image_key(image, grid=None) -> Optional[bytes]:
        """16 bytes that name a decoded image for the prefix cache: blake2b over its mode, size and bytes (and the grid it was resized to,
        where the caller knows it: generate() adds it itself)"""
        if image is None:
            return None
        import hashlib
        h = hashlib.blake2b(digest_size=16)
        h.update(repr((image.mode, image.size, None if grid is None else grid.tolist())).encode())
        h.update(image.tobytes())
        return h.digest()

    def _chunk_kw(self) -> dict:
        kw = {} if self.prefill_chunk is None else {"prefill_chunk": self.prefill_chunk}
        if self.shared_prefix_attention:
            kw["shared_prefix_attention"] = True
        return dict(kw, prefix_caching=True) if self.enable_prefix_caching else kw

    def _cut_loops(self, rows):
        """rows the loop guard ended (their last token is the firing one) cut back to one copy of the cycle -> (rows, the hits or None)"""
        if self.loop_guard is None:
            return rows, [None] * len(rows)
        from .loop_guard import last_loop, trimmed
        pad, hits = self.processor.tokenizer.pad_token_id, []
        rows = list(rows)
        for i, ids in enumerate(rows):
            toks = [int(t) for t in ids.tolist()]
            while toks and toks[-1] == pad:
                toks.pop()
            hits.append(last_loop(toks, self.loop_guard))
            if hits[-1] is not None:
                rows[i] = ids[:len(trimmed(toks, hits[-1]))]
        return rows, hits

    @staticmethod
    def _mark_loops(texts, loops) -> List[str]:
        out = []
        for text, hit in zip(texts, loops):
            if hit is not None:
                text = PageText(text)
                text.repetition = {"period": int(hit[1]), "span": int(hit[2])}
            out.append(text)
        return out

    def _cut_at_stops(self, trimmed, texts) -> List[str]:
        if self.stop:                               # the ids end at the token that completed a match: cut the text where the match starts
            from .stop_strings import first_stop, stopped_text
            tb, pad = self.model.engine.token_bytes.token, self.processor.tokenizer.pad_token_id
            for i, ids in enumerate(trimmed):
                toks = [int(t) for t in ids.tolist()]
                while toks and toks[-1] == pad:
                    toks.pop()
                hit = first_stop([tb(t) for t in toks], self.stop)
                if hit is not None:
                    texts[i] = stopped_text(toks, hit, tb)
        return texts

    # ------------------------------------------------------------------ several prompts over one page
    MAX_PROMPTS = 8                                  # prompts of one request (scheduler.ContinuousBatcher.MAX_SUFFIXES)

    def _inference_prompts_with_hf(self, image, prompts) -> List[str]:
        """one fan-out through model.generate(prompt_suffixes=): the page's tower and the prefill of what the prompts share run once"""
        import torch
        from .scheduler import split_common_prefix
        inputs = self._build_inputs([image], [prompts[0]])
        ids0 = inputs["input_ids"][0][inputs["attention_mask"][0].bool()].tolist()
        grids = inputs["image_grid_thw"].tolist()
        seqs = [ids0]
        for p in prompts[1:]:
            messages = [{"role": "user", "content": [{"type": "image", "image": image}, {"type": "text", "text": p}]}]
            seqs.append(self.processor.encode_prompt(self.processor.apply_chat_template(messages, tokenize=False, add_generation_prompt=True), grids))
        prefix, suffixes = split_common_prefix(seqs)
        if any(self.model.config.image_token_id in s for s in suffixes):
            raise ValueError("the prompts do not share the page: their common prefix does not cover every image token")
        kw = self._ngram_fields()
        if self.stop:
            if getattr(self.model.engine, "token_bytes", None) is None:
                self.model.engine.set_token_bytes(self.processor.guide_token_bytes())
            kw["stop_strings"] = self.stop
        if self.loop_guard is not None:
            kw["loop_guard"] = self.loop_guard
        dev = inputs["input_ids"].device
        generated = self.model.generate(input_ids=torch.tensor([prefix], dtype=torch.long, device=dev), pixel_values=inputs["pixel_values"],
                                        image_grid_thw=inputs["image_grid_thw"], max_new_tokens=self.hf_max_new_tokens,
                                        prompt_suffixes=suffixes, **kw)
        trimmed, loops = self._cut_loops([out[len(prefix):] for out in generated])
        texts = self.processor.batch_decode(trimmed, skip_special_tokens=True, clean_up_tokenization_spaces=False)
        return self._mark_loops(self._cut_at_stops(trimmed, texts), loops)

    def _inference_prompts_with_vllm(self, image, prompts) -> List[str]:
        """one request that carries the server's `prompts` field: choice i answers prompts[i]"""
        from dots_ocr.model.inference import inference_prompts_with_vllm
        extra = {**self._ngram_fields(), **({"stop": self.stop} if self.stop else {}), **self._loop_field()}
        return inference_prompts_with_vllm(image, prompts, model_name=self.model_name, protocol=self.protocol, ip=self.ip, port=self.port,
                                           temperature=self.temperature, top_p=self.top_p, max_completion_tokens=self.max_completion_tokens,
                                           **({"extra_body": extra} if extra else {}))

    def parse_image_regions(self, input_path, bboxes, save_dir=None, filename=None, fitz_preprocess=False):
        """Grounding OCR of many boxes of ONE image: the page is read once — one `prompts` request on the server path, one fan-out through
        model.generate(prompt_suffixes=) on the in-process path (groups of MAX_PROMPTS boxes) — instead of one tower and one prefill per
        box.  Returns one result per box, in order: what parse_image(..., prompt_mode="prompt_grounding_ocr", bbox=b) returns for it,
        saved as <filename>_box_<i>."""
        mode = "prompt_grounding_ocr"
        if self.num_beams or self.speculative_ngram:
            raise ValueError("parse_image_regions cannot be combined with num_beams or speculative_ngram")
        bboxes = [list(b) for b in bboxes]
        if not bboxes:
            return []
        origin_image = fetch_image(input_path)
        save_dir = save_dir or self.output_dir
        filename = filename or os.path.splitext(os.path.basename(str(input_path)))[0]
        os.makedirs(save_dir, exist_ok=True)
        image, first, mn, mx = self._prepare(origin_image, mode, "image", bboxes[0], fitz_preprocess)
        prompts = [first] + [self.get_prompt(mode, b, origin_image, image, min_pixels=mn, max_pixels=mx) for b in bboxes[1:]]
        responses = []
        for lo in range(0, len(prompts), self.MAX_PROMPTS):
            group = prompts[lo:lo + self.MAX_PROMPTS]
            if len(group) == 1:                     # a lone box is an ordinary request
                responses.append(self._inference_with_hf(image, group[0]) if self.use_hf else self._inference_with_vllm(image, group[0]))
            else:
                responses += self._inference_prompts_with_hf(image, group) if self.use_hf else self._inference_prompts_with_vllm(image, group)
        results = []
        for i, response in enumerate(responses):
            result = self._save(response, origin_image, image, mode, save_dir, f"{filename}_box_{i}", 0, mn, mx)
            result["file_path"] = input_path
            results.append(result)
        return results

    # ------------------------------------------------------------------ score given texts against a page
    def score_image(self, input_path, candidates, prompt_mode="prompt_layout_all_en", bbox=None, top_logprobs=0):
        """How probable is each of `candidates` (1 .. 8 texts) as the model's answer to this image under prompt_mode?  Nothing is
        generated: the page is read once and every candidate's tokens — and the EOS behind them — are scored teacher-forced, through the
        server's `score_candidates` field or, with use_hf, model.score.  Returns one {text, tokens, token_logprobs, cumulative_logprob,
        mean_logprob} per candidate, in order; with top_logprobs > 0 also top_logprobs: per token its [(token, logprob), ...]."""
        candidates = list(candidates)
        if not 1 <= len(candidates) <= self.MAX_PROMPTS or not all(isinstance(c, str) and c for c in candidates):
            raise ValueError(f"candidates must be 1 .. {self.MAX_PROMPTS} non-empty strings")
        origin_image = fetch_image(input_path)
        image, prompt, _, _ = self._prepare(origin_image, prompt_mode, "image", bbox, False)
        if not self.use_hf:
            from dots_ocr.model.inference import score_with_vllm
            choices = score_with_vllm(image, prompt, candidates, model_name=self.model_name, protocol=self.protocol, ip=self.ip, port=self.port,
                                      top_logprobs=top_logprobs)
            if choices is None:
                return None
            out = []
            for cand, ch in zip(candidates, choices):
                content = ch["logprobs"]["content"]
                lps = [float(e["logprob"]) for e in content]
                out.append({"text": cand, "tokens": [e["token"] for e in content], "token_logprobs": lps,
                            "cumulative_logprob": float(ch["cumulative_logprob"]), "mean_logprob": sum(lps) / max(1, len(lps))})
                if top_logprobs:
                    out[-1]["top_logprobs"] = [[(t["token"], float(t["logprob"])) for t in e["top_logprobs"]] for e in content]
            return out
        import numpy as np
        import torch
        inputs = self._build_inputs([image], [prompt])
        P = inputs["input_ids"][0][inputs["attention_mask"][0].bool()].tolist()
        if len(P) < 2 or P[-1] == self.model.config.image_token_id:
            raise ValueError("the chat template must end in a text token behind at least one other token")
        tok = self.processor.tokenizer
        eos = int(self.model.config.eos_token_ids[0])
        fed = [[P[-1]] + [int(t) for t in tok.encode(c)] + [eos] for c in candidates]      # every candidate token, and the EOS, gets an entry
        scores = self.model.score(torch.tensor([P[:-1]], dtype=torch.long), inputs["pixel_values"], inputs["image_grid_thw"], candidates=fed,
                                  top_logprobs=top_logprobs)
        out = []
        for cand, ids, (tok_lp, top_ids, top_lp) in zip(candidates, fed, scores):
            lps = [float(v) for v in tok_lp]
            out.append({"text": cand, "tokens": [tok.decode([t], skip_special_tokens=False) for t in ids[1:]], "token_logprobs": lps,
                        "cumulative_logprob": float(np.asarray(tok_lp, np.float32).astype(np.float64).sum()), "mean_logprob": sum(lps) / max(1, len(lps))})
            if top_logprobs:
                out[-1]["top_logprobs"] = [[(tok.decode([int(i)], skip_special_tokens=False), float(v)) for i, v in zip(top_ids[j][:top_logprobs],
                                                                                                                       top_lp[j][:top_logprobs])]
                                           for j in range(len(lps))]
        return out

    def _inference_with_hf(self, image, prompt, page_idx: int = 0) -> str:
        return self._inference_batch_with_hf([image], [prompt], page_idx)[0]

    def _inference_with_vllm(self, image, prompt, page_idx: int = 0):
        from dots_ocr.model.inference import inference_with_vllm
        pred = self._prediction_text(page_idx, image)
        extra = {**({"guided_layout": True} if self._guided_layout([prompt]) else {}), **self._ngram_fields(),
                 **({"prediction": {"type": "content", "content": pred}} if pred else {}),
                 **({"stop": self.stop} if self.stop else {}), **self._loop_field(),
                 **({"use_beam_search": True, "beam_width": self.num_beams, "length_penalty": self.length_penalty} if self.num_beams else {})}
        return inference_with_vllm(image, prompt, model_name=self.model_name, protocol=self.protocol, ip=self.ip,
                                   port=self.port, temperature=0.0 if self.num_beams else self.temperature,
                                   top_p=1.0 if self.num_beams else self.top_p,
                                   max_completion_tokens=self.max_completion_tokens,
                                   **({"extra_body": extra} if extra else {}))

    # ------------------------------------------------------------------ per-page pipeline
    def get_prompt(self, prompt_mode, bbox=None, origin_image=None, image=None, min_pixels=None, max_pixels=None):
        prompt = dict_promptmode_to_prompt[prompt_mode]
        if prompt_mode == "prompt_grounding_ocr":
            assert bbox is not None
            box = pre_process_bboxes(origin_image, [bbox], input_width=image.width, input_height=image.height,
                                     min_pixels=min_pixels, max_pixels=max_pixels)[0]
            prompt = prompt + str(box)
        return prompt

    def _prepare(self, origin_image, prompt_mode, source, bbox, fitz_preprocess):
        min_pixels, max_pixels = self.min_pixels, self.max_pixels
        if prompt_mode == "prompt_grounding_ocr":
            min_pixels, max_pixels = min_pixels or MIN_PIXELS, max_pixels or MAX_PIXELS
        if min_pixels is not None:
            assert min_pixels >= MIN_PIXELS, f"min_pixels should >= {MIN_PIXELS}"
        if max_pixels is not None:
            assert max_pixels <= MAX_PIXELS, f"max_pixels should <= {MAX_PIXELS}"
        src = get_image_by_fitz_doc(origin_image, target_dpi=self.dpi) if (source == "image" and fitz_preprocess) else origin_image
        image = fetch_image(src, min_pixels=min_pixels, max_pixels=max_pixels)
        prompt = self.get_prompt(prompt_mode, bbox, origin_image, image, min_pixels=min_pixels, max_pixels=max_pixels)
        return image, prompt, min_pixels, max_pixels

    def _save(self, response, origin_image, image, prompt_mode, save_dir, save_name, page_idx, min_pixels, max_pixels):
        ih, iw = smart_resize(image.height, image.width)
        result = {"page_no": page_idx, "input_height": ih, "input_width": iw}
        if getattr(response, "repetition", None):   # the loop guard ended the page
            result["repetition"] = dict(response.repetition)
        j = os.path.join(save_dir, f"{save_name}.json")
        jpg = os.path.join(save_dir, f"{save_name}.jpg")
        md = os.path.join(save_dir, f"{save_name}.md")

        def write(path, text):
            with open(path, "w", encoding="utf-8") as f:
                f.write(text)

        if prompt_mode in _LAYOUT_MODES:
            cells, filtered = post_process_output(response, prompt_mode, origin_image, image, min_pixels=min_pixels, max_pixels=max_pixels)
            if filtered and prompt_mode != "prompt_layout_only_en":
                write(j, json.dumps(response, ensure_ascii=False))
                origin_image.save(jpg)
                write(md, cells)
                result.update({"layout_info_path": j, "layout_image_path": jpg, "md_content_path": md, "filtered": True})
                return result
            try:
                drawn = draw_layout_on_image(origin_image, cells)
            except Exception as e:
                print(f"Error drawing layout on image: {e}")
                drawn = origin_image
            write(j, json.dumps(cells, ensure_ascii=False))
            drawn.save(jpg)
            result.update({"layout_info_path": j, "layout_image_path": jpg})
            if prompt_mode != "prompt_layout_only_en":
                nohf = os.path.join(save_dir, f"{save_name}_nohf.md")
                write(md, layoutjson2md(origin_image, cells, text_key="text"))
                write(nohf, layoutjson2md(origin_image, cells, text_key="text", no_page_hf=True))
                result.update({"md_content_path": md, "md_content_nohf_path": nohf})
        else:
            origin_image.save(jpg)
            write(md, response)
            result.update({"layout_image_path": jpg, "md_content_path": md})
        return result

    def _parse_single_image(self, origin_image, prompt_mode, save_dir, save_name, source="image", page_idx=0, bbox=None,
                            fitz_preprocess=False):
        image, prompt, mn, mx = self._prepare(origin_image, prompt_mode, source, bbox, fitz_preprocess)
        response = self._inference_with_hf(image, prompt, page_idx) if self.use_hf else self._inference_with_vllm(image, prompt, page_idx)
        if source == "pdf":
            save_name = f"{save_name}_page_{page_idx}"
        return self._save(response, origin_image, image, prompt_mode, save_dir, save_name, page_idx, mn, mx)

    def parse_image(self, input_path, filename, prompt_mode, save_dir, bbox=None, fitz_preprocess=False):
        origin_image = fetch_image(input_path)
        result = self._parse_single_image(origin_image, prompt_mode, save_dir, filename, source="image", bbox=bbox,
                                          fitz_preprocess=fitz_preprocess)
        result["file_path"] = input_path
        return [result]

    def _parse_pages_pipelined(self, images, filename, prompt_mode, save_dir, input_path):
        """prepare (host threads) -> preprocess + admit (this thread, GPU) -> decode (GPU, continuous batching) -> post-process
        (host threads).  Only this thread talks to the engine (one handle per GPU, not thread-safe)."""
        from multiprocessing.pool import ThreadPool
        from .scheduler import ContinuousBatcher, Request
        from .modeling import resolve_sampling
        engine = self.model.engine
        # generate(**inputs, max_new_tokens=...) (parser.py:110): greedy unless the checkpoint's generation_config.json samples
        t, p_ = resolve_sampling(getattr(self.model, "generation_config", None))
        engine.set_sampling(t, p_, 0)
        eos = list(self.model.config.eos_token_ids)
        cb = ContinuousBatcher(engine, eos_ids=eos, **self._chunk_kw())
        n = len(images)
        results = [None] * n
        with ThreadPool(max(1, min(8, self.num_thread, n))) as prep_pool, ThreadPool(max(1, min(8, self.num_thread, n))) as post_pool:
            prep = [prep_pool.apply_async(self._prepare, (im, prompt_mode, "pdf", None, False)) for im in images]
            prepared, posts, nxt = {}, {}, 0
            while nxt < n or not cb.idle:
                # admit pages in order, without stalling the GPU on a page whose host preparation is still running
                while nxt < n and len(cb.pending) < cb.n_slots and (prep[nxt].ready() or cb.idle):
                    image, prompt, mn, mx = prepared[nxt] = prep[nxt].get()
                    inputs = self._build_inputs([image], [prompt])
                    ids = inputs["input_ids"][0]
                    ids = ids[inputs["attention_mask"][0].bool()].cpu().numpy()
                    grid = None if "image_grid_thw" not in inputs else inputs["image_grid_thw"].cpu().numpy()
                    cb.submit(Request(ids, inputs.get("pixel_values"), grid, self.hf_max_new_tokens, tag=nxt,
                                      image_key=self._image_key(image, grid) if self.enable_prefix_caching and grid is not None else None,
                                      prediction=self._prediction_ids(nxt, image)))
                    nxt += 1
                for _, req, toks in cb.step():
                    i = req.tag
                    toks = [int(t) for t in toks]
                    text = self.processor.batch_decode([toks], skip_special_tokens=True, clean_up_tokenization_spaces=False)[0]
                    image, _, mn, mx = prepared.pop(i)
                    posts[i] = post_pool.apply_async(self._save, (text, images[i], image, prompt_mode, save_dir, f"{filename}_page_{i}", i, mn, mx))
            for i, fut in posts.items():
                results[i] = fut.get()
                results[i]["file_path"] = input_path
        return results

    def parse_pages(self, images, filename, prompt_mode, save_dir, input_path=None):
        """All pages of one document through the engine at once — the caller-side half of page batching (SURVEY §8(f)
        rows 2 and 4): pipelined over the engine's sequence slots when the model has them, else ONE batched generate."""
        if self.use_hf and hasattr(getattr(self.model, "engine", None), "slots_prefill") and len(images) > 1:
            return self._parse_pages_pipelined(images, filename, prompt_mode, save_dir, input_path)
        prepared = [self._prepare(im, prompt_mode, "pdf", None, False) for im in images]
        if self.use_hf:
            responses = self._inference_batch_with_hf([p[0] for p in prepared], [p[1] for p in prepared])
        else:
            from multiprocessing.pool import ThreadPool
            with ThreadPool(max(1, min(len(images), self.num_thread))) as pool:
                responses = pool.starmap(self._inference_with_vllm, [(p[0], p[1], i) for i, p in enumerate(prepared)])
        results = []
        for i, (im, p, resp) in enumerate(zip(images, prepared, responses)):
            r = self._save(resp, im, p[0], prompt_mode, save_dir, f"{filename}_page_{i}", i, p[2], p[3])
            r["file_path"] = input_path
            results.append(r)
        return results

    def parse_pdf(self, input_path, filename, prompt_mode, save_dir):
        from .doc_utils import load_images_from_pdf
        print(f"loading pdf: {input_path}")
        images = load_images_from_pdf(input_path, dpi=self.dpi)
        print(f"Parsing PDF with {len(images)} pages in one batch...")
        return self.parse_pages(images, filename, prompt_mode, save_dir, input_path=input_path)

    def parse_file(self, input_path, output_dir="", prompt_mode="prompt_layout_all_en", bbox=None, fitz_preprocess=False):
        output_dir = os.path.abspath(output_dir or self.output_dir)
        filename, ext = os.path.splitext(os.path.basename(input_path))
        save_dir = os.path.join(output_dir, filename)
        os.makedirs(save_dir, exist_ok=True)
        if ext == ".pdf":
            results = self.parse_pdf(input_path, filename, prompt_mode, save_dir)
        elif ext in image_extensions:
            results = self.parse_image(input_path, filename, prompt_mode, save_dir, bbox=bbox, fitz_preprocess=fitz_preprocess)
        else:
            raise ValueError(f"file extension {ext} not supported, supported extensions are {image_extensions} and pdf")
        print(f"Parsing finished, results saving to {save_dir}")
        with open(os.path.join(output_dir, os.path.basename(filename) + ".jsonl"), "w", encoding="utf-8") as w:
            for r in results:
                w.write(json.dumps(r, ensure_ascii=False) + "\n")
        return results


def main(argv=None):
    """The reference's command line (dots_ocr/parser.py:326-430), same arguments and defaults: `python dots_ocr/parser.py
    <pdf or image> [--use_hf true] ...`.  --use_hf selects the in-process MI355X engine, otherwise the OpenAI-compatible
    server at --protocol://--ip:--port (dots_ocr_amd.server, or any vLLM deployment)."""
    import argparse
    from .prompts import dict_promptmode_to_prompt
    ap = argparse.ArgumentParser(description="dots.ocr Multilingual Document Layout Parser")
    ap.add_argument("input_path", type=str, help="Input PDF/image file path")
    ap.add_argument("--output", type=str, default="./output", help="Output directory (default: ./output)")
    ap.add_argument("--prompt", choices=list(dict_promptmode_to_prompt.keys()), type=str, default="prompt_layout_all_en",
                    help="prompt to query the model, different prompts for different tasks")
    ap.add_argument("--bbox", type=int, nargs=4, metavar=("x1", "y1", "x2", "y2"), help="needed for prompt_grounding_ocr")
    ap.add_argument("--protocol", type=str, choices=["http", "https"], default="http")
    ap.add_argument("--ip", type=str, default="localhost")
    ap.add_argument("--port", type=int, default=8000)
    ap.add_argument("--model_name", type=str, default="model")
    ap.add_argument("--temperature", type=float, default=0.1)
    ap.add_argument("--top_p", type=float, default=1.0)
    ap.add_argument("--dpi", type=int, default=200)
    ap.add_argument("--max_completion_tokens", type=int, default=16384)
    ap.add_argument("--num_thread", type=int, default=16)
    ap.add_argument("--no_fitz_preprocess", action="store_true",
                    help="skip the PDF round trip that re-renders low-dpi images at --dpi (needs PyMuPDF)")
    ap.add_argument("--min_pixels", type=int, default=None)
    ap.add_argument("--max_pixels", type=int, default=None)
    ap.add_argument("--use_hf", type=bool, default=False)
    a = ap.parse_args(argv)
    parser = DotsOCRParser(protocol=a.protocol, ip=a.ip, port=a.port, model_name=a.model_name, temperature=a.temperature, top_p=a.top_p,
                           max_completion_tokens=a.max_completion_tokens, num_thread=a.num_thread, dpi=a.dpi, output_dir=a.output,
                           min_pixels=a.min_pixels, max_pixels=a.max_pixels, use_hf=a.use_hf)
    fitz_preprocess = not a.no_fitz_preprocess
    if fitz_preprocess:
        print("Using fitz preprocess for image input, check the change of the image pixels")
    return parser.parse_file(a.input_path, prompt_mode=a.prompt, bbox=a.bbox, fitz_preprocess=fitz_preprocess)


if __name__ == "__main__":
    main()
