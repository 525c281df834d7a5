"""``DotsOcrHipForCausalLM`` — the object DotsOCRParser installs as ``self.model``.

It honours the one model call the reference makes, ``self.model.generate(**inputs,
max_new_tokens=...) -> LongTensor[B, T+n]`` (dots_ocr/parser.py:110; demo/demo_hf.py:44), and the
``from_pretrained`` entry of parser.py:68-74, but everything underneath is the HIP engine: ViT,
merger, prefill and the hipGraph'd greedy decode loop run inside ``dots_generate`` on one GPU.

Greedy decoding only (``do_sample=False``): sampling at temperature is a SURVEY §8(f) "next" row.
There is no CPU fallback — constructing the model without the built library or without a GPU raises.
"""
from __future__ import annotations

import os
from dataclasses import dataclass
from pathlib import Path
from typing import Optional, Sequence

import numpy as np

from .config import DotsConfig
from .engine import SPEC_ROWS, Engine, LogitRules, NgramRule, SamplingParams, spec_rows_flags, spec_shaped_flags
from .row_features import apply_row, clear_rows
from .weights import load_state_dict, random_state_dict


def resolve_sampling(generation_config: dict, do_sample=None, temperature=None, top_p=None):
    """HF semantics: explicit generate() arguments win, otherwise the checkpoint's generation_config.json decides
    (GenerationMixin.generate merges it the same way; the reference calls generate(**inputs, max_new_tokens=...) only,
    parser.py:110).  Returns (temperature, top_p) for the engine: temperature 0 = greedy."""
    g = generation_config or {}
    do_sample = g.get("do_sample", False) if do_sample is None else do_sample
    temperature = g.get("temperature", 1.0) if temperature is None else temperature
    top_p = g.get("top_p", 1.0) if top_p is None else top_p
    if not do_sample or temperature is None or temperature <= 0:
        return 0.0, 1.0
    return float(temperature), float(min(max(top_p if top_p is not None else 1.0, 1e-6), 1.0))


def plan_batches(patches_per_seq: Sequence[int], max_batch: int, max_patches: int):
    """Consecutive sequences -> engine batches of <= max_batch sequences and <= max_patches vision patches (ViT workspace).
    A single sequence larger than the patch budget is rejected (it cannot be split: attention spans the whole image)."""
    batches, cur, used = [], [], 0
    for i, n in enumerate(patches_per_seq):
        if n > max_patches:
            raise ValueError(f"sequence {i} has {n} vision patches, more than the engine's max_patches={max_patches}")
        if cur and (len(cur) == max_batch or used + n > max_patches):
            batches.append(cur)
            cur, used = [], 0
        cur.append(i)
        used += n
    if cur:
        batches.append(cur)
    return batches


def split_kv_scales(state_dict, num_layers: int, num_kv_heads: int):
    """The fp8-KV checkpoint convention: per-layer scalars model.layers.{i}.self_attn.k_scale / v_scale.  Returns (the state dict
    without them, scales [num_layers, num_kv_heads, 2] fp32 broadcast over the kv heads — 1.0 where a layer has none — or None when the
    checkpoint carries no such tensor).  The scale tensors are never engine weights."""
    names = {f"model.layers.{i}.self_attn.{kv}_scale": (i, j) for i in range(num_layers) for j, kv in enumerate(("k", "v"))}
    if not any(n in names for n in state_dict):
        return state_dict, None
    scales = np.ones((num_layers, num_kv_heads, 2), np.float32)
    rest = {}
    for n, t in state_dict.items():
        if n in names:
            i, j = names[n]
            v = np.asarray(t.detach().float().cpu() if hasattr(t, "detach") else t, dtype=np.float32).reshape(-1)
            if v.size != 1:
                raise ValueError(f"{n}: expected one scale per layer, got {v.size} values")
            scales[i, :, j] = v[0]
        else:
            rest[n] = t
    return rest, scales


@dataclass
class CallSettings:
    """What one generate() call gives every sequence besides its SamplingParams, and how the call runs: _generate's one record."""
    rules: Optional[LogitRules] = None           # the same LogitRules, guide handle, NgramRule and stop strings on every row
    guide: Optional[int] = None
    ngram: Optional[NgramRule] = None
    stop: Optional[tuple] = None
    loop: Optional[object] = None                # loop_guard.LoopRule
    nrs: int = 1                                 # num_return_sequences
    beam: Optional[tuple] = None                 # (num_beams, length_penalty)
    suffixes: Optional[list] = None              # prompt_suffixes
    prefill_chunk: Optional[int] = None
    shared_prefix_attention: bool = False        # engine-wide for the call's continuous run
    image_keys: Optional[list] = None            # one entry per sequence when prefix caching is on, else None
    streamer: object = None
    predictions: Optional[list] = None           # prediction_ids: one token list or None per sequence


class DotsOcrHipForCausalLM:
    def __init__(self, cfg: DotsConfig, state_dict, device: int = 0, max_batch: int = 8, max_seq_len: int = 32768,
                 max_patches: Optional[int] = None, fp8_weights: bool = False, kv_cache_dtype: Optional[str] = None):
        """fp8_weights: quantise the linears to e4m3 with per-output-channel scales at load time (DotsConfig.fp8_weights of the C ABI;
        DOTS_OCR_FP8=1 in the environment turns it on for callers that cannot pass the keyword, e.g. DotsOCRParser(use_hf=True)).
        kv_cache_dtype: "bf16" or "fp8" (e4m3fn paged KV cache, DotsConfig.kv_cache_dtype); None = $DOTS_OCR_KV_CACHE_DTYPE, unset = bf16.
        The checkpoint's self_attn.k_scale / v_scale tensors, if any, become the fp8 cache's scales (split_kv_scales)."""
        self.config = cfg
        self.device_index = device
        max_patches = max_patches or max(max_batch * 19824 + 64, 57600 + 64)
        fp8_weights = bool(fp8_weights) or os.environ.get("DOTS_OCR_FP8", "0") not in ("", "0")
        state_dict, kv_scales = split_kv_scales(state_dict, cfg.num_hidden_layers, cfg.num_key_value_heads)
        self.engine = Engine(cfg, device=device, max_batch=max_batch, max_seq_len=max_seq_len, max_patches=max_patches, fp8_weights=fp8_weights,
                             kv_cache_dtype=kv_cache_dtype)
        self.engine.load_state_dict(state_dict)
        if kv_scales is not None:
            self.engine.set_kv_scales(kv_scales)
        self.max_batch = max_batch
        self.max_seq_len = max_seq_len
        self.max_patches = max_patches
        self.generation_config = {"do_sample": False, "eos_token_id": list(cfg.eos_token_ids), "pad_token_id": cfg.pad_token_id}

    # ------------------------------------------------------------------ constructors
    @classmethod
    def from_pretrained(cls, model_path, device_map=None, torch_dtype=None, attn_implementation=None,
                        trust_remote_code=None, device: Optional[int] = None, **kw):
        """Accepts (and ignores) the HF keyword arguments the reference passes at parser.py:68-74."""
        model_path = Path(model_path)
        cfg = DotsConfig.from_pretrained(model_path)
        if device is None:
            device = int(os.environ.get("LOCAL_RANK", "0"))
        model = cls(cfg, load_state_dict(model_path), device=device, **kw)
        gen = model_path / "generation_config.json"
        if gen.exists():                                   # sampling defaults of the checkpoint (HF merges them into generate())
            import json
            g = json.loads(gen.read_text())
            for k in ("do_sample", "temperature", "top_p"):
                if k in g:
                    model.generation_config[k] = g[k]
        return model

    @classmethod
    def from_random(cls, cfg: Optional[DotsConfig] = None, seed: int = 0, device: int = 0, **kw):
        cfg = cfg or DotsConfig()
        return cls(cfg, random_state_dict(cfg, seed=seed), device=device, **kw)

    def eval(self):
        return self

    @property
    def device(self):
        import torch
        return torch.device("cuda", self.device_index)

    # ------------------------------------------------------------------ generate
    def generate(self, input_ids=None, attention_mask=None, pixel_values=None, image_grid_thw=None,
                 max_new_tokens: int = 128, do_sample: Optional[bool] = None, temperature: Optional[float] = None,
                 top_p: Optional[float] = None, seed: int = 0, eos_token_id=None, pad_token_id=None, continuous: Optional[bool] = None,
                 top_k: Optional[int] = None, repetition_penalty: Optional[float] = None, frequency_penalty: Optional[float] = None,
                 presence_penalty: Optional[float] = None, logit_bias=None, allowed_token_ids=None, min_tokens: int = 0,
                 stop_token_ids=None, ignore_eos: bool = False, guided_regex=None, guided_choice=None, guided_json=None,
                 guided_whitespace_pattern=None, no_repeat_ngram_size: Optional[int] = None, no_repeat_ngram_window: Optional[int] = None,
                 no_repeat_ngram_whitelist=None, speculative_ngram: Optional[int] = None, prompt_lookup_min: int = 2, prompt_lookup_max: int = 4,
                 num_return_sequences: int = 1, stop_strings=None, speculative_rows=None, num_beams: Optional[int] = None,
                 length_penalty: float = 1.0, early_stopping=None, speculative_guided: bool = False, prompt_suffixes=None, speculative_shaped=None,
                 prefill_chunk: Optional[int] = None, enable_prefix_caching: bool = False, image_keys=None, speculative_logprobs: bool = False, streamer=None,
                 loop_guard=None, shared_prefix_attention: bool = False, prediction_ids=None, **_):
        """HF-shaped generate.  do_sample / temperature / top_p default to the checkpoint's generation_config.json (greedy when it
        is absent); with sampling on, tokens are drawn on the GPU from softmax(logits / temperature) restricted to the top_p
        nucleus, reproducibly from `seed`.  Returns LongTensor
        [B, T + n]: the (padded) prompt followed by the new tokens, positions after a sequence's EOS filled with pad_token_id.

        More sequences than engine slots (B > max_batch) run with continuous batching: a slot is refilled with the next
        sequence as soon as its page hits EOS instead of waiting for the slowest page of a static batch
        (`continuous=True/False` forces either mode; greedy results are identical).

        top_k / repetition_penalty (HF) and frequency_penalty / presence_penalty (OpenAI), when given with a non-neutral value, switch
        to per-row selection (Engine.set_row_sampling): sequence b is drawn with seed + b, whatever row or batch it lands
        in; the rows are cleared afterwards.  These keys are deliberately not read from generation_config.json: that would change the
        default output of existing checkpoints.

        logit_bias ({id: value}, -inf = a ban) / allowed_token_ids / min_tokens / stop_token_ids / ignore_eos (vLLM SamplingParams) give
        every sequence the same LogitRules (Engine.set_row_logit_rules) and switch to per-row selection in the same way;
        a stop id ends its sequence as an EOS does and is kept as its last token.

        guided_regex / guided_choice / guided_json (at most one; guided_whitespace_pattern with the last) compile to one guide that every
        sequence follows on the GPU (dots_ocr_amd/guided.py, Engine.set_row_guide); the engine needs its token bytes first
        (Engine.set_token_bytes).  A sequence ends with an EOS id once its text matches; cut at max_new_tokens it is a prefix of a match.

        no_repeat_ngram_size (n >= 1; None or 0 = off) with no_repeat_ngram_window (0 / None = the whole output) and
        no_repeat_ngram_whitelist (token ids never banned) give every sequence the same NgramRule (Engine.set_row_ngram): a
        sequence never completes an n-gram its own OUTPUT already holds.  Unlike HF generate, the prompt is not part of the history.

        speculative_ngram (k >= 1; None or 0 = off) with prompt_lookup_min / prompt_lookup_max (vLLM's speculative_config names) runs the
        call with n-gram speculative decoding (Engine.set_speculation): it takes the continuous path, where a greedy
        sequence verifies up to k drafted tokens per decode step, max_batch // (k + 1) sequences at a time.  The tokens are exactly
        those of the call without it; sampled or rule-carrying sequences simply run unspeculated.  The engine is left with speculation
        off.

        speculative_rows (with speculative_ngram; None = the above) lets more sequences verify drafts: "sampled", "stop", a tuple of
        both, or "all" (Engine.set_speculation_rows).  With "stop" a greedy sequence with stop_strings speculates and ends at the same
        token.  With "sampled" a sampled call (temperature > 0) without penalties speculates: every sequence is then drawn by the
        per-row sampler with seed + b (as a call with top_k is) instead of the engine-wide one, and its tokens are exactly those of the
        same call on an engine that does not speculate.  Sequences with penalties, logit rules or an n-gram rule run
        unspeculated without speculative_shaped, and so do guided ones without speculative_guided.  The engine is left with the setting off.

        speculative_guided (with speculative_ngram; False = the above) lets a sequence that follows a guide verify drafts too
        (Engine.set_speculation_guided): every draft row is selected under the state its guide would hold there, so the tokens are
        again exactly those of the call without it.  A sampled guided call also needs speculative_rows "sampled", one with
        stop_strings "stop".  The engine is left with the setting off.

        speculative_logprobs (with speculative_ngram; False = a sequence that returns logprobs runs unspeculated) lets such a sequence
        verify drafts too (Engine.set_speculation_logprobs): the logprobs of every accepted token are reduced from its draft row's raw
        logits and land at the token's own position, bit for bit the values of the call without it.  The engine is left with the
        setting off.

        speculative_shaped (with speculative_ngram; None = the above) lets sequences whose logits are shaped verify drafts
        (Engine.set_speculation_shaped): "ngram" (no_repeat_ngram_size), "rules" (logit_bias, allowed_token_ids, min_tokens,
        stop_token_ids, ignore_eos), "penalties" (repetition / frequency / presence penalty; such a call also needs speculative_rows
        "sampled"), a comma list or a tuple of them, or "all".  Every draft row is selected under the history, the output counts and
        the output index the sequence would have there, so the tokens are again exactly those of the call without it.  The engine is
        left with the setting off.

        prediction_ids (one list of token ids or None per sequence) hands each sequence a PREDICTION, a text its output is expected to
        resemble.  With speculative_ngram the engine drafts from it on the GPU and re-aligns after the output diverges;
        the returned tokens are exactly those of the call without it.  Without speculative_ngram it is carried and inert.  It takes the
        continuous path and one sequence per prompt: not with num_return_sequences > 1, num_beams, prompt_suffixes or continuous=False.

        stop_strings (HF's name: a str or a list of at most 16 str of at most 64 UTF-8 bytes) ends a sequence on the GPU at the token that
        completes one of them in its generated text (Engine.set_row_stop; with min_tokens, no match is taken below it).  The
        returned ids end at that token, as HF's do; cutting the TEXT at the match is the caller's (stop_strings.cut_text).  The engine
        needs its token bytes first (Engine.set_token_bytes).

        num_return_sequences (n >= 1, HF's name) returns n sequences per prompt from one vision tower and one prefill of it (parallel
        sampling: Engine.slots_fork): LongTensor [B * n, T + new], row i * n + j = sequence j of prompt i as HF lays it out,
        drawn with seed + i * n + j.  It runs on the continuous path; continuous=False with n > 1 is a ValueError.

        num_beams (2 .. 8; None or 1 = off) runs beam search (Engine.slots_beam): every prompt becomes a group of num_beams
        beams over one tower and one prefill, and its num_return_sequences (<= num_beams) best hypotheses come back best first, laid out
        as above, ranked by cum / max(1, len) ** length_penalty.  These are vLLM's beam-search semantics with HF's length normalisation,
        not HF's BeamSearchScorer: early_stopping is not offered (given, it raises), and the call is refused — nothing is silently
        dropped — together with sampling (a temperature > 0, top_k, penalties), logit rules, a guide, an n-gram rule, stop strings,
        speculation or continuous=False.

        prompt_suffixes ([[ids...], ...], 2 .. 8 lists; one input row only) reads several prompts off one page (Engine.slots_extend,
        DESIGN §6.11): input_ids is the prefix they share — the image and whatever text comes before the prompts part ways — and
        sequence j continues prefix + prompt_suffixes[j] from one tower, one prefill of the prefix and one extend.  Returns LongTensor
        [m, T + new]: row j = the prefix followed by the new tokens of suffix j (the suffix ids are not repeated), drawn with seed + j.
        It runs on the continuous path and is refused together with num_return_sequences > 1, num_beams, penalties, speculation or
        continuous=False.

        prefill_chunk (N, a multiple of 64 and at most the engine's max_prefill_tokens; None = off) fills every prompt in passes of N
        positions between which the sequences already running keep decoding (ContinuousBatcher(prefill_chunk=)), and
        admits prompts longer than the prefill workspace.  The tokens do not depend on N.  It runs on the continuous path and is refused
        together with speculative_ngram or continuous=False.

        enable_prefix_caching (with prefill_chunk) keeps the full KV pages of the prompts it fills, in this call and in later ones, and
        starts a prompt that begins with the same tokens and the same image behind them (ContinuousBatcher(prefix_caching=True), DESIGN
        §6.13): the same tokens as without it.  image_keys: per sequence 16 bytes that name its image (or None) — the caller's promise that
        equal keys mean equal pixels and grid, for instance a digest of the decoded image's bytes and size; a sequence with an image and
        no key bypasses the cache.

        shared_prefix_attention=True lets the rows of the call that share prompt KV pages — num_return_sequences > 1, num_beams,
        prompt_suffixes, prefix-cache hits — read each shared KV split once per decode step (ContinuousBatcher(shared_prefix_attention=True),
        DESIGN §6.17): the same tokens and logprobs as without it.  Nothing is refused: on the static path and with speculative_ngram it
        is accepted and has no effect.

        loop_guard (True = loop_guard.LoopRule's defaults, a LoopRule, or a dict of its fields; None / False = off) ends a sequence on the
        GPU at the token after which its output has cycled for the rule's span (Engine.set_row_loop).  The returned ids end
        at that token; loop_guard.last_loop finds the hit again and loop_guard.trimmed cuts the ids back to one copy of the cycle.  A
        sequence with a rule verifies no draft of a speculating call; num_beams refuses it.

        streamer (Hugging Face's protocol, duck-typed: put(ids) and end()) receives the prompt ids, then the new ids of every scheduler
        chunk as they are generated (Request(stream=)), then end().  It is for one sequence, as in HF: a batch above 1,
        num_return_sequences > 1 or num_beams with a streamer raise ValueError.  It runs on the continuous path."""
        import dataclasses
        import torch
        t_eff, p_eff = resolve_sampling(self.generation_config, do_sample, temperature, top_p)
        self.engine.set_sampling(t_eff, p_eff, seed if t_eff > 0 else 0)
        from .loop_guard import as_rule
        loop = as_rule(loop_guard)
        if loop is not None and not hasattr(self.engine, "set_row_loop"):
            raise ValueError("this engine has no loop guard (no set_row_loop)")
        nrs = num_return_sequences
        if isinstance(nrs, bool) or not isinstance(nrs, int) or nrs < 1:
            raise ValueError(f"num_return_sequences must be an integer >= 1, got {nrs!r}")
        if nrs > 1 and continuous is False:
            raise ValueError("num_return_sequences > 1 runs on the continuous path: continuous=False cannot be combined with it")
        if prefill_chunk is not None:
            if continuous is False:
                raise ValueError("prefill_chunk runs on the continuous path: continuous=False cannot be combined with it")
            if speculative_ngram:
                raise ValueError("prefill_chunk cannot be combined with speculative_ngram: a speculating engine fills a prompt in one pass")
            continuous = True
        if enable_prefix_caching and prefill_chunk is None:
            raise ValueError("enable_prefix_caching needs prefill_chunk: only pages written by a chunked fill are cached")
        if image_keys is not None and (not enable_prefix_caching or len(image_keys) != int(input_ids.shape[0])):
            raise ValueError("image_keys needs enable_prefix_caching and one entry (16 bytes or None) per sequence")
        if streamer is not None:
            refused = [name for name, on in (("a batch above 1", int(input_ids.shape[0]) != 1), ("num_return_sequences > 1", nrs > 1),
                                             ("num_beams", num_beams not in (None, 1)), ("prompt_suffixes", prompt_suffixes is not None),
                                             ("continuous=False", continuous is False)) if on]
            if refused:
                raise ValueError(f"a streamer takes one sequence: it cannot be combined with {', '.join(refused)}")
            if not (hasattr(streamer, "put") and hasattr(streamer, "end")):
                raise ValueError("streamer needs put(ids) and end()")
            if not hasattr(self.engine, "slots_drain"):
                raise ValueError("this engine cannot stream (no slots_drain)")
            continuous = True
        predictions = None
        if prediction_ids is not None:           # predicted outputs: a hint per sequence, for the continuous path
            predictions = [None if p is None else [int(t) for t in p] for p in prediction_ids]
            if len(predictions) != int(input_ids.shape[0]):
                raise ValueError("prediction_ids takes one token list or None per sequence")
            refused = [name for name, on in (("num_return_sequences > 1", nrs > 1), ("num_beams", num_beams not in (None, 1)),
                                             ("prompt_suffixes", prompt_suffixes is not None), ("continuous=False", continuous is False)) if on]
            if refused:
                raise ValueError(f"a prediction belongs to one generated sequence: prediction_ids cannot be combined with {', '.join(refused)}")
            if not hasattr(self.engine, "set_row_prediction"):
                raise ValueError("this engine takes no prediction (no set_row_prediction)")
            continuous = True
        if early_stopping is not None:
            raise ValueError("early_stopping is not offered: a beam group ends at its cap, or early only where that is exact (DESIGN §6.9)")
        beam = None
        if num_beams is not None and num_beams != 1:
            from .beam import MAX_BEAMS
            if isinstance(num_beams, bool) or not isinstance(num_beams, int) or not 2 <= num_beams <= MAX_BEAMS:
                raise ValueError(f"num_beams must be an integer in [1, {MAX_BEAMS}], got {num_beams!r}")
            if nrs > num_beams:
                raise ValueError(f"num_return_sequences = {nrs} exceeds num_beams = {num_beams}")
            refused = [name for name, on in (
                ("sampling (temperature > 0)", t_eff > 0), ("top_k", (top_k or 0) > 0), ("repetition_penalty", repetition_penalty not in (None, 1.0)),
                ("frequency_penalty", (frequency_penalty or 0.0) != 0.0), ("presence_penalty", (presence_penalty or 0.0) != 0.0),
                ("logit_bias", bool(logit_bias)), ("allowed_token_ids", allowed_token_ids is not None), ("min_tokens", int(min_tokens or 0) > 0),
                ("stop_token_ids", bool(stop_token_ids)), ("ignore_eos", bool(ignore_eos)),
                ("a guide", any(g is not None for g in (guided_regex, guided_choice, guided_json))),
                ("no_repeat_ngram_size", bool(no_repeat_ngram_size)), ("stop_strings", stop_strings is not None),
                ("loop_guard", loop is not None), ("speculative_ngram", bool(speculative_ngram)), ("continuous=False", continuous is False)) if on]
            if refused:
                raise ValueError(f"num_beams cannot be combined with {', '.join(refused)}")
            if not hasattr(self.engine, "slots_beam"):
                raise ValueError("this engine cannot run a beam group (no slots_beam)")
            beam = (int(num_beams), float(length_penalty))
            continuous = True
        suffixes = None
        if prompt_suffixes is not None:
            suffixes = [[int(t) for t in x] for x in prompt_suffixes]
            refused = [name for name, on in (
                ("more than one input row", input_ids.shape[0] != 1), ("num_return_sequences > 1", nrs > 1), ("num_beams", beam is not None),
                ("repetition_penalty", repetition_penalty not in (None, 1.0)), ("frequency_penalty", (frequency_penalty or 0.0) != 0.0),
                ("presence_penalty", (presence_penalty or 0.0) != 0.0), ("speculative_ngram", bool(speculative_ngram)),
                ("continuous=False", continuous is False)) if on]
            if refused:
                raise ValueError(f"prompt_suffixes cannot be combined with {', '.join(refused)}")
            if not hasattr(self.engine, "slots_extend"):
                raise ValueError("this engine cannot extend a live sequence (no slots_extend)")
            continuous = True
        def call_params():                       # the call's SamplingParams, the seed of sequence 0; built at most once
            return SamplingParams(temperature=t_eff, top_p=p_eff, top_k=int(top_k or 0),
                                  repetition_penalty=1.0 if repetition_penalty is None else float(repetition_penalty),
                                  frequency_penalty=float(frequency_penalty or 0.0), presence_penalty=float(presence_penalty or 0.0), seed=seed)
        base = None
        if (top_k or 0) > 0 or repetition_penalty not in (None, 1.0) or (frequency_penalty or 0.0) != 0.0 or (presence_penalty or 0.0) != 0.0:
            base = call_params()
        rules = None
        if logit_bias or allowed_token_ids is not None or int(min_tokens or 0) > 0 or stop_token_ids or ignore_eos:
            rules = LogitRules(bias={int(k): float(v) for k, v in dict(logit_bias or {}).items()}, allowed=allowed_token_ids,
                               min_tokens=int(min_tokens or 0), stop=tuple(stop_token_ids or ()), ignore_eos=bool(ignore_eos),
                               vocab_size=self.config.vocab_size,
                               eos_ids=self.config.eos_token_ids if eos_token_id is None else
                               ([eos_token_id] if isinstance(eos_token_id, int) else list(eos_token_id)))
        from .guided import compile_request
        guide_obj = compile_request(guided_regex, guided_choice, guided_json, whitespace=guided_whitespace_pattern)
        guide = None
        if guide_obj is not None:
            if getattr(self.engine, "token_bytes", None) is None:
                raise ValueError("guided decoding needs the vocabulary's bytes: call engine.set_token_bytes(...) once (DotsOcrProcessor.token_bytes)")
            guide = self.engine.create_guide(guide_obj)
        ngram = None
        if no_repeat_ngram_size:
            ngram = NgramRule(no_repeat_ngram_size, no_repeat_ngram_window or 0, tuple(no_repeat_ngram_whitelist or ()),
                              vocab_size=self.config.vocab_size, max_seq_len=self.max_seq_len)
        elif no_repeat_ngram_window or no_repeat_ngram_whitelist:
            raise ValueError("no_repeat_ngram_window / no_repeat_ngram_whitelist need no_repeat_ngram_size")
        stop = None
        if stop_strings is not None:
            from .stop_strings import check_stop_strings
            stop = check_stop_strings(stop_strings)
            if getattr(self.engine, "token_bytes", None) is None:
                raise ValueError("stop strings need the vocabulary's bytes: call engine.set_token_bytes(...) once (DotsOcrProcessor.token_bytes)")
        if nrs > 1 and beam is None:
            continuous = True
        spec_k = int(speculative_ngram or 0)
        spec_rows = spec_rows_flags(speculative_rows)
        if spec_rows and not spec_k:
            raise ValueError("speculative_rows needs speculative_ngram")
        if speculative_guided and not spec_k:
            raise ValueError("speculative_guided needs speculative_ngram")
        if speculative_logprobs and not spec_k:
            raise ValueError("speculative_logprobs needs speculative_ngram")
        spec_shaped = spec_shaped_flags(speculative_shaped)
        if spec_shaped and not spec_k:
            raise ValueError("speculative_shaped needs speculative_ngram")
        if spec_k and continuous is False:
            raise ValueError("speculative_ngram runs on the continuous path: continuous=False cannot be combined with it")
        # the engine-wide sampler hashes the slot index and never speculates: sampled sequences that may speculate take parameters of their own
        spec_sampled = bool(spec_k and (spec_rows & SPEC_ROWS["sampled"]) and t_eff > 0)
        # Does any setting of this call force per-row selection?  Penalties and top_k, every row feature (a sampled row that carries one
        # draws with a seed of its own, as the penalised rows do), sampled suffixes, several sequences per prompt, sampled speculation.
        # Sequence b then draws with seed + b; with num_return_sequences prompt b's sequences take seed + b * n .. + n - 1 and with
        # suffixes the one prompt's take seed .. + m - 1 (the scheduler adds the index within a request to the seed it is given)
        row_sp = None
        if (base is not None or rules is not None or guide is not None or ngram is not None or stop is not None or loop is not None
                or (suffixes is not None and t_eff > 0) or (nrs > 1 and beam is None) or spec_sampled):
            base = call_params() if base is None else base
            stride = 0 if suffixes is not None else nrs if nrs > 1 and beam is None else 1

            def row_sp(b):
                return dataclasses.replace(base, seed=int(seed) + b * stride)
        spec = dict(rows=spec_rows, guided=bool(speculative_guided), logprobs=bool(speculative_logprobs), shaped=spec_shaped)
        if spec_k:
            continuous = True
            if spec_sampled:
                self.engine.set_sampling(0.0, 1.0, 0)
            self.engine.slots_reset()            # speculation changes only while no slot is occupied
            Engine.speculation_on(self.engine, spec_k, prompt_lookup_min, prompt_lookup_max, **spec)
        call = CallSettings(rules=rules, guide=guide, ngram=ngram, stop=stop, loop=loop, nrs=nrs, beam=beam, suffixes=suffixes, prefill_chunk=prefill_chunk,
                            shared_prefix_attention=bool(shared_prefix_attention),
                            image_keys=(image_keys or [None] * int(input_ids.shape[0])) if enable_prefix_caching else None, streamer=streamer,
                            predictions=predictions)
        try:
            return self._generate(input_ids, attention_mask, pixel_values, image_grid_thw, max_new_tokens, eos_token_id, pad_token_id, continuous,
                                  row_sp, call)
        finally:
            if spec_k:
                try:
                    self.engine.slots_reset()
                    Engine.speculation_off(self.engine, **spec)
                except Exception as e:               # the run's own error is the one to raise
                    import warnings
                    warnings.warn(f"speculation could not be switched off: {e}")
            if guide is not None:
                try:
                    self.engine.destroy_guide(guide)
                except Exception as e:               # a run that failed with rows still holding the guide: its own error is the one to
                    import warnings                  # raise; the handle stays until the rows are cleared (slots_reset)
                    warnings.warn(f"guide {guide} could not be destroyed: {e}")

    def score(self, input_ids, pixel_values=None, image_grid_thw=None, candidates=None, top_logprobs: int = 0):
        """Teacher-forced log-probabilities of given continuations (Engine.slots_score; vLLM's prompt_logprobs over a
        suffix).  input_ids (LongTensor [1, T] or [T]) is the prefix the candidates share — the page's image tokens and the text before
        them — and candidates 1 .. 8 lists of token ids; candidate i is scored as prefix + candidates[i] from one tower, one prefill of
        the prefix, one fork and one scoring pass, and nothing is generated.  Returns one (tok_lp float32 [m - 1], top_ids int32
        [m - 1, 20], top_lp float32 [m - 1, 20]) per candidate of m ids: entry j is log p(candidates[i][j + 1] | prefix,
        candidates[i][:j + 1]) with the top_logprobs (0 .. 20) largest alternatives beside it, bit for bit what forcing the tokens one
        decode step at a time returns.  To score a candidate's FIRST token too, move the prefix's last id to the head of every candidate,
        as the server's `score_candidates` does."""
        import torch
        from .scheduler import ContinuousBatcher, Request
        if candidates is None:
            raise ValueError("score needs candidates: 1 .. 8 lists of token ids")
        ids = (input_ids.detach().cpu().numpy() if isinstance(input_ids, torch.Tensor) else np.asarray(input_ids)).astype(np.int32)
        if ids.ndim == 2 and ids.shape[0] == 1:
            ids = ids[0]
        if ids.ndim != 1:
            raise ValueError("score takes one input row: the prefix the candidates share")
        pix = grid = None
        if pixel_values is not None:
            pix = pixel_values.contiguous().float() if getattr(pixel_values, "is_cuda", False) else \
                np.ascontiguousarray(pixel_values.detach().cpu().numpy() if isinstance(pixel_values, torch.Tensor) else pixel_values, dtype=np.float32)
            grid = (image_grid_thw.detach().cpu().numpy() if isinstance(image_grid_thw, torch.Tensor) else np.asarray(image_grid_thw)).astype(np.int64)
        self.engine.set_sampling(0.0, 1.0, 0)
        req = Request(ids, pix, grid, 1, score=[[int(t) for t in c] for c in candidates], score_top_logprobs=top_logprobs)
        ContinuousBatcher(self.engine, eos_ids=self.config.eos_token_ids).run([req])
        return req.scores_out

    def _generate(self, input_ids, attention_mask, pixel_values, image_grid_thw, max_new_tokens, eos_token_id, pad_token_id, continuous, row_sp,
                  call: CallSettings):
        """row_sp: b -> the SamplingParams of sequence b, or None = the engine-wide setting; call: everything else the rows are given"""
        import torch
        from .scheduler import ContinuousBatcher, Request
        suffixes, beam, streamer, image_keys = call.suffixes, call.beam, call.streamer, call.image_keys
        nrs = len(suffixes) if suffixes else call.nrs    # the rows of the result: one per suffix, laid out as num_return_sequences lays them out
        ids = input_ids.detach().cpu().numpy()
        B, T = ids.shape
        mask = attention_mask.detach().cpu().numpy().astype(bool) if attention_mask is not None else np.ones_like(ids, bool)
        eos = self.config.eos_token_ids if eos_token_id is None else eos_token_id
        eos = [eos] if isinstance(eos, int) else list(eos)
        pad = self.config.pad_token_id if pad_token_id is None else pad_token_id
        grid = image_grid_thw.detach().cpu().numpy().astype(np.int64) if image_grid_thw is not None else np.zeros((0, 3), np.int64)
        merge2 = self.config.vision.spatial_merge_size ** 2

        # which images belong to which sequence: image tokens are consumed in order
        prompts = [ids[b][mask[b]].astype(np.int32) for b in range(B)]
        n_img_tok = [int((p == self.config.image_token_id).sum()) for p in prompts]
        per_img_tok = (grid[:, 0] * grid[:, 1] * grid[:, 2] // merge2).tolist()
        img_of_seq, gi = [], 0
        for b in range(B):
            need, lst = n_img_tok[b], []
            while need > 0:
                if gi >= len(per_img_tok):
                    raise ValueError("image tokens do not match image_grid_thw")
                need -= per_img_tok[gi]
                lst.append(gi)
                gi += 1
            if need != 0:
                raise ValueError("image tokens do not match image_grid_thw")
            img_of_seq.append(lst)
        patch_off = np.concatenate([[0], np.cumsum(grid[:, 0] * grid[:, 1] * grid[:, 2])]).astype(np.int64)

        pv_dev, pv_host = None, None
        if pixel_values is not None:
            if pixel_values.is_cuda:
                pv_dev = pixel_values.contiguous().float()
                torch.cuda.synchronize(pv_dev.device)
            else:
                pv_host = np.ascontiguousarray(pixel_values.detach().numpy(), dtype=np.float32)

        # like HF, generation stops at the context capacity instead of failing: the reference asks for 24 000 new tokens
        # (parser.py:110) on top of prompts of up to 14 400 vision tokens; the KV pool is sized for max_seq_len per sequence
        longest = max(len(p) for p in prompts)
        if longest >= self.max_seq_len:
            raise ValueError(f"prompt of {longest} tokens does not fit max_seq_len={self.max_seq_len}")
        max_new_tokens = max(1, min(int(max_new_tokens), self.max_seq_len - longest - max((len(x) for x in suffixes or ()), default=0)))
        new_tokens = np.full((B * nrs, max_new_tokens), pad, dtype=np.int64)
        n_max = 0
        seq_patches = [int(sum(patch_off[g + 1] - patch_off[g] for g in img_of_seq[b])) for b in range(B)]
        if continuous is None:
            continuous = B > self.max_batch

        def request(b, pix=None, g=None):        # sequence b with the call's row settings: what both paths give their rows
            return Request(prompts[b], pix, g, max_new_tokens, sampling=row_sp(b) if row_sp else None, rules=call.rules, guide=call.guide,
                           ngram=call.ngram, n=1 if suffixes else nrs, stop=call.stop, loop=call.loop, suffixes=suffixes,
                           prediction=call.predictions[b] if call.predictions else None)
        if continuous:
            reqs = []
            for b in range(B):
                if img_of_seq[b]:
                    lo, hi = int(patch_off[img_of_seq[b][0]]), int(patch_off[img_of_seq[b][-1] + 1])
                    reqs.append(request(b, pv_dev[lo:hi] if pv_dev is not None else pv_host[lo:hi], grid[img_of_seq[b][0]:img_of_seq[b][-1] + 1]))
                    if image_keys and image_keys[b] is not None:      # the caller names the image; the grid it was resized to is part of what is cached
                        import hashlib
                        reqs[-1].image_key = hashlib.blake2b(bytes(image_keys[b]) + reqs[-1].grid_thw.tobytes(), digest_size=16).digest()
                else:
                    reqs.append(request(b))
                if beam is not None:             # a group of beam[0] beams that returns its nrs best hypotheses
                    reqs[-1].n, reqs[-1].num_beams, reqs[-1].num_return, reqs[-1].length_penalty = 1, beam[0], nrs, beam[1]
            if streamer is not None:             # one sequence (generate() checked): the prompt, then every chunk's new ids, then end()
                streamer.put(input_ids.detach().cpu())
                reqs[0].stream = lambda rid, index, toks, lp, fin: len(toks) and streamer.put(torch.as_tensor(np.asarray(toks), dtype=torch.long))
            chunk_kw = {} if call.prefill_chunk is None else {"prefill_chunk": call.prefill_chunk}
            if image_keys is not None:           # enable_prefix_caching
                chunk_kw["prefix_caching"] = True
            if call.shared_prefix_attention:     # for this call's run: the switch goes back off behind it
                chunk_kw["shared_prefix_attention"] = True
            try:
                outs = ContinuousBatcher(self.engine, eos_ids=eos, **chunk_kw).run(reqs)
            finally:
                if call.shared_prefix_attention:
                    self.engine.set_shared_prefix_attention(False)
            if streamer is not None:
                streamer.end()
            if beam is not None:                 # row i * n + j = the j-th best hypothesis of prompt i (a prompt with fewer: pad rows)
                outs = [r.outputs[j] if j < len(r.outputs) else np.zeros(0, np.int64) for r in reqs for j in range(nrs)]
            elif nrs > 1:                        # row i * n + j = sequence j of prompt i
                outs = [o for r in reqs for o in r.outputs]
            for b, o in enumerate(outs):
                new_tokens[b, :len(o)] = o
                n_max = max(n_max, len(o))
        # static batches within the engine's capacity.  With several batches the vision tower of batch k+1 is prefetched on the engine's
        # CU-masked side stream while batch k is prefilled and decoded (Engine.vit_prefetch: same tokens, ~20 % more pages/s at 8 x A4).
        plan = [] if continuous else plan_batches(seq_patches, self.max_batch, self.max_patches)

        def pixels_of(sl):
            imgs = [g for b in sl for g in img_of_seq[b]]
            if not imgs:
                return None, None, False
            lo, hi = int(patch_off[imgs[0]]), int(patch_off[imgs[-1] + 1])         # images of a slice are contiguous
            g = grid[imgs[0]:imgs[-1] + 1]
            if pv_dev is not None:
                return pv_dev.data_ptr() + lo * pv_dev.shape[1] * 4, g, True
            return pv_host[lo:hi], g, False
        pipelined = len(plan) > 1 and all(pixels_of(sl)[0] is not None for sl in plan) and hasattr(self.engine, "vit_prefetch")
        if pipelined:
            pix, g, on_dev = pixels_of(plan[0])
            self.engine.vit_prefetch(pix, g, on_device=on_dev)
        prefetched = pipelined                   # a tower is in flight / waiting to be taken
        held = {}                                # what the rows of the static batches hold (cleared on the way out)
        try:
            for k, sl in enumerate(plan):
                if call.rules is not None:
                    self.engine.set_eos(eos)         # the engine checks a row's rules against the EOS ids of THIS call
                for j, b in enumerate(sl):
                    apply_row(self.engine, held, j, request(b))
                lens = np.array([len(prompts[b]) for b in sl], np.int32)
                packed = np.concatenate([prompts[b] for b in sl])
                pix, g, on_dev = pixels_of(sl)
                if pipelined:
                    self.engine.vit_take()
                    prefetched = False
                    if k + 1 < len(plan):
                        npix, ng, non_dev = pixels_of(plan[k + 1])
                        self.engine.vit_prefetch(npix, ng, on_device=non_dev, after_prefill=True)
                        prefetched = True
                    out, out_lens = self.engine.generate(packed, lens, max_new_tokens=max_new_tokens, eos_ids=eos, vision_taken=True)
                elif pix is not None:
                    out, out_lens = self.engine.generate(packed, lens, pix, g, max_new_tokens, eos, on_dev)
                else:
                    out, out_lens = self.engine.generate(packed, lens, None, None, max_new_tokens, eos)
                for j, b in enumerate(sl):
                    new_tokens[b, :out_lens[j]] = out[j, :out_lens[j]]
                    n_max = max(n_max, int(out_lens[j]))
        except Exception:
            if prefetched:                           # leave the engine usable: a waiting prefetch would refuse the next one
                try:
                    self.engine.vit_take()
                except Exception:
                    pass
            raise
        finally:
            clear_rows(self.engine, held, sorted(held))
        full = np.concatenate([np.repeat(ids.astype(np.int64), nrs, axis=0), new_tokens[:, :n_max]], axis=1)    # HF stops at the longest sequence
        res = torch.from_numpy(full)
        return res.to(input_ids.device) if input_ids.is_cuda else res

    def stats(self) -> dict:
        return self.engine.stats()
