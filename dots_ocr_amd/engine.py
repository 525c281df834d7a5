"""ctypes binding of include/dots_ocr_hip.h — the only way Python reaches the HIP kernels.

No torch types cross this boundary: numpy arrays for host buffers, integers for device pointers
(torch CUDA tensors are passed by ``data_ptr()``; torch and this library share one HIP runtime).
"""
from __future__ import annotations

import ctypes as C
import math
import os
from collections import OrderedDict
from dataclasses import dataclass
from typing import Dict, Optional, Sequence

import numpy as np

from . import _lib
from .config import DotsConfig

EPI_NONE, EPI_RESIDUAL, EPI_SWIGLU, EPI_GELU, EPI_F32 = range(5)
DTYPE_BF16, DTYPE_F32, DTYPE_F16 = 0, 1, 2


class CDotsConfig(C.Structure):
    _fields_ = [
        ("hidden_size", C.c_int32), ("num_layers", C.c_int32), ("num_heads", C.c_int32), ("num_kv_heads", C.c_int32),
        ("head_dim", C.c_int32), ("intermediate_size", C.c_int32), ("vocab_size", C.c_int32),
        ("rope_theta", C.c_float), ("rms_norm_eps", C.c_float),
        ("attention_bias", C.c_int32), ("image_token_id", C.c_int32),
        ("v_embed_dim", C.c_int32), ("v_layers", C.c_int32), ("v_heads", C.c_int32), ("v_intermediate", C.c_int32),
        ("v_patch", C.c_int32), ("v_merge", C.c_int32), ("v_channels", C.c_int32), ("v_temporal_patch", C.c_int32),
        ("v_rms_eps", C.c_float), ("v_ln_eps", C.c_float),
        ("v_use_bias", C.c_int32), ("v_post_norm", C.c_int32),
        ("max_batch", C.c_int32), ("max_seq_len", C.c_int32),
        ("max_patches", C.c_int64), ("max_prefill_tokens", C.c_int64), ("kv_pool_tokens", C.c_int64),
        ("fp8_weights", C.c_int32), ("kv_cache_dtype", C.c_int32),
    ]


class CDotsStats(C.Structure):
    _fields_ = [
        ("vit_ms", C.c_float), ("prefill_ms", C.c_float), ("decode_ms", C.c_float), ("total_ms", C.c_float),
        ("vit_attn_ms", C.c_float), ("vit_attn_launches", C.c_int32),
        ("vit_gemm_ms", C.c_float), ("decode_steps", C.c_int32),
        ("vit_patches", C.c_int64), ("prefill_tokens", C.c_int64), ("new_tokens", C.c_int64),
        ("vit_attn_flops", C.c_double), ("vit_flops", C.c_double), ("prefill_flops", C.c_double),
        ("decode_bytes", C.c_double),
    ]


class CDotsSamplingParams(C.Structure):
    _fields_ = [
        ("temperature", C.c_float), ("top_p", C.c_float), ("top_k", C.c_int32),
        ("repetition_penalty", C.c_float), ("frequency_penalty", C.c_float), ("presence_penalty", C.c_float),
        ("seed", C.c_uint64),
    ]


@dataclass(frozen=True)
class SamplingParams:
    """Token selection of one request / decode row (include/dots_ocr_hip.h DotsSamplingParams).

    temperature 0 = greedy; top_k <= 0 = off, and top_k is clamped to TOP_K_MAX (a k at or above the vocabulary keeps every token);
    top_p is clamped to (0, 1]; repetition_penalty 1 and frequency / presence 0 = off.  The float fields are checked as the fp32 values
    the engine receives.  Invalid values raise ValueError."""
    temperature: float = 0.0
    top_p: float = 1.0
    top_k: int = 0
    repetition_penalty: float = 1.0
    frequency_penalty: float = 0.0
    presence_penalty: float = 0.0
    seed: int = 0

    TOP_K_MAX = 2 ** 31 - 1                      # int32_t top_k of DotsSamplingParams

    def __post_init__(self):
        f32 = lambda v: C.c_float(float(v)).value                                      # noqa: E731 (what the C struct holds)
        t, p, r = f32(self.temperature), float(self.top_p), f32(self.repetition_penalty)
        f, pr = f32(self.frequency_penalty), f32(self.presence_penalty)
        if not (math.isfinite(t) and t >= 0):
            raise ValueError(f"temperature must be finite and >= 0, got {self.temperature!r}")
        if not (p > 0) or math.isnan(p):
            raise ValueError(f"top_p must be in (0, 1], got {self.top_p!r}")
        if not (math.isfinite(r) and r > 0):
            raise ValueError(f"repetition_penalty must be finite and > 0, got {self.repetition_penalty!r}")
        for name, v in (("frequency_penalty", f), ("presence_penalty", pr)):
            if not (-2.0 <= v <= 2.0):
                raise ValueError(f"{name} must be in [-2, 2], got {v!r}")
        k = int(self.top_k)
        if k != self.top_k:
            raise ValueError(f"top_k must be an integer, got {self.top_k!r}")
        object.__setattr__(self, "temperature", t)
        object.__setattr__(self, "top_p", min(p, 1.0))
        object.__setattr__(self, "top_k", min(max(k, 0), self.TOP_K_MAX))
        object.__setattr__(self, "repetition_penalty", r)
        object.__setattr__(self, "frequency_penalty", f)
        object.__setattr__(self, "presence_penalty", pr)
        object.__setattr__(self, "seed", int(self.seed) & (2 ** 64 - 1))

    @property
    def has_penalty(self) -> bool:
        return self.repetition_penalty != 1.0 or self.frequency_penalty != 0.0 or self.presence_penalty != 0.0

    def to_c(self) -> CDotsSamplingParams:
        return CDotsSamplingParams(self.temperature, self.top_p, self.top_k, self.repetition_penalty, self.frequency_penalty,
                                   self.presence_penalty, self.seed)


MAX_LOGIT_BIAS = 1024                        # DOTS_MAX_LOGIT_BIAS: (id, value) pairs per row
MAX_STOP_IDS = 16                            # DOTS_MAX_STOP_IDS: stop ids per row
MAX_STOP_STRINGS = 16                        # DOTS_MAX_STOP_STRINGS: stop strings per row
MAX_STOP_BYTES = 64                          # DOTS_MAX_STOP_BYTES: UTF-8 bytes of one stop string; so at most 16 x 64 + 1 = 1025 states


class CDotsLogitRules(C.Structure):
    _fields_ = [
        ("bias_ids", C.POINTER(C.c_int32)), ("bias_values", C.POINTER(C.c_float)), ("n_bias", C.c_int32),
        ("allowed_ids", C.POINTER(C.c_int32)), ("n_allowed", C.c_int32), ("min_tokens", C.c_int32),
        ("stop_ids", C.c_int32 * MAX_STOP_IDS), ("n_stop", C.c_int32), ("ignore_eos", C.c_int32),
    ]


def _id_tuple(name, ids):
    out = []
    for v in ids:
        if isinstance(v, bool) or int(v) != v:
            raise ValueError(f"{name} must hold integer token ids, got {v!r}")
        if not 0 <= int(v) < 2 ** 31:
            raise ValueError(f"{name} must hold token ids >= 0, got {v!r}")
        out.append(int(v))
    return tuple(out)


@dataclass(frozen=True)
class LogitRules:
    """Logit rules of one request / decode row (include/dots_ocr_hip.h DotsLogitRules).

    bias: {id: value} or (id, value) pairs, at most MAX_LOGIT_BIAS, value finite or -inf (a ban), no id twice; allowed: None or a non-empty
    id list (every other id is -inf); min_tokens: EOS and stop ids are -inf while fewer tokens exist; stop: at most MAX_STOP_IDS ids that
    finish this row only; ignore_eos: the engine's EOS ids do not finish it.  vocab_size (optional) bounds every id.  Rules that could
    never select a token raise ValueError: an allowed list the bans cover, or — with min_tokens > 0 — one that bans, stop ids and
    eos_ids (optional: the engine's EOS ids the row will run under) cover together; the engine repeats the check with its own EOS ids."""
    bias: tuple = ()
    allowed: Optional[tuple] = None
    min_tokens: int = 0
    stop: tuple = ()
    ignore_eos: bool = False
    vocab_size: Optional[int] = None
    eos_ids: Optional[tuple] = None

    def __post_init__(self):
        pairs = list(self.bias.items()) if isinstance(self.bias, dict) else [tuple(x) for x in self.bias]
        if len(pairs) > MAX_LOGIT_BIAS:
            raise ValueError(f"at most {MAX_LOGIT_BIAS} bias entries, got {len(pairs)}")
        ids = _id_tuple("bias", [p[0] for p in pairs])
        if len(set(ids)) != len(ids):
            raise ValueError("bias holds an id twice")
        vals = []
        for _, v in pairs:
            f = C.c_float(float(v)).value if math.isfinite(float(v)) else float(v)
            if math.isnan(f) or f == math.inf:
                raise ValueError(f"a bias value must be finite or -inf, got {v!r}")
            vals.append(f)
        allowed = None
        if self.allowed is not None:
            allowed = tuple(sorted(set(_id_tuple("allowed", self.allowed))))
            if not allowed:
                raise ValueError("allowed must be None or a non-empty id list")
        stop = _id_tuple("stop", self.stop)
        if len(stop) > MAX_STOP_IDS:
            raise ValueError(f"at most {MAX_STOP_IDS} stop ids, got {len(stop)}")
        if isinstance(self.min_tokens, bool) or int(self.min_tokens) != self.min_tokens or not 0 <= int(self.min_tokens) < 2 ** 31:
            raise ValueError(f"min_tokens must be an integer >= 0, got {self.min_tokens!r}")
        if self.vocab_size is not None:
            V = int(self.vocab_size)
            for name, seq in (("bias", ids), ("allowed", allowed or ()), ("stop", stop)):
                for t in seq:
                    if t >= V:
                        raise ValueError(f"{name} id {t} outside [0, {V})")
        if allowed is not None:
            banned = {t for t, v in zip(ids, vals) if v == -math.inf}
            free = [t for t in allowed if t not in banned]
            if not free:
                raise ValueError("every allowed id is banned by the bias: nothing could be selected")
            held = set(stop) | set(int(t) for t in (self.eos_ids or ()))
            if int(self.min_tokens) > 0 and all(t in held for t in free):
                raise ValueError("below min_tokens every allowed id is an EOS or a stop id: nothing could be selected")
        object.__setattr__(self, "bias", tuple(zip(ids, vals)))
        object.__setattr__(self, "allowed", allowed)
        object.__setattr__(self, "min_tokens", int(self.min_tokens))
        object.__setattr__(self, "stop", stop)
        object.__setattr__(self, "ignore_eos", bool(self.ignore_eos))
        object.__setattr__(self, "vocab_size", None if self.vocab_size is None else int(self.vocab_size))
        object.__setattr__(self, "eos_ids", None if self.eos_ids is None else tuple(int(t) for t in self.eos_ids))

    @property
    def empty(self) -> bool:
        """no rule at all: the row behaves as one without LogitRules"""
        return not self.bias and self.allowed is None and self.min_tokens == 0 and not self.stop and not self.ignore_eos

    def to_c(self) -> CDotsLogitRules:
        """The C struct; the arrays it points to are kept alive on the returned object (`_keep`)."""
        ids = np.asarray([t for t, _ in self.bias], np.int32)
        vals = np.asarray([v for _, v in self.bias], np.float32)
        allowed = None if self.allowed is None else np.asarray(self.allowed, np.int32)
        c = CDotsLogitRules()
        c.bias_ids = _i32p(ids) if len(ids) else None
        c.bias_values = vals.ctypes.data_as(C.POINTER(C.c_float)) if len(ids) else None
        c.n_bias = len(ids)
        c.allowed_ids = _i32p(allowed) if allowed is not None else None
        c.n_allowed = 0 if allowed is None else len(allowed)
        c.min_tokens = self.min_tokens
        for j, t in enumerate(self.stop):
            c.stop_ids[j] = t
        c.n_stop = len(self.stop)
        c.ignore_eos = int(self.ignore_eos)
        c._keep = (ids, vals, allowed)
        return c


MAX_NGRAM_SIZE = 64                          # DOTS_MAX_NGRAM_SIZE: the longest n-gram a rule may name
MAX_NGRAM_WHITELIST = 16                     # DOTS_MAX_NGRAM_WHITELIST: whitelisted ids per row


class CDotsNgramRule(C.Structure):
    _fields_ = [("size", C.c_int32), ("window", C.c_int32), ("n_whitelist", C.c_int32), ("whitelist", C.c_int32 * MAX_NGRAM_WHITELIST)]


@dataclass(frozen=True)
class NgramRule:
    """No-repeat n-gram rule of one request / decode row (include/dots_ocr_hip.h DotsNgramRule).

    size: n in [1, MAX_NGRAM_SIZE] — the row never completes an n-gram its own output already holds; window: 0 = the whole output, else
    W >= size — only n-grams inside the last W generated tokens count; whitelist: at most MAX_NGRAM_WHITELIST distinct ids the rule never
    bans (table tags, EOS).  vocab_size / max_seq_len (optional) bound the ids and the window; the engine repeats the check.  The prompt
    is not part of the history (vLLM's convention; Hugging Face generate() counts it)."""
    size: int
    window: int = 0
    whitelist: tuple = ()
    vocab_size: Optional[int] = None
    max_seq_len: Optional[int] = None

    def __post_init__(self):
        for name in ("size", "window"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise ValueError(f"{name} must be an integer, got {v!r}")
        n, w = int(self.size), int(self.window)
        if not 1 <= n <= MAX_NGRAM_SIZE:
            raise ValueError(f"size must be in [1, {MAX_NGRAM_SIZE}], got {n}")
        if w != 0 and w < n:
            raise ValueError(f"window must be 0 (the whole output) or >= size = {n}, got {w}")
        if self.max_seq_len is not None and w > int(self.max_seq_len):
            raise ValueError(f"window {w} exceeds max_seq_len {int(self.max_seq_len)}")
        white = _id_tuple("whitelist", self.whitelist)
        if len(white) > MAX_NGRAM_WHITELIST:
            raise ValueError(f"at most {MAX_NGRAM_WHITELIST} whitelist ids, got {len(white)}")
        if len(set(white)) != len(white):
            raise ValueError("whitelist holds an id twice")
        if self.vocab_size is not None:
            for t in white:
                if t >= int(self.vocab_size):
                    raise ValueError(f"whitelist id {t} outside [0, {int(self.vocab_size)})")
        object.__setattr__(self, "size", n)
        object.__setattr__(self, "window", w)
        object.__setattr__(self, "whitelist", white)
        object.__setattr__(self, "vocab_size", None if self.vocab_size is None else int(self.vocab_size))
        object.__setattr__(self, "max_seq_len", None if self.max_seq_len is None else int(self.max_seq_len))

    def to_c(self) -> CDotsNgramRule:
        c = CDotsNgramRule(self.size, self.window, len(self.whitelist))
        for j, t in enumerate(self.whitelist):
            c.whitelist[j] = t
        return c


class CDotsLoopRule(C.Structure):
    _fields_ = [("min_period", C.c_int32), ("max_period", C.c_int32), ("repeats", C.c_int32), ("min_span", C.c_int32)]


def banned_ngram_ids(out, n: int, window: int = 0, whitelist=()) -> set:
    """The ids an NgramRule(n, window, whitelist) bans after the generated tokens `out` — the restatement the kernels are
    tested against.  With L = len(out) and P = out[L - n + 1:], every i in [max(0, L - window), L - n] (window 0: from 0) with
    out[i:i + n - 1] == P bans out[i + n - 1] unless it is whitelisted."""
    out = [int(t) for t in out]
    L, n, window = len(out), int(n), int(window)
    if n < 1 or L < n - 1:
        return set()
    prefix = out[L - n + 1:] if n > 1 else []
    white = set(int(t) for t in whitelist)
    banned = set()
    for i in range(max(0, L - window) if window > 0 else 0, L - n + 1):
        if out[i:i + n - 1] == prefix and out[i + n - 1] not in white:
            banned.add(out[i + n - 1])
    return banned


class DotsEngineError(RuntimeError):
    code = None                                      # the DOTS_E_* code of the failed call, where there was one


E_INVALID, E_HIP, E_STATE, E_CAPACITY = -1, -2, -3, -4      # include/dots_ocr_hip.h


_SIGNATURES_SET = False


def _signatures() -> dict:
    """every symbol the library exports -> (result type, argument types): the one list of them (EXPORTED_SYMBOLS are its keys)"""
    vp, i32, i64, f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float
    P = C.POINTER
    return {
        "dots_create": (i32, [P(CDotsConfig), i32, P(vp)]),
        "dots_destroy": (None, [vp]),
        "dots_last_error": (C.c_char_p, [vp]),
        "dots_stream": (vp, [vp]),
        "dots_load_weight": (i32, [vp, C.c_char_p, vp, i32, P(i64), i32]),
        "dots_finalize_weights": (i32, [vp]),
        "dots_vit_forward": (i32, [vp, vp, i32, i64, P(i64), i32, vp]),
        "dots_vit_prefetch": (i32, [vp, vp, i32, i64, P(i64), i32, i32]),
        "dots_vit_take_prefetched": (i32, [vp]),
        "dots_vit_prefetch_ready": (i32, [vp, P(i32)]),
        "dots_prefill": (i32, [vp, P(i32), P(i32), i32]),
        "dots_decode_step": (i32, [vp]),
        "dots_generate": (i32, [vp, P(i32), P(i32), i32, vp, i32, i64, P(i64), i32, i32, P(i32), i32, P(i32), P(i32)]),
        "dots_preprocess_image": (i32, [vp, vp, i32, i32, i32, i32, i32, P(i32), P(i32), i32, P(i32), P(i32), i32, P(f32), P(f32), f32, vp]),
        "dots_set_sampling": (i32, [vp, f32, f32, C.c_uint64]),
        "dots_set_row_sampling": (i32, [vp, i32, P(CDotsSamplingParams)]),
        "dots_set_decode_plan": (i32, [vp, i32]),
        "dots_set_gemm_plan": (i32, [vp, i32]),
        "dots_tower_tail": (i32, [vp, i32, P(i32)]),
        "dots_slot_capacity": (i32, [vp, i32, P(i32), P(i32)]),
        "dots_slots_reset": (i32, [vp]),
        "dots_set_eos": (i32, [vp, P(i32), i32]),
        "dots_slots_prefill": (i32, [vp, P(i32), i32, P(i32), P(i32), P(i32)]),
        "dots_slots_prefill_begin": (i32, [vp, P(i32), i32, P(i32), P(i32), P(i32)]),
        "dots_slots_prefill_advance": (i32, [vp, i32, P(i32)]),
        "dots_prefix_cache_enable": (i32, [vp, i32]),
        "dots_prefix_cache_lookup": (i32, [vp, P(i32), i32, C.c_char_p, P(i32), P(i32), P(i32)]),
        "dots_prefix_cache_release": (i32, [vp, i32]),
        "dots_slots_prefill_begin_cached": (i32, [vp, P(i32), i32, P(i32), P(i32), P(i32), P(i32), P(C.c_char_p)]),
        "dots_prefix_cache_info": (i32, [vp, P(i64)]),
        "dots_slots_decode": (i32, [vp, i32]),
        "dots_slots_fork": (i32, [vp, i32, P(i32), i32]),
        "dots_slot_logits": (i32, [vp, i32, P(C.c_float)]),
        "dots_slots_extend": (i32, [vp, P(i32), i32, P(i32), P(i32), P(i32), P(i32)]),
        "dots_slots_score": (i32, [vp, P(i32), i32, P(i32), P(i32), P(i32), P(i32), P(i32)]),
        "dots_slot_scores": (i32, [vp, i32, i32, i32, P(f32), P(i32), P(f32), P(i32)]),
        "dots_slots_beam": (i32, [vp, i32, P(i32), i32]),
        "dots_beam_info": (i32, [vp, i32, P(i32), P(i32), P(i32)]),
        "dots_beam_read": (i32, [vp, i32, P(i32), P(i32), P(f32), P(i32), P(i32), i32, P(i32), i32, P(i32)]),
        "dots_slots_poll": (i32, [vp, P(i32), P(i32)]),
        "dots_set_row_stream": (i32, [vp, i32, i32]),
        "dots_slots_drain": (i32, [vp, P(i32), P(i32), P(i32), P(i32), P(i32), P(i32), i32, P(f32), P(i32), P(f32), i32, P(i32), P(i32)]),
        "dots_slot_read": (i32, [vp, i32, P(i32), i32, P(i32)]),
        "dots_slot_release": (i32, [vp, i32]),
        "dots_kv_pool_info": (i32, [vp, P(i32), P(i32)]),
        "dots_kv_swap_reserve": (i32, [vp, i32]),
        "dots_kv_swap_info": (i32, [vp, P(i32), P(i32)]),
        "dots_slot_suspend": (i32, [vp, i32]),
        "dots_slot_resume": (i32, [vp, i32]),
        "dots_slots_pages_short": (i32, [vp, i32, P(i32)]),
        "dots_set_shared_prefix_attention": (i32, [vp, i32]),
        "dots_shared_prefix_info": (i32, [vp, P(i64)]),
        "dots_set_kv_scales": (i32, [vp, P(f32)]),
        "dots_get_logits": (i32, [vp, P(f32)]),
        "dots_set_next_tokens": (i32, [vp, P(i32), i32]),
        "dots_get_last_tokens": (i32, [vp, P(i32)]),
        "dots_get_stats": (i32, [vp, P(CDotsStats)]),
        "dots_synchronize": (i32, [vp]),
        "dots_debug_capture_hidden": (i32, [vp, i64]),
        "dots_debug_read_hidden": (i32, [vp, i32, i32, vp, P(i64)]),
        "dots_debug_read_kv": (i32, [vp, i32, i32, i32, i32, i32, vp]),
        "dots_dev_alloc": (i32, [vp, i64, P(vp)]),
        "dots_dev_free": (i32, [vp, vp]),
        "dots_memcpy_h2d": (i32, [vp, vp, vp, i64]),
        "dots_memcpy_d2h": (i32, [vp, vp, vp, i64]),
        "dots_op_rmsnorm": (i32, [vp, vp, vp, vp, i64, i32, f32]),
        "dots_op_layernorm": (i32, [vp, vp, vp, vp, vp, i64, i32, f32]),
        "dots_op_gemm": (i32, [vp, vp, vp, vp, vp, vp, i64, i32, i32, i32, vp]),
        "dots_op_quant_fp8": (i32, [vp, vp, vp, i64, i32]),
        "dots_op_gemm_fp8": (i32, [vp, vp, vp, vp, vp, vp, i64, i32, i32, i32]),
        "dots_op_flash_attn": (i32, [vp, vp, vp, vp, vp, P(i32), i32, i32, i32, i32, f32]),
        "dots_op_flash_attn_paged": (i32, [vp, vp, vp, vp, i32, i32, vp, P(i32), P(i32), P(i32), i32, i32, i32, f32, vp]),
        "dots_plan_flash_xcd": (i32, [P(i32), i32, i32, P(i32), P(i32), P(i64)]),
        "dots_op_qkv_rope_split": (i32, [vp, vp, vp, vp, vp, P(i32), i32, P(i32), i32, i32, i32, f32]),
        "dots_op_qkv_proj_rope": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, P(i32), i32, P(i32), i32, i32, i32, i32, f32, i32]),
        "dots_op_dec_qkv": (i32, [vp, vp, vp, vp, vp, vp, vp, i32, vp, vp, i32, i32, i32, i32, f32, f32, i32]),
        "dots_op_decode_attn": (i32, [vp, vp, vp, vp, vp, i32, vp, i32, i32, i32, i32]),
        "dots_op_dec_qkv_kv8": (i32, [vp, vp, vp, vp, vp, vp, vp, i32, vp, vp, i32, i32, i32, i32, f32, f32, i32, vp]),
        "dots_op_decode_attn_kv8": (i32, [vp, vp, vp, vp, vp, i32, vp, i32, i32, i32, i32, vp]),
        "dots_op_decode_attn_shared": (i32, [vp, vp, vp, vp, vp, i32, vp, i32, i32, i32, i32, vp, P(i32)]),
        "dots_plan_shared_prefix": (i32, [P(i32), P(i32), i32, P(i32), i32, i32, i32, P(i32), P(i32), P(C.c_uint64)]),
        "dots_op_dec_proj": (i32, [vp, vp, vp, vp, i32, i32, i32, i32]),
        "dots_op_dec_gateup": (i32, [vp, vp, vp, vp, vp, vp, i32, i32, i32, f32, i32]),
        "dots_op_dec_lmhead": (i32, [vp, vp, vp, vp, vp, i32, i32, i32, f32, i32]),
        "dots_op_select_tokens": (i32, [vp, vp, i32, i32, P(CDotsSamplingParams), vp, vp, i32, vp, vp]),
        "dots_bench_select_tokens": (i32, [vp, vp, i32, i32, P(CDotsSamplingParams), vp, vp, i32, vp, i32, i32, P(f32)]),
        "dots_set_row_logit_rules": (i32, [vp, i32, P(CDotsLogitRules)]),
        "dots_op_select_tokens_rules": (i32, [vp, vp, i32, i32, P(CDotsSamplingParams), P(CDotsLogitRules), P(i32), vp, vp, i32, vp, vp]),
        "dots_bench_select_tokens_rules": (i32, [vp, vp, i32, i32, P(CDotsSamplingParams), P(CDotsLogitRules), P(i32), vp, vp, i32, vp, i32, P(f32)]),
        "dots_set_token_bytes": (i32, [vp, P(i32), vp]),
        "dots_guide_create": (i32, [vp, vp, i32, vp, i32, P(i32)]),
        "dots_guide_destroy": (i32, [vp, i32]),
        "dots_set_row_guide": (i32, [vp, i32, i32]),
        "dots_row_guide_state": (i32, [vp, i32, P(i32)]),
        "dots_op_select_tokens_guided": (i32, [vp, vp, i32, i32, P(CDotsSamplingParams), P(CDotsLogitRules), P(i32), P(i32), P(i32), vp, vp, i32, vp, vp,
                                               P(i32)]),
        "dots_bench_select_tokens_guided": (i32, [vp, vp, i32, i32, P(CDotsSamplingParams), P(CDotsLogitRules), P(i32), P(i32), P(i32), vp, vp, i32, vp,
                                                  i32, P(f32)]),
        "dots_set_row_ngram": (i32, [vp, i32, P(CDotsNgramRule)]),
        "dots_op_select_tokens_ngram": (i32, [vp, vp, i32, i32, P(CDotsSamplingParams), P(CDotsLogitRules), P(CDotsNgramRule), vp, vp, i32, vp, vp]),
        "dots_bench_select_tokens_ngram": (i32, [vp, vp, i32, i32, P(CDotsSamplingParams), P(CDotsLogitRules), P(CDotsNgramRule), vp, vp, i32, vp, i32,
                                                 P(f32)]),
        "dots_stop_create": (i32, [vp, vp, i32, vp, vp, P(i32)]),
        "dots_stop_destroy": (i32, [vp, i32]),
        "dots_set_row_stop": (i32, [vp, i32, i32, i32]),
        "dots_row_stop_hit": (i32, [vp, i32, P(i32)]),
        "dots_set_row_loop": (i32, [vp, i32, P(CDotsLoopRule)]),
        "dots_row_loop_hit": (i32, [vp, i32, P(i32)]),
        "dots_loop_probe": (i32, [vp, vp, vp, i32, i32, P(CDotsLoopRule), vp]),
        "dots_set_speculation": (i32, [vp, i32, i32, i32]),
        "dots_set_speculation_rows": (i32, [vp, i32]),
        "dots_set_speculation_guided": (i32, [vp, i32]),
        "dots_set_speculation_shaped": (i32, [vp, i32]),
        "dots_set_speculation_logprobs": (i32, [vp, i32]),
        "dots_op_spec_guide_masks": (i32, [vp, i32, i32, P(i32), P(i32), P(i32), P(i32), P(i32), P(C.c_uint32)]),
        "dots_set_row_drafts": (i32, [vp, i32, P(i32), i32]),
        "dots_spec_stats": (i32, [vp, i32, P(i64), P(i64), P(i64)]),
        "dots_op_ngram_draft": (i32, [vp, vp, vp, i32, i32, i32, i32, i32, vp, vp]),
        "dots_set_row_prediction": (i32, [vp, i32, P(i32), i32]),
        "dots_row_prediction_stats": (i32, [vp, i32, P(i64), P(i64)]),
        "dots_op_predict_draft": (i32, [vp, vp, vp, i32, vp, vp, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp]),
        "dots_set_row_logprobs": (i32, [vp, i32, i32]),
        "dots_row_logprobs": (i32, [vp, i32, i32, i32, P(f32), P(i32), P(f32), P(i32)]),
        "dots_op_logprobs": (i32, [vp, vp, i32, i32, i32, P(i32), vp, vp, vp, vp]),
        "dots_bench_logprobs": (i32, [vp, vp, i32, i32, i32, P(i32), i32, i32, P(f32)]),
        "dots_probe_mfma": (i32, [i32, vp, vp, vp, vp]),
        "dots_probe_grid_barrier": (i32, [i32, i32, i32, i32, i32, P(f32), P(i32)]),
        "dots_probe_cu_mask": (i32, [P(C.c_uint32), i32, i32, i32, i32, P(C.c_uint32)]),
    }


def _prototypes(lib):
    global _SIGNATURES_SET
    if _SIGNATURES_SET:
        return
    older = bool(os.environ.get("DOTS_OCR_LIB"))     # another build of the library (A/B runs): it may predate a symbol, whose call then fails
    for name, (res, args) in _signatures().items():
        fn = getattr(lib, name, None) if older else getattr(lib, name)
        if fn is None:
            continue
        fn.restype = res
        fn.argtypes = args
    _SIGNATURES_SET = True


EXPORTED_SYMBOLS = list(_signatures())

MAX_SPEC_DRAFTS = 15                         # DOTS_MAX_SPEC_DRAFTS: drafts per slot and step; the drafter looks up n-grams of up to MAX_NGRAM_SIZE


def ngram_draft(history: Sequence[int], k: int, min_n: int = 2, max_n: int = 4) -> list:
    """The drafting rule of the speculative step (include/dots_ocr_hip.h), stated on the host: what ngram_draft_kernel must
    produce.  history = the tokens a row has generated, out[0 .. L).  For n from max_n down to min_n with n + 1 <= L the key is the
    suffix out[L - n .. L); among the matches out[i .. i + n) == key with i + n < L the largest i with a full continuation
    (i + n + k <= L) wins, else the smallest i; the draft is out[i + n .. min(i + n + k, L)).  The first n with a match wins."""
    out = [int(t) for t in history]
    L = len(out)
    if k < 1 or min_n < 1 or max_n < min_n:
        raise ValueError("ngram_draft needs k >= 1 and 1 <= min_n <= max_n")
    for n in range(max_n, min_n - 1, -1):
        if n + 1 > L:
            continue
        key = out[L - n:]
        hits = [i for i in range(L - n) if out[i:i + n] == key]
        if not hits:
            continue
        full = [i for i in hits if i + n + k <= L]
        i = max(full) if full else min(hits)
        return out[i + n:min(i + n + k, L)]
    return []


def predicted_draft(out: Sequence[int], pred: Sequence[int], cur: int, at: int, k: int, min_n: int = 2, max_n: int = 4):
    """The drafting rule of predicted outputs (include/dots_ocr_hip.h), stated on the host: what predict_draft_kernel must
    produce.  out = the tokens a row has generated, pred = its prediction, (cur, at) its alignment: prediction index cur was where the
    next token was expected when the output was `at` long, so now it is expected at e* = cur + (L - at).
      1. anchor: m = min(min_n, L, e*); if m >= 1, e* < P and pred[e* - m .. e*) == out[L - m .. L) then e = e*.
      2. search: else for n from min(max_n, L) down to min_n, key = out[L - n .. L); candidates e = i + n < P with pred[i .. i + n) == key;
         the first n with a candidate wins, among them the one nearest to e*, the larger e on a tie.
    -> (drafts, cur, at): found, drafts = pred[e .. min(e + k, P)) with the new alignment (e, L); else (None, cur, at) — the row keeps
    the drafts its own output gave it and the alignment stays."""
    out, pred = [int(t) for t in out], [int(t) for t in pred]
    L, P, cur, at = len(out), len(pred), int(cur), int(at)
    if k < 1 or min_n < 1 or max_n < min_n:
        raise ValueError("predicted_draft needs k >= 1 and 1 <= min_n <= max_n")
    es = cur + (L - at)
    e = None
    m = min(min_n, L, es)
    if m >= 1 and es < P and pred[es - m:es] == out[L - m:]:
        e = es
    if e is None:
        for n in range(min(max_n, L), min_n - 1, -1):
            key = out[L - n:]
            cands = [i + n for i in range(P - n) if pred[i:i + n] == key]
            if cands:
                e = min(cands, key=lambda c: (abs(c - es), -c))
                break
    if e is None:
        return None, cur, at
    return pred[e:min(e + k, P)], e, L


def predicted_run(tokens: Sequence[int], pred: Sequence[int], k: int, min_n: int = 2, max_n: int = 4, cap: Optional[int] = None) -> dict:
    """A row's speculating run replayed on the host.  tokens = everything the row committed in the end (the first token,
    which the prefill selects, included), pred = its prediction (empty: none), cap = its generation cap (default: len(tokens)).  Every
    step commits one token, then walks its live drafts while each equals the token committed before it; then the drafters run: the
    own-output rule (ngram_draft), then predicted_draft, which replaces its drafts where it finds a position.  The drafts a step
    verifies are cut to the tokens the cap leaves room for.  -> {"steps": [{"drafts", "source" ("prediction" | "own" | None), "live",
    "accepted"} per step], "n_steps", "drafted", "accepted" (what dots_spec_stats counts), "pred_drafted", "pred_accepted" (what
    dots_row_prediction_stats counts)}."""
    T, pred = [int(t) for t in tokens], [int(t) for t in pred]
    N = len(T)
    cap = N if cap is None else int(cap)
    if N < 1 or cap < N:
        raise ValueError("predicted_run needs at least the first token and cap >= len(tokens)")
    L, cur, at = 1, 0, 0
    drafts, source = [], None
    steps = []
    tot = {"drafted": 0, "accepted": 0, "pred_drafted": 0, "pred_accepted": 0}
    while L < N:
        live = max(0, min(len(drafts), k, cap - L - 1))
        L += 1                                               # the selection stage commits row 0
        acc = 0
        while acc < live and L < N and drafts[acc] == T[L - 1]:
            L += 1
            acc += 1
        steps.append({"drafts": list(drafts), "source": source if drafts else None, "live": live, "accepted": acc})
        tot["drafted"] += live
        tot["accepted"] += acc
        if source == "prediction" and drafts:
            tot["pred_drafted"] += live
            tot["pred_accepted"] += acc
        drafts, source = [], None
        if L < N:                                            # a finished row drafts nothing
            drafts, source = ngram_draft(T[:L], k, min_n, max_n), "own"
            if pred:
                d, cur, at = predicted_draft(T[:L], pred, cur, at, k, min_n, max_n)
                if d is not None:
                    drafts, source = d, "prediction"
    return {"steps": steps, "n_steps": len(steps), **tot}


def spec_usable_slots(max_batch: int, k: int) -> int:
    """slots a speculating engine can fill: a slot takes k + 1 rows of a step"""
    return int(max_batch) // (int(k) + 1)


SPEC_ROWS = {"sampled": 1, "stop": 2}        # DOTS_SPEC_ROWS_SAMPLED / DOTS_SPEC_ROWS_STOP


def spec_rows_flags(value) -> int:
    """The DOTS_SPEC_ROWS_* bits of a speculative_rows setting: None or "greedy" = 0 (plain greedy rows only), "all" = every bit, or one
    name / a tuple or list of names out of "sampled" and "stop".  ValueError on anything else."""
    if value is None:
        return 0
    names = (value,) if isinstance(value, str) else tuple(value)
    flags = 0
    for n in names:
        if n == "all":
            flags |= sum(SPEC_ROWS.values())
        elif n == "greedy" and len(names) == 1:
            pass
        elif isinstance(n, str) and n in SPEC_ROWS:
            flags |= SPEC_ROWS[n]
        else:
            raise ValueError(f"speculative_rows takes \"all\", \"greedy\" or names out of {sorted(SPEC_ROWS)}, got {value!r}")
    return flags


SPEC_SHAPED = {"ngram": 1, "rules": 2, "penalties": 4}      # DOTS_SPEC_SHAPED_NGRAM / _RULES / _PENALTY


def spec_shaped_flags(value) -> int:
    """The DOTS_SPEC_SHAPED_* bits of a speculative_shaped setting: None, False or "" = 0, True or "all" = every bit, or names out of
    "ngram", "rules" and "penalties" as a comma list, a tuple or a list.  ValueError on anything else."""
    if value is None or value is False or value == "":
        return 0
    if value is True:
        return sum(SPEC_SHAPED.values())
    names = tuple(n.strip() for n in value.split(",")) if isinstance(value, str) else tuple(value)
    flags = 0
    for n in names:
        if n == "all":
            flags |= sum(SPEC_SHAPED.values())
        elif isinstance(n, str) and n in SPEC_SHAPED:
            flags |= SPEC_SHAPED[n]
        else:
            raise ValueError(f"speculative_shaped takes \"all\" or names out of {sorted(SPEC_SHAPED)}, got {value!r}")
    return flags


def draft_row_history(out, drafts, j: int) -> list:
    """The history draft row j >= 1 of a speculating step is selected under ("Why a shaped row is exact"): the tokens the
    row has generated followed by drafts 1 .. j, which the row takes as committed.  banned_ngram_ids(draft_row_history(out, drafts, j),
    n, window, whitelist) is what ngram_ban_drafts_kernel must leave for that row."""
    j = int(j)
    if not 1 <= j <= len(drafts):
        raise ValueError(f"draft row {j} of {len(drafts)} drafts")
    return [int(t) for t in out] + [int(t) for t in drafts[:j]]


def draft_row_counts(counts, drafts, j: int) -> dict:
    """The output counts draft row j >= 1 is penalised with: counts (id -> occurrences in the row's output at the head of the step) plus the
    occurrences among drafts 1 .. j.  The row's own counts are not touched: they move only when a token is committed."""
    j = int(j)
    if not 1 <= j <= len(drafts):
        raise ValueError(f"draft row {j} of {len(drafts)} drafts")
    c = {int(t): int(v) for t, v in dict(counts).items()}
    for t in drafts[:j]:
        c[int(t)] = c.get(int(t), 0) + 1
    return c


STREAM_ROW_CAP = 256                         # DOTS_STREAM_ROW_CAP: tokens one row delivers per slots_drain at the most
MAX_TOP_LOGPROBS = 20                        # DOTS_MAX_TOP_LOGPROBS: top entries kept per position

KV_CACHE_DTYPES = {"bf16": 0, "fp8": 1}      # DotsConfig.kv_cache_dtype; "fp8" = OCP e4m3fn (vLLM's --kv-cache-dtype fp8)


def resolve_kv_cache_dtype(kv_cache_dtype: Optional[str]) -> str:
    """"bf16" | "fp8"; None reads DOTS_OCR_KV_CACHE_DTYPE (unset or empty = bf16).  Anything else raises ValueError."""
    if kv_cache_dtype is None:
        kv_cache_dtype = os.environ.get("DOTS_OCR_KV_CACHE_DTYPE", "") or "bf16"
    if kv_cache_dtype not in KV_CACHE_DTYPES:
        raise ValueError(f"kv_cache_dtype must be one of {sorted(KV_CACHE_DTYPES)}, got {kv_cache_dtype!r}")
    return kv_cache_dtype


def c_config(cfg: DotsConfig, max_batch: int, max_seq_len: int, max_patches: int, max_prefill_tokens: int, kv_pool_tokens: int = 0,
             fp8_weights: bool = False, kv_cache_dtype: str = "bf16") -> CDotsConfig:
    v = cfg.vision
    return CDotsConfig(
        hidden_size=cfg.hidden_size, num_layers=cfg.num_hidden_layers, num_heads=cfg.num_attention_heads,
        num_kv_heads=cfg.num_key_value_heads, head_dim=cfg.head_dim, intermediate_size=cfg.intermediate_size,
        vocab_size=cfg.vocab_size, rope_theta=cfg.rope_theta, rms_norm_eps=cfg.rms_norm_eps,
        attention_bias=int(cfg.attention_bias), image_token_id=cfg.image_token_id,
        v_embed_dim=v.embed_dim, v_layers=v.num_hidden_layers, v_heads=v.num_attention_heads,
        v_intermediate=v.intermediate_size, v_patch=v.patch_size, v_merge=v.spatial_merge_size,
        v_channels=v.num_channels, v_temporal_patch=v.temporal_patch_size, v_rms_eps=v.rms_norm_eps,
        v_ln_eps=v.merger_ln_eps, v_use_bias=int(v.use_bias), v_post_norm=int(v.post_norm),
        max_batch=max_batch, max_seq_len=max_seq_len, max_patches=max_patches,
        max_prefill_tokens=max_prefill_tokens, kv_pool_tokens=kv_pool_tokens, fp8_weights=int(bool(fp8_weights)),
        kv_cache_dtype=KV_CACHE_DTYPES[kv_cache_dtype])


def plan_flash_xcd(lens: Sequence[int], heads: int):
    """Host-only: (base[8], cnt[8], cost[8], n_items) — how the flash-attention work list of a packed batch of sequences of `lens` patches
    is cut across the XCDs (dots_plan_flash_xcd: equal KV-tile cost per XCD).  Needs the library, not a GPU."""
    lib = _lib.load()
    _prototypes(lib)
    L = np.ascontiguousarray(lens, dtype=np.int32)
    base, cnt, cost = np.zeros(8, np.int32), np.zeros(8, np.int32), np.zeros(8, np.int64)
    n = lib.dots_plan_flash_xcd(_i32p(L), int(L.shape[0]), int(heads), _i32p(base), _i32p(cnt), _i64p(cost))
    if n < 0:
        raise DotsEngineError(f"dots_plan_flash_xcd failed ({n})")
    return base, cnt, cost, int(n)


def plan_shared_prefix(active: Sequence[int], block_table, static_pages: Sequence[int], n_splits: int, waves: int = 4):
    """Host-only: the shared-prefix attention plan (dots_plan_shared_prefix) of a step over the rows of block_table
    [rows, max_pages] -> (items, masks): items = [(split, [member rows ascending]), ...] split by split, masks[b] = the splits of row b
    that an item covers, as bits.  Needs the library, not a GPU."""
    lib = _lib.load()
    _prototypes(lib)
    table = np.ascontiguousarray(block_table, dtype=np.int32)
    act = np.ascontiguousarray(active, dtype=np.int32)
    stat = np.ascontiguousarray(static_pages, dtype=np.int32)
    rows, max_pages = table.shape
    assert act.shape == stat.shape == (rows,)
    items3 = np.zeros(3 * 32 * max(int(n_splits), 1), np.int32)
    members = np.zeros(max(rows * int(n_splits), 1), np.int32)
    masks = np.zeros(rows, np.uint64)
    n = lib.dots_plan_shared_prefix(_i32p(act), _i32p(table), int(max_pages), _i32p(stat), int(rows), int(n_splits), int(waves), _i32p(items3),
                                    _i32p(members), masks.ctypes.data_as(C.POINTER(C.c_uint64)))
    if n < 0:
        raise DotsEngineError(f"dots_plan_shared_prefix failed ({n})")
    items = [(int(items3[3 * k]), [int(r) for r in members[items3[3 * k + 1]:items3[3 * k + 1] + items3[3 * k + 2]]]) for k in range(n)]
    return items, [int(m) for m in masks]


def _i32p(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def _i64p(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_int64))


class Engine:
    """One GPU, one HIP stream, one model replica."""

    def __init__(self, cfg: DotsConfig, device: int = 0, max_batch: int = 8, max_seq_len: int = 8192,
                 max_patches: int = 8 * 19824 + 64, max_prefill_tokens: Optional[int] = None, kv_pool_tokens: int = 0,
                 fp8_weights: bool = False, kv_cache_dtype: Optional[str] = None):
        # kv_cache_dtype: "bf16" | "fp8" (e4m3fn paged KV cache, include/dots_ocr_hip.h DotsConfig.kv_cache_dtype); None = $DOTS_OCR_KV_CACHE_DTYPE or bf16
        self.kv_cache_dtype = resolve_kv_cache_dtype(kv_cache_dtype)        # before the library or the GPU is touched
        self.lib = _lib.load()
        _prototypes(self.lib)
        self.cfg = cfg
        self.device = device
        self.max_batch = max_batch
        self.max_seq_len = max_seq_len
        self.max_patches = max_patches
        if max_prefill_tokens is None:
            max_prefill_tokens = max_batch * max_seq_len
        self.max_prefill_tokens = max_prefill_tokens
        self.kv_pool_tokens = kv_pool_tokens
        self.fp8_weights = bool(fp8_weights)
        self._cc = c_config(cfg, max_batch, max_seq_len, max_patches, max_prefill_tokens, kv_pool_tokens, fp8_weights, self.kv_cache_dtype)
        h = C.c_void_p()
        rc = self.lib.dots_create(C.byref(self._cc), device, C.byref(h))
        if rc != 0:
            raise DotsEngineError(f"dots_create failed ({rc}): {self.lib.dots_last_error(None).decode()}")
        self.h = h
        self.token_bytes = None                  # guided.TokenBytes once set_token_bytes has run
        self._stops = OrderedDict()              # tuple of stop strings -> handle (create_stop): a small LRU of uploaded automata
        self._drain_tok = None                   # slots_drain's host buffers, kept between calls: tokens, and — once a row has had logprobs
        self._drain_lp = None                    # switched on (_drain_wants_lp) — the three logprob arrays
        self._drain_wants_lp = False

    # ------------------------------------------------------------------ plumbing
    def _ck(self, rc: int, what: str):
        if rc != 0:
            err = DotsEngineError(f"{what} failed ({rc}): {self.lib.dots_last_error(self.h).decode()}")
            err.code = rc                            # the DOTS_E_* code: E_STATE / E_CAPACITY tell a refusal from a failure
            raise err

    def close(self):
        if getattr(self, "h", None):
            self.lib.dots_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def stream(self) -> int:
        return int(self.lib.dots_stream(self.h) or 0)

    def synchronize(self):
        self._ck(self.lib.dots_synchronize(self.h), "dots_synchronize")

    # ------------------------------------------------------------------ weights
    def load_state_dict(self, sd: Dict[str, "torch.Tensor"]):  # noqa: F821 (torch only used by the caller)
        import torch
        dt = {torch.bfloat16: DTYPE_BF16, torch.float32: DTYPE_F32, torch.float16: DTYPE_F16}
        for name, t in sd.items():
            t = t.detach().cpu().contiguous()
            if t.dtype not in dt:
                t = t.float()
            shape = (C.c_int64 * t.dim())(*t.shape)
            self._ck(self.lib.dots_load_weight(self.h, name.encode(), C.c_void_p(t.data_ptr()), dt[t.dtype], shape, t.dim()),
                     f"dots_load_weight({name})")
        self._ck(self.lib.dots_finalize_weights(self.h), "dots_finalize_weights")

    # ------------------------------------------------------------------ device memory helpers
    def dev_alloc(self, nbytes: int) -> int:
        p = C.c_void_p()
        self._ck(self.lib.dots_dev_alloc(self.h, nbytes, C.byref(p)), "dots_dev_alloc")
        return int(p.value)

    def dev_free(self, ptr: int):
        self._ck(self.lib.dots_dev_free(self.h, C.c_void_p(ptr)), "dots_dev_free")

    def to_device(self, a: np.ndarray) -> int:
        a = np.ascontiguousarray(a)
        p = self.dev_alloc(a.nbytes)
        self._ck(self.lib.dots_memcpy_h2d(self.h, C.c_void_p(p), a.ctypes.data_as(C.c_void_p), a.nbytes), "dots_memcpy_h2d")
        return p

    def copy_to_device(self, ptr: int, a: np.ndarray):
        """host array -> an existing device buffer (blocking)"""
        a = np.ascontiguousarray(a)
        self._ck(self.lib.dots_memcpy_h2d(self.h, C.c_void_p(ptr), a.ctypes.data_as(C.c_void_p), a.nbytes), "dots_memcpy_h2d")

    def to_host(self, ptr: int, shape: Sequence[int], dtype) -> np.ndarray:
        out = np.empty(shape, dtype=dtype)
        self._ck(self.lib.dots_memcpy_d2h(self.h, out.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), out.nbytes), "dots_memcpy_d2h")
        return out

    # ------------------------------------------------------------------ hot path
    def vit_forward(self, pixel_values, grid_thw: np.ndarray, on_device: bool = False, out_dev: int = 0) -> int:
        """pixel_values: np.float32 [N, patch_dim] (host) or a device pointer when on_device."""
        grid = np.ascontiguousarray(grid_thw, dtype=np.int64)
        n = int((grid[:, 0] * grid[:, 1] * grid[:, 2]).sum())
        if on_device:
            ptr = C.c_void_p(int(pixel_values))
        else:
            pv = np.ascontiguousarray(pixel_values, dtype=np.float32)
            assert pv.shape[0] == n, (pv.shape, n)
            ptr = pv.ctypes.data_as(C.c_void_p)
        self._ck(self.lib.dots_vit_forward(self.h, ptr, int(on_device), n, _i64p(grid), grid.shape[0],
                                           C.c_void_p(out_dev) if out_dev else None), "dots_vit_forward")
        return n // (self.cfg.vision.spatial_merge_size ** 2)

    def vit_prefetch(self, pixel_values, grid_thw: np.ndarray, on_device: bool = False, after_prefill: bool = False) -> int:
        """The tower of the NEXT page batch, asynchronously on the CU-masked side stream (include/dots_ocr_hip.h "Software
        pipelining"); pixel_values must stay alive until vit_take().  after_prefill: launch it behind the next prefill."""
        grid = np.ascontiguousarray(grid_thw, dtype=np.int64)
        n = int((grid[:, 0] * grid[:, 1] * grid[:, 2]).sum())
        if on_device:
            ptr = C.c_void_p(int(pixel_values))
        else:
            self._pref_keep = np.ascontiguousarray(pixel_values, dtype=np.float32)
            assert self._pref_keep.shape[0] == n, (self._pref_keep.shape, n)
            ptr = self._pref_keep.ctypes.data_as(C.c_void_p)
        self._ck(self.lib.dots_vit_prefetch(self.h, ptr, int(on_device), n, _i64p(grid), grid.shape[0], int(after_prefill)), "dots_vit_prefetch")
        return n // (self.cfg.vision.spatial_merge_size ** 2)

    def vit_take(self):
        """Put the prefetched vision rows in place for the next prefill / generate(..., vision_taken=True)."""
        self._ck(self.lib.dots_vit_take_prefetched(self.h), "dots_vit_take_prefetched")

    def vit_ready(self) -> bool:
        """True when the prefetched tower has finished: vit_take() then makes nothing wait (a serving loop keeps decoding until then)."""
        r = C.c_int32(0)
        self._ck(self.lib.dots_vit_prefetch_ready(self.h, C.byref(r)), "dots_vit_prefetch_ready")
        return bool(r.value)

    def preprocess_image(self, rgb, out_dev: int, min_pixels: Optional[int] = None, max_pixels: Optional[int] = None,
                         shape: Optional[Sequence[int]] = None):
        """uint8 [h, w, 3] image -> float32 patches written at device pointer `out_dev`; returns [t, gh, gw].
        `rgb` is a host numpy array, or (with shape=(h, w)) a device pointer to the uint8 pixels already in HBM.
        Bit-identical to image_utils.preprocess_image (Pillow BICUBIC + normalise + patchify), computed on the GPU."""
        from .image_utils import bicubic_resample_tables, smart_resize
        on_device = shape is not None
        if on_device:
            h, w = int(shape[0]), int(shape[1])
            rgb_ptr = C.c_void_p(int(rgb))
        else:
            rgb = np.ascontiguousarray(rgb, dtype=np.uint8)
            h, w, _ = rgb.shape
            rgb_ptr = rgb.ctypes.data_as(C.c_void_p)
        v = self.cfg.vision
        rh, rw = smart_resize(h, w, v.patch_size * v.spatial_merge_size, min_pixels or self.cfg.min_pixels, max_pixels or self.cfg.max_pixels)
        hc = hb = vc = vb = None
        hk = vk = 0
        if rw != w:
            hc, hb = bicubic_resample_tables(w, rw)
            hk = hc.shape[1]
        if rh != h:
            vc, vb = bicubic_resample_tables(h, rh)
            vk = vc.shape[1]
        mean = np.asarray(self.cfg.image_mean, np.float32)
        std = np.asarray(self.cfg.image_std, np.float32)
        fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
        self._ck(self.lib.dots_preprocess_image(
            self.h, rgb_ptr, int(on_device), h, w, rh, rw,
            _i32p(hc) if hc is not None else None, _i32p(hb) if hb is not None else None, hk,
            _i32p(vc) if vc is not None else None, _i32p(vb) if vb is not None else None, vk,
            fp(mean), fp(std), float(np.float32(1.0 / 255.0)), C.c_void_p(out_dev)), "dots_preprocess_image")
        return [1, rh // v.patch_size, rw // v.patch_size]

    def prefill(self, input_ids: np.ndarray, prompt_lens: np.ndarray):
        ids = np.ascontiguousarray(input_ids, dtype=np.int32)
        lens = np.ascontiguousarray(prompt_lens, dtype=np.int32)
        assert ids.shape[0] == int(lens.sum())
        self._ck(self.lib.dots_prefill(self.h, _i32p(ids), _i32p(lens), lens.shape[0]), "dots_prefill")
        self._B = int(lens.shape[0])

    def set_sampling(self, temperature: float = 0.0, top_p: float = 1.0, seed: int = 0):
        """temperature 0 = greedy; otherwise softmax(logits/T) restricted to the top_p nucleus, reproducible from seed."""
        self._ck(self.lib.dots_set_sampling(self.h, float(temperature), float(top_p), int(seed) & (2 ** 64 - 1)), "dots_set_sampling")

    def set_row_sampling(self, row: int, params: Optional[SamplingParams]):
        """Give decode row `row` (a slot, or sequence `row` of a static batch) its own SamplingParams from the next selected token on;
        None returns it to the set_sampling setting.  Captured decode graphs are kept.  Set a row's penalties BEFORE its prefill: for a
        penalty switched on mid-run, only tokens selected after the switch are counted, and the prompt counts only if some row had used a
        penalty before that row's prefill (include/dots_ocr_hip.h)."""
        if params is None:
            self._ck(self.lib.dots_set_row_sampling(self.h, int(row), None), "dots_set_row_sampling")
            return
        if not isinstance(params, SamplingParams):
            raise TypeError("params must be a SamplingParams or None")
        c = params.to_c()
        self._ck(self.lib.dots_set_row_sampling(self.h, int(row), C.byref(c)), "dots_set_row_sampling")

    def select_tokens(self, logits, B: int, V: int, params: Sequence[SamplingParams], hist, hist_lens, hist_stride: int, n_prompt, out_tokens):
        """The per-row selection stage on device buffers (dots_op_select_tokens): logits fp32 [B, V], hist int32 [B, hist_stride]
        (prompt ids then generated ids), hist_lens / n_prompt / out_tokens int32 [B]."""
        if len(params) != B:
            raise ValueError("one SamplingParams per row")
        arr = (CDotsSamplingParams * B)(*[p.to_c() for p in params])
        self._ck(self.lib.dots_op_select_tokens(self.h, logits, int(B), int(V), arr, hist, hist_lens, int(hist_stride), n_prompt, out_tokens),
                 "dots_op_select_tokens")

    def bench_select_tokens(self, logits, B: int, V: int, params: Sequence[SamplingParams], hist, hist_lens, hist_stride: int, n_prompt,
                            mode: int, iters: int) -> float:
        """mean ms of one selection stage: mode 0 = arg max pair, 1 = engine-wide sampler (params[0]), 2 = per-row stage"""
        arr = (CDotsSamplingParams * B)(*[p.to_c() for p in params])
        ms = C.c_float()
        self._ck(self.lib.dots_bench_select_tokens(self.h, logits, int(B), int(V), arr, hist, hist_lens, int(hist_stride), n_prompt, int(mode),
                                                   int(iters), C.byref(ms)), "dots_bench_select_tokens")
        return float(ms.value)

    def set_row_logit_rules(self, row: int, rules: Optional["LogitRules"]):
        """Give decode row `row` (a slot, or sequence `row` of a static batch) LogitRules from the next selected token on (set, then
        prefill); None or empty rules clear them.  Captured decode graphs are kept; slot release and slots_reset clear the row.  A row
        with rules but no SamplingParams of its own is selected with the engine-wide temperature / top_p / seed as they stand now
        (DESIGN §6.3)."""
        if rules is None or (isinstance(rules, LogitRules) and rules.empty):
            self._ck(self.lib.dots_set_row_logit_rules(self.h, int(row), None), "dots_set_row_logit_rules")
            return
        if not isinstance(rules, LogitRules):
            raise TypeError("rules must be a LogitRules or None")
        c = rules.to_c()
        self._ck(self.lib.dots_set_row_logit_rules(self.h, int(row), C.byref(c)), "dots_set_row_logit_rules")

    @staticmethod
    def _rules_array(rules: Sequence[Optional["LogitRules"]]):
        cs = [(r if r is not None else LogitRules()).to_c() for r in rules]
        arr = (CDotsLogitRules * len(cs))(*cs)
        arr._keep = cs
        return arr

    def select_tokens_rules(self, logits, B: int, V: int, params: Sequence[SamplingParams], rules: Sequence[Optional["LogitRules"]],
                            n_gen: Optional[Sequence[int]], hist, hist_lens, hist_stride: int, n_prompt, out_tokens):
        """select_tokens with LogitRules per row (None / empty = a row without rules) and each row's generated count n_gen (None:
        hist_lens - n_prompt); the engine's EOS ids are live (dots_op_select_tokens_rules)."""
        if len(params) != B or len(rules) != B:
            raise ValueError("one SamplingParams and one LogitRules (or None) per row")
        arr = (CDotsSamplingParams * B)(*[p.to_c() for p in params])
        rarr = self._rules_array(rules)
        ng = None if n_gen is None else np.ascontiguousarray(n_gen, dtype=np.int32)
        self._ck(self.lib.dots_op_select_tokens_rules(self.h, logits, int(B), int(V), arr, rarr, None if ng is None else _i32p(ng), hist, hist_lens,
                                                      int(hist_stride), n_prompt, out_tokens), "dots_op_select_tokens_rules")

    def bench_select_tokens_rules(self, logits, B: int, V: int, params: Sequence[SamplingParams], rules: Sequence[Optional["LogitRules"]],
                                  n_gen: Optional[Sequence[int]], hist, hist_lens, hist_stride: int, n_prompt, iters: int) -> float:
        """mean ms of one per-row selection stage with these rules"""
        arr = (CDotsSamplingParams * B)(*[p.to_c() for p in params])
        rarr = self._rules_array(rules)
        ng = None if n_gen is None else np.ascontiguousarray(n_gen, dtype=np.int32)
        ms = C.c_float()
        self._ck(self.lib.dots_bench_select_tokens_rules(self.h, logits, int(B), int(V), arr, rarr, None if ng is None else _i32p(ng), hist,
                                                         hist_lens, int(hist_stride), n_prompt, int(iters), C.byref(ms)),
                 "dots_bench_select_tokens_rules")
        return float(ms.value)

    # ------------------------------------------------------------------ guided decoding
    def set_token_bytes(self, tokens, special_ids: Sequence[int] = ()):
        """The bytes of every vocabulary entry, once per engine: a guided.TokenBytes, or a sequence of vocab_size bytes objects.  Ids in
        special_ids (chat and image tokens) and entries without bytes can never be selected on a guided row."""
        from .guided import TokenBytes
        tb = tokens if isinstance(tokens, TokenBytes) and not special_ids else TokenBytes(
            [tokens.token(t) for t in range(tokens.vocab_size)] if isinstance(tokens, TokenBytes) else tokens, special_ids)
        if tb.vocab_size != self.cfg.vocab_size:
            raise ValueError(f"token bytes for {tb.vocab_size} entries, the engine's vocabulary has {self.cfg.vocab_size}")
        off = np.ascontiguousarray(tb.offsets, dtype=np.int32)
        data = np.ascontiguousarray(tb.data, dtype=np.uint8)
        self._ck(self.lib.dots_set_token_bytes(self.h, _i32p(off), data.ctypes.data_as(C.c_void_p) if data.size else None), "dots_set_token_bytes")
        self.token_bytes = tb

    def create_guide(self, guide) -> int:
        """Upload a guided.Guide; returns the handle set_row_guide takes.  Any number of rows may hold one guide."""
        table = np.ascontiguousarray(guide.table, dtype=np.uint16)
        acc = np.ascontiguousarray(guide.accepting, dtype=np.uint8)
        if table.ndim != 2 or table.shape[1] != 256 or acc.shape != (table.shape[0],):
            raise ValueError("a guide's table must be uint16 [S, 256] with accepting uint8 [S]")
        gid = C.c_int32(-1)
        self._ck(self.lib.dots_guide_create(self.h, table.ctypes.data_as(C.c_void_p), int(table.shape[0]), acc.ctypes.data_as(C.c_void_p),
                                            int(guide.start), C.byref(gid)), "dots_guide_create")
        return int(gid.value)

    def destroy_guide(self, handle: int):
        """Free a guide; refused (DotsEngineError) while a row holds it."""
        self._ck(self.lib.dots_guide_destroy(self.h, int(handle)), "dots_guide_destroy")

    def set_row_guide(self, row: int, handle: Optional[int]):
        """Row `row` (a slot, or sequence `row` of a static batch) follows the guide from its start state, from the next selected token on
        (set, then prefill: the prefill starts the automaton over and selects its first token under the guide); None clears.  Captured
        decode graphs are kept; slot release and slots_reset clear the row.  Needs set_token_bytes first."""
        self._ck(self.lib.dots_set_row_guide(self.h, int(row), -1 if handle is None else int(handle)), "dots_set_row_guide")

    def row_guide_state(self, row: int) -> int:
        """the state of the row's automaton, -1 for a row without a guide"""
        st = C.c_int32(-1)
        self._ck(self.lib.dots_row_guide_state(self.h, int(row), C.byref(st)), "dots_row_guide_state")
        return int(st.value)

    # ------------------------------------------------------------------ stop strings
    STOP_CACHE = 32                              # automata kept on the engine, keyed by their strings

    def create_stop(self, strings) -> int:
        """Upload the automaton of 1 .. 16 stop strings (a list of str, or a stop_strings.StopAutomaton); returns the handle set_row_stop
        takes.  Handles are cached by the tuple of strings, so a server does not upload half a megabyte per request; the least recently
        used automaton no row holds is freed when the cache is full.  Needs set_token_bytes first; bad strings raise ValueError."""
        from .stop_strings import StopAutomaton, compile_stop
        key = strings.strings if isinstance(strings, StopAutomaton) else None
        if key is None:
            from .stop_strings import check_stop_strings
            key = check_stop_strings(strings)
        h = self._stops.get(key)
        if h is not None:
            self._stops.move_to_end(key)
            return h
        a = strings if isinstance(strings, StopAutomaton) else compile_stop(key)
        table = np.ascontiguousarray(a.table, dtype=np.uint16)
        mlen = np.ascontiguousarray(a.match_len, dtype=np.uint16)
        mid = np.ascontiguousarray(a.match_id, dtype=np.uint8)
        if table.ndim != 2 or table.shape[1] != 256 or mlen.shape != (table.shape[0],) or mid.shape != mlen.shape:
            raise ValueError("a stop automaton's table must be uint16 [S, 256] with match_len uint16 [S] and match_id uint8 [S]")
        hid = C.c_int32(0)
        self._ck(self.lib.dots_stop_create(self.h, table.ctypes.data_as(C.c_void_p), int(table.shape[0]), mlen.ctypes.data_as(C.c_void_p),
                                           mid.ctypes.data_as(C.c_void_p), C.byref(hid)), "dots_stop_create")
        for old in list(self._stops)[:max(0, len(self._stops) + 1 - self.STOP_CACHE)]:
            if self.lib.dots_stop_destroy(self.h, int(self._stops[old])) == 0:       # refused while a row holds it: it stays cached
                del self._stops[old]
        self._stops[key] = int(hid.value)
        return int(hid.value)

    def destroy_stop(self, handle: int):
        """Free an automaton; refused (DotsEngineError) while a row holds it."""
        self._ck(self.lib.dots_stop_destroy(self.h, int(handle)), "dots_stop_destroy")
        for k in [k for k, h in self._stops.items() if h == int(handle)]:
            del self._stops[k]

    def set_row_stop(self, row: int, handle: Optional[int], min_tokens: int = 0):
        """Row `row` (a slot, or sequence `row` of a static batch) ends at the token that completes one of the automaton's strings, taken
        only at token index >= min_tokens (set, then prefill: the prefill starts the automaton over, clears the hit and walks its first
        token); None or 0 clears.  Captured decode graphs are kept; slot release and slots_reset clear the row, slots_fork hands the
        source's automaton to its children."""
        self._ck(self.lib.dots_set_row_stop(self.h, int(row), int(handle or 0), int(min_tokens)), "dots_set_row_stop")

    def row_stop_hit(self, row: int):
        """(token index, bytes of that token consumed, match length in bytes, match id) of the row's stop, or None: no hit (yet)"""
        out = (C.c_int32 * 4)(-1, 0, 0, -1)
        self._ck(self.lib.dots_row_stop_hit(self.h, int(row), out), "dots_row_stop_hit")
        return None if out[0] < 0 else (int(out[0]), int(out[1]), int(out[2]), int(out[3]))

    # ------------------------------------------------------------------ loop guard
    @staticmethod
    def _loop_c(rule) -> CDotsLoopRule:
        from .loop_guard import LoopRule
        if not isinstance(rule, LoopRule):
            raise TypeError("rule must be a loop_guard.LoopRule or None")
        return CDotsLoopRule(rule.min_period, rule.max_period, rule.repeats, rule.min_span)

    def set_row_loop(self, row: int, rule):
        """Row `row` (a slot, or sequence `row` of a static batch) ends at the token after which its output has repeated with some period
        for the rule's span (loop_guard.LoopRule; set, then prefill: the window is the output since it last started over); None clears.
        The first call allocates the counters and drops the captured decode graphs once, later calls keep them; slot release and
        slots_reset clear the row, slots_fork hands the source's rule to its children.  A row with a rule verifies no draft."""
        if rule is None:
            self._ck(self.lib.dots_set_row_loop(self.h, int(row), None), "dots_set_row_loop")
            return
        c = self._loop_c(rule)
        self._ck(self.lib.dots_set_row_loop(self.h, int(row), C.byref(c)), "dots_set_row_loop")

    def row_loop_hit(self, row: int):
        """(index of the firing token, period, span) of the row's loop hit, or None: no hit (yet)"""
        out = (C.c_int32 * 3)(-1, 0, 0)
        self._ck(self.lib.dots_row_loop_hit(self.h, int(row), out), "dots_row_loop_hit")
        return None if out[0] < 0 else (int(out[0]), int(out[1]), int(out[2]))

    def loop_probe(self, ids, lens, rule):
        """The device check over explicit histories (a test entry): ids int32 [cases, stride], lens [cases]; returns one
        (n, period, span) or None per case, as first_loop of loop_guard states it."""
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        lens = np.ascontiguousarray(lens, dtype=np.int32)
        if ids.ndim != 2 or lens.shape != (ids.shape[0],):
            raise ValueError("ids must be [cases, stride] and lens [cases]")
        c = self._loop_c(rule)
        hits = np.empty((ids.shape[0], 3), dtype=np.int32)
        self._ck(self.lib.dots_loop_probe(self.h, ids.ctypes.data_as(C.c_void_p), lens.ctypes.data_as(C.c_void_p), int(ids.shape[0]), int(ids.shape[1]),
                                          C.byref(c), hits.ctypes.data_as(C.c_void_p)), "dots_loop_probe")
        return [None if h[0] < 0 else (int(h[0]), int(h[1]), int(h[2])) for h in hits]

    def _guided_args(self, B, params, rules, n_gen, guides, states):
        if len(params) != B or len(rules) != B or len(guides) != B or len(states) != B:
            raise ValueError("one SamplingParams, LogitRules (or None), guide handle (or None) and state per row")
        arr = (CDotsSamplingParams * B)(*[p.to_c() for p in params])
        rarr = self._rules_array(rules)
        ng = None if n_gen is None else np.ascontiguousarray(n_gen, dtype=np.int32)
        gid = np.ascontiguousarray([-1 if g is None else int(g) for g in guides], dtype=np.int32)
        st = np.ascontiguousarray([0 if g is None else int(s) for g, s in zip(guides, states)], dtype=np.int32)
        return arr, rarr, ng, gid, st

    def select_tokens_guided(self, logits, B: int, V: int, params: Sequence[SamplingParams], rules: Sequence[Optional["LogitRules"]],
                             n_gen: Optional[Sequence[int]], guides: Sequence[Optional[int]], states: Sequence[int], hist, hist_lens,
                             hist_stride: int, n_prompt, out_tokens) -> np.ndarray:
        """select_tokens_rules with a guide handle (None = an unguided row) and an explicit automaton state per row; V must be the engine's
        vocabulary.  Returns the rows' states after the commit (-1 for an unguided row)."""
        arr, rarr, ng, gid, st = self._guided_args(B, params, rules, n_gen, guides, states)
        out = np.full((B,), -1, np.int32)
        self._ck(self.lib.dots_op_select_tokens_guided(self.h, logits, int(B), int(V), arr, rarr, None if ng is None else _i32p(ng), _i32p(gid), _i32p(st),
                                                       hist, hist_lens, int(hist_stride), n_prompt, out_tokens, _i32p(out)), "dots_op_select_tokens_guided")
        return out

    def bench_select_tokens_guided(self, logits, B: int, V: int, params: Sequence[SamplingParams], rules: Sequence[Optional["LogitRules"]],
                                   n_gen: Optional[Sequence[int]], guides: Sequence[Optional[int]], states: Sequence[int], hist, hist_lens,
                                   hist_stride: int, n_prompt, iters: int) -> float:
        """mean ms of one per-row selection stage with these guides, the mask kernel included"""
        arr, rarr, ng, gid, st = self._guided_args(B, params, rules, n_gen, guides, states)
        ms = C.c_float()
        self._ck(self.lib.dots_bench_select_tokens_guided(self.h, logits, int(B), int(V), arr, rarr, None if ng is None else _i32p(ng), _i32p(gid),
                                                          _i32p(st), hist, hist_lens, int(hist_stride), n_prompt, int(iters), C.byref(ms)),
                 "dots_bench_select_tokens_guided")
        return float(ms.value)

    # ------------------------------------------------------------------ no-repeat n-gram blocking
    def set_row_ngram(self, row: int, rule: Optional["NgramRule"]):
        """Give decode row `row` (a slot, or sequence `row` of a static batch) an NgramRule from the next selected token on; None clears
        it.  Exact for a row that is already running: the ban is computed on the device from the row's own output at every step.
        Captured decode graphs are kept; slot release and slots_reset clear the row.  A row with a rule but no SamplingParams of its own
        is selected with the engine-wide temperature / top_p / seed as they stand now."""
        if rule is None:
            self._ck(self.lib.dots_set_row_ngram(self.h, int(row), None), "dots_set_row_ngram")
            return
        if not isinstance(rule, NgramRule):
            raise TypeError("rule must be an NgramRule or None")
        c = rule.to_c()
        self._ck(self.lib.dots_set_row_ngram(self.h, int(row), C.byref(c)), "dots_set_row_ngram")

    def _ngram_args(self, B, params, rules, ngrams):
        if len(params) != B or len(rules) != B or len(ngrams) != B:
            raise ValueError("one SamplingParams, LogitRules (or None) and NgramRule (or None) per row")
        arr = (CDotsSamplingParams * B)(*[p.to_c() for p in params])
        rarr = self._rules_array(rules)
        narr = (CDotsNgramRule * B)(*[CDotsNgramRule() if g is None else g.to_c() for g in ngrams])
        return arr, rarr, narr

    def select_tokens_ngram(self, logits, B: int, V: int, params: Sequence[SamplingParams], rules: Sequence[Optional["LogitRules"]],
                            ngrams: Sequence[Optional["NgramRule"]], hist, hist_lens, hist_stride: int, n_prompt, out_tokens):
        """select_tokens_rules with an NgramRule per row (None = a row without); a row's history is hist[n_prompt .. hist_lens)
        (dots_op_select_tokens_ngram)."""
        arr, rarr, narr = self._ngram_args(B, params, rules, ngrams)
        self._ck(self.lib.dots_op_select_tokens_ngram(self.h, logits, int(B), int(V), arr, rarr, narr, hist, hist_lens, int(hist_stride), n_prompt,
                                                      out_tokens), "dots_op_select_tokens_ngram")

    def bench_select_tokens_ngram(self, logits, B: int, V: int, params: Sequence[SamplingParams], rules: Sequence[Optional["LogitRules"]],
                                  ngrams: Sequence[Optional["NgramRule"]], hist, hist_lens, hist_stride: int, n_prompt, iters: int) -> float:
        """mean ms of one per-row selection stage with these n-gram rules, the ban kernel included"""
        arr, rarr, narr = self._ngram_args(B, params, rules, ngrams)
        ms = C.c_float()
        self._ck(self.lib.dots_bench_select_tokens_ngram(self.h, logits, int(B), int(V), arr, rarr, narr, hist, hist_lens, int(hist_stride), n_prompt,
                                                         int(iters), C.byref(ms)), "dots_bench_select_tokens_ngram")
        return float(ms.value)

    # ------------------------------------------------------------------ n-gram speculative decoding
    def set_speculation(self, k: int, min_n: int = 2, max_n: int = 4):
        """k drafts per slot and decode step for the plain greedy rows of the continuous path (0 = off, the default); the built-in drafter
        continues the row's longest repeated suffix n-gram, min_n <= n <= max_n (max_n = 0: no drafter, set_row_drafts only).  Tokens are
        exactly those of the unspeculated engine.  Only while no slot is occupied; the usable slots become usable_slots.  generate()
        (the static batch) ignores it."""
        k = int(k)
        if not 0 <= k <= MAX_SPEC_DRAFTS:
            raise ValueError(f"k must be in [0, {MAX_SPEC_DRAFTS}], got {k!r}")
        self._ck(self.lib.dots_set_speculation(self.h, k, int(min_n), int(max_n)), "dots_set_speculation")
        self.spec_k = k

    def set_speculation_rows(self, sampled: bool = False, stop: bool = False):
        """Which rows beside the plain greedy ones verify drafts: sampled = rows with SamplingParams that carry no penalty
        (any temperature, top_k, top_p, seed: the draft rows are drawn by the row's own sampler with the counter of their output index, so
        the tokens are those of the unspeculated engine for the same seed), stop = rows with stop strings (the row ends at the same token).
        A row with both needs both.  Default: neither.  Only while no slot is occupied; the setting survives set_speculation."""
        flags = (SPEC_ROWS["sampled"] if sampled else 0) | (SPEC_ROWS["stop"] if stop else 0)
        self._ck(self.lib.dots_set_speculation_rows(self.h, flags), "dots_set_speculation_rows")
        self.spec_rows = flags

    spec_guided = False                      # Engine.set_speculation_guided: off until switched on

    def set_speculation_guided(self, on: bool = True):
        """May a row that holds a guide verify drafts?  Off by default.  A guide's state depends on the committed tokens
        only, so every draft row is selected under the state the sequential engine would hold there: the tokens are those of the
        unspeculated engine.  A guided row with SamplingParams also needs set_speculation_rows(sampled=True), one with stop strings
        stop=True.  Only while no slot is occupied; the setting survives set_speculation."""
        self._ck(self.lib.dots_set_speculation_guided(self.h, 1 if on else 0), "dots_set_speculation_guided")
        self.spec_guided = bool(on)

    spec_shaped = 0                          # Engine.set_speculation_shaped: the DOTS_SPEC_SHAPED_* bits, 0 until switched on

    def set_speculation_shaped(self, ngram: bool = False, rules: bool = False, penalties: bool = False):
        """Which rows whose logits are shaped verify drafts: ngram = rows with an NgramRule, rules = rows with LogitRules,
        penalties = rows whose SamplingParams carry a repetition / frequency / presence penalty (such a row needs
        set_speculation_rows(sampled=True) too, as any row with parameters).  Every draft row is selected under the history, the output
        counts and the output index the sequential engine would hold there, and a rejected draft leaves nothing behind: the tokens are
        those of the unspeculated engine.  Default: none.  Only while no slot is occupied; the setting survives set_speculation."""
        flags = (SPEC_SHAPED["ngram"] if ngram else 0) | (SPEC_SHAPED["rules"] if rules else 0) | (SPEC_SHAPED["penalties"] if penalties else 0)
        self._ck(self.lib.dots_set_speculation_shaped(self.h, flags), "dots_set_speculation_shaped")
        self.spec_shaped = flags

    spec_logprobs = False                    # Engine.set_speculation_logprobs: off until switched on

    def set_speculation_logprobs(self, on: bool = True):
        """May a row that returns logprobs (set_row_logprobs) verify drafts?  Off by default.  A row's logprobs are a
        function of its raw logits row alone and a draft row's logits are those of the sequential step at its position, so the entries of
        the accepted tokens are bit for bit those of the unspeculated engine, at the same output positions; rejected drafts write
        nothing.  Every other feature the row carries still needs its own switch.  Only while no slot is occupied; the setting survives
        set_speculation."""
        self._ck(self.lib.dots_set_speculation_logprobs(self.h, 1 if on else 0), "dots_set_speculation_logprobs")
        self.spec_logprobs = bool(on)

    @staticmethod
    def speculation_on(engine, k: int, min_n: int = 2, max_n: int = 4, rows: int = 0, guided: bool = False, logprobs: bool = False, shaped: int = 0):
        """Speculation and the row classes that may speculate, switched on together while no slot is occupied: set_speculation(k, min_n,
        max_n), then rows (SPEC_ROWS bits), guided, logprobs and shaped (SPEC_SHAPED bits) — a setter is called only where its setting is
        not the default, so `engine` may be a stand-in that lacks the others.  speculation_off with the same settings undoes it."""
        engine.set_speculation(k, int(min_n), int(max_n))
        if rows:
            engine.set_speculation_rows(sampled=bool(rows & SPEC_ROWS["sampled"]), stop=bool(rows & SPEC_ROWS["stop"]))
        if guided:
            engine.set_speculation_guided(True)
        if logprobs:
            engine.set_speculation_logprobs(True)
        if shaped:
            engine.set_speculation_shaped(ngram=bool(shaped & SPEC_SHAPED["ngram"]), rules=bool(shaped & SPEC_SHAPED["rules"]),
                                          penalties=bool(shaped & SPEC_SHAPED["penalties"]))

    @staticmethod
    def speculation_off(engine, rows: int = 0, guided: bool = False, logprobs: bool = False, shaped: int = 0):
        """the inverse of speculation_on: every setting it changed goes back to its default"""
        engine.set_speculation(0)
        if rows:
            engine.set_speculation_rows()
        if guided:
            engine.set_speculation_guided(False)
        if logprobs:
            engine.set_speculation_logprobs(False)
        if shaped:
            engine.set_speculation_shaped()

    def spec_guide_masks_op(self, guides: Sequence[Optional[int]], states: Sequence[int], drafts: Sequence[Sequence[int]], n_live: Sequence[int], k: int):
        """The state chain and the draft-row mask kernels alone (dots_op_spec_guide_masks) for `rows` slots: guide handle (None = an
        unguided slot), state, at most k drafts and live draft rows per slot.  -> (states int32 [rows * (k + 1)], allowed bool
        [rows * (k + 1)][V]), both indexed by step row r = j * rows + b; state -1 = dead, idle or unguided (its bits are all clear)."""
        rows, k = len(guides), int(k)
        if not (len(states) == len(drafts) == len(n_live) == rows):
            raise ValueError("one guide handle (or None), state, draft list and live count per slot")
        V = int(self.cfg.vocab_size)
        words = 2 * ((V + 63) // 64)
        gid = np.ascontiguousarray([-1 if g is None else int(g) for g in guides], dtype=np.int32)
        st = np.ascontiguousarray([0 if g is None else int(s) for g, s in zip(guides, states)], dtype=np.int32)
        dr = np.zeros((rows, k), np.int32)
        for b, d in enumerate(drafts):
            dr[b, :len(d)] = np.asarray(list(d), np.int32)
        nl = np.ascontiguousarray(n_live, dtype=np.int32)
        s_out = np.full((rows * (k + 1),), -2, np.int32)
        m_out = np.zeros((rows * (k + 1), words), np.uint32)
        self._ck(self.lib.dots_op_spec_guide_masks(self.h, rows, k, _i32p(gid), _i32p(st), _i32p(dr), _i32p(nl), _i32p(s_out),
                                                   m_out.ctypes.data_as(C.POINTER(C.c_uint32))), "dots_op_spec_guide_masks")
        bits = np.unpackbits(m_out.view(np.uint8), axis=1, bitorder="little")[:, :V].astype(bool)
        return s_out, bits

    @property
    def usable_slots(self) -> int:
        """slots slots_prefill accepts: max_batch, or max_batch // (k + 1) while speculating"""
        return spec_usable_slots(self.max_batch, getattr(self, "spec_k", 0))

    def set_row_drafts(self, row: int, ids: Sequence[int]):
        """The drafts slot `row` verifies in its next step (at most k), replacing what the drafter left; spent by that step."""
        a = np.ascontiguousarray(list(ids), dtype=np.int32)
        self._ck(self.lib.dots_set_row_drafts(self.h, int(row), _i32p(a) if a.size else None, int(a.size)), "dots_set_row_drafts")

    def spec_stats(self, row: int = -1) -> dict:
        """{"steps", "drafted", "accepted"} of slot `row` since its prefill, or (row = -1) of the engine since set_speculation"""
        st, dr, ac = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        self._ck(self.lib.dots_spec_stats(self.h, int(row), C.byref(st), C.byref(dr), C.byref(ac)), "dots_spec_stats")
        return {"steps": int(st.value), "drafted": int(dr.value), "accepted": int(ac.value)}

    def ngram_draft_op(self, histories: Sequence[Sequence[int]], k: int, min_n: int = 2, max_n: int = 4) -> list:
        """ngram_draft_kernel alone (dots_op_ngram_draft): one launch over the rows of `histories`, -> one draft list per row."""
        B = len(histories)
        stride = max(1, max(len(h) for h in histories))
        hist = np.zeros((B, stride), np.int32)
        for b, h in enumerate(histories):
            hist[b, :len(h)] = np.asarray(h, np.int32)
        lens = np.asarray([len(h) for h in histories], np.int32)
        d_hist, d_lens = self.to_device(hist), self.to_device(lens)
        d_out, d_n = self.to_device(np.full((B, int(k)), -1, np.int32)), self.to_device(np.full((B,), -1, np.int32))
        try:
            self._ck(self.lib.dots_op_ngram_draft(self.h, C.c_void_p(d_hist), C.c_void_p(d_lens), stride, B, int(k), int(min_n), int(max_n),
                                                  C.c_void_p(d_out), C.c_void_p(d_n)), "dots_op_ngram_draft")
            out, n = self.to_host(d_out, (B, int(k)), np.int32), self.to_host(d_n, (B,), np.int32)
        finally:
            for ptr in (d_hist, d_lens, d_out, d_n):
                self.dev_free(ptr)
        return [out[b, :int(n[b])].tolist() for b in range(B)]

    def set_row_prediction(self, row: int, ids: Optional[Sequence[int]]):
        """Slot `row` holds the prediction `ids` from now on: a text the output is expected to resemble, which the second
        drafter of a speculating step proposes as drafts where the output aligns with it.  None or empty clears.  Only which tokens are
        proposed changes: the committed tokens are the unspeculated engine's.  May be called before the slot's prefill; slot release and
        slots_reset clear it; stored and inert on an engine that does not speculate."""
        a = np.ascontiguousarray([] if ids is None else list(ids), dtype=np.int32)
        self._ck(self.lib.dots_set_row_prediction(self.h, int(row), _i32p(a) if a.size else None, int(a.size)), "dots_set_row_prediction")

    def row_prediction_stats(self, row: int) -> dict:
        """{"drafted", "accepted"}: prediction tokens slot `row` verified as drafts and committed, since its prefill"""
        dr, ac = C.c_int64(0), C.c_int64(0)
        self._ck(self.lib.dots_row_prediction_stats(self.h, int(row), C.byref(dr), C.byref(ac)), "dots_row_prediction_stats")
        return {"drafted": int(dr.value), "accepted": int(ac.value)}

    def predict_draft_op(self, predictions: Sequence[Sequence[int]], histories: Sequence[Sequence[int]], cur: Sequence[int], at: Sequence[int],
                         k: int, min_n: int = 2, max_n: int = 4) -> list:
        """predict_draft_kernel alone (dots_op_predict_draft): one launch over the rows, -> one (drafts | None, cur, at) per row, as
        predicted_draft returns it."""
        B = len(histories)
        if not (len(predictions) == len(cur) == len(at) == B):
            raise ValueError("predict_draft_op: one prediction, cur and at per history")

        def pack(rows):
            stride = max(1, max(len(r) for r in rows))
            a = np.zeros((B, stride), np.int32)
            for b, r in enumerate(rows):
                a[b, :len(r)] = np.asarray(r, np.int32)
            return a, np.asarray([len(r) for r in rows], np.int32), stride

        pred, plens, pstride = pack(predictions)
        hist, hlens, hstride = pack(histories)
        ptrs = [self.to_device(a) for a in (pred, plens, hist, hlens, np.asarray(cur, np.int32), np.asarray(at, np.int32),
                                            np.full((B, int(k)), -1, np.int32), np.full((B,), -1, np.int32), np.full((B,), -1, np.int32))]
        d_pred, d_plens, d_hist, d_hlens, d_cur, d_at, d_out, d_n, d_src = ptrs
        try:
            self._ck(self.lib.dots_op_predict_draft(self.h, C.c_void_p(d_pred), C.c_void_p(d_plens), pstride, C.c_void_p(d_hist), C.c_void_p(d_hlens), hstride,
                                                    B, int(k), int(min_n), int(max_n), C.c_void_p(d_cur), C.c_void_p(d_at), C.c_void_p(d_out),
                                                    C.c_void_p(d_n), C.c_void_p(d_src)), "dots_op_predict_draft")
            out, n, src = self.to_host(d_out, (B, int(k)), np.int32), self.to_host(d_n, (B,), np.int32), self.to_host(d_src, (B,), np.int32)
            c, a = self.to_host(d_cur, (B,), np.int32), self.to_host(d_at, (B,), np.int32)
        finally:
            for ptr in ptrs:
                self.dev_free(ptr)
        res = []
        for b in range(B):
            if int(src[b]) not in (0, 1) or (int(src[b]) == 1) != (int(n[b]) >= 0):
                raise RuntimeError(f"predict_draft_op: row {b} left src {int(src[b])} with n_drafts {int(n[b])}")
            res.append((out[b, :int(n[b])].tolist() if src[b] else None, int(c[b]), int(a[b])))
        return res

    def set_row_logprobs(self, row: int, top_n: Optional[int]):
        """Row `row` (a slot, or sequence `row` of a static batch) returns log-probabilities of the raw logits for every token selected
        from now on, the first token of a following prefill included: the chosen token's and the top_n (0..20) largest.  None = off.
        Slot release and slots_reset switch the row off."""
        n = -1 if top_n is None else int(top_n)
        if top_n is not None and not 0 <= n <= MAX_TOP_LOGPROBS:
            raise ValueError(f"top_n must be None or in [0, {MAX_TOP_LOGPROBS}], got {top_n!r}")
        self._ck(self.lib.dots_set_row_logprobs(self.h, int(row), n), "dots_set_row_logprobs")
        if n >= 0:
            self._drain_wants_lp = True              # slots_drain keeps room for logprob entries from now on

    def row_logprobs(self, row: int, n: int, pos0: int = 0):
        """Positions [pos0, pos0 + n) of the row's generated tokens, cut to the positions that exist: (tok_lp float32 [m],
        top_ids int32 [m, 20], top_lp float32 [m, 20]); -1 / NaN beyond the row's top_n and where the row was off.  An occupied slot
        (before slot_release), or a row of the last static batch."""
        n = max(0, int(n))
        K = MAX_TOP_LOGPROBS
        tok = np.empty((max(1, n),), np.float32)
        ids = np.empty((max(1, n), K), np.int32)
        top = np.empty((max(1, n), K), np.float32)
        m = C.c_int32(0)
        fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))                          # noqa: E731
        self._ck(self.lib.dots_row_logprobs(self.h, int(row), int(pos0), n, fp(tok), _i32p(ids), fp(top), C.byref(m)), "dots_row_logprobs")
        k = int(m.value)
        return tok[:k].copy(), ids[:k].copy(), top[:k].copy()

    def op_logprobs(self, logits, B: int, V: int, ld: int, top_n: Sequence[int], chosen, tok_lp, top_ids, top_lp):
        """The logprob stage on device buffers (dots_op_logprobs): logits fp32 [B, ld], chosen int32 [B]; writes tok_lp fp32 [B],
        top_ids int32 [B, 20], top_lp fp32 [B, 20] of the rows with top_n[b] >= 0 (-1 = skipped)."""
        tn = np.ascontiguousarray(top_n, dtype=np.int32)
        if tn.shape != (B,):
            raise ValueError("one top_n per row")
        self._ck(self.lib.dots_op_logprobs(self.h, logits, int(B), int(V), int(ld), _i32p(tn), chosen, tok_lp, top_ids, top_lp),
                 "dots_op_logprobs")

    def bench_logprobs(self, logits, B: int, V: int, ld: int, top_n: Sequence[int], which: int = 0, iters: int = 200) -> float:
        """mean ms of one replay of the logprob stage: which 0 = both kernels, 1 = the partial kernel, 2 = the final kernel"""
        tn = np.ascontiguousarray(top_n, dtype=np.int32)
        ms = C.c_float()
        self._ck(self.lib.dots_bench_logprobs(self.h, logits, int(B), int(V), int(ld), _i32p(tn), int(which), int(iters), C.byref(ms)),
                 "dots_bench_logprobs")
        return float(ms.value)

    def set_decode_plan(self, plan: int):
        """0 = launch plan by stream (whole chip / CU partition beside a prefetched tower), 1 = the partition plan (whole-tile projections,
        pair-walking gate|up) on every step; + 2 = streaming decode attention wherever legal, + 4 = per-split decode attention (default: by
        items per CU); bit-identical results."""
        self._ck(self.lib.dots_set_decode_plan(self.h, int(plan)), "dots_set_decode_plan")

    def set_gemm_plan(self, plan: int):
        """0 = 8-wave ping-pong GEMM, 1 = one wave per SIMD (round 5); process-wide, bit-identical results."""
        self._ck(self.lib.dots_set_gemm_plan(self.h, int(plan)), "dots_set_gemm_plan")

    def tower_tail(self, set: int = -2) -> int:
        """Blocks of a prefetched tower that run on the whole chip instead of the tower's CU partition: set >= 0 fixed (0 = off, the engine's
        DEFAULT), -1 adaptive (opt-in: sized from the previous launch's events so that the partition part ends with the decode loop — the rule
        reads "the host stopped issuing decode chunks" as "the decode loop drained", which holds for bench.py's closed a4 pipeline and NOT for a
        serving loop that keeps slots occupied: do not copy it into one), -2 = query only (this method's default argument).
        Returns the tail of the tower launched last."""
        now = C.c_int32(0)
        self._ck(self.lib.dots_tower_tail(self.h, int(set), C.byref(now)), "dots_tower_tail")
        return int(now.value)

    def decode_step(self):
        self._ck(self.lib.dots_decode_step(self.h), "dots_decode_step")

    # ------------------------------------------------------------------ continuous batching (sequence slots)
    def set_eos(self, eos_ids: Sequence[int]):
        eos = np.ascontiguousarray(list(eos_ids), dtype=np.int32)
        self._ck(self.lib.dots_set_eos(self.h, _i32p(eos) if len(eos) else None, len(eos)), "dots_set_eos")

    def slots_prefill(self, slots: Sequence[int], input_ids: np.ndarray, prompt_lens: Sequence[int], max_new_tokens: Sequence[int]):
        sl = np.ascontiguousarray(slots, dtype=np.int32)
        ids = np.ascontiguousarray(input_ids, dtype=np.int32)
        lens = np.ascontiguousarray(prompt_lens, dtype=np.int32)
        cap = np.ascontiguousarray(max_new_tokens, dtype=np.int32)
        assert sl.shape == lens.shape == cap.shape and ids.shape[0] == int(lens.sum())
        self._ck(self.lib.dots_slots_prefill(self.h, _i32p(sl), sl.shape[0], _i32p(ids), _i32p(lens), _i32p(cap)), "dots_slots_prefill")

    # chunked prefill
    def slots_prefill_begin(self, slots: Sequence[int], input_ids: np.ndarray, prompt_lens: Sequence[int], max_new_tokens: Sequence[int]):
        """slots_prefill's arguments; the prompts may together be longer than max_prefill_tokens.  Reserves the pages, embeds the prompts
        (the vision rows of vit_forward are consumed here) and leaves the slots filling (slots_poll reports 3): slots_prefill_advance fills
        them.  Refused on a speculating engine."""
        sl = np.ascontiguousarray(slots, dtype=np.int32)
        ids = np.ascontiguousarray(input_ids, dtype=np.int32)
        lens = np.ascontiguousarray(prompt_lens, dtype=np.int32)
        cap = np.ascontiguousarray(max_new_tokens, dtype=np.int32)
        assert sl.shape == lens.shape == cap.shape and ids.shape[0] == int(lens.sum())
        self._ck(self.lib.dots_slots_prefill_begin(self.h, _i32p(sl), sl.shape[0], _i32p(ids), _i32p(lens), _i32p(cap)), "dots_slots_prefill_begin")

    def slots_prefill_advance(self, max_tokens: int) -> int:
        """One pass over up to max_tokens positions (a multiple of 64, at most max_prefill_tokens) of the filling slots, oldest first; a slot
        whose prompt ends in the pass is then what slots_prefill would have left.  -> positions still to fill."""
        left = C.c_int32(0)
        self._ck(self.lib.dots_slots_prefill_advance(self.h, int(max_tokens), C.byref(left)), "dots_slots_prefill_advance")
        return int(left.value)

    def slots_prefill_chunked(self, slots: Sequence[int], input_ids: np.ndarray, prompt_lens: Sequence[int], max_new_tokens: Sequence[int], chunk: int):
        """slots_prefill in passes of at most `chunk` positions: the same logits, KV and tokens whatever the chunk."""
        self.slots_prefill_begin(slots, input_ids, prompt_lens, max_new_tokens)
        while self.slots_prefill_advance(chunk) > 0:
            pass

    # prefix cache over the chunked prefill
    def prefix_cache_enable(self, on: bool = True):
        """Full prompt pages written by chunked fills stay resident and are reused by later prompts that begin with the same blocks (and the
        same image key).  Refused while a slot is occupied or filling and on a speculating engine; off drops every block."""
        self._ck(self.lib.dots_prefix_cache_enable(self.h, 1 if on else 0), "dots_prefix_cache_enable")

    @staticmethod
    def _image_key(key):
        if key is None:
            return None
        key = bytes(key)
        if len(key) != 16:
            raise ValueError(f"an image key is 16 bytes, got {len(key)}")
        return key

    def prefix_cache_lookup(self, input_ids: np.ndarray, image_key: Optional[bytes] = None):
        """-> (lease, hit_tokens, needs_tower).  The lease (0: none) pins the matched pages until slots_prefill_begin_cached takes it or
        prefix_cache_release gives it back; needs_tower False: the prompt's fill needs no vit_forward."""
        ids = np.ascontiguousarray(input_ids, dtype=np.int32)
        lease, hit, tower = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        self._ck(self.lib.dots_prefix_cache_lookup(self.h, _i32p(ids), ids.shape[0], self._image_key(image_key), C.byref(lease), C.byref(hit), C.byref(tower)),
                 "dots_prefix_cache_lookup")
        return int(lease.value), int(hit.value), bool(tower.value)

    def prefix_cache_release(self, lease: int):
        self._ck(self.lib.dots_prefix_cache_release(self.h, int(lease)), "dots_prefix_cache_release")

    def slots_prefill_begin_cached(self, slots: Sequence[int], input_ids: np.ndarray, prompt_lens: Sequence[int], max_new_tokens: Sequence[int],
                                   leases: Sequence[int], image_keys: Sequence[Optional[bytes]]):
        """slots_prefill_begin with one lease (0: none) and one image key (None: none) per prompt: a leased prompt starts behind its cached
        pages, and the full prompt pages these fills complete enter the cache.  A refused call leaves the leases held."""
        sl = np.ascontiguousarray(slots, dtype=np.int32)
        ids = np.ascontiguousarray(input_ids, dtype=np.int32)
        lens = np.ascontiguousarray(prompt_lens, dtype=np.int32)
        cap = np.ascontiguousarray(max_new_tokens, dtype=np.int32)
        ls = np.ascontiguousarray(leases, dtype=np.int32)
        assert sl.shape == lens.shape == cap.shape == ls.shape and ids.shape[0] == int(lens.sum()) and len(image_keys) == sl.shape[0]
        keys = (C.c_char_p * sl.shape[0])(*[self._image_key(k) for k in image_keys])
        self._ck(self.lib.dots_slots_prefill_begin_cached(self.h, _i32p(sl), sl.shape[0], _i32p(ids), _i32p(lens), _i32p(cap), _i32p(ls), keys),
                 "dots_slots_prefill_begin_cached")

    def prefix_cache_info(self) -> dict:
        out = (C.c_int64 * 6)()
        self._ck(self.lib.dots_prefix_cache_info(self.h, out), "dots_prefix_cache_info")
        return dict(zip(("lookups", "hit_tokens", "inserted", "evicted", "resident", "evictable"), (int(v) for v in out)))

    # shared-prefix decode attention
    def set_shared_prefix_attention(self, on: bool = True):
        """Rows that share prompt pages (forks, beams, prompt fan-outs, prefix-cache hits) read each shared KV split once per decode step.
        The same bits either way; takes effect from the next slots_decode, keeps the captured graphs, and is inert (not refused) while the
        engine speculates."""
        self._ck(self.lib.dots_set_shared_prefix_attention(self.h, 1 if on else 0), "dots_set_shared_prefix_attention")

    def shared_prefix_info(self) -> dict:
        """of the plan in force: items, rows in at least one, (row, split) pairs covered; cumulative: KV pages (one kv head, one layer) not read"""
        out = (C.c_int64 * 4)()
        self._ck(self.lib.dots_shared_prefix_info(self.h, out), "dots_shared_prefix_info")
        return dict(zip(("items", "rows", "pairs", "pages_not_read"), (int(v) for v in out)))

    def slots_fork(self, src: int, dst_slots: Sequence[int]):
        """Parallel sampling: every free slot of dst_slots becomes a copy of the sequence slots_prefill just put into slot src (no decode
        step since): the same prompt over the same KV pages, and its own first token under the row parameters already set on it.  From
        then on each is an independent sequence, equal bit for bit to a prefill of the prompt into that slot."""
        dst = np.ascontiguousarray(dst_slots, dtype=np.int32)
        assert dst.ndim == 1
        self._ck(self.lib.dots_slots_fork(self.h, int(src), _i32p(dst) if dst.shape[0] else None, dst.shape[0]), "dots_slots_fork")

    def slots_extend(self, slots: Sequence[int], ids_list: Sequence[Sequence[int]], keep_pending=False, max_new_tokens=1):
        """More prompt tokens behind live sequences: slot slots[i] is fed ids_list[i] (at least one id) behind the KV it
        holds.  keep_pending (a scalar or one per slot): True keeps the slot's pending token — the last token it selected, whose K/V is
        not written yet — in the sequence (a next turn behind a generated answer); False drops it (a prefix that was prefilled only to be
        extended).  Afterwards every slot is what slots_prefill of the longer prompt would have left, with max_new_tokens (a scalar or one
        per slot) as its cap and its first token selected under everything set on the row.  Read the earlier output first: the call
        discards it.  A fork of the most recent prefill comes before an extend."""
        sl = np.ascontiguousarray(slots, dtype=np.int32)
        assert sl.ndim == 1 and len(ids_list) == sl.shape[0]
        lens = np.ascontiguousarray([len(x) for x in ids_list], dtype=np.int32)
        ids = np.ascontiguousarray([t for x in ids_list for t in x] or [0], dtype=np.int32)
        keep = np.ascontiguousarray(np.broadcast_to(np.asarray(keep_pending, dtype=bool), sl.shape), dtype=np.int32)
        cap = np.ascontiguousarray(np.broadcast_to(np.asarray(max_new_tokens, dtype=np.int64), sl.shape), dtype=np.int32)
        self._ck(self.lib.dots_slots_extend(self.h, _i32p(sl) if sl.shape[0] else None, sl.shape[0], _i32p(ids), _i32p(lens), _i32p(keep), _i32p(cap)),
                 "dots_slots_extend")

    def slots_score(self, slots: Sequence[int], ids_list: Sequence[Sequence[int]], top_n=0, keep_pending=False, max_new_tokens=1):
        """Given tokens scored on live sequences: slots_extend with the same arguments, which also records the
        log-probability of every fed token but the first under the model: entry j of a slot is log p(F[j + 1] | ..., F[j]) over
        F = [pending] + ids (keep_pending) or ids, with the top_n (0..20, a scalar or one per slot) largest raw logits beside it, bit
        for bit what row_logprobs returns for a step forced to that token.  The slots are left as slots_extend leaves them.  Returns
        one (tok_lp float32 [m], top_ids int32 [m, 20], top_lp float32 [m, 20]) per slot, m = len(F) - 1."""
        sl = np.ascontiguousarray(slots, dtype=np.int32)
        assert sl.ndim == 1 and len(ids_list) == sl.shape[0]
        lens = np.ascontiguousarray([len(x) for x in ids_list], dtype=np.int32)
        ids = np.ascontiguousarray([t for x in ids_list for t in x] or [0], dtype=np.int32)
        keep = np.ascontiguousarray(np.broadcast_to(np.asarray(keep_pending, dtype=bool), sl.shape), dtype=np.int32)
        cap = np.ascontiguousarray(np.broadcast_to(np.asarray(max_new_tokens, dtype=np.int64), sl.shape), dtype=np.int32)
        top = np.ascontiguousarray(np.broadcast_to(np.asarray(top_n, dtype=np.int64), sl.shape), dtype=np.int32)
        self._ck(self.lib.dots_slots_score(self.h, _i32p(sl) if sl.shape[0] else None, sl.shape[0], _i32p(ids), _i32p(lens), _i32p(keep), _i32p(cap),
                                           _i32p(top)), "dots_slots_score")
        return [self.slot_scores(int(b)) for b in sl]

    def slot_scores(self, slot: int, n: Optional[int] = None, pos0: int = 0):
        """Entries [pos0, pos0 + n) of the slot's last slots_score (n = None: from pos0 to the last one it recorded), as row_logprobs
        returns positions.  Entries past the last recorded one read as NaN / -1.  Readable until the slot's next prefill, extend,
        score or release."""
        K = MAX_TOP_LOGPROBS
        m = C.c_int32(0)
        fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))                          # noqa: E731
        if n is None:
            self._ck(self.lib.dots_slot_scores(self.h, int(slot), int(pos0), 0, None, None, None, C.byref(m)), "dots_slot_scores")
            n = max(0, int(m.value) - int(pos0))
        n = max(0, int(n))
        tok = np.empty((max(1, n),), np.float32)
        ids = np.empty((max(1, n), K), np.int32)
        top = np.empty((max(1, n), K), np.float32)
        self._ck(self.lib.dots_slot_scores(self.h, int(slot), int(pos0), n, fp(tok), _i32p(ids), fp(top), C.byref(m)), "dots_slot_scores")
        return tok[:n].copy(), ids[:n].copy(), top[:n].copy()

    def slots_beam(self, src: int, dst_slots: Sequence[int]):
        """Beam search: slot src (just prefilled, no decode step since) and the free slots dst_slots become a group of
        1 + len(dst_slots) beams, in that order, fully reserved over the source's shared prompt pages; the group's first selection replaces
        the source's own first token.  slots_decode steps it; slot_release of any of its slots releases all of them."""
        dst = np.ascontiguousarray(dst_slots, dtype=np.int32)
        assert dst.ndim == 1
        self._ck(self.lib.dots_slots_beam(self.h, int(src), _i32p(dst) if dst.shape[0] else None, dst.shape[0]), "dots_slots_beam")

    def beam_info(self, slot: int):
        """(beams, steps done, completed records so far) of the group that `slot` belongs to"""
        b, st, nd = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        self._ck(self.lib.dots_beam_info(self.h, int(slot), C.byref(b), C.byref(st), C.byref(nd)), "dots_beam_info")
        return int(b.value), int(st.value), int(nd.value)

    def beam_read(self, slot: int) -> dict:
        """The trace of the group that `slot` belongs to: B, steps, cum float32 [B] (-inf: a dead beam), tokens / parents int32 [B, steps]
        (-1: dead; parents[j, t] = the beam of step t - 1 that beam j of step t extends) and completed = [(step, parent beam, EOS id,
        np.float32 cum)] in (step, beam, rank) order: the arguments of dots_ocr_amd.beam.rank_hypotheses."""
        B, steps, nd = self.beam_info(slot)
        b, st, n = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        cum = np.empty((8,), dtype=np.float32)
        tokens = np.empty((B, max(1, steps)), dtype=np.int32)
        parents = np.empty((B, max(1, steps)), dtype=np.int32)
        done = np.empty((max(1, nd), 4), dtype=np.int32)
        self._ck(self.lib.dots_beam_read(self.h, int(slot), C.byref(b), C.byref(st), cum.ctypes.data_as(C.POINTER(C.c_float)), _i32p(tokens),
                                         _i32p(parents), tokens.shape[1], _i32p(done), done.shape[0], C.byref(n)), "dots_beam_read")
        steps, nd = min(steps, int(st.value)), min(nd, int(n.value))
        s = done[:nd, 3].copy().view(np.float32)
        return {"B": B, "steps": steps, "cum": cum[:B].copy(), "tokens": tokens[:, :steps].copy(), "parents": parents[:, :steps].copy(),
                "completed": [(int(done[k, 0]), int(done[k, 1]), int(done[k, 2]), s[k]) for k in range(nd)]}

    def slots_reset(self):
        """Slot mode, every slot free, every KV page in the pool."""
        self._ck(self.lib.dots_slots_reset(self.h), "dots_slots_reset")

    def slots_decode(self, n_steps: int):
        self._ck(self.lib.dots_slots_decode(self.h, int(n_steps)), "dots_slots_decode")

    def slots_poll(self):
        """-> (finished [max_batch]: -1 free / 0 running / 1 finished / 2 suspended / 3 filling, out_lens [max_batch])"""
        fin = np.empty((self.max_batch,), dtype=np.int32)
        lens = np.empty((self.max_batch,), dtype=np.int32)
        self._ck(self.lib.dots_slots_poll(self.h, _i32p(fin), _i32p(lens)), "dots_slots_poll")
        return fin, lens

    def set_row_stream(self, row: int, on: bool = True):
        """Slot `row` streams: slots_drain delivers its new tokens (and logprob entries, with set_row_logprobs).  Set before the slot's
        prefill or fork; slot release and slots_reset switch it off.  Refused for a row of a beam group."""
        self._ck(self.lib.dots_set_row_stream(self.h, int(row), 1 if on else 0), "dots_set_row_stream")

    def slots_drain(self):
        """slots_poll plus what every streaming row committed since the last drain, in one launch and one synchronisation:
        -> (finished, out_lens, deltas); deltas maps slot -> (tokens int32 [m], None | (tok_lp [m], top_ids [m, 20], top_lp [m, 20])) for
        the streaming rows with m > 0, the second member in the layout of row_logprobs for rows that return logprobs.  A row delivers
        at most STREAM_ROW_CAP tokens per call, the oldest first; the rest come with the next call."""
        mb, K = self.max_batch, MAX_TOP_LOGPROBS
        n = mb * STREAM_ROW_CAP
        if self._drain_tok is None:
            self._drain_tok = np.empty((n,), np.int32)
        if self._drain_lp is None and self._drain_wants_lp:
            self._drain_lp = (np.empty((n,), np.float32), np.empty((n, K), np.int32), np.empty((n, K), np.float32))
        tok, lp = self._drain_tok, self._drain_lp
        fin, lens = np.empty((mb,), np.int32), np.empty((mb,), np.int32)
        first, count, lpf = np.empty((mb,), np.int32), np.empty((mb,), np.int32), np.empty((mb,), np.int32)
        nt, nl = C.c_int32(0), C.c_int32(0)
        fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))                          # noqa: E731
        null_f, null_i = C.POINTER(C.c_float)(), C.POINTER(C.c_int32)()
        self._ck(self.lib.dots_slots_drain(self.h, _i32p(fin), _i32p(lens), _i32p(first), _i32p(count), _i32p(lpf), _i32p(tok),
                                           tok.shape[0], fp(lp[0]) if lp else null_f, _i32p(lp[1]) if lp else null_i,
                                           fp(lp[2]) if lp else null_f, lp[0].shape[0] if lp else 0, C.byref(nt), C.byref(nl)),
                 "dots_slots_drain")
        deltas = {}
        for b in np.nonzero(count)[0].tolist():
            f, m, l = int(first[b]), int(count[b]), int(lpf[b])
            entries = None if l < 0 else (lp[0][l:l + m].copy(), lp[1][l:l + m].copy(), lp[2][l:l + m].copy())
            deltas[b] = (tok[f:f + m].copy(), entries)
        return fin, lens, deltas

    def slot_read(self, slot: int, capacity: int) -> np.ndarray:
        out = np.empty((max(1, capacity),), dtype=np.int32)
        n = C.c_int32(0)
        self._ck(self.lib.dots_slot_read(self.h, int(slot), _i32p(out), int(capacity), C.byref(n)), "dots_slot_read")
        return out[:min(int(n.value), capacity)].copy()

    def slot_logits(self, slot: int) -> np.ndarray:
        """fp32 logits [vocab] of an occupied slot's row, as the most recent prefill, extend or plain decode step over it left them"""
        out = np.empty((self.cfg.vocab_size,), dtype=np.float32)
        self._ck(self.lib.dots_slot_logits(self.h, int(slot), out.ctypes.data_as(C.POINTER(C.c_float))), "dots_slot_logits")
        return out

    def slot_release(self, slot: int):
        self._ck(self.lib.dots_slot_release(self.h, int(slot)), "dots_slot_release")

    def slot_capacity(self, slot: int):
        """(pages owned, limit on prompt + generated tokens) of an occupied slot; the limit is prompt + max_new_tokens unless the KV
        pool ran dry while the sequence was growing."""
        pg, lim = C.c_int32(0), C.c_int32(0)
        self._ck(self.lib.dots_slot_capacity(self.h, int(slot), C.byref(pg), C.byref(lim)), "dots_slot_capacity")
        return pg.value, lim.value

    def kv_pool_info(self):
        """(total, free) pages of 64 tokens in the paged KV pool."""
        tot, free = C.c_int32(0), C.c_int32(0)
        self._ck(self.lib.dots_kv_pool_info(self.h, C.byref(tot), C.byref(free)), "dots_kv_pool_info")
        return int(tot.value), int(free.value)

    # ------------------------------------------------------------------ suspend / resume
    def kv_swap_reserve(self, pages: int):
        """Pinned host space for `pages` 64-token KV pages (each across all layers); 0 frees it.  Refused while a slot is suspended."""
        self._ck(self.lib.dots_kv_swap_reserve(self.h, int(pages)), "dots_kv_swap_reserve")

    def kv_swap_info(self):
        """(total, free) pages of the host space."""
        tot, free = C.c_int32(0), C.c_int32(0)
        self._ck(self.lib.dots_kv_swap_info(self.h, C.byref(tot), C.byref(free)), "dots_kv_swap_info")
        return int(tot.value), int(free.value)

    def slot_suspend(self, slot: int):
        """Park a running sequence: the pages it holds alone go to the host space and back to the pool, the slot keeps all its row state
        and idles (slots_poll reports 2).  DotsEngineError with code DOTS_E_STATE / DOTS_E_CAPACITY and nothing changed when refused."""
        self._ck(self.lib.dots_slot_suspend(self.h, int(slot)), "dots_slot_suspend")

    def slot_resume(self, slot: int):
        """Continue a suspended sequence on fresh pages: it generates exactly what it would have generated undisturbed."""
        self._ck(self.lib.dots_slot_resume(self.h, int(slot)), "dots_slot_resume")

    def slots_pages_short(self, n_steps: int) -> int:
        """Pages the next slots_decode(n_steps) would fail to obtain (0: it caps no sequence)."""
        n = C.c_int32(0)
        self._ck(self.lib.dots_slots_pages_short(self.h, int(n_steps), C.byref(n)), "dots_slots_pages_short")
        return int(n.value)

    def set_kv_scales(self, scales):
        """fp8 KV cache scales, fp32 [num_layers, num_kv_heads, 2] (K, V; anything broadcastable to it), each finite and > 0.  Refused
        (DotsEngineError) while any sequence holds KV pages; accepted and unused with a bf16 cache."""
        shape = (self.cfg.num_hidden_layers, self.cfg.num_key_value_heads, 2)
        s = np.ascontiguousarray(np.broadcast_to(np.asarray(scales, dtype=np.float32), shape))
        self._ck(self.lib.dots_set_kv_scales(self.h, s.ctypes.data_as(C.POINTER(C.c_float))), "dots_set_kv_scales")

    def read_kv(self, layer: int, seq: int, pos0: int, n: int, which: str = "k") -> np.ndarray:
        """Cached K ("k") or V ("v") of LM layer `layer`, positions pos0 .. pos0 + n - 1 of block-table row `seq` (static batch index or
        slot): [num_kv_heads, n, 128], uint16 (raw bf16) or uint8 (raw e4m3fn) as the cache stores it."""
        dt = np.uint8 if self.kv_cache_dtype == "fp8" else np.uint16
        out = np.empty((self.cfg.num_key_value_heads, int(n), 128), dtype=dt)
        self._ck(self.lib.dots_debug_read_kv(self.h, int(layer), int(seq), int(pos0), int(n), {"k": 0, "v": 1}[which],
                                             out.ctypes.data_as(C.c_void_p)), "dots_debug_read_kv")
        return out

    def get_logits(self) -> np.ndarray:
        out = np.empty((self._B, self.cfg.vocab_size), dtype=np.float32)
        self._ck(self.lib.dots_get_logits(self.h, out.ctypes.data_as(C.POINTER(C.c_float))), "dots_get_logits")
        return out

    def get_last_tokens(self) -> np.ndarray:
        out = np.empty((self._B,), dtype=np.int32)
        self._ck(self.lib.dots_get_last_tokens(self.h, _i32p(out)), "dots_get_last_tokens")
        return out

    def set_next_tokens(self, tokens: Sequence[int]):
        t = np.ascontiguousarray(tokens, dtype=np.int32)
        self._ck(self.lib.dots_set_next_tokens(self.h, _i32p(t), t.shape[0]), "dots_set_next_tokens")

    def generate(self, input_ids: np.ndarray, prompt_lens: np.ndarray, pixel_values=None,
                 grid_thw: Optional[np.ndarray] = None, max_new_tokens: int = 128, eos_ids: Sequence[int] = (),
                 pixel_on_device: bool = False, vision_taken: bool = False):
        """Packed prompts + packed patches -> (out_ids [B, max_new_tokens] int32, out_lens [B]).
        vision_taken: the vision rows were prefetched and taken (vit_prefetch / vit_take); pixel_values / grid_thw are ignored."""
        ids = np.ascontiguousarray(input_ids, dtype=np.int32)
        lens = np.ascontiguousarray(prompt_lens, dtype=np.int32)
        B = int(lens.shape[0])
        assert ids.shape[0] == int(lens.sum())
        out_ids = np.zeros((B, max_new_tokens), dtype=np.int32)
        out_lens = np.zeros((B,), dtype=np.int32)
        eos = np.ascontiguousarray(list(eos_ids), dtype=np.int32)
        if vision_taken:
            ptr, n, gp, n_img = None, 0, None, -1
        elif grid_thw is not None and len(grid_thw):
            grid = np.ascontiguousarray(grid_thw, dtype=np.int64)
            n = int((grid[:, 0] * grid[:, 1] * grid[:, 2]).sum())
            if pixel_on_device:
                ptr = C.c_void_p(int(pixel_values))
            else:
                pv = np.ascontiguousarray(pixel_values, dtype=np.float32)
                assert pv.shape[0] == n
                ptr = pv.ctypes.data_as(C.c_void_p)
            gp, n_img = _i64p(grid), grid.shape[0]
        else:
            ptr, n, gp, n_img = None, 0, None, 0
        self._ck(self.lib.dots_generate(self.h, _i32p(ids), _i32p(lens), B, ptr, int(pixel_on_device), n, gp, n_img,
                                        max_new_tokens, _i32p(eos) if len(eos) else None, len(eos),
                                        _i32p(out_ids), _i32p(out_lens)), "dots_generate")
        self._B = B
        return out_ids, out_lens

    def capture_hidden(self, capacity_elems: int):
        """Debug: keep the residual stream after every ViT block / LM prefill layer of the next calls (0 = off)."""
        self._ck(self.lib.dots_debug_capture_hidden(self.h, int(capacity_elems)), "dots_debug_capture_hidden")

    def read_hidden(self, which: str, layer: int) -> np.ndarray:
        """which = "vit" | "lm" -> uint16 (raw bf16) [rows, dim] of that layer's output."""
        dim = self.cfg.vision.embed_dim if which == "vit" else self.cfg.hidden_size
        cap = (self.max_patches if which == "vit" else self.max_prefill_tokens) * dim
        buf = np.empty(cap, dtype=np.uint16)
        rows = C.c_int64(0)
        self._ck(self.lib.dots_debug_read_hidden(self.h, 0 if which == "vit" else 1, int(layer), buf.ctypes.data_as(C.c_void_p), C.byref(rows)),
                 "dots_debug_read_hidden")
        return buf[: rows.value * dim].reshape(rows.value, dim).copy()

    def stats(self) -> dict:
        st = CDotsStats()
        self._ck(self.lib.dots_get_stats(self.h, C.byref(st)), "dots_get_stats")
        return {k: getattr(st, k) for k, _ in CDotsStats._fields_}

    # ------------------------------------------------------------------ single kernels (device pointers)
    def op_rmsnorm(self, x, w, y, rows, dim, eps):
        self._ck(self.lib.dots_op_rmsnorm(self.h, x, w, y, rows, dim, eps), "dots_op_rmsnorm")

    def op_layernorm(self, x, w, b, y, rows, dim, eps):
        self._ck(self.lib.dots_op_layernorm(self.h, x, w, b, y, rows, dim, eps), "dots_op_layernorm")

    def op_gemm(self, A, W, bias, residual, Cout, M, N, K, epilogue=EPI_NONE, colscale=None):
        self._ck(self.lib.dots_op_gemm(self.h, A, W, bias or None, residual or None, Cout, M, N, K, epilogue, colscale or None), "dots_op_gemm")

    def op_gemm_fp8(self, A, W, bias, residual, Cout, M, N, K, epilogue=EPI_NONE):
        self._ck(self.lib.dots_op_gemm_fp8(self.h, A, W, bias or None, residual or None, Cout, M, N, K, epilogue), "dots_op_gemm_fp8")

    def op_quant_fp8(self, w_inout, scale_out, N, K):
        self._ck(self.lib.dots_op_quant_fp8(self.h, w_inout, scale_out, N, K), "dots_op_quant_fp8")

    def op_flash_attn(self, q, k, vt, out, cu_seqlens, Hq, Hkv, causal, scale):
        cu = np.ascontiguousarray(cu_seqlens, dtype=np.int32)
        self._ck(self.lib.dots_op_flash_attn(self.h, q, k, vt, out, _i32p(cu), cu.shape[0] - 1, Hq, Hkv, int(causal), scale),
                 "dots_op_flash_attn")

    def op_qkv_rope_split(self, qkv, q, k, vt, cu_seqlens, pos, Hq, Hkv, rope2d, theta):
        cu = np.ascontiguousarray(cu_seqlens, dtype=np.int32)
        pos = np.ascontiguousarray(pos, dtype=np.int32)
        self._ck(self.lib.dots_op_qkv_rope_split(self.h, qkv, q, k, vt, _i32p(cu), cu.shape[0] - 1, _i32p(pos), Hq, Hkv,
                                                 int(rope2d), theta), "dots_op_qkv_rope_split")

    def op_qkv_proj_rope(self, x, w, bias, qkv_ws, q, k, vt, cu_seqlens, pos, K, Hq, Hkv, rope2d, theta, fused):
        cu = np.ascontiguousarray(cu_seqlens, dtype=np.int32)
        pos = np.ascontiguousarray(pos, dtype=np.int32)
        self._ck(self.lib.dots_op_qkv_proj_rope(self.h, x, w, bias, qkv_ws, q, k, vt, _i32p(cu), cu.shape[0] - 1, _i32p(pos), K, Hq, Hkv,
                                                int(rope2d), theta, int(fused)), "dots_op_qkv_proj_rope")

    # ---- single kernels of the decode step (row-major device tensors; packing happens inside the library)
    def op_dec_qkv(self, h, ln_w, wqkv, bias, ctx_len, block_table, max_pages, pool_layer, q_out, B, H, Hq, Hkv, eps, rope_theta, fp8=False):
        self._ck(self.lib.dots_op_dec_qkv(self.h, h, ln_w, wqkv, bias or None, ctx_len, block_table, max_pages, pool_layer, q_out,
                                          B, H, Hq, Hkv, eps, rope_theta, int(fp8)), "dots_op_dec_qkv")

    def op_decode_attn(self, q, pool_layer, ctx_len, block_table, max_pages, out, B, Hq, Hkv, max_seq_len):
        self._ck(self.lib.dots_op_decode_attn(self.h, q, pool_layer, ctx_len, block_table, max_pages, out, B, Hq, Hkv, max_seq_len),
                 "dots_op_decode_attn")

    def op_dec_qkv_kv8(self, h, ln_w, wqkv, bias, ctx_len, block_table, max_pages, pool_layer, q_out, B, H, Hq, Hkv, eps, rope_theta, kv_scales,
                       fp8=False):
        """op_dec_qkv on an fp8 (e4m3fn) page pool; kv_scales: device fp32 [Hkv, 2] (K, V)."""
        self._ck(self.lib.dots_op_dec_qkv_kv8(self.h, h, ln_w, wqkv, bias or None, ctx_len, block_table, max_pages, pool_layer, q_out,
                                              B, H, Hq, Hkv, eps, rope_theta, int(fp8), kv_scales), "dots_op_dec_qkv_kv8")

    def op_flash_attn_paged(self, q, pool_layer, block_table, max_pages, table_rows, out, prefix, n_new, Hq, Hkv, scale, kv_scales=None, rows=None):
        """Causal attention of new query rows over keys that lie in the page pool (csrc/attn_paged.hip).  Sequence b: prefix[b] positions
        (a multiple of 64) before its n_new[b] rows, pages = row rows[b] (None: b) of the device table [table_rows, max_pages];
        q device bf16 [Hq, sum n_new, 128]; kv_scales: device fp32 [Hkv, 2] of an fp8 pool, or None for a bf16 pool."""
        pre = np.ascontiguousarray(prefix, dtype=np.int32)
        new = np.ascontiguousarray(n_new, dtype=np.int32)
        if pre.ndim != 1 or pre.shape != new.shape:
            raise ValueError("prefix and n_new must be 1-D and of equal length")
        rw = None if rows is None else np.ascontiguousarray(rows, dtype=np.int32)
        if rw is not None and rw.shape != pre.shape:
            raise ValueError("rows must match prefix")
        self._ck(self.lib.dots_op_flash_attn_paged(self.h, q, pool_layer, block_table, max_pages, table_rows, out, None if rw is None else _i32p(rw),
                                                   _i32p(pre), _i32p(new), pre.shape[0], Hq, Hkv, scale, kv_scales), "dots_op_flash_attn_paged")

    def op_decode_attn_shared(self, q, pool_layer, ctx_len, block_table, max_pages, out, B, Hq, Hkv, max_seq_len, kv_scales=None) -> int:
        """op_decode_attn (kv_scales None) / op_decode_attn_kv8 under the shared-prefix plan of the given block table; -> the (row, split)
        pairs the plan covers.  The partials are NaN-filled first: a pair neither kernel wrote shows in out."""
        pairs = C.c_int32(0)
        self._ck(self.lib.dots_op_decode_attn_shared(self.h, q, pool_layer, ctx_len, block_table, max_pages, out, B, Hq, Hkv, max_seq_len, kv_scales,
                                                     C.byref(pairs)), "dots_op_decode_attn_shared")
        return int(pairs.value)

    def op_decode_attn_kv8(self, q, pool_layer, ctx_len, block_table, max_pages, out, B, Hq, Hkv, max_seq_len, kv_scales):
        """op_decode_attn on an fp8 (e4m3fn) page pool; kv_scales: device fp32 [Hkv, 2] (K, V)."""
        self._ck(self.lib.dots_op_decode_attn_kv8(self.h, q, pool_layer, ctx_len, block_table, max_pages, out, B, Hq, Hkv, max_seq_len,
                                                  kv_scales), "dots_op_decode_attn_kv8")

    def op_dec_proj(self, x, w, h_inout, B, N, K, fp8=False):
        self._ck(self.lib.dots_op_dec_proj(self.h, x, w, h_inout, B, N, K, int(fp8)), "dots_op_dec_proj")

    def op_dec_gateup(self, h, ln_w, gate_w, up_w, act_out, B, H, I, eps, fp8=False):
        self._ck(self.lib.dots_op_dec_gateup(self.h, h, ln_w, gate_w, up_w, act_out, B, H, I, eps, int(fp8)), "dots_op_dec_gateup")

    def op_dec_lmhead(self, h, ln_w, w, logits_out, B, H, V, eps, fp8=False):
        self._ck(self.lib.dots_op_dec_lmhead(self.h, h, ln_w, w, logits_out, B, H, V, eps, int(fp8)), "dots_op_dec_lmhead")
