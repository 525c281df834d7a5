"""Continuous batching over the engine's sequence slots.

The reference gets this from its vLLM server: ``DotsOCRParser`` fires one request per page from a thread pool
(dots_ocr/parser.py:138-166, model/inference.py:8-50) and the server keeps its running batch full, admitting a new
page whenever one finishes.  Here the same policy runs in-process on top of the C-ABI slot calls
(include/dots_ocr_hip.h "Continuous batching"): FIFO admission into free slots within the ViT / prefill workspace
budgets, fixed-size decode chunks replayed from a captured graph, finished sequences read out and their slots reused.

A page's tokens do not depend on what shares the batch with it (every kernel on the path is row-independent), so the
result of a request is the same as a single-sequence ``generate`` — tests/test_model_gpu.py checks exactly that.
"""
from __future__ import annotations

from collections import deque
from dataclasses import dataclass
from typing import Deque, Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np

from .row_features import FEATURES, ROW_FEATURES, apply_row, cancel_rows, clear_rows, engine_takes, release_row


def split_common_prefix(seqs: Sequence[Sequence[int]]) -> Tuple[List[int], List[List[int]]]:
    """(prefix, suffixes) of several token sequences: their longest common prefix, cut back so that every suffix keeps at least one
    token (a sequence that is a prefix of another still has something to feed: Request.suffixes)."""
    seqs = [[int(t) for t in s] for s in seqs]
    if not seqs or any(not s for s in seqs):
        raise ValueError("every sequence needs at least one token")
    k, shortest = 0, min(len(s) for s in seqs)
    while k < shortest and all(s[k] == seqs[0][k] for s in seqs):
        k += 1
    k = min(k, shortest - 1)
    return seqs[0][:k], [s[k:] for s in seqs]


class RequestRejected(ValueError):
    """The engine refused a request's own per-row parameters (sampling, logprobs, logit rules) at admission."""


@dataclass
class Request:
    input_ids: np.ndarray                       # int32 [T]; image pad tokens already expanded (processor output)
    pixel_values: Optional[object] = None       # float32 [n_patches, patch_dim]: numpy array or torch CUDA tensor
    grid_thw: Optional[np.ndarray] = None       # int64 [n_img, 3]
    max_new_tokens: int = 128
    tag: object = None
    sampling: Optional[object] = None           # engine.SamplingParams of this request, or None = the engine-wide setting
    logprobs: Optional[int] = None              # top_n (0..20) of per-token log-probabilities to return, None = off; a finished request
                                                # then carries logprobs_out = Engine.row_logprobs(slot, its token count)
    rules: Optional[object] = None              # engine.LogitRules of this request (bias, allowed ids, min_tokens, stop ids, ignore_eos), or None
    guide: Optional[int] = None                 # handle of Engine.create_guide the request's output must follow, or None
    ngram: Optional[object] = None              # engine.NgramRule of this request (no-repeat n-gram blocking), or None
    n: int = 1                                  # parallel sampling: n sequences from one tower and one prefill; sequence i runs under
                                                # `sampling` with seed + i, everything else shared.  A finished request with n > 1 carries outputs
                                                # (the n token arrays in index order), logprobs_out as a list in that order and kv_truncated_each
    stop: Optional[Sequence[str]] = None        # stop strings: the row ends on the device at the token that completes one of them.  A
                                                # finished request carries stop_hit = Engine.row_stop_hit(slot) — (token index, bytes into it,
                                                # match length, match id) or None — as a list in index order when n > 1
    include_stop_str_in_output: bool = False    # vLLM's field: where text built from the tokens is cut (stop_strings.cut_text); the tokens
                                                # always end at the one that completed the match
    loop: Optional[object] = None               # loop_guard.LoopRule: the row ends on the device at the token after which its output
                                                # has cycled for the rule's span.  A finished request carries loop_hit = Engine.row_loop_hit(slot)
                                                # — (token index, period, span) or None — as a list in index order when n > 1
    num_beams: Optional[int] = None             # beam search: a group of 2 .. 8 beams from one tower and one prefill, in num_beams slots.
                                                # vLLM's beam-search semantics with HF's length normalisation, not HF's BeamSearchScorer.  A finished
                                                # request carries outputs (the num_return best hypotheses, best first, a final EOS included),
                                                # cumulative_logprobs, beam_scores and finish_reasons ("stop" | "length") in that order
    num_return: int = 1                         # hypotheses returned, 1 .. num_beams
    length_penalty: float = 1.0                 # score = cum / max(1, len) ** length_penalty, len without a final EOS
    suffixes: Optional[Sequence[Sequence[int]]] = None   # several prompts over one page: 2 .. 8 token lists; input_ids is then the
                                                # prefix they share (image tokens and pixel values as always) and sequence i reads prefix +
                                                # suffixes[i] — one tower, one prefill of the prefix, one fork, one Engine.slots_extend.  Sequence i
                                                # runs under `sampling` with seed + i; the finished request carries outputs, logprobs_out, stop_hit
                                                # and kv_truncated_each in suffix order, exactly like n > 1
    score: Optional[Sequence[Sequence[int]]] = None      # score given tokens: 1 .. 8 token lists; input_ids is the prefix they share and
                                                # candidate i is scored as prefix + score[i] — one tower, one prefill of the prefix, one fork, one
                                                # Engine.slots_score.  Nothing is generated: the request finishes at admission, its slots released,
                                                # carrying scores_out[i] = (tok_lp [len - 1], top_ids [len - 1, 20], top_lp [len - 1, 20]) in
                                                # candidate order — entry j is log p(score[i][j + 1] | prefix, score[i][:j + 1]) — and empty outputs
    score_top_logprobs: int = 0                 # top_n (0..20) of the top lists beside every scored token
    stream: Optional[object] = None             # streaming: callback(rid, index, tokens, logprobs_or_None, finished), called on the
                                                # scheduler's thread once per sequence that has new tokens or has just finished, before the request is
                                                # reported; index = 0, the fork index of n > 1, or the prompt index of suffixes.  The tokens of all calls
                                                # for an index, concatenated, are the request's outputs[index]; logprobs in the layout of row_logprobs
    prediction: Optional[Sequence[int]] = None  # predicted outputs: token ids the output is expected to resemble; a speculating engine
                                                # drafts from them, and the tokens are those of the same request without it.  A hint: stored and inert
                                                # on an engine that does not speculate.  One sequence only (no n > 1, beams, suffixes or score).  A
                                                # finished request carries prediction_stats = Engine.row_prediction_stats(slot)
    image_key: Optional[bytes] = None           # prefix caching: 16 bytes, the caller's promise that equal keys mean equal pixels and
                                                # grid.  An image request without one bypasses the cache.  A finished request carries cached_tokens

    @property
    def seqs(self) -> int:
        """independent sequences of the request: one per suffix or scored candidate, else n"""
        return len(self.tails) if self.tails else int(self.n)

    @property
    def tails(self):
        """what is fed behind the shared prefix, one list per sequence: the suffixes, or the candidates of a score; None = nothing"""
        return self.suffixes if self.suffixes else (self.score if self.score else None)

    @property
    def width(self) -> int:
        """slots the request takes: its beams, or its sequences"""
        return int(self.num_beams) if self.num_beams else self.seqs

    def n_patches(self) -> int:
        if self.grid_thw is None:
            return 0
        g = np.asarray(self.grid_thw, dtype=np.int64).reshape(-1, 3)
        return int((g[:, 0] * g[:, 1] * g[:, 2]).sum())


class ContinuousBatcher:
    """submit() requests at any time, call step() in a loop (or run() for a closed set)."""

    def __init__(self, engine, eos_ids: Sequence[int] = (), chunk: int = 16, headroom_pages: Optional[int] = 2, prefetch: int = 0,
                 tower_steps_per_page: int = 48, admit_group: Optional[int] = None, preemption: Optional[str] = None,
                 swap_pages: Optional[int] = None, prefill_chunk: Optional[int] = None, prefix_caching: Optional[bool] = None,
                 shared_prefix_attention: Optional[bool] = None):
        self.engine = engine
        # shared-prefix attention: an engine-wide switch, not a row feature — rows that share prompt pages (n > 1, beams,
        # several prompts over one page, prefix-cache hits) read each shared KV split once per decode step; the same bits either way.
        # Nothing is refused: a speculating engine takes the switch and its steps ignore it.  None leaves the engine as it is
        if shared_prefix_attention is not None:
            if shared_prefix_attention and not hasattr(engine, "set_shared_prefix_attention"):
                raise ValueError("this engine has no shared-prefix attention (no set_shared_prefix_attention)")
            if hasattr(engine, "set_shared_prefix_attention"):
                engine.set_shared_prefix_attention(bool(shared_prefix_attention))
        self.shared_prefix_attention = bool(shared_prefix_attention)
        self._shared_base = self._shared_pages_now()
        # prefix caching, over the chunked prefill only.  Admission and the look-ahead ask the engine first
        # (Engine.prefix_cache_lookup): a request starts its fill behind the pages it hit, takes that many pages less, and — when the lookup
        # says so — sends no pixels to the tower.  The lease a lookup returns pins those pages until the begin that takes it; every path that
        # gives a request back to the queue gives its lease back to the engine
        if prefix_caching:
            if prefill_chunk is None:
                raise ValueError("prefix_caching needs prefill_chunk: only pages written by a chunked fill are cached")
            if not all(hasattr(engine, f) for f in ("prefix_cache_enable", "prefix_cache_lookup", "prefix_cache_release", "slots_prefill_begin_cached")):
                raise ValueError("this engine has no prefix cache (no prefix_cache_lookup): prefix_caching is not available")
        self.prefix_caching = bool(prefix_caching)
        self._leases: Dict[int, Tuple[int, int, bool]] = {}      # request id -> (lease, hit tokens, needs the tower) of a lookup not yet consumed
        self.prefix_hits = 0                                     # requests whose fill began behind cached pages
        self.prefix_hit_tokens = 0                               # ... and the positions they skipped
        # chunked prefill.  None: an admitted group is prefilled in one pass (Engine.slots_prefill), during which nothing
        # decodes.  N: admission only BEGINS the group's fill (Engine.slots_prefill_begin); every step then runs at most one pass of N
        # positions (Engine.slots_prefill_advance) and its decode chunk, so no decode chunk waits for more than one pass, and a prompt
        # may be longer than the engine's max_prefill_tokens.  A request joins `running` in the step whose pass completed its fill
        if prefill_chunk is not None:
            if isinstance(prefill_chunk, bool) or not isinstance(prefill_chunk, (int, np.integer)) or prefill_chunk < 64 or prefill_chunk % 64:
                raise ValueError(f"prefill_chunk must be a positive multiple of 64, got {prefill_chunk!r}")
            if prefill_chunk > int(engine.max_prefill_tokens):
                raise ValueError(f"prefill_chunk = {prefill_chunk} exceeds the engine's max_prefill_tokens = {int(engine.max_prefill_tokens)}")
            if not all(hasattr(engine, f) for f in ("slots_prefill_begin", "slots_prefill_advance")):
                raise ValueError("this engine cannot fill a prompt in passes (no slots_prefill_begin): prefill_chunk is not available")
            if getattr(engine, "spec_k", 0):
                raise ValueError("prefill_chunk cannot be combined with a speculating engine")
        self.prefill_chunk = None if prefill_chunk is None else int(prefill_chunk)
        self.filling: List[Tuple[int, int, Request]] = []        # (slot, request id, request) whose fill has begun, oldest first
        self._fill_kids: Dict[int, List[int]] = {}               # request id -> the slots its fork / beam group takes once its fill completes
        self.fill_passes = 0
        # preemption.  None: a dry KV pool ends a sequence early at what its pages hold ("kv_pool_exhausted").  "swap":
        # before a decode chunk that would run short, the most recently admitted sequences are suspended — their KV parked in swap_pages
        # pages of pinned host memory (default: as many as the pool has) — and resumed, oldest suspension first, when the pool has room
        # again; every sequence generates exactly what it would have generated alone (vLLM's swap preemption)
        if preemption not in (None, "swap"):
            raise ValueError(f"preemption must be None or 'swap', got {preemption!r}")
        if preemption == "swap":
            if not all(hasattr(engine, f) for f in ("slot_suspend", "slot_resume", "slots_pages_short", "kv_swap_reserve", "kv_swap_info")):
                raise ValueError("this engine cannot suspend a sequence (no slot_suspend): preemption='swap' is not available")
            if getattr(engine, "spec_k", 0):
                raise ValueError("preemption='swap' cannot be combined with a speculating engine: a suspended row idles, a draft row cannot")
        elif swap_pages is not None:
            raise ValueError("swap_pages needs preemption='swap'")
        self.preemption = preemption
        self.chunk = max(1, int(chunk))
        # free KV pages kept per running sequence when admitting (see plan_admission).  None = FULL RESERVATION: a sequence is admitted only
        # when the pool could hold prompt + max_new_tokens of every running sequence and of this one, so nothing is ever truncated by a dry
        # pool (the policy of rounds 1-2; fewer sequences in flight when caps are generous, as with the reference's max_new_tokens=24000).
        self.full_reservation = headroom_pages is None
        self.headroom_pages = 0 if headroom_pages is None else max(0, int(headroom_pages))
        # look-ahead: the vision tower of the next `prefetch` queued requests runs on the engine's CU-masked side stream while the
        # occupied slots keep decoding on the other CU partition (Engine.vit_prefetch); that group is then admitted as a whole — prefill
        # only, no tower in the decode loop's way — as soon as it has the slots and pages.  1 suits requests that finish at different
        # times (a slot is refilled as soon as it frees), n_slots suits closed sets of equal length.  0 = off.
        self.prefetch = max(0, int(prefetch)) if hasattr(engine, "vit_prefetch") else 0
        # decode steps that pass while ONE page's tower runs on the side partition (A4 on 160-192 CUs: ~150 ms against 2.6-3.3 ms per step)
        self.tower_steps_per_page = max(1, int(tower_steps_per_page))
        # at most this many requests per ORDINARY admission (None: as many as fit).  With look-ahead on, the ordinary path only runs when
        # nothing is prefetched — the cold start of a queue: admitting `prefetch`-sized groups there too starts the decode loop after ONE
        # small tower instead of after the towers of every free slot, and the later groups' towers run beside it (a closed set of equal
        # caps then also finishes staggered, one group per tower, instead of all at once with nothing left to overlap)
        self.admit_group = None if admit_group is None else max(1, int(admit_group))
        self._ahead: List[Tuple[int, Request]] = []             # requests whose tower has been prefetched, in packed order
        self._ahead_keep = None                                  # their (device) pixels stay alive until the rows are taken
        # a speculating engine (Engine.set_speculation) fills max_batch // (k + 1) slots: a slot takes up to k + 1 rows of a
        # step.  A chunk of c steps may then finish a row before c tokens; nothing else changes, the lengths come from the poll
        self.n_slots = int(getattr(engine, "usable_slots", engine.max_batch))
        self.max_patches = int(engine.max_patches)
        self.max_prefill_tokens = int(engine.max_prefill_tokens)
        self.max_seq_len = int(engine.max_seq_len)
        self.pending: Deque[Tuple[int, Request]] = deque()
        self.running: Dict[int, Tuple[int, Request]] = {}        # slot -> (request id, request)
        self._next_id = 0
        self.decode_steps = 0
        self.admissions = 0
        self._last_lens: Dict[int, int] = {}                     # slot -> tokens generated as of the last poll
        self._rows: Dict[int, Dict[str, object]] = {}            # slot -> feature name -> the value set on it (row_features.ROW_FEATURES)
        self._predicted: set = set()                             # slots that hold a prediction (beside the table: row_features)
        self._streamed: Dict[int, int] = {}                      # streaming slot -> tokens of its sequence handed to the callback so far
        self._cancel: set = set()                                # request ids cancelled while being admitted: cancelled by the first collect that sees them running
        self._cancelled: List[Tuple[int, Request, np.ndarray]] = []   # cancelled requests (reported by step())
        self._kids: Dict[int, List[int]] = {}                    # request id -> the slots planned for sequences 1 .. n - 1 of a request with n > 1
        self._seq_index: Dict[int, int] = {}                     # slot -> index of its sequence within a request with n > 1
        self.kv_truncated = 0                                    # sequences ended early by a dry KV pool (finish reason "kv_pool_exhausted")
        self.preemptions = 0                                     # sequences suspended (preemption="swap")
        self.resumes = 0                                         # ... and resumed
        self.swapped_pages = 0                                   # KV pages copied out to host memory (each comes back once)
        self.suspended: List[int] = []                           # suspended slots, longest suspended first (they stay in `running`)
        self._parked_pages: Dict[int, int] = {}                  # suspended slot -> host pages it holds = pool pages its resume takes
        self._admit_seq: Dict[int, int] = {}                     # slot -> admission counter (the victim order: most recent first)
        self._admit_count = 0
        self._rejected: List[Tuple[int, Request]] = []           # requests whose own parameters the engine refused (reported by step())
        self._scored: List[Tuple[int, Request]] = []             # score requests finished at their admission (reported by the step's collect)
        self.eos_ids = tuple(int(t) for t in eos_ids)
        engine.set_eos(list(eos_ids))
        if hasattr(engine, "slots_reset"):           # start from an empty engine: no occupied slot, every KV page in the pool
            engine.slots_reset()                     # (a static batch or a failed run may have left both behind)
        else:
            fin, _ = engine.slots_poll()
            for s in range(self.n_slots):
                if fin[s] >= 0:
                    engine.slot_release(s)
        if self.prefix_caching:                      # after the reset: no slot is occupied or filling
            engine.prefix_cache_enable(True)
        if preemption == "swap":                     # after the reset: nothing is parked any more, the host space may change
            engine.kv_swap_reserve(int(engine.kv_pool_info()[0]) if swap_pages is None else max(0, int(swap_pages)))

    # ------------------------------------------------------------------ queue
    def submit(self, req: Request) -> int:
        ids = np.ascontiguousarray(req.input_ids, dtype=np.int32).reshape(-1)
        if ids.shape[0] < 1 or ids.shape[0] >= self.max_seq_len:
            raise ValueError(f"prompt of {ids.shape[0]} tokens does not fit max_seq_len={self.max_seq_len}")
        if ids.shape[0] > self.max_prefill_tokens and self.prefill_chunk is None:
            raise ValueError(f"prompt of {ids.shape[0]} tokens exceeds max_prefill_tokens={self.max_prefill_tokens}")
        if req.n_patches() > self.max_patches:
            raise ValueError(f"request has {req.n_patches()} vision patches, more than max_patches={self.max_patches}")
        if isinstance(req.n, bool) or not isinstance(req.n, (int, np.integer)) or req.n < 1:
            raise ValueError(f"n must be an integer >= 1, got {req.n!r}")
        if req.n > self.n_slots:
            raise ValueError(f"n = {req.n} sequences need more than the {self.n_slots} usable slots")
        if req.prediction is not None:
            self._check_prediction(req)
        if req.stream is not None:
            self._check_stream(req)
        if req.score is not None:
            self._check_score(req)
        if req.suffixes is not None or req.score is not None:
            self._check_suffixes(req, ids.shape[0])
        if req.num_beams is not None:
            self._check_beam(req)
        if req.n > 1 and not hasattr(self.engine, "slots_fork"):
            raise ValueError("this engine cannot fork a prefilled sequence (no slots_fork): n > 1 is not available")
        for f in ROW_FEATURES:
            if f.noun and getattr(req, f.name) is not None and not engine_takes(self.engine, f):
                raise ValueError(f"this engine cannot honour {f.noun} (no {f.setter})")
        if req.stop is not None:
            from .stop_strings import check_stop_strings
            try:
                req.stop = check_stop_strings(req.stop)
            except ValueError as e:
                raise RequestRejected(str(e))
        if req.rules is not None and hasattr(req.rules, "eos_ids"):
            # what the engine will check at admission, checked here against the EOS ids and the vocabulary this batcher runs under: rules
            # that could never select a token are refused before the request is queued, where it fails alone
            import dataclasses
            try:
                dataclasses.replace(req.rules, eos_ids=self.eos_ids,
                                    vocab_size=getattr(getattr(self.engine, "cfg", None), "vocab_size", req.rules.vocab_size))
            except ValueError as e:
                raise RequestRejected(str(e))
        req.input_ids = ids
        # like HF generate, stop at the context capacity instead of failing
        longest = max((len(x) for x in req.tails), default=0) if req.tails else 0
        req.max_new_tokens = max(1, min(int(req.max_new_tokens), self.max_seq_len - ids.shape[0] - longest))
        if hasattr(self.engine, "kv_pool_info") and self._group_pages(req) > self.engine.kv_pool_info()[0]:
            raise ValueError(f"prompt of {ids.shape[0]} tokens needs {self._group_pages(req)} KV pages, "
                             f"the pool holds {self.engine.kv_pool_info()[0]}")
        if self.full_reservation and hasattr(self.engine, "kv_pool_info") and self._worst_pages(req) > self.engine.kv_pool_info()[0]:
            raise ValueError(f"prompt + max_new_tokens = {ids.shape[0]} + {req.max_new_tokens} tokens need {self._worst_pages(req)} KV pages under full "
                             f"reservation, the pool holds {self.engine.kv_pool_info()[0]}")
        if self.preemption == "swap" and self._worst_pages(req) > self.engine.kv_pool_info()[0]:
            # with everything else suspended a request must be able to finish on its own: otherwise preemption could not help it
            raise ValueError(f"prompt + max_new_tokens = {ids.shape[0]} + {req.max_new_tokens} tokens need {self._worst_pages(req)} KV pages, the pool "
                             f"holds {self.engine.kv_pool_info()[0]}: with preemption='swap' a request must fit the pool alone")
        rid = self._next_id
        self._next_id += 1
        self.pending.append((rid, req))
        return rid

    MAX_SUFFIXES = 8

    def _check_prediction(self, req: Request):
        """a prediction belongs to one generated sequence: what would need several, or generates nothing, is refused whole"""
        for bad, what in ((req.n > 1, "n > 1"), (req.num_beams is not None, "num_beams"), (req.score is not None, "score"),
                          (req.suffixes is not None, "suffixes")):
            if bad:
                raise RequestRejected(f"a prediction cannot be combined with {what}: it belongs to one generated sequence")
        if not hasattr(self.engine, "set_row_prediction"):
            raise RequestRejected("a prediction needs continuous batching on an engine that takes one (Engine.set_row_prediction): not with static batching")
        try:
            ids = [int(t) for t in req.prediction]
        except (TypeError, ValueError):
            raise RequestRejected(f"prediction must be a list of token ids, got {req.prediction!r}")
        vocab = getattr(getattr(self.engine, "cfg", None), "vocab_size", None)
        if any(t < 0 or (vocab is not None and t >= vocab) for t in ids):
            raise RequestRejected(f"the prediction holds a token id outside [0, {vocab})")
        if len(ids) > self.max_seq_len:
            raise RequestRejected(f"a prediction of {len(ids)} tokens is longer than max_seq_len = {self.max_seq_len}")
        req.prediction = ids

    def _check_score(self, req: Request):
        """what only a score request is asked; _check_suffixes then asks what it asks of several prompts.  There is nothing
        to select, so every selection setting is refused by name rather than dropped"""
        if req.suffixes is not None:
            raise RequestRejected("score cannot be combined with suffixes")
        for name, what in (("sampling", "sampling parameters"), ("guide", "a guide"), ("rules", "logit rules"), ("ngram", "an n-gram rule"),
                           ("stop", "stop strings"), ("loop", "a loop guard"), ("logprobs", "logprobs (score_top_logprobs sets the top lists of the scored tokens)")):
            if getattr(req, name) is not None:
                raise RequestRejected(f"a score request selects nothing and takes no {what}")
        t = req.score_top_logprobs
        if isinstance(t, bool) or not isinstance(t, (int, np.integer)) or not 0 <= t <= 20:
            raise RequestRejected(f"score_top_logprobs must be an integer in [0, 20], got {t!r}")
        if not hasattr(self.engine, "slots_score"):
            raise RequestRejected("score needs continuous batching on an engine that scores given tokens (Engine.slots_score): not with static batching")
        req.max_new_tokens = 1                       # the token the extend selects is discarded

    def _check_suffixes(self, req: Request, prefix: int):
        """a request with several prompts, or with scored candidates, is refused whole rather than run with anything dropped (DESIGN §6.11,
        §6.14)"""
        scoring = req.score is not None
        what, each, tails = ("score", "candidate", req.score) if scoring else ("suffixes", "suffix", req.suffixes)
        m = len(tails)
        if not (1 if scoring else 2) <= m <= self.MAX_SUFFIXES:
            raise RequestRejected(f"{what} must hold {1 if scoring else 2} .. {self.MAX_SUFFIXES} token lists, got {m}")
        if req.n != 1:
            raise RequestRejected(f"{what} cannot be combined with n > 1: every {each} is one sequence")
        if req.num_beams is not None:
            raise RequestRejected(f"{what} cannot be combined with num_beams")
        if not all(hasattr(self.engine, f) for f in ("slots_fork", "slots_extend")):
            raise RequestRejected(f"{what} need continuous batching on an engine that extends a live sequence (Engine.slots_extend): "
                                  "not with static batching")
        if getattr(self.engine, "spec_k", 0):
            raise RequestRejected(f"{what} cannot run while the engine speculates")
        sp = req.sampling
        if sp is not None and (float(getattr(sp, "repetition_penalty", 1.0)) != 1.0 or float(getattr(sp, "frequency_penalty", 0.0)) != 0.0
                               or float(getattr(sp, "presence_penalty", 0.0)) != 0.0):
            raise RequestRejected("suffixes cannot be combined with a penalty: an extended row's prompt-presence image would be wrong")
        if m > self.n_slots:
            raise ValueError(f"{m} {what if scoring else 'suffixes'} need more than the {self.n_slots} usable slots")
        vocab = getattr(getattr(self.engine, "cfg", None), "vocab_size", None)
        clean = []
        for i, x in enumerate(tails):
            x = [int(t) for t in x]
            if not x:
                raise RequestRejected(f"{each} {i} is empty: every {each} keeps at least one token")
            if vocab is not None and not all(0 <= t < vocab for t in x):
                raise RequestRejected(f"{each} {i} holds a token id outside [0, {vocab})")
            if prefix + len(x) >= self.max_seq_len:
                raise ValueError(f"prefix + {each} {i} = {prefix} + {len(x)} tokens do not fit max_seq_len={self.max_seq_len}")
            clean.append(x)
        if scoring:
            req.score = clean
        else:
            req.suffixes = clean

    def _check_stream(self, req: Request):
        """a streaming request is refused whole rather than run without its callback"""
        if not callable(req.stream):
            raise ValueError(f"stream must be a callable (rid, index, tokens, logprobs, finished), got {req.stream!r}")
        if req.num_beams is not None:
            raise RequestRejected("a beam request cannot stream: a group's outputs are reordered until it ends")
        if req.score is not None:
            raise RequestRejected("a score request generates nothing and cannot stream")
        if not engine_takes(self.engine, FEATURES["stream"]):
            raise ValueError("this engine cannot stream (no slots_drain): stream is not available")

    def _check_beam(self, req: Request):
        """a beam request is refused whole rather than run with anything dropped"""
        from .beam import MAX_BEAMS
        B = req.num_beams
        if isinstance(B, bool) or not isinstance(B, (int, np.integer)) or not 2 <= B <= MAX_BEAMS:
            raise RequestRejected(f"num_beams must be an integer in [2, {MAX_BEAMS}], got {B!r}")
        if isinstance(req.num_return, bool) or not isinstance(req.num_return, (int, np.integer)) or not 1 <= req.num_return <= B:
            raise RequestRejected(f"num_return must be an integer in [1, num_beams = {B}], got {req.num_return!r}")
        if not np.isfinite(float(req.length_penalty)):
            raise RequestRejected(f"length_penalty must be finite, got {req.length_penalty!r}")
        if req.n != 1:
            raise RequestRejected("beam search returns num_return hypotheses: n must be 1")
        if B > self.n_slots:
            raise ValueError(f"num_beams = {B} needs more than the {self.n_slots} usable slots")
        if not hasattr(self.engine, "slots_beam"):
            raise ValueError("this engine cannot run a beam group (no slots_beam): num_beams is not available")
        if getattr(self.engine, "spec_k", 0):
            raise RequestRejected("beam search cannot run while the engine speculates")
        sp = req.sampling
        if sp is not None:
            plain = (float(getattr(sp, "temperature", 0.0)) == 0.0 and int(getattr(sp, "top_k", 0) or 0) == 0 and float(getattr(sp, "top_p", 1.0)) == 1.0
                     and float(getattr(sp, "repetition_penalty", 1.0)) == 1.0 and float(getattr(sp, "frequency_penalty", 0.0)) == 0.0
                     and float(getattr(sp, "presence_penalty", 0.0)) == 0.0)
            if not plain:
                raise RequestRejected("a beam request takes no sampling parameters other than temperature = 0 (no top_k, top_p or penalties)")
            req.sampling = None                      # plain greedy parameters say nothing a beam row could honour or break
        for name, what in (("rules", "logit rules"), ("guide", "a guide"), ("ngram", "an n-gram rule"), ("stop", "stop strings"), ("loop", "a loop guard"),
                           ("logprobs", "logprobs")):
            if getattr(req, name) is not None:
                raise RequestRejected(f"a beam request takes no {what}")

    @property
    def idle(self) -> bool:
        return (not self.pending and not self.running and not self._ahead and not self._rejected and not self.filling and not self._scored
                and not self._cancelled)

    def free_slots(self) -> List[int]:
        held = {s for s, _, _ in self.filling} | {k for ks in self._fill_kids.values() for k in ks}
        return [s for s in range(self.n_slots) if s not in self.running and s not in held]

    # ------------------------------------------------------------------ admission
    ADMIT_AHEAD = 64                                 # tokens beyond the prompt dots_slots_prefill reserves (slots.hip KV_ADMIT_AHEAD)

    def _admit_pages(self, prompt: int, max_new: int) -> int:
        return (min(prompt + min(int(max_new), self.ADMIT_AHEAD), self.max_seq_len) + 63) // 64

    def _group_pages(self, r: Request) -> int:
        """pages a request takes at admission: sequence 0 its prompt + ADMIT_AHEAD, each further sequence of n > 1 the same less the full
        prompt pages it shares with sequence 0 (Engine.slots_fork)"""
        t = int(r.input_ids.shape[0])
        if r.num_beams:
            return self._beam_pages(r)
        if r.tails:                                  # after the extend (or score): every sequence holds its own longer prompt + ADMIT_AHEAD
            return sum(self._admit_pages(t + len(x), r.max_new_tokens) for x in r.tails) - (len(r.tails) - 1) * (t // 64)
        need = self._admit_pages(t, r.max_new_tokens)
        return need + (int(r.n) - 1) * (need - t // 64)

    def _beam_pages(self, r: Request) -> int:
        """a beam group is fully reserved when it is made (Engine.slots_beam): the floor(t / 64) full prompt pages once, and per beam the
        pages of the positions [64 floor(t / 64), t + max_new) plus one spare"""
        t = int(r.input_ids.shape[0])
        shared = t // 64
        return shared + int(r.num_beams) * ((t + int(r.max_new_tokens) + 63) // 64 - shared + 1)

    def _worst_pages(self, r: Request, n: Optional[int] = None) -> int:
        """pages of the request's sequences at their caps, the shared prompt pages counted once; n: of that many of its sequences only
        (what is still running: a conservative count, as if sequence 0 were among them)"""
        if r.num_beams:
            return self._beam_pages(r)               # the whole group holds its pages until it is released together
        t, n = int(r.input_ids.shape[0]), r.seqs if n is None else n
        if r.tails:                                  # the n longest of its sequences: conservative for whatever is still running
            each = sorted(((min(t + len(x) + int(r.max_new_tokens), self.max_seq_len) + 63) // 64 for x in r.tails), reverse=True)[:n]
            return sum(each) - (len(each) - 1) * (t // 64)
        worst = (min(t + int(r.max_new_tokens), self.max_seq_len) + 63) // 64
        return worst + (n - 1) * (worst - t // 64)

    def _running_worst(self) -> int:
        seqs: Dict[int, Tuple[Request, int]] = {}
        for rid, r in self.running.values():
            seqs[rid] = (r, seqs.get(rid, (r, 0))[1] + 1)
        for _, rid, r in self.filling:                # a filling request will run all its sequences
            seqs[rid] = (r, r.seqs)
        return sum(self._worst_pages(r, k) for r, k in seqs.values())

    def _fits_full_reservation(self, admitted: Sequence[Request], new: Sequence[Request]) -> bool:
        """Full reservation (headroom_pages=None): the worst case of everything in flight — running, already in this group, prefetched —
        plus `new` must fit the pool.  Applied on EVERY admission path (ordinary, look-ahead, prefetched group)."""
        if not self.full_reservation or not hasattr(self.engine, "kv_pool_info"):
            return True
        total = self.engine.kv_pool_info()[0]
        committed = self._running_worst() + sum(self._worst_pages(r) for r in admitted)
        return committed + sum(self._worst_pages(r) for r in new) <= total

    # ------------------------------------------------------------------ prefix caching
    def _lookup(self, rid: int, req: Request) -> Tuple[int, int, bool]:
        """(lease, hit tokens, needs the tower) of the request: the engine's answer, held until _prefill consumes it or _unlease drops it.
        Off: no lease, no hit, the tower whenever there are patches — and no engine call"""
        if not self.prefix_caching:
            return 0, 0, req.n_patches() > 0
        if rid not in self._leases:
            ids = np.ascontiguousarray(req.input_ids, dtype=np.int32).reshape(-1)
            self._leases[rid] = self.engine.prefix_cache_lookup(ids, req.image_key)
        return self._leases[rid]

    def _unlease(self, rids):
        """the requests go back to the queue (or nowhere): their leases go back to the engine"""
        for rid in rids:
            lease = self._leases.pop(rid, (0, 0, True))[0]
            if lease:
                self.engine.prefix_cache_release(lease)

    def _tower_patches(self, rid: int, req: Request) -> int:
        """patches the request sends to the tower: none when its image rows are cached"""
        return req.n_patches() if self._lookup(rid, req)[2] else 0

    def plan_admission(self) -> List[Tuple[int, int, Request]]:
        """FIFO: pop requests while a slot is free and the group fits the ViT and prefill workspaces.
        Lowest slots first, so the decode graph covers as few rows as possible."""
        if self.suspended:
            return []                                # nothing new while anything is suspended: the pool's room goes to the resumes first
        free = self.free_slots()
        group, patches, tokens, planned = [], 0, 0, 0
        pages_free = self.engine.kv_pool_info()[1] if hasattr(self.engine, "kv_pool_info") else 1 << 30
        while self.pending and free and (self.admit_group is None or len(group) < self.admit_group):
            rid, req = self.pending[0]
            if req.width > len(free):
                break                                # n sequences (or beams) need n slots: the head of the queue waits for them, nothing overtakes it
            p, t = self._tower_patches(rid, req), int(req.input_ids.shape[0])
            # the prefill workspace bounds a group that is prefilled in one pass; a group filled in passes is bounded by the pool alone
            if group and (patches + p > self.max_patches or (self.prefill_chunk is None and tokens + t > self.max_prefill_tokens)):
                self._unlease([rid])                 # not in this group: it is looked up again when its turn comes
                break
            # paged KV, on demand: a sequence reserves its prompt + ADMIT_AHEAD tokens now and grows page by page; admit only while every
            # running sequence (and this one) could still take `headroom` more pages, so that a dry pool — which ends a sequence early
            # at what its pages hold — stays the exception.  Nothing running: admit whatever fits (submit() checked that it can).
            need = self._group_pages(req) - self._lookup(rid, req)[1] // 64      # the pages it hit are there already
            if self.prefix_caching:                  # ... and its lease took them out of the free count: read it again, less what this group plans to take
                pages_free = self.engine.kv_pool_info()[1] - planned
            taken = len(self.running) + sum(r.width for _, _, r in self.filling) + sum(r.width for _, _, r in group)
            busy = bool(self.running or self.filling or group)
            reserve = self.headroom_pages * (taken + req.width) if busy else 0
            if (busy and not self._fits_full_reservation([r for _, _, r in group], [req])) or need + reserve > pages_free:
                # the worst case of everything in flight must fit the pool (submit() checked a lone request), and the admission pages must
                # be free now: wait for a running sequence to return its pages
                self._unlease([rid])
                break
            pages_free -= need
            planned += need
            self.pending.popleft()
            group.append((free.pop(0), rid, req))
            if req.width > 1:
                self._kids[rid] = [free.pop(0) for _ in range(req.width - 1)]
            patches += p
            tokens += t
        return group

    def _pixels(self, with_img):
        """(pixel values, grid, on_device, keep-alive) of the requests' images, packed in order"""
        grid = np.concatenate([np.asarray(r.grid_thw, dtype=np.int64).reshape(-1, 3) for _, r in with_img])
        pvs = [r.pixel_values for _, r in with_img]
        if all(hasattr(p, "is_cuda") and p.is_cuda for p in pvs):
            import torch
            pv = pvs[0] if len(pvs) == 1 else torch.cat(pvs, dim=0)
            pv = pv.contiguous().float()
            torch.cuda.synchronize(pv.device)
            return pv.data_ptr(), grid, True, pv
        host = [p.detach().cpu().numpy() if hasattr(p, "detach") else np.asarray(p) for p in pvs]
        return np.concatenate(host).astype(np.float32, copy=False), grid, False, None

    def _clear_rows(self, slots):
        """no per-row entry stays on these (free) slots: it would keep the per-row stage on"""
        clear_rows(self.engine, self._rows, slots)
        for s in slots:
            if s in self._predicted:
                self._predicted.discard(s)
                self.engine.set_row_prediction(s, None)

    def _set_rows(self, s, r, index: int = 0):
        """per-row parameters of request r on slot s; they apply from the first token the prefill selects.  index: the sequence of a
        request with n > 1 — its seed is the request's + index (vLLM's rule), everything else is shared"""
        apply_row(self.engine, self._rows, s, r, index)
        # the prediction travels beside the table (row_features): set before the prefill, cleared when the slot is admitted without one
        if r.prediction:
            self._predicted.add(s)
            self.engine.set_row_prediction(s, r.prediction)
        elif s in self._predicted:
            self._predicted.discard(s)
            self.engine.set_row_prediction(s, None)

    def _prefill(self, group, rows_set: bool = False):
        # image rows are consumed in packed order, so sequences with images keep their relative order: pack the group as is
        slots = [s for s, _, _ in group]
        lens = [int(r.input_ids.shape[0]) for _, _, r in group]
        caps = [int(r.max_new_tokens) for _, _, r in group]
        kids = {rid: self._kids.pop(rid) for _, rid, r in group if r.width > 1}   # the slots of sequences 1 .. n - 1 (parallel sampling) or of beams 1 .. B - 1
        every = slots + [k for ks in kids.values() for k in ks]
        for s, rid, r in ([] if rows_set else group):     # a prefetched group: its tower has run, so it goes in (or fails) as a whole
            try:
                self._set_rows(s, r)
                for j, k in enumerate(kids.get(rid, ()), 1):
                    self._set_rows(k, r, j)
            except Exception:
                self._clear_rows(every)              # nothing of this group stays behind; the caller puts the group back in the queue
                self._unlease([rid for _, rid, _ in group])
                raise
        try:
            if self.prefix_caching:
                got = [self._lookup(rid, r) for _, rid, r in group]
                self.engine.slots_prefill_begin_cached(slots, np.concatenate([r.input_ids for _, _, r in group]), lens, caps, [g[0] for g in got],
                                                       [r.image_key for _, _, r in group])
                for (_, rid, r), (_, hit, _) in zip(group, got):             # the begin consumed the leases
                    del self._leases[rid]
                    r.cached_tokens = hit
                    self.prefix_hits += hit > 0
                    self.prefix_hit_tokens += hit
            elif self.prefill_chunk is not None:
                self.engine.slots_prefill_begin(slots, np.concatenate([r.input_ids for _, _, r in group]), lens, caps)
            else:
                self.engine.slots_prefill(slots, np.concatenate([r.input_ids for _, _, r in group]), lens, caps)
        except Exception:
            self._clear_rows(every)                  # the slots stay free
            self._unlease([rid for _, rid, _ in group])
            raise
        if self.prefill_chunk is not None:           # the slots are filling: _advance_fill takes it from here, pass by pass
            self.filling += group
            self._fill_kids.update(kids)
            self.admissions += 1
            return
        self._after_prefill(group, kids)
        self.admissions += 1

    def _after_prefill(self, group, kids):
        """the requests of `group` hold a fresh prefill (one pass, or the pass that completed their fill): fork, beam group or extend of a
        request with several sequences, before any decode step; then they are running"""
        slots = [s for s, _, _ in group]
        every = slots + [k for ks in kids.values() for k in ks]
        forked: List[int] = []
        try:                                         # one fork per request with n > 1, before any decode step: the prefill is still fresh
            for s, rid, r in group:
                if rid in kids:
                    if r.num_beams:                  # a group's slots go back with its source
                        self.engine.slots_beam(s, kids[rid])
                    else:
                        self.engine.slots_fork(s, kids[rid])
                        forked += kids[rid]
            for s, rid, r in group:                  # after every fork (an extend ends the prefill's fork window): one extend per request with suffixes
                if r.suffixes:
                    self.engine.slots_extend([s] + kids[rid], r.suffixes, keep_pending=False, max_new_tokens=int(r.max_new_tokens))
            for s, rid, r in group:                  # likewise one score per request with candidates: its entries are read here, nothing decodes
                if r.score:
                    r.scores_out = self.engine.slots_score([s] + kids.get(rid, []), r.score, top_n=int(r.score_top_logprobs), keep_pending=False,
                                                           max_new_tokens=1)
        except Exception:
            for s in slots + forked:                 # the prefill went in: give its slots back, the caller re-queues the group
                self.engine.slot_release(s)
            self._clear_rows(every)
            raise
        for s, rid, r in group:
            if r.score:                              # finished at once: the selected token is discarded, the slots go back
                for k in [s] + kids.get(rid, []):
                    self.engine.slot_release(k)
                r.outputs = [np.zeros(0, np.int32) for _ in r.score]
                r.kv_truncated, r.kv_truncated_each = False, [False] * len(r.score)
                self._scored.append((rid, r))
                continue
            for j, k in enumerate([s] + kids.get(rid, [])):
                self.running[k] = (rid, r)
                self._admit_count += 1
                self._admit_seq[k] = self._admit_count
                self._streamed.pop(k, None)
                self._last_lens[k] = 0               # a reused slot must not inherit its previous occupant's length (_soon_free counted a
                                                     # just-admitted long request as "about to finish" and the look-ahead group was sized for slots that stayed busy)
                if r.seqs > 1:
                    self._seq_index[k] = j
            if r.seqs > 1:
                r._parts = {}

    def _advance_fill(self) -> bool:
        """One pass over the filling slots, oldest first.  The requests whose fill it completed do their fork, beam conversion or extend
        now — the pass is their fresh prefill — and join `running`.  -> whether any did"""
        self.engine.slots_prefill_advance(self.prefill_chunk)
        self.fill_passes += 1
        fin, _ = self.engine.slots_poll()
        joined = [(s, rid, r) for s, rid, r in self.filling if fin[s] != 3]
        if not joined:
            return False
        self.filling = [(s, rid, r) for s, rid, r in self.filling if fin[s] == 3]
        kids = {rid: self._fill_kids.pop(rid) for _, rid, _ in joined if rid in self._fill_kids}
        try:
            self._after_prefill(joined, kids)
        except Exception:                            # their slots were given back: the requests return to the head of the queue for the caller
            self.pending.extendleft(reversed([(rid, r) for _, rid, r in joined]))
            raise
        return True

    def _admit(self, group):
        # per-row parameters first, before the tower runs: a request whose own parameters the engine refuses (submit() and the server
        # validate what they can see; this is the engine's last word) is rejected alone — the rest of the group goes on without it
        kept = []
        for s, rid, r in group:
            try:
                self._set_rows(s, r)
                for j, k in enumerate(self._kids.get(rid, ()), 1):
                    self._set_rows(k, r, j)
                kept.append((s, rid, r))
            except Exception as e:
                self._clear_rows([s] + self._kids.pop(rid, []))
                self._unlease([rid])
                r.error = RequestRejected(str(e))
                self._rejected.append((rid, r))
        if not kept:
            return
        with_img = [(rid, r) for _, rid, r in kept if self._tower_patches(rid, r) > 0]      # a request whose image rows are cached sends no pixels
        if with_img:
            pv, grid, on_dev, keep = self._pixels(with_img)
            self.engine.vit_forward(pv, grid, on_device=on_dev)
            if on_dev:
                self.engine.synchronize()            # `keep` may be a temporary
        self._prefill(kept, rows_set=True)

    # ------------------------------------------------------------------ look-ahead (prefetched towers)
    def _admit_ahead(self) -> bool:
        """The group whose tower was prefetched goes in as a whole as soon as it has the slots and the pages."""
        free = self.free_slots()
        if self.suspended or len(free) < sum(r.width for _, r in self._ahead):
            return False
        # sequences are decoding and the tower is still running: taking the group now would queue every decode chunk behind the tower
        # (vit_take makes the engine's stream wait for it) — keep decoding, take it when its rows exist.  Nothing running: wait for it.
        if self.running and hasattr(self.engine, "vit_ready") and not self.engine.vit_ready():
            return False
        if hasattr(self.engine, "kv_pool_info"):
            need = sum(self._group_pages(r) - self._lookup(rid, r)[1] // 64 for rid, r in self._ahead)
            reserve = self.headroom_pages * (len(self.running) + sum(r.width for _, r in self._ahead)) if self.running else 0
            if need + reserve > self.engine.kv_pool_info()[1]:
                return False
            if self.running and not self._fits_full_reservation([], [r for _, r in self._ahead]):
                return False
        group = self._ahead
        placed = []
        for rid, r in group:                         # lowest slots first; the sequences of a request with n > 1 side by side
            placed.append((free.pop(0), rid, r))
            if r.width > 1:
                self._kids[rid] = [free.pop(0) for _ in range(r.width - 1)]
        try:
            self.engine.vit_take()
            self._prefill(placed)
        except Exception:
            for rid, _ in group:
                self._kids.pop(rid, None)
            # the rows are gone (or were never there): the group goes back to the head of the queue so that the caller's failure
            # handling — which walks `pending` and `running` — sees its requests, and the next step does not take a stale batch
            self._ahead, self._ahead_keep = [], None
            self._unlease([rid for rid, _ in group])
            self.pending.extendleft(reversed(group))
            raise
        self._ahead, self._ahead_keep = [], None
        return True

    def _look_ahead(self):
        """Start the tower of the next queued requests (FIFO prefix, image requests only) on the side stream."""
        if not self.prefetch or self._ahead or not self.pending:
            return
        total_pages = self.engine.kv_pool_info()[0] if hasattr(self.engine, "kv_pool_info") else 1 << 30
        group, patches, tokens, pages = [], 0, 0, 0
        # A prefetched group goes in only as a whole, and nothing may overtake it: a group larger than the slots that are free — or will be
        # by the time its tower is done — would hold freed slots idle while it waits for the rest; with uneven output lengths (the
        # reference's max_new_tokens=24000) for a long time.  The tower of k pages lasts about k * tower_steps_per_page decode
        # steps, so the group is the LARGEST k <= prefetch for which k slots are free or within that horizon (+ two chunks) of their caps:
        # equal caps (a document's pages: everything finishes together) prefetch the whole next group while the current one decodes — the
        # round-5 rule "free now or within two chunks" started ONE tower there and ran the other 31 at admission, nothing beside them
        # (mixed64: 4.40 -> 4.00 pages/s, profiles/r05_mixed64_lookahead_regression.txt).  At least one, so that a full engine still
        # hides the next tower.
        cap = 1
        for k in range(min(self.prefetch, self.n_slots), 1, -1):
            if len(self.free_slots()) + self._soon_free(2 * self.chunk + k * self.tower_steps_per_page) >= k:
                cap = k
                break
        while self.pending and sum(r.width for _, r in group) + self.pending[0][1].width <= cap:      # cap counts slots: a request takes n of them
            rid, req = self.pending[0]
            # a request whose image rows are cached needs no tower: like a text-only request it ends the group and goes through the ordinary
            # admission in its turn.  The others keep their lease while their tower runs ahead: _admit_ahead's begin relies on it
            p, t = self._tower_patches(rid, req), int(req.input_ids.shape[0])
            pg = self._group_pages(req) - self._lookup(rid, req)[1] // 64
            if (p == 0 or patches + p > self.max_patches or (self.prefill_chunk is None and tokens + t > self.max_prefill_tokens)
                    or pages + pg > total_pages):
                self._unlease([rid])
                break                                # a text-only request goes through the ordinary admission, in its turn
            if self.full_reservation and sum(self._worst_pages(r) for _, r in group) + self._worst_pages(req) > total_pages:
                self._unlease([rid])
                break                                # full reservation: the group must fit an EMPTY pool by its worst case (its tower may run ahead;
                                                     # _admit_ahead holds it back until it also fits beside what is still running)
            self.pending.popleft()
            group.append((rid, req))
            patches, tokens, pages = patches + p, tokens + t, pages + pg
        if not group:
            return
        try:
            pv, grid, on_dev, keep = self._pixels(group)
            self.engine.vit_prefetch(pv, grid, on_device=on_dev)
        except Exception:
            self._unlease([rid for rid, _ in group])
            self.pending.extendleft(reversed(group))     # nothing was prefetched: the requests keep their place in the queue
            raise
        self._ahead, self._ahead_keep = group, keep

    def _soon_free(self, horizon: Optional[int] = None) -> int:
        """running sequences within `horizon` decode steps (default: two chunks) of their generation cap (lengths as of the last poll)"""
        horizon = 2 * self.chunk if horizon is None else horizon
        return sum(1 for s, (_, r) in self.running.items() if self._last_lens.get(s, 0) + horizon >= int(r.max_new_tokens))

    # ------------------------------------------------------------------ main loop
    def _collect(self) -> List[Tuple[int, Request, np.ndarray]]:
        for rid in sorted(self._cancel & {rid for rid, _ in self.running.values()}):      # cancelled while they were being admitted
            self.cancel(rid)
        # one drain for every streaming row's new tokens while anything streams, else the plain poll
        deltas = {}
        if any(r.stream is not None for _, r in self.running.values()):
            fin, lens, deltas = self.engine.slots_drain()
        else:
            fin, lens = self.engine.slots_poll()
        done = [(rid, r, r.outputs[0]) for rid, r in self._scored]
        self._scored = []
        for s in sorted(self.running):
            if s not in self.running:                # a slot of a beam group that has just been reported
                continue
            if self.running[s][1].stream is not None and fin[s] != 1 and s in deltas:
                rid, req = self.running[s]
                toks, entries = deltas[s]
                self._streamed[s] = self._streamed.get(s, 0) + len(toks)
                req.stream(rid, self._seq_index.get(s, 0), toks, entries, False)
            if self.running[s][1].num_beams:
                out = self._collect_beam(s, bool(fin[s] == 1))
                if out is not None:
                    done.append(out)
                continue
            if fin[s] == 1:
                rid, req = self.running.pop(s)
                self._admit_seq.pop(s, None)
                toks = self.engine.slot_read(s, int(lens[s]))
                # a sequence the engine ended early because the KV pool ran dry (its cap was lowered to what its pages hold) is not an
                # ordinary "length" stop: say so on the request, count it, let the server report it
                req.kv_truncated = False
                if hasattr(self.engine, "slot_capacity"):
                    _, limit = self.engine.slot_capacity(s)
                    req.kv_truncated = bool(limit < int(req.input_ids.shape[0]) + int(req.max_new_tokens) and len(toks) >= limit - int(req.input_ids.shape[0]))
                    self.kv_truncated += int(req.kv_truncated)
                lp_out = None
                if req.logprobs is not None:         # read before the release switches the slot's logprobs off
                    lp_out = self.engine.row_logprobs(s, len(toks))
                hit = None
                if req.stop is not None:             # read before the release clears the row's automaton and its hit record
                    hit = self.engine.row_stop_hit(s)
                loop_hit = None
                if req.loop is not None:             # likewise: the release clears the row's rule and its hit record
                    loop_hit = self.engine.row_loop_hit(s)
                if req.prediction:                   # likewise: the release clears the prediction, the next prefill its counters
                    req.prediction_stats = self.engine.row_prediction_stats(s)
                if req.stream is not None:
                    # its last tokens, before it is reported: what the drain brought, and — a row that held more than one drain
                    # delivers — the rest of what was just read
                    sent = self._streamed.pop(s, 0)
                    entries = None if lp_out is None else tuple(a[sent:] for a in lp_out)
                    req.stream(rid, self._seq_index.get(s, 0), np.asarray(toks[sent:], np.int32), entries, True)
                if req.seqs == 1:
                    if req.stop is not None:
                        req.stop_hit = hit
                    if req.loop is not None:
                        req.loop_hit = loop_hit
                    if req.logprobs is not None:
                        req.logprobs_out = lp_out
                    done.append((rid, req, toks))
                else:
                    # one sequence of n: its slot goes back now, the request is reported once, when its last sequence has finished
                    req._parts[self._seq_index.pop(s)] = (toks, lp_out, req.kv_truncated, hit, loop_hit)
                    if len(req._parts) == req.seqs:
                        parts = [req._parts[j] for j in range(req.seqs)]
                        req.outputs = [part[0] for part in parts]
                        if req.logprobs is not None:
                            req.logprobs_out = [part[1] for part in parts]
                        if req.stop is not None:
                            req.stop_hit = [part[3] for part in parts]
                        if req.loop is not None:
                            req.loop_hit = [part[4] for part in parts]
                        req.kv_truncated_each = [part[2] for part in parts]
                        req.kv_truncated = any(req.kv_truncated_each)
                        del req._parts
                        done.append((rid, req, req.outputs[0]))
                release_row(self.engine, self._rows, s, self.engine.slot_release)    # each feature by its release rule (row_features)
        self._last_lens = {s: int(lens[s]) for s in self.running}      # after the finished slots have left: only what is still decoding
        return done

    def _collect_beam(self, s: int, finished: bool):
        """The beam group that slot s belongs to, at a poll: finished (its cap, or no live beam), or — exact for length_penalty >= 0 —
        ended early because num_return completed hypotheses already outscore whatever a live beam could still become (beam.may_stop).
        The request is reported once, best hypothesis first, and its slots go back together."""
        from .beam import may_stop, rank_hypotheses
        rid, req = self.running[s]
        tr = self.engine.beam_read(s)
        if not finished and not may_stop(tr["completed"], tr["cum"], req.max_new_tokens, req.length_penalty, req.num_return):
            return None
        # a group ended early is ranked on its completed hypotheses alone: at the cap no live beam could have outscored the returned ones
        live = tr["cum"] if finished else np.full_like(tr["cum"], -np.inf)
        hyps = rank_hypotheses(tr["completed"], tr["parents"], tr["tokens"], live, tr["steps"], req.length_penalty, req.num_return)
        req.outputs = [np.asarray(h["tokens"], np.int32) for h in hyps]
        req.cumulative_logprobs = [h["cum"] for h in hyps]
        req.beam_scores = [h["score"] for h in hyps]
        req.finish_reasons = [h["finish_reason"] for h in hyps]
        req.kv_truncated = False                     # a group is fully reserved: the pool cannot run dry under it
        for k in [k for k, (r2, _) in self.running.items() if r2 == rid]:
            del self.running[k]
            self._admit_seq.pop(k, None)
        self.engine.slot_release(s)                  # one slot of the group releases all of them
        return rid, req, req.outputs[0] if req.outputs else np.zeros(0, np.int32)

    def step(self) -> List[Tuple[int, Request, np.ndarray]]:
        """Admit what fits, run one decode chunk, return the requests that finished: (id, request, new token ids).  A request the engine
        refused at admission comes back at once with no tokens and `request.error` set (RequestRejected)."""
        out = self._step()
        rejected, self._rejected = self._rejected, []
        cancelled, self._cancelled = self._cancelled, []
        return [(rid, r, np.zeros(0, np.int32)) for rid, r in rejected] + cancelled + out

    # ------------------------------------------------------------------ cancellation
    def cancel(self, rid: int) -> bool:
        """Stop request `rid` wherever it is.  Pending: it leaves the queue.  Running or suspended: its slots, their pages (parked host
        pages too) and row handles go back.  Inside a chunked fill or a prefetched group: flagged, and cancelled by the first collect
        that sees it running.  A member of an n group cancels the group.  The request is reported once by step(), with
        request.cancelled = True and the tokens it had (outputs in index order for several sequences).  -> whether rid was found"""
        for i, (pid, r) in enumerate(self.pending):
            if pid == rid:
                del self.pending[i]
                self._unlease([rid])
                self._cancel.discard(rid)
                self._report_cancelled(rid, r, [np.zeros(0, np.int32) for _ in range(r.seqs)])
                return True
        slots = sorted(s for s, (k, _) in self.running.items() if k == rid)
        if not slots:
            if any(k == rid for _, k, _ in self.filling) or any(k == rid for k, _ in self._ahead):
                self._cancel.add(rid)
                return True
            return False
        self._cancel.discard(rid)
        req = self.running[slots[0]][1]
        _, lens = self.engine.slots_poll()
        parts = dict(getattr(req, "_parts", {}))     # the sequences of an n group that had finished already: (tokens, ...)
        outs = {j: t[0] for j, t in parts.items()}
        for s in slots:
            if not req.num_beams:
                outs[self._seq_index.get(s, 0)] = self.engine.slot_read(s, int(lens[s]))
        for s in slots:
            if not req.num_beams or s == slots[0]:   # one slot of a beam group releases all of them
                self.engine.slot_release(s)
            del self.running[s]
            for d in (self._admit_seq, self._seq_index, self._last_lens, self._streamed, self._parked_pages):
                d.pop(s, None)
            if s in self.suspended:
                self.suspended.remove(s)
        cancel_rows(self.engine, self._rows, slots)  # the release switched the rows off: the handles' records go too
        self._predicted.difference_update(slots)     # ... and cleared their predictions
        if hasattr(req, "_parts"):
            del req._parts
        self._report_cancelled(rid, req, [outs.get(j, np.zeros(0, np.int32)) for j in range(max(1, req.seqs if not req.num_beams else 1))])
        return True

    def _report_cancelled(self, rid: int, req: Request, outs):
        req.cancelled = True
        req.kv_truncated = False
        if len(outs) > 1:
            req.outputs = outs
            req.kv_truncated_each = [False] * len(outs)
        self._cancelled.append((rid, req, outs[0]))

    # ------------------------------------------------------------------ preemption
    def _active(self) -> List[int]:
        """slots of the sequences that take decode steps: running and not suspended"""
        return [s for s in self.running if s not in self._parked_pages]

    def _resume(self):
        """The longest-suspended sequence comes back once the pool can hold its pages, the next chunk of every active sequence and of
        itself, and the admission headroom; with nothing else active it comes back as soon as its pages fit (submit() made sure that a
        request can finish alone).  One at a time, in suspension order: nothing overtakes the head."""
        ahead = -(-self.chunk // 64)                 # pages a sequence can take in one chunk
        while self.suspended:
            s = self.suspended[0]
            need, active = self._parked_pages[s], len(self._active())
            room = need + ((ahead + self.headroom_pages) * (active + 1) if active else 0)
            if self.engine.kv_pool_info()[1] < room:
                return
            self.engine.slot_resume(s)
            self.suspended.pop(0)
            del self._parked_pages[s]
            self.resumes += 1

    def _preempt(self):
        """Before a decode chunk: while the engine says the chunk would run short of pages, suspend the most recently admitted active
        sequence — never a beam-group row (a group is fully reserved and cannot be parked), never the last active sequence.  A full host
        space ends the loop: the engine then caps a sequence as it does without preemption (counted in kv_truncated)."""
        from .engine import E_CAPACITY, E_STATE, DotsEngineError
        while self.engine.slots_pages_short(self.chunk) > 0:
            active = self._active()
            victims = [s for s in active if not self.running[s][1].num_beams]
            if len(active) <= 1 or not victims:
                return
            s = max(victims, key=lambda k: self._admit_seq.get(k, 0))
            host_free = self.engine.kv_swap_info()[1]
            try:
                self.engine.slot_suspend(s)
            except DotsEngineError as e:
                if getattr(e, "code", None) not in (E_STATE, E_CAPACITY):
                    raise
                return                               # the host space is full (or the row cannot be parked): cap as before
            self._parked_pages[s] = host_free - self.engine.kv_swap_info()[1]
            self.suspended.append(s)
            self.preemptions += 1
            self.swapped_pages += self._parked_pages[s]

    def _step(self) -> List[Tuple[int, Request, np.ndarray]]:
        if self.suspended:
            self._resume()                           # before admission: a suspended sequence is older than anything in the queue
            if self.suspended and not self._active():
                raise RuntimeError(f"slot {self.suspended[0]} is suspended and cannot be resumed into an otherwise idle engine "
                                   f"(KV pool {self.engine.kv_pool_info()}, {self._parked_pages[self.suspended[0]]} pages parked)")
        if self._ahead:                              # a prefetched group waits for its slots: nothing may overtake it
            admitted = self._admit_ahead()
        else:
            group = self.plan_admission()
            admitted = bool(group)
            if group:
                try:
                    self._admit(group)
                except Exception:
                    # vit_forward / slots_prefill failed: plan_admission popped these requests and nothing registered them yet — put them
                    # back at the head of the queue (in order) so that the caller's failure handling, which walks `pending`, `running` and
                    # the prefetched group, finds every request (server.py fails their futures; a lost request would hang its HTTP call)
                    for s, rid, _ in group:
                        for k in [s] + self._kids.pop(rid, []):
                            self.running.pop(k, None)
                            self._seq_index.pop(k, None)
                    self._unlease([rid for _, rid, _ in group])
                    self.pending.extendleft(reversed([(rid, r) for _, rid, r in group if getattr(r, "error", None) is None]))
                    raise
        self._look_ahead()
        if self.prefill_chunk is not None:           # at most one pass per step, then the step's decode chunk over the running rows
            admitted = bool(self.filling) and self._advance_fill()
        if admitted:
            done = self._collect()                   # a 1-token cap or an immediate EOS finishes at prefill
            if done:
                return done
        if not self.running:
            if self.filling:                         # nothing decodes yet: the next step runs the next pass
                return []
            if self._rejected:                       # the whole group was refused: report it, admit the next one on the next step
                return []
            if self._ahead:                          # nothing runs, so every slot and page is free: the group fits by construction
                raise RuntimeError("a prefetched group could not be admitted into an empty engine")
            if self.pending:                         # nothing runs, nothing could be admitted: it never will be
                rid, req = self.pending[0]           # left in the queue: whoever handles the error finds (and fails) it there
                raise RuntimeError(f"request {rid} ({req.input_ids.shape[0]} prompt tokens, {req.n_patches()} patches) cannot be admitted "
                                   f"into an empty engine (KV pool {self.engine.kv_pool_info() if hasattr(self.engine, 'kv_pool_info') else '?'})")
            return []
        if self.preemption == "swap":
            self._preempt()
        self.engine.slots_decode(self.chunk)
        self.decode_steps += self.chunk
        return self._collect()

    def _shared_pages_now(self) -> int:
        info = getattr(self.engine, "shared_prefix_info", None)
        return int(info()["pages_not_read"]) if info is not None else 0

    @property
    def shared_pages_not_read(self) -> int:
        """KV pages (one kv head of one layer each) this batcher's decode steps did not read because rows shared them"""
        return self._shared_pages_now() - self._shared_base

    def run_pull(self, pull, low_water: Optional[int] = None) -> Dict[object, np.ndarray]:
        """An open-ended job: `pull(k)` returns up to k (key, Request) pairs from a source shared with other ranks ([] = the source is dry;
        dots_ocr_amd.dp.PageQueue).  Requests are pulled only as they can be used — while fewer than `low_water` (default: the look-ahead
        group size, at least one) are queued beyond what the free slots can take — so a rank never hoards pages another rank could start.
        Returns {key: new token ids}."""
        low = max(1, self.prefetch) if low_water is None else max(1, int(low_water))
        keys: Dict[int, object] = {}
        out: Dict[object, np.ndarray] = {}
        dry = False
        while True:
            want = low + len(self.free_slots()) - len(self._ahead) - len(self.pending)       # what the free slots can take now + the look-ahead's next group
            if not dry and want > 0:
                got = pull(want)
                dry = not got
                for key, req in got:
                    keys[self.submit(req)] = key
            if self.idle:
                if dry:
                    return out
                continue
            for rid, _, toks in self.step():
                out[keys.pop(rid)] = toks

    def run(self, requests: Iterable[Request]) -> List[np.ndarray]:
        ids = [self.submit(r) for r in requests]
        out: Dict[int, np.ndarray] = {}
        refused = None
        while not self.idle:
            for rid, req, toks in self.step():
                out[rid] = toks
                refused = refused or getattr(req, "error", None)
        if refused is not None:                      # every other request has finished
            raise refused
        return [out[i] for i in ids]
