"""What a request can ask of its decode row, in one table: the host-side mirror of RowFeature in csrc/row_stage.h, plus the two row
settings the selection stage does not own (logprobs, stream).  The scheduler, generate()'s static batches and the server's capability
probes all walk ROW_FEATURES; a new per-row feature is one entry here (DESIGN §6.1 lists the other places to touch).  A request's
prediction is not in the table: it shapes nothing a row selects, only what a speculating step drafts, and travels beside
it — the scheduler sets it with the row's features before the prefill and clears it when the slot is admitted without one.

Host-only: no torch, no engine import.  A "request" is anything with the eight fields (scheduler.Request); `held` is the caller's record
of what its rows hold, row -> {feature name -> the value given to the engine}, and has no entry for a row that holds nothing."""
from __future__ import annotations

import dataclasses
from typing import Callable, Dict, Iterable, NamedTuple, Optional, Tuple

# What happens to a feature when its request finishes and the slot is released.  The real engine clears every feature of a row in
# dots_slot_release, so the three rules differ only in what a stand-in engine sees; they are kept apart because the CPU tests pin the
# call sequences, not because the engine needs them to be.
KEEP = "keep"                  # the record survives the release; an explicit call clears the row when the slot is next admitted without it
CLEAR_FIRST = "clear_first"    # cleared by an explicit call before slot_release
FORGET = "forget"              # the record is dropped after slot_release, with no engine call


class RowFeature(NamedTuple):
    name: str                  # the Request field it reads; also its key in `held`
    setter: str                # the Engine method: setter(row, *args) sets it, setter(row, *off) clears it
    args: Callable             # (engine, request, index) -> the set call's arguments behind the row; the first is what `held` records
    off: Tuple                 # the clear call's arguments behind the row
    noun: Optional[str]        # "this engine cannot honour <noun>" at submit; None: submit has no refusal of its own for it
    needs: Tuple[str, ...]     # what the engine must offer to take it
    token_bytes: bool          # ... and whether it must also know its vocabulary's bytes (Engine.set_token_bytes)
    release: str               # KEEP, CLEAR_FIRST or FORGET
    cancel_forgets: bool       # cancel() drops the record without a call (the release cleared the handle); else it clears the row by a call


def _sampling(engine, r, index):
    """sequence `index` of a request with several draws with the request's seed + index (vLLM's rule); everything else is shared"""
    return (r.sampling if index == 0 else dataclasses.replace(r.sampling, seed=int(r.sampling.seed) + index),)


def _stop(engine, r, index):
    """the automaton handle (cached by the engine per tuple of strings) and the request's min_tokens, below which no match is taken"""
    return engine.create_stop(r.stop), int(getattr(r.rules, "min_tokens", 0) or 0)


def _field(name):
    return lambda engine, r, index: (getattr(r, name),)


# in call order: a row's settings apply from the first token its prefill selects, so all of them are set before it
ROW_FEATURES = (
    RowFeature("sampling", "set_row_sampling", _sampling, (None,), None, ("set_row_sampling",), False, KEEP, False),
    RowFeature("logprobs", "set_row_logprobs", _field("logprobs"), (None,), None, ("set_row_logprobs",), False, KEEP, False),
    RowFeature("rules", "set_row_logit_rules", _field("rules"), (None,), "logit rules", ("set_row_logit_rules",), False, KEEP, False),
    RowFeature("guide", "set_row_guide", _field("guide"), (None,), "a guide", ("set_row_guide",), True, FORGET, True),
    RowFeature("ngram", "set_row_ngram", _field("ngram"), (None,), "an n-gram rule", ("set_row_ngram",), False, CLEAR_FIRST, False),
    RowFeature("stop", "set_row_stop", _stop, (None,), "stop strings", ("set_row_stop",), True, FORGET, True),
    RowFeature("loop", "set_row_loop", _field("loop"), (None,), "a loop guard", ("set_row_loop", "row_loop_hit"), False, CLEAR_FIRST, False),
    RowFeature("stream", "set_row_stream", lambda engine, r, index: (True,), (False,), None, ("slots_drain", "set_row_stream"), False, FORGET,
               False),
)
FEATURES: Dict[str, RowFeature] = {f.name: f for f in ROW_FEATURES}
_CLEAR_FIRST = tuple(f for f in ROW_FEATURES if f.release == CLEAR_FIRST)
_FORGET = tuple(f for f in ROW_FEATURES if f.release == FORGET)
_CANCEL_FORGETS = tuple(f for f in ROW_FEATURES if f.cancel_forgets)


def engine_takes(engine, feature: RowFeature, token_bytes: bool = False) -> bool:
    """whether `engine` offers the feature; token_bytes: and knows its vocabulary's bytes where the feature matches on them"""
    return all(hasattr(engine, a) for a in feature.needs) and not (
        token_bytes and feature.token_bytes and getattr(engine, "token_bytes", None) is None)


def rows_holding(held, name: str) -> list:
    """the rows whose record holds feature `name`"""
    return sorted(row for row, mine in held.items() if name in mine)


def _drop(engine, held, row, features, call: bool):
    mine = held.get(row)
    if not mine:
        return
    for f in features:
        if mine.pop(f.name, None) is not None and call:
            getattr(engine, f.setter)(row, *f.off)
    if not mine:
        del held[row]


def apply_row(engine, held, row: int, request, index: int = 0):
    """The request's features onto `row`, before its prefill; what the row held and the request does not carry is cleared.  index: the
    sequence within a request with several.  Each value is recorded before its setter is called, so a call that raises half way is
    still cleared by clear_rows."""
    for f in ROW_FEATURES:
        if getattr(request, f.name) is not None:
            args = f.args(engine, request, index)
            held.setdefault(row, {})[f.name] = args[0]
            getattr(engine, f.setter)(row, *args)
        elif row in held:
            _drop(engine, held, row, (f,), True)


def clear_rows(engine, held, rows: Iterable[int]):
    """no feature stays on these (free) rows: it would keep the per-row stage on"""
    for row in rows:
        _drop(engine, held, row, ROW_FEATURES, True)


def release_row(engine, held, row: int, release: Callable[[int], None]):
    """A finished row goes back: release(row) between the features cleared before it and the records forgotten after it."""
    _drop(engine, held, row, _CLEAR_FIRST, True)
    release(row)
    _drop(engine, held, row, _FORGET, False)


def cancel_rows(engine, held, rows: Iterable[int]):
    """Rows of a cancelled request, already released: the handles the release cleared are forgotten, the rest is cleared by a call."""
    for row in rows:
        _drop(engine, held, row, _CANCEL_FORGETS, False)
    clear_rows(engine, held, rows)
