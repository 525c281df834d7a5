"""The loop guard: end a row when its output starts to cycle.  Host-only: no torch, no engine import.

LoopRule is what a request carries; first_loop restates the rule by brute force from its definition (the device check,
csrc/loop_dev.h, is tested against it); last_loop asks the same of a row's last token only (a row the device ended fires there);
trimmed cuts a finished row back to one copy of the cycle."""
from __future__ import annotations

import numbers
from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

MAX_LOOP_PERIOD = 1024                       # DOTS_MAX_LOOP_PERIOD
MAX_LOOP_REPEATS = 64
MAX_LOOP_SPAN = 65535


@dataclass(frozen=True)
class LoopRule:
    """Loop rule of one request / decode row (include/dots_ocr_hip.h DotsLoopRule).

    With out[0 .. n] the row's output (the prefill's token is index 0) and L(p) = max(repeats * p, min_span), period p in
    [min_period, max_period] fires after the token at index n iff n + 1 >= L(p) and out[i] == out[i - p] for every i in
    [n + 1 - L(p) + p, n]: the last L(p) tokens repeat with period p.  The row ends at the first n at which any period fires.

    Limits: 1 <= min_period <= max_period <= MAX_LOOP_PERIOD, 2 <= repeats <= MAX_LOOP_REPEATS, 0 <= min_span <= MAX_LOOP_SPAN.

    The defaults (max_period 512, repeats 4, min_span 256) have NOT been tuned on a real checkpoint: none was available where this was
    written.  They are sized so that a legitimate 30-column table row of empty cells passes (a cycle of a few tokens that stands for
    one or two hundred): a cycle must stand four times AND cover 256 tokens before the row is ended."""
    min_period: int = 1
    max_period: int = 512
    repeats: int = 4
    min_span: int = 256

    def __post_init__(self):
        for name in ("min_period", "max_period", "repeats", "min_span"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, numbers.Integral):
                raise ValueError(f"{name} must be an integer, got {v!r}")
            object.__setattr__(self, name, int(v))
        if not 1 <= self.min_period <= self.max_period <= MAX_LOOP_PERIOD:
            raise ValueError(f"periods must satisfy 1 <= min_period <= max_period <= {MAX_LOOP_PERIOD}, got {self.min_period} .. {self.max_period}")
        if not 2 <= self.repeats <= MAX_LOOP_REPEATS:
            raise ValueError(f"repeats must be in [2, {MAX_LOOP_REPEATS}], got {self.repeats}")
        if not 0 <= self.min_span <= MAX_LOOP_SPAN:
            raise ValueError(f"min_span must be in [0, {MAX_LOOP_SPAN}], got {self.min_span}")

    def span(self, p: int) -> int:
        """L(p): how many tokens a cycle of period p must cover"""
        return max(self.repeats * int(p), self.min_span)


_FIELDS = ("min_period", "max_period", "repeats", "min_span")


def as_rule(value) -> Optional[LoopRule]:
    """What a caller may write for `loop_guard`: None / False (off), True (the defaults), a LoopRule, or a mapping with some of the four
    fields.  Anything else, an unknown field or a value out of range: ValueError."""
    if value is None or value is False:
        return None
    if value is True:
        return LoopRule()
    if isinstance(value, LoopRule):
        return value
    if isinstance(value, dict):
        unknown = sorted(set(value) - set(_FIELDS))
        if unknown:
            raise ValueError(f"loop_guard: unknown field(s) {', '.join(map(str, unknown))} (known: {', '.join(_FIELDS)})")
        return LoopRule(**value)
    raise ValueError(f"loop_guard must be true, false or an object with {', '.join(_FIELDS)}, got {value!r}")


def first_loop(ids: Sequence[int], rule: LoopRule) -> Optional[Tuple[int, int, int]]:
    """(n, p, span) of the first hit of `rule` on the output `ids`, or None — by brute force from the definition: for n = 0, 1, ... and
    p = min_period .. max_period, whether the last L(p) tokens of ids[: n + 1] repeat with period p."""
    ids = [int(t) for t in ids]
    for n in range(len(ids)):
        for p in range(rule.min_period, rule.max_period + 1):
            L = rule.span(p)
            if n + 1 < L:
                continue
            if all(ids[i] == ids[i - p] for i in range(n + 1 - L + p, n + 1)):
                return n, p, L
    return None


def last_loop(ids: Sequence[int], rule: LoopRule) -> Optional[Tuple[int, int, int]]:
    """The hit of `rule` at the LAST token of `ids`, or None: what first_loop returns for a row the device ended at its hit (the row's
    last token is then the firing one), without walking the positions before it."""
    ids = [int(t) for t in ids]
    n = len(ids) - 1
    for p in range(rule.min_period, rule.max_period + 1):
        L = rule.span(p)
        if n + 1 >= L and all(ids[i] == ids[i - p] for i in range(n + 1 - L + p, n + 1)):
            return n, p, L
    return None


def trimmed(ids: Sequence[int], hit) -> list:
    """The output of a row that ended with `hit` = (n, p, span), cut back to one copy of the cycle: ids[: n + 1 - span + p].  hit None:
    the ids as they are."""
    ids = list(ids)
    if hit is None:
        return ids
    n, p, span = (int(v) for v in hit)
    return ids[: max(0, n + 1 - span + p)]
