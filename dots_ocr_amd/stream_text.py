"""Text of a streamed completion, piece by piece (host only).

`IncrementalText` turns the token deltas of one sequence into text deltas under two promises:

  equal to the unstreamed text   "".join(pushes) + finish(hit) == server.completion_text(...) of the whole sequence with the same hit
                                 and include_stop_str flag — the text the unstreamed response carries;
  nothing retracted              every emitted prefix is a prefix of that final text.

So the bytes of an incomplete UTF-8 sequence are held until they complete (an incremental decoder with errors="replace" gives what
decoding the whole gives), ids without bytes (specials) add nothing, and while the row has stop strings the longest suffix of the pending
bytes that is a proper prefix of one of them is held back — as is everything from the first complete occurrence of one on, which the
finishing token's push can hold: finish() cuts there, or keeps the string under include_stop_str.

Where the two decoders can disagree.  completion_text's stop-less branch is the tokenizer's batch_decode(skip_special_tokens=True), the
other branch joins the engine's per-token bytes.  For the byte-level BPE vocabulary of the processor these are the same bytes, with two
exceptions: an ADDED token that is not marked special has text under batch_decode but may have no bytes in the engine's table
(Engine.set_token_bytes gives specials none), and a tokenizer whose decoder does more than join bytes (normalisers, clean-up).  With
`decode` given (ids -> str, the stop-less branch itself) the streamed text follows completion_text: a row without stop strings is decoded by
it on every push (trailing U+FFFD held back: an incomplete character), and a row with stop strings that ends without a hit is reconciled
with it at finish()."""
from __future__ import annotations

import codecs
from typing import Callable, Optional, Sequence


class IncrementalText:
    def __init__(self, token_bytes: Callable[[int], bytes], stop: Optional[Sequence[str]] = None, include_stop_str: bool = False,
                 decode: Optional[Callable[[Sequence[int]], str]] = None):
        self.token_bytes = token_bytes
        self.stops = [s.encode("utf-8") for s in (stop or ()) if s]
        self.include = bool(include_stop_str)
        self.decode = decode
        self.ids = []
        self.ends = []                            # byte position behind every token
        self.pending = bytearray()                # bytes not yet given to the decoder: all bytes from `released` on
        self.released = 0
        self.emitted = ""
        self.dec = codecs.getincrementaldecoder("utf-8")(errors="replace")

    def _emit(self, text: str) -> str:
        self.emitted += text
        return text

    def _hold(self) -> int:
        """bytes at the end of `pending` that may still belong to a stop string"""
        data = bytes(self.pending)
        first = min((at for at in (data.find(p) for p in self.stops) if at >= 0), default=-1)
        if first >= 0:
            return len(data) - first              # a complete occurrence: the text may be cut where it starts
        for k in range(min(len(data), max(len(p) for p in self.stops) - 1), 0, -1):
            tail = data[-k:]
            if any(len(p) > k and p.startswith(tail) for p in self.stops):
                return k
        return 0

    def push(self, tokens) -> str:
        toks = [int(t) for t in tokens]
        self.ids += toks
        if self.decode is not None and not self.stops:
            text = self.decode(self.ids).rstrip("�")
            return self._emit(text[len(self.emitted):]) if text.startswith(self.emitted) else ""
        for t in toks:
            self.pending += self.token_bytes(t) or b""
            self.ends.append(self.released + len(self.pending))
        n = len(self.pending) - (self._hold() if self.stops else 0)
        out = self.dec.decode(bytes(self.pending[:n]))
        del self.pending[:n]
        self.released += n
        return self._emit(out)

    def finish(self, hit=None) -> str:
        """the rest of the text; hit: the row's stop hit (token index, bytes into it, match length, match id) or None"""
        if hit is None:
            if self.decode is not None:
                text = self.decode(self.ids)
                return self._emit(text[len(self.emitted):]) if text.startswith(self.emitted) else ""
            out = self.dec.decode(bytes(self.pending), final=True)
            self.released += len(self.pending)
            self.pending.clear()
            return self._emit(out)
        tok, used, length = int(hit[0]), int(hit[1]), int(hit[2])
        end = (self.ends[tok - 1] if tok > 0 else 0) + used
        cut = end if self.include else max(0, end - length)
        out = self.dec.decode(bytes(self.pending[:max(0, cut - self.released)]), final=True)
        self.pending.clear()
        return self._emit(out)
