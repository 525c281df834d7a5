"""Stop strings: the host compiler of the automaton the engine walks, and the rule itself restated in plain Python.

The rule, the same on the GPU (csrc/step_dev.h stop_walk) and here:

  * a row's output is scanned as a byte stream, the concatenated token bytes of the tokens it generated; the prompt is not part of it, and
    a token without bytes (a special) contributes nothing and leaves the state alone;
  * the row stops at the first byte at which any listed string ends;
  * if several strings end at that byte the longest one is the match (it has the earliest start);
  * while the index of the token that holds the byte is below ``min_tokens`` the scan goes on but no match is taken, so a string that
    straddles the boundary is still found (vLLM does not check stop strings below min_tokens either).

``compile_stop`` builds the Aho-Corasick automaton of the strings and folds its failure links into a dense byte DFA: every transition is
defined, there is no dead state, and one table read per byte is the whole walk.  ``first_stop`` states the rule with ``bytes.find`` and
shares nothing with the automaton; the tests hold the two (and the device) against each other.
"""
from __future__ import annotations

from collections import deque
from dataclasses import dataclass
from typing import Iterable, Optional, Sequence, Tuple

import numpy as np

from .engine import MAX_STOP_BYTES, MAX_STOP_STRINGS      # the limits live beside MAX_STOP_IDS

MAX_STOP_STATES = MAX_STOP_STRINGS * MAX_STOP_BYTES + 1


def check_stop_strings(strings) -> Tuple[str, ...]:
    """1 .. MAX_STOP_STRINGS non-empty str of at most MAX_STOP_BYTES UTF-8 bytes each -> the tuple without duplicates, order kept
    (ValueError otherwise).  A single str is a list of one."""
    if isinstance(strings, str):
        strings = (strings,)
    try:
        strings = tuple(strings)
    except TypeError:
        raise ValueError("stop must be a string or a list of strings")
    out = []
    for s in strings:
        if not isinstance(s, str):
            raise ValueError(f"a stop string must be a str, got {type(s).__name__}")
        if not s:
            raise ValueError("a stop string must not be empty")
        if len(s.encode("utf-8")) > MAX_STOP_BYTES:
            raise ValueError(f"a stop string is at most {MAX_STOP_BYTES} UTF-8 bytes, got {len(s.encode('utf-8'))}")
        if s not in out:
            out.append(s)
    if not out:
        raise ValueError("stop needs at least one string")
    if len(out) > MAX_STOP_STRINGS:
        raise ValueError(f"at most {MAX_STOP_STRINGS} stop strings, got {len(out)}")
    return tuple(out)


@dataclass
class StopAutomaton:
    strings: Tuple[str, ...]                 # the caller's list without duplicates: match_id indexes it
    table: np.ndarray                        # uint16 [S][256]: every entry < S, state 0 is the root
    match_len: np.ndarray                    # uint16 [S]: bytes of the longest listed string that ends at the state, 0 = none
    match_id: np.ndarray                     # uint8 [S]: its index in `strings` (0 where match_len is 0)

    @property
    def n_states(self) -> int:
        return int(self.table.shape[0])

    def walk(self, chunks: Iterable[bytes], min_tokens: int = 0) -> Optional[Tuple[int, int, int, int]]:
        """The device's walk, token by token: (token index, bytes of that token consumed including the matching byte, match length, match
        id) of the first hit, or None."""
        s = 0
        for n, chunk in enumerate(chunks):
            for j, b in enumerate(bytes(chunk)):
                s = int(self.table[s, b])
                if self.match_len[s] and n >= min_tokens:
                    return n, j + 1, int(self.match_len[s]), int(self.match_id[s])
        return None


def compile_stop(strings) -> StopAutomaton:
    """The Aho-Corasick automaton of the strings as a dense byte DFA (ValueError on bad input: check_stop_strings)."""
    strings = check_stop_strings(strings)
    pats = [s.encode("utf-8") for s in strings]
    goto = [dict()]                          # the trie
    ends = [(0, 0)]                          # (length, id) of the string that ends exactly at the state
    for i, p in enumerate(pats):
        s = 0
        for b in p:
            nxt = goto[s].get(b)
            if nxt is None:
                nxt = len(goto)
                goto[s][b] = nxt
                goto.append(dict())
                ends.append((0, 0))
            s = nxt
        ends[s] = (len(p), i)                # no duplicates: one string per end state
    S = len(goto)
    table = np.zeros((S, 256), dtype=np.uint16)
    fail = [0] * S
    best = list(ends)                        # the longest listed string that is a suffix of the state's path
    q = deque()
    for b, s in goto[0].items():
        table[0, b] = s
        q.append(s)
    while q:                                 # breadth first: a state's failure state is shallower, its row is already complete
        s = q.popleft()
        f = fail[s]
        if not best[s][0]:
            best[s] = best[f]                # the state's own string, when it has one, is the longest: it is the whole path
        table[s] = table[f]
        for b, t in goto[s].items():
            fail[t] = int(table[f, b])
            table[s, b] = t
            q.append(t)
    return StopAutomaton(strings, table, np.asarray([l for l, _ in best], dtype=np.uint16), np.asarray([i for _, i in best], dtype=np.uint8))


def first_stop(byte_chunks: Sequence[bytes], strings, min_tokens: int = 0) -> Optional[Tuple[int, int, int, int]]:
    """The rule restated without the automaton: (token_index, bytes_into_token, match_len, match_id) of the first stop in the stream
    b"".join(byte_chunks), or None.  Per string, every occurrence is found with bytes.find; an occurrence counts when the token that
    holds its last byte has index >= min_tokens; the earliest end wins, then the longest string."""
    strings = check_stop_strings(strings)
    chunks = [bytes(c) for c in byte_chunks]
    data = b"".join(chunks)
    owner = []                               # byte position -> (token index, bytes into that token)
    for n, c in enumerate(chunks):
        owner += [(n, j + 1) for j in range(len(c))]
    found = None                             # (end position, -length, id)
    for i, s in enumerate(strings):
        p = s.encode("utf-8")
        at = data.find(p)
        while at >= 0:
            end = at + len(p) - 1
            if owner[end][0] >= min_tokens:
                if found is None or (end, -len(p)) < found[:2]:
                    found = (end, -len(p), i)
                break                        # later occurrences of this string end later
            at = data.find(p, at + 1)
    if found is None:
        return None
    end, neg, i = found
    return owner[end][0], owner[end][1], -neg, i


def cut_text(token_bytes: Sequence[bytes], hit, include_stop_str: bool = False) -> bytes:
    """The bytes of a stopped output: everything before the byte where the match starts, or through the byte where it ends with
    include_stop_str.  token_bytes: the bytes of the generated tokens through the hit token; hit as first_stop returns it."""
    tok, used, length, _ = hit
    end = sum(len(bytes(c)) for c in token_bytes[:tok]) + used
    data = b"".join(bytes(c) for c in token_bytes[:tok + 1])
    return data[:end] if include_stop_str else data[:max(0, end - length)]


def stopped_text(token_ids: Sequence[int], hit, token_bytes, include_stop_str: bool = False) -> str:
    """The text of an output that ended at a stop string.  token_ids: the generated ids (at least through the hit token); hit: (token
    index, bytes into it, match length, match id); token_bytes: id -> bytes, the table the match was found over.  A cut in the middle of
    a multi-byte character is decoded with errors="replace"."""
    chunks = [token_bytes(int(t)) for t in list(token_ids)[:int(hit[0]) + 1]]
    return cut_text(chunks, hit, include_stop_str).decode("utf-8", errors="replace")
