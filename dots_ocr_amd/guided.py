"""Guided decoding, host side: a pattern -> a trimmed, minimised DFA over BYTES.

The engine keeps one automaton state per guided row on the device and advances it at every commit (csrc/guided.hip, decode.hip), so all
the host does is compile: ``compile_regex`` / ``compile_choice`` / ``compile_json_schema`` return a ``Guide`` (table uint16 [S][256],
0xFFFF = dead; accepting uint8 [S]; start) that ``Engine.create_guide`` uploads.  Pure Python and numpy: nothing to install.

Regex subset, with the meaning ``re.fullmatch`` gives it on the UTF-8 decoded text: literals, the escapes
``\\d \\w \\s \\n \\t \\r \\\\ \\" \\/ \\. \\[ \\] \\( \\) \\{ \\} \\| \\* \\+ \\? \\- \\^ \\$``, ``.`` (any character but ``\\n``), classes with ranges and
negation, groups ``( )`` and ``(?: )``, alternation, ``* + ? {m} {m,} {m,n}``.  The automaton runs over bytes: a non-ASCII character is
its UTF-8 sequence, and ``.``, ``\\w`` and negated classes accept exactly the well-formed sequences of the characters they cover (never a
surrogate: decoded text holds none).  Anything else — anchors, back-references, look-around, lazy / possessive quantifiers, flags, named
groups, other escapes — raises ValueError naming the construct.

Pipeline: parse -> Thompson NFA over byte ranges -> subset construction -> trim (every state left can reach an accepting one, so on the
device "the walk never met 0xFFFF" is the whole test of a token) -> minimise (Moore, over byte equivalence classes).
"""
from __future__ import annotations

import json
import re as _re
import threading
from bisect import bisect_left
from collections import OrderedDict
from dataclasses import dataclass, field
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np

DEAD = 0xFFFF
MAX_GUIDE_STATES = 4096                       # DOTS_MAX_GUIDE_STATES: 4096 x 512 B = 2 MB of table
_BUILD_LIMIT = 2 * MAX_GUIDE_STATES           # subset construction stops here (a pattern from a client must fail fast, well under a second:
                                              # the construction is pure Python); minimisation rarely halves an automaton this large
_NFA_LIMIT = 100000                           # Thompson states: bounded repetitions are copied out, {m,n} of a large group ends here
MAX_PATTERN_CHARS = 65536                     # compile_request refuses longer regex text (a schema's regex included) before parsing it

_MAX_CP = 0x10FFFF
_SURR = (0xD800, 0xDFFF)


# ------------------------------------------------------------------------------------------------ code point sets
def _norm(ranges: Iterable[Tuple[int, int]]) -> List[Tuple[int, int]]:
    """sorted, merged, without surrogates"""
    out: List[Tuple[int, int]] = []
    for lo, hi in sorted(ranges):
        if lo > hi:
            continue
        if out and lo <= out[-1][1] + 1:
            out[-1] = (out[-1][0], max(out[-1][1], hi))
        else:
            out.append((lo, hi))
    res = []
    for lo, hi in out:                          # cut the surrogate block out
        if hi < _SURR[0] or lo > _SURR[1]:
            res.append((lo, hi))
        else:
            if lo < _SURR[0]:
                res.append((lo, _SURR[0] - 1))
            if hi > _SURR[1]:
                res.append((_SURR[1] + 1, hi))
    return res


def _negate(ranges: List[Tuple[int, int]]) -> List[Tuple[int, int]]:
    out, at = [], 0
    for lo, hi in _norm(ranges):
        if lo > at:
            out.append((at, lo - 1))
        at = hi + 1
    if at <= _MAX_CP:
        out.append((at, _MAX_CP))
    return _norm(out)


_CLASS_CACHE: Dict[str, List[Tuple[int, int]]] = {}


def _escape_class(ch: str) -> List[Tuple[int, int]]:
    """\\d \\w \\s as ``re`` defines them on str (Unicode decimal digits / alphanumerics and '_' / whitespace), computed once"""
    if ch not in _CLASS_CACHE:
        test = {"d": str.isdecimal, "w": lambda c: c.isalnum() or c == "_", "s": str.isspace}[ch]
        ranges, start = [], None
        for cp in range(_MAX_CP + 2):
            ok = cp <= _MAX_CP and not (_SURR[0] <= cp <= _SURR[1]) and test(chr(cp))
            if ok and start is None:
                start = cp
            elif not ok and start is not None:
                ranges.append((start, cp - 1))
                start = None
        _CLASS_CACHE[ch] = _norm(ranges)
    return _CLASS_CACHE[ch]


def _enc(cp: int) -> bytes:
    return chr(cp).encode("utf-8")


def _utf8_sequences(lo: int, hi: int) -> List[List[Tuple[int, int]]]:
    """[lo, hi] (no surrogates inside) -> byte-range sequences whose union is exactly the UTF-8 encodings of its code points"""
    out: List[List[Tuple[int, int]]] = []
    for blo, bhi in ((0, 0x7F), (0x80, 0x7FF), (0x800, 0xFFFF), (0x10000, _MAX_CP)):      # one encoded length at a time
        a, b = max(lo, blo), min(hi, bhi)
        if a <= b:
            _split_same_len(a, b, len(_enc(a)), out)
    return out


def _split_same_len(lo: int, hi: int, n: int, out: list):
    if n == 1:
        out.append([(lo, hi)])
        return
    for i in range(1, n):
        m = (1 << (6 * i)) - 1
        if (lo & ~m) != (hi & ~m):
            if lo & m:
                _split_same_len(lo, lo | m, n, out)
                _split_same_len((lo | m) + 1, hi, n, out)
                return
            if (hi & m) != m:
                _split_same_len(lo, (hi & ~m) - 1, n, out)
                _split_same_len(hi & ~m, hi, n, out)
                return
    out.append(list(zip(_enc(lo), _enc(hi))))


# ------------------------------------------------------------------------------------------------ parser -> AST
# AST: ("set", ranges) | ("cat", [nodes]) | ("alt", [nodes]) | ("rep", node, m, n or None)
_ESC_LITERAL = {"n": "\n", "t": "\t", "r": "\r"}
_ESC_SELF = set('\\"/.[](){}|*+?-^$')


class _Parser:
    def __init__(self, pattern: str):
        self.p = pattern
        self.i = 0

    def fail(self, what: str):
        raise ValueError(f"unsupported regex construct: {what} (at offset {self.i} of {self.p!r})")

    def peek(self) -> str:
        return self.p[self.i] if self.i < len(self.p) else ""

    def parse(self):
        node = self.alt()
        if self.i < len(self.p):
            self.fail("unbalanced ')'")
        return node

    def alt(self):
        branches = [self.cat()]
        while self.peek() == "|":
            self.i += 1
            branches.append(self.cat())
        return branches[0] if len(branches) == 1 else ("alt", branches)

    def cat(self):
        items = []
        while self.i < len(self.p) and self.peek() not in "|)":
            items.append(self.quantified())
        return ("cat", items)

    def quantified(self):
        atom = self.atom()
        c = self.peek()
        if c and c in "*+?{":
            m, n = self.quantifier()
            nxt = self.peek()
            if nxt == "?":
                self.fail("lazy quantifier")
            if nxt == "+":
                self.fail("possessive quantifier")
            if nxt and nxt in "*{":
                self.fail("repeated quantifier")
            return ("rep", atom, m, n)
        return atom

    def quantifier(self):
        c = self.p[self.i]
        self.i += 1
        if c == "*":
            return 0, None
        if c == "+":
            return 1, None
        if c == "?":
            return 0, 1
        j = self.p.find("}", self.i)
        body = self.p[self.i:j] if j >= 0 else ""
        mt = _re.fullmatch(r"(\d*)(,(\d*))?", body)
        if j < 0 or not mt or body in ("", ","):
            self.i -= 1
            self.fail("'{' that is not a repetition count (escape a literal brace)")
        self.i = j + 1
        lo = int(mt.group(1)) if mt.group(1) else 0
        if mt.group(2) is None:
            return lo, lo
        hi = int(mt.group(3)) if mt.group(3) else None
        if hi is not None and hi < lo:
            self.fail("repetition {m,n} with n < m")
        return lo, hi

    def atom(self):
        c = self.p[self.i]
        if c == "(":
            self.i += 1
            if self.peek() == "?":
                nxt = self.p[self.i + 1:self.i + 2]
                if nxt == ":":
                    self.i += 2
                elif nxt in ("=", "!"):
                    self.fail("look-ahead")
                elif nxt == "<" and self.p[self.i + 2:self.i + 3] in ("=", "!"):
                    self.fail("look-behind")
                elif nxt in ("P", "<"):
                    self.fail("named group / named back-reference")
                else:
                    self.fail("inline flags / extension group")
            node = self.alt()
            if self.peek() != ")":
                self.fail("unbalanced '('")
            self.i += 1
            return node
        if c == "[":
            return self.char_class()
        if c == ".":
            self.i += 1
            return ("set", _negate([(10, 10)]))
        if c in "^$":
            self.fail(f"anchor {c!r} (a guide always matches the whole output)")
        if c in "*+?{":
            self.fail(f"quantifier {c!r} with nothing to repeat")
        if c == "\\":
            return ("set", self.escape(in_class=False))
        self.i += 1
        return ("set", [(ord(c), ord(c))])

    def escape(self, in_class: bool) -> List[Tuple[int, int]]:
        c = self.p[self.i + 1:self.i + 2]
        if not c:
            self.fail("trailing backslash")
        if c in "dws":
            self.i += 2
            return _escape_class(c)
        if c in _ESC_LITERAL:
            self.i += 2
            return [(ord(_ESC_LITERAL[c]),) * 2]
        if c in _ESC_SELF:
            self.i += 2
            return [(ord(c), ord(c))]
        if c.isdigit():
            self.fail(f"back-reference or octal escape \\{c}")
        if c in "bBAZ":
            self.fail(f"anchor \\{c}")
        self.fail(f"escape \\{c}")

    def char_class(self):
        self.i += 1
        neg = self.peek() == "^"
        if neg:
            self.i += 1
        ranges: List[Tuple[int, int]] = []
        first = True
        while True:
            c = self.peek()
            if not c:
                self.fail("unterminated character class")
            if c == "]" and not first:
                self.i += 1
                break
            first = False
            if c == "\\":
                lo_set = self.escape(in_class=True)
                single = len(lo_set) == 1 and lo_set[0][0] == lo_set[0][1]
            else:
                self.i += 1
                lo_set, single = [(ord(c), ord(c))], True
            if self.peek() == "-" and self.p[self.i + 1:self.i + 2] not in ("]", ""):
                if not single:
                    self.fail("range that starts at a class escape")
                self.i += 1
                d = self.peek()
                if d == "\\":
                    hi_set = self.escape(in_class=True)
                    if not (len(hi_set) == 1 and hi_set[0][0] == hi_set[0][1]):
                        self.fail("range that ends at a class escape")
                    hi = hi_set[0][0]
                else:
                    self.i += 1
                    hi = ord(d)
                if hi < lo_set[0][0]:
                    self.fail("reversed character range")
                ranges.append((lo_set[0][0], hi))
            else:
                ranges.extend(lo_set)
        ranges = _norm(ranges)
        return ("set", _negate(ranges) if neg else ranges)


# ------------------------------------------------------------------------------------------------ NFA
class _NFA:
    def __init__(self):
        self.eps: List[List[int]] = []
        self.edges: List[List[Tuple[int, int, int]]] = []          # (byte lo, byte hi, target)

    def new(self) -> int:
        self.eps.append([])
        self.edges.append([])
        if len(self.eps) > _NFA_LIMIT:
            raise ValueError(f"the pattern needs more than {MAX_GUIDE_STATES} automaton states (DOTS_MAX_GUIDE_STATES)")
        return len(self.eps) - 1

    def build(self, node) -> Tuple[int, int]:
        kind = node[0]
        if kind == "set":
            a, b = self.new(), self.new()
            for lo, hi in node[1]:
                for seq in _utf8_sequences(lo, hi):
                    cur = a
                    for k, (blo, bhi) in enumerate(seq):
                        nxt = b if k == len(seq) - 1 else self.new()
                        self.edges[cur].append((blo, bhi, nxt))
                        cur = nxt
            return a, b
        if kind == "cat":
            a = self.new()
            cur = a
            for sub in node[1]:
                s, t = self.build(sub)
                self.eps[cur].append(s)
                cur = t
            return a, cur
        if kind == "alt":
            a, b = self.new(), self.new()
            for sub in node[1]:
                s, t = self.build(sub)
                self.eps[a].append(s)
                self.eps[t].append(b)
            return a, b
        _, sub, m, n = node
        a = self.new()
        cur = a
        for _ in range(m):
            s, t = self.build(sub)
            self.eps[cur].append(s)
            cur = t
        if n is None:                           # sub*
            s, t = self.build(sub)
            loop, out = self.new(), self.new()
            self.eps[cur].append(loop)
            self.eps[loop] += [s, out]
            self.eps[t].append(loop)
            return a, out
        out = self.new()
        self.eps[cur].append(out)
        for _ in range(n - m):                  # (sub(sub(...)?)?)?
            s, t = self.build(sub)
            self.eps[cur].append(s)
            self.eps[t].append(out)
            cur = t
        return a, out


def _closure(nfa: _NFA, states: Iterable[int]) -> frozenset:
    seen = set(states)
    stack = list(seen)
    while stack:
        for t in nfa.eps[stack.pop()]:
            if t not in seen:
                seen.add(t)
                stack.append(t)
    return frozenset(seen)


def _determinise(nfa: _NFA, start: int, accept: int) -> Tuple[np.ndarray, np.ndarray]:
    d0 = _closure(nfa, [start])
    index = {d0: 0}
    order = [d0]
    rows: List[np.ndarray] = []
    closures: Dict[frozenset, frozenset] = {}
    k = 0
    while k < len(order):
        cur = order[k]
        k += 1
        row = np.full(256, -1, np.int64)
        edges = [e for s in cur for e in nfa.edges[s]]
        if edges:
            cuts = sorted({lo for lo, _, _ in edges} | {hi + 1 for _, hi, _ in edges})
            sets = [set() for _ in cuts]
            for elo, ehi, t in edges:                # every edge starts and ends at a cut
                for q in range(bisect_left(cuts, elo), bisect_left(cuts, ehi + 1)):
                    sets[q].add(t)
            for lo, nxt, tgt in zip(cuts, cuts[1:] + [256], sets):
                if not tgt:
                    continue
                key = frozenset(tgt)
                d = closures.get(key)
                if d is None:
                    d = closures[key] = _closure(nfa, key)
                j = index.get(d)
                if j is None:
                    j = index[d] = len(order)
                    order.append(d)
                    if j >= _BUILD_LIMIT:
                        raise ValueError(f"the pattern needs more than {MAX_GUIDE_STATES} automaton states (DOTS_MAX_GUIDE_STATES)")
                row[lo:nxt] = j
        rows.append(row)
    table = np.stack(rows)
    acc = np.array([accept in d for d in order], bool)
    return table, acc


def _trim(table: np.ndarray, acc: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """keep the states that can reach an accepting one (all are reachable from state 0 by construction); -1 = dead"""
    S = table.shape[0]
    live = acc.copy()
    while True:
        reach = np.concatenate([live, [False]])[table].any(axis=1) | live        # table -1 indexes the appended False
        if (reach == live).all():
            break
        live = reach
    if not live[0]:
        raise ValueError("the pattern matches nothing (empty language)")
    new = np.full(S + 1, -1, np.int64)
    new[:S][live] = np.arange(int(live.sum()))
    return new[table[live]], acc[live]


def _minimise(table: np.ndarray, acc: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    S = table.shape[0]
    cols, col_of = np.unique(table.T, axis=0, return_inverse=True)                # byte equivalence classes
    t = cols.T                                                                    # [S][K]
    cls = acc.astype(np.int64)
    n_cls = len(np.unique(cls))
    while True:
        ext = np.concatenate([cls, [-1]])                                        # dead target -> class -1
        sig = np.concatenate([cls[:, None], ext[t]], axis=1)
        _, cls_new = np.unique(sig, axis=0, return_inverse=True)
        cls_new = cls_new.reshape(-1)
        n_new = int(cls_new.max()) + 1
        cls = cls_new
        if n_new == n_cls:
            break
        n_cls = n_new
    # renumber in BFS order from the start state's class, so that equal languages give equal tables
    rep = np.zeros(n_cls, np.int64)
    rep[cls[::-1]] = np.arange(S)[::-1]
    order, seen = [int(cls[0])], {int(cls[0])}
    k = 0
    tt = table
    while k < len(order):
        row = tt[rep[order[k]]]
        k += 1
        for tgt in row[np.sort(np.unique(row, return_index=True)[1])]:
            if tgt >= 0 and int(cls[tgt]) not in seen:
                seen.add(int(cls[tgt]))
                order.append(int(cls[tgt]))
    pos = np.full(n_cls + 1, -1, np.int64)
    pos[order] = np.arange(len(order))
    reps = rep[order]
    ext = np.concatenate([cls, [n_cls]])
    return pos[ext[table[reps]]], acc[reps]


# ------------------------------------------------------------------------------------------------ Guide
class TokenBytes:
    """The packed byte image of a vocabulary: offsets int32 [V + 1], data uint8.  An entry without bytes is unguidable (never allowed on a
    guided row); ``special`` ids are given none."""

    def __init__(self, tokens: Sequence[bytes], special: Iterable[int] = ()):
        special = set(int(t) for t in special)
        toks = [b"" if i in special else bytes(t) for i, t in enumerate(tokens)]
        lens = np.fromiter((len(t) for t in toks), np.int64, len(toks))
        if int(lens.sum()) >= 2 ** 31:
            raise ValueError("token bytes exceed 2 GiB")
        self.offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
        self.data = np.frombuffer(b"".join(toks), np.uint8).copy()

    @property
    def vocab_size(self) -> int:
        return int(self.offsets.shape[0] - 1)

    def token(self, t: int) -> bytes:
        return self.data[self.offsets[t]:self.offsets[t + 1]].tobytes()


@dataclass
class Guide:
    table: np.ndarray                            # uint16 [S][256], DEAD = no transition
    accepting: np.ndarray                        # uint8 [S]
    start: int
    pattern: str
    _dist: Optional[np.ndarray] = field(default=None, repr=False, compare=False)

    @property
    def n_states(self) -> int:
        return int(self.table.shape[0])

    def walk(self, state: int, data: bytes) -> int:
        """the state after `data` from `state`; DEAD once a byte has no transition (and from DEAD)"""
        s = int(state)
        for b in bytes(data):
            if s == DEAD:
                break
            s = int(self.table[s, b])
        return s

    def draft_states(self, state: int, drafts: Sequence[int], tokens: "TokenBytes", eos_ids: Iterable[int] = ()) -> List[int]:
        """The state each draft row of a speculating step is selected under (what spec_guide_chain_kernel computes): entry j
        is `state` walked over the bytes of drafts[0 .. j], or -1 from the first draft on that the guide could not have committed at its
        position: one without bytes, an EOS id (it finishes the row and is not walked) or one whose walk meets DEAD."""
        eos = set(int(t) for t in eos_ids)
        out, s = [], int(state)
        for t in drafts:
            data = tokens.token(int(t)) if s >= 0 else b""
            s = -1 if s < 0 or not data or int(t) in eos else self.walk(s, data)
            s = -1 if s == DEAD else s
            out.append(s)
        return out

    def matches(self, data: bytes) -> bool:
        s = self.walk(self.start, data)
        return s != DEAD and bool(self.accepting[s])

    def mask(self, state: int, tokens: TokenBytes) -> np.ndarray:
        """bool [V]: token t has bytes and walking them from `state` never meets DEAD (what guide_mask_kernel computes)"""
        off, data = tokens.offsets.astype(np.int64), tokens.data
        lens = off[1:] - off[:-1]
        ext = np.vstack([self.table.astype(np.int64), np.full((1, 256), DEAD, np.int64)])      # row S: DEAD stays DEAD
        S = self.n_states
        cur = np.full(lens.shape, int(state) if int(state) != DEAD else S, np.int64)
        for j in range(int(lens.max()) if lens.size else 0):
            on = np.nonzero(lens > j)[0]
            nxt = ext[cur[on], data[off[on] + j]]
            cur[on] = np.where(nxt == DEAD, S, nxt)
        return (lens > 0) & (cur != S)

    def distance(self) -> np.ndarray:
        """int [S]: bytes on the shortest way from each state to an accepting one"""
        if self._dist is None:
            S = self.n_states
            dist = np.where(self.accepting != 0, 0, 1 << 30).astype(np.int64)
            ext_t = np.where(self.table == DEAD, S, self.table).astype(np.int64)
            while True:
                ext = np.concatenate([dist, [1 << 30]])
                new = np.minimum(dist, ext[ext_t].min(axis=1) + 1)
                if (new == dist).all():
                    break
                dist = new
            self._dist = dist
        return self._dist

    @property
    def min_length(self) -> int:
        """bytes of the shortest match"""
        return int(self.distance()[self.start])

    def sample(self, rng: np.random.Generator, soft_len: int = 24, p_stop: float = 0.3) -> bytes:
        """a random member of the language: a random walk that stops at accepting states with probability p_stop and heads for the nearest
        accepting state once it is soft_len bytes long"""
        dist = self.distance()
        s, out = self.start, bytearray()
        while True:
            if self.accepting[s] and (rng.random() < p_stop or len(out) >= soft_len or not (self.table[s] != DEAD).any()):
                return bytes(out)
            row = self.table[s]
            nxt = np.nonzero(row != DEAD)[0]
            if len(out) >= soft_len:
                d = dist[row[nxt]]
                nxt = nxt[d == d.min()]
            b = int(nxt[rng.integers(len(nxt))])
            out.append(b)
            s = int(row[b])


def _compile_ast(ast, pattern: str) -> Guide:
    nfa = _NFA()
    a, b = nfa.build(ast)
    table, acc = _determinise(nfa, a, b)
    table, acc = _trim(table, acc)
    table, acc = _minimise(table, acc)
    if table.shape[0] > MAX_GUIDE_STATES:
        raise ValueError(f"the pattern needs {table.shape[0]} automaton states, more than {MAX_GUIDE_STATES} (DOTS_MAX_GUIDE_STATES)")
    t16 = np.where(table < 0, DEAD, table).astype(np.uint16)
    return Guide(np.ascontiguousarray(t16), np.ascontiguousarray(acc.astype(np.uint8)), 0, pattern)


def compile_regex(pattern: str) -> Guide:
    if not isinstance(pattern, str):
        raise ValueError("a guide's pattern must be a string")
    return _compile_ast(_Parser(pattern).parse(), pattern)


_SPECIAL = set('\\.[](){}|*+?^$-"/')


def escape(text: str) -> str:
    """`text` as a literal of the regex subset"""
    out = []
    for c in text:
        if c in _SPECIAL:
            out.append("\\" + c)
        elif c in "\n\t\r":
            out.append({"\n": "\\n", "\t": "\\t", "\r": "\\r"}[c])
        else:
            out.append(c)
    return "".join(out)


def choice_regex(choices: Sequence[str]) -> str:
    """the alternation of the escaped literals"""
    if isinstance(choices, (str, bytes)) or not isinstance(choices, (list, tuple)):
        raise ValueError("guided_choice must be a list of strings")
    choices = list(choices)
    if not choices:
        raise ValueError("guided_choice needs at least one string")
    if any(not isinstance(c, str) for c in choices):
        raise ValueError("guided_choice must hold strings")
    if len(set(choices)) != len(choices):
        raise ValueError("guided_choice holds a string twice")
    return "|".join(escape(c) for c in choices)


def compile_choice(choices: Sequence[str]) -> Guide:
    return compile_regex(choice_regex(choices))


# ------------------------------------------------------------------------------------------------ JSON schema -> regex
DEFAULT_WHITESPACE = r"[ \n\t]*"
_STRING_CHAR = r'(?:[^"\\\x00-\x1f]|\\["\\/bfnrt]|\\u[0-9a-fA-F]{4})'.replace("\\x00", "\x00").replace("\\x1f", "\x1f")
_INTEGER = r"-?(?:0|[1-9][0-9]*)"
_NUMBER = _INTEGER + r"(?:\.[0-9]+)?(?:[eE][+\-]?[0-9]+)?"
_IGNORED = {"title", "description", "default", "examples", "$schema", "$id", "$comment", "additionalProperties"}
_KNOWN = {"type", "properties", "required", "items", "minItems", "maxItems", "enum", "const", "minLength", "maxLength", "pattern", "anyOf"}


def _count(schema: dict, key: str, default):
    v = schema.get(key, default)
    if v is None:
        return None
    if isinstance(v, bool) or not isinstance(v, int) or v < 0:
        raise ValueError(f"schema keyword {key!r} must be an integer >= 0, got {v!r}")
    return v


def _scalar_literal(v) -> str:
    if isinstance(v, (dict, list)):
        raise ValueError("schema keyword 'enum' / 'const' supports scalars only")
    return escape(json.dumps(v, ensure_ascii=False))


def schema_to_regex(schema, whitespace: str = DEFAULT_WHITESPACE) -> str:
    """A non-recursive subset of JSON Schema as a regex of the subset above.  object: `properties` in declared order, all required unless
    `required` names a prefix of them (the rest are optional trailing properties, each present only
    after the ones before it); additionalProperties is ignored (nothing undeclared is ever emitted); array: items / minItems / maxItems; string:
    enum / minLength / maxLength / pattern; integer, number, boolean, null; enum / const of scalars; anyOf; a list of types.  Anything
    else raises ValueError naming the keyword."""
    if isinstance(schema, str):
        try:
            schema = json.loads(schema)
        except json.JSONDecodeError as e:
            raise ValueError(f"guided_json is not valid JSON: {e}")
    if not isinstance(schema, dict):
        raise ValueError("a JSON schema must be an object")
    _Parser(whitespace).parse()                                                  # the caller's whitespace pattern must be in the subset
    ws = f"(?:{whitespace})"
    return _schema(schema, ws)


def _schema(s: dict, ws: str) -> str:
    if not isinstance(s, dict):
        raise ValueError(f"a sub-schema must be an object, got {s!r}")
    for k in s:
        if k not in _KNOWN and k not in _IGNORED:
            raise ValueError(f"unsupported schema keyword {k!r}")
    if "anyOf" in s:
        if not isinstance(s["anyOf"], list) or not s["anyOf"]:
            raise ValueError("schema keyword 'anyOf' must be a non-empty list")
        return "(?:" + "|".join(_schema(x, ws) for x in s["anyOf"]) + ")"
    if "const" in s:
        return _scalar_literal(s["const"])
    if "enum" in s:
        if not isinstance(s["enum"], list) or not s["enum"]:
            raise ValueError("schema keyword 'enum' must be a non-empty list")
        return "(?:" + "|".join(_scalar_literal(v) for v in s["enum"]) + ")"
    t = s.get("type")
    if isinstance(t, list):
        if not t:
            raise ValueError("schema keyword 'type' must not be an empty list")
        return "(?:" + "|".join(_schema({**s, "type": x}, ws) for x in t) + ")"
    if t == "string":
        if "pattern" in s:
            pat = s["pattern"]
            if not isinstance(pat, str):
                raise ValueError("schema keyword 'pattern' must be a string")
            pat = pat[1:] if pat.startswith("^") else pat
            pat = pat[:-1] if pat.endswith("$") and not pat.endswith("\\$") else pat
            return f'"(?:{pat})"'
        lo, hi = _count(s, "minLength", 0), _count(s, "maxLength", None)
        if hi is not None and hi < lo:
            raise ValueError("schema: maxLength < minLength")
        q = "*" if (lo, hi) == (0, None) else "{%d,%s}" % (lo, "" if hi is None else hi)
        return f'"{_STRING_CHAR}{q}"'
    if t == "integer":
        return _INTEGER
    if t == "number":
        return _NUMBER
    if t == "boolean":
        return "(?:true|false)"
    if t == "null":
        return "null"
    if t == "array":
        if "items" not in s or not isinstance(s["items"], dict):
            raise ValueError("schema: an array needs 'items' (free-form items are recursive)")
        item = _schema(s["items"], ws)
        lo, hi = _count(s, "minItems", 0), _count(s, "maxItems", None)
        if hi is not None and hi < lo:
            raise ValueError("schema: maxItems < minItems")
        if hi == 0:
            return rf"\[{ws}\]"
        more = "{%d,%s}" % (max(lo - 1, 0), "" if hi is None else hi - 1)
        body = f"{item}(?:{ws},{ws}{item}){more}"
        return rf"\[{ws}{body}{ws}\]" if lo > 0 else rf"\[{ws}(?:{body}{ws})?\]"
    if t == "object":
        props = s.get("properties")
        if not isinstance(props, dict):
            raise ValueError("schema: an object needs 'properties' (free-form JSON is recursive; give a schema)")
        names = list(props)
        req = s.get("required", names)
        if not isinstance(req, list) or any(r not in props for r in req):
            raise ValueError("schema keyword 'required' must list declared properties")
        n_req = len(set(req))
        if set(names[:n_req]) != set(req):
            raise ValueError("schema keyword 'required': optional properties are supported only after all required ones, in declared order")
        parts = [f'"{escape(json.dumps(k, ensure_ascii=False)[1:-1])}"{ws}:{ws}{_schema(props[k], ws)}' for k in names]
        if not parts:
            return rf"\{{{ws}\}}"
        tail = ""
        for k in range(len(parts) - 1, n_req - 1, -1):                          # optional trailing properties, innermost last
            sep = f"{ws},{ws}" if k > 0 else ""
            tail = f"(?:{sep}{parts[k]}{tail})?"
        head = f"{ws},{ws}".join(parts[:n_req])
        return rf"\{{{ws}{head}{tail}{ws}\}}"
    if t is None:
        raise ValueError("schema: a sub-schema without 'type' accepts any JSON (free-form JSON is recursive; give a schema)")
    raise ValueError(f"unsupported schema type {t!r}")


def compile_json_schema(schema, whitespace: str = DEFAULT_WHITESPACE) -> Guide:
    return compile_regex(schema_to_regex(schema, whitespace))


# Compiled guides by pattern text, for callers that see the same pattern again and again (the server: every page of a document posts the
# same guided_layout).  The key is the regex text — for a schema the output of schema_to_regex, which costs microseconds — so equal
# requests meet in one entry however they were spelled.  A Guide is never modified after it is built.
GUIDE_CACHE_SIZE = 64
_guide_cache: "OrderedDict[str, Guide]" = OrderedDict()
_guide_cache_lock = threading.Lock()


def compile_cached(pattern: str) -> Guide:
    """compile_regex through an LRU of GUIDE_CACHE_SIZE compiled guides keyed by the pattern text (thread-safe)"""
    if not isinstance(pattern, str):
        raise ValueError("a guide's pattern must be a string")
    if len(pattern) > MAX_PATTERN_CHARS:
        raise ValueError(f"the guide's pattern is {len(pattern)} characters long, more than {MAX_PATTERN_CHARS}")
    with _guide_cache_lock:
        g = _guide_cache.get(pattern)
        if g is not None:
            _guide_cache.move_to_end(pattern)
            return g
    g = compile_regex(pattern)                               # outside the lock: two first requests may both compile, one entry stays
    with _guide_cache_lock:
        g = _guide_cache.setdefault(pattern, g)
        _guide_cache.move_to_end(pattern)
        while len(_guide_cache) > GUIDE_CACHE_SIZE:
            _guide_cache.popitem(last=False)
    return g


def compile_request(guided_regex=None, guided_choice=None, guided_json=None, guided_layout=False,
                    whitespace: Optional[str] = None) -> Optional[Guide]:
    """The guide of one request from vLLM's fields (at most one of them, else ValueError); None when none is given.  Compiled guides are
    cached by pattern text (compile_cached): a request that repeats an earlier one compiles nothing.  `whitespace` belongs to the JSON
    fields; with guided_regex or guided_choice it is refused, not ignored."""
    given = [k for k, v in (("guided_regex", guided_regex), ("guided_choice", guided_choice), ("guided_json", guided_json)) if v is not None]
    if guided_layout:
        given.append("guided_layout")
    if len(given) > 1:
        raise ValueError(f"at most one of the guided decoding fields may be given, got {', '.join(given)}")
    if not given:
        if whitespace is not None:
            raise ValueError("guided_whitespace_pattern needs guided_json, guided_layout or a json_schema response_format")
        return None
    ws = DEFAULT_WHITESPACE if whitespace is None else whitespace
    if not isinstance(ws, str):
        raise ValueError("guided_whitespace_pattern must be a string")
    if whitespace is not None and (guided_regex is not None or guided_choice is not None):
        raise ValueError(f"guided_whitespace_pattern needs guided_json, guided_layout or a json_schema response_format, not {given[0]}")
    if guided_regex is not None:
        return compile_cached(guided_regex)
    if guided_choice is not None:
        return compile_cached(choice_regex(guided_choice))
    if guided_json is not None:
        return compile_cached(schema_to_regex(guided_json, ws))
    return compile_cached(_layout_regex(ws))


_layout_regex_cache: Dict[str, str] = {}


def _layout_regex(ws: str) -> str:
    """schema_to_regex(layout_schema(), ws), built once per whitespace pattern"""
    if ws not in _layout_regex_cache:
        if len(_layout_regex_cache) >= GUIDE_CACHE_SIZE:
            _layout_regex_cache.clear()
        _layout_regex_cache[ws] = schema_to_regex(layout_schema(), ws)
    return _layout_regex_cache[ws]


def layout_categories() -> Tuple[str, ...]:
    """the categories of the layout prompts (the overlay table's, without its two fall-backs)"""
    from .layout_utils import dict_layout_type_to_color
    return tuple(sorted(k for k in dict_layout_type_to_color if k not in ("Other", "Unknown")))


def layout_schema(categories: Optional[Sequence[str]] = None) -> dict:
    """The layout prompts' output: an array of {"bbox": [x1, y1, x2, y2], "category": <one of the list>, "text": <string>}, `text` optional
    (a Picture carries none; the layout-only prompt asks for none)."""
    cats = list(layout_categories() if categories is None else categories)
    if not cats:
        raise ValueError("layout_schema needs at least one category")
    return {"type": "array", "items": {
        "type": "object",
        "properties": {"bbox": {"type": "array", "items": {"type": "integer"}, "minItems": 4, "maxItems": 4},
                       "category": {"enum": cats},
                       "text": {"type": "string"}},
        "required": ["bbox", "category"]}}
