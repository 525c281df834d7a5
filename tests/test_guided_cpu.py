"""Guided decoding, host side: the pattern -> byte DFA compiler against Python's `re`, the JSON-schema subset against
json.loads and a hand-written checker, Guide.mask against a brute-force walk, the scheduler / server plumbing through fakes, and the new
symbols of the C ABI.  No GPU."""
import json
import re
import time
from pathlib import Path

import numpy as np
import pytest

from dots_ocr_amd import guided as G
from dots_ocr_amd.config import DotsConfig
from dots_ocr_amd.row_features import rows_holding

GOLDEN = Path(__file__).parent / "golden"

# every supported construct: literals and escapes, '.', classes (ranges, negation, escapes inside), groups, alternation, all quantifiers,
# non-ASCII literals, a negated class beside multi-byte text, bounded repetition
PATTERNS = [
    r"abc",
    r"a|bc|def",
    r"(ab|cd)*e",
    r"(?:ab)+c?",
    r"a{3}b{2,}c{1,3}d{,2}",
    r"[a-f0-9]+",
    r"[^a-c]x",
    r"[^\"\\]*é[^é]{1,3}",
    r"日本(語|ご)?[^日本]{2,4}",
    r".{2,5}",
    r"a.c\.",
    r"\d+(\.\d+)?",
    r"\w+\s\w*",
    r"[\w\-]{2,6}@[\d.]+",
    r"\n\t\r\\\"\/",
    r"\[\]\(\)\{\}\|\*\+\?\-\^\$",
    r"[]a]+[a\]]",
    r"[a\-z]+-?",
    r"(a|b|)(c|)d",
    r"x(|y)z",
    r"(a(b(c|d)*)?)+",
    r"\{\"k\": (true|false|null)\}",
    r"[€-₿]{1,2}|[܀-ऀ]",
    r"[^\x00-\x7f]{1,2}".replace("\\x00", "\x00").replace("\\x7f", "\x7f"),
    r"😀+[^😀]",
]


def _mutate(rng, data: bytes) -> bytes:
    b = bytearray(data)
    kind = int(rng.integers(0, 3)) if b else 1
    at = int(rng.integers(0, len(b) + (kind == 1)))
    if kind == 0:
        b[at] = int(rng.integers(0, 256))
    elif kind == 1:
        b.insert(at, int(rng.integers(0, 256)))
    else:
        del b[at]
    return bytes(b)


def _re_accepts(pattern: str, data: bytes) -> bool:
    try:
        text = data.decode("utf-8")
    except UnicodeDecodeError:
        return False                                         # not text at all: nothing `re` could match
    return re.fullmatch(pattern, text) is not None


@pytest.mark.parametrize("pattern", PATTERNS)
def test_compiler_agrees_with_re_fullmatch(pattern):
    g = G.compile_regex(pattern)
    rng = np.random.default_rng(len(pattern) * 7919 + PATTERNS.index(pattern))
    members = [g.sample(rng, soft_len=int(rng.integers(4, 40))) for _ in range(60)]
    strings = list(members)
    for m in members[:50]:
        strings.append(_mutate(rng, m))
    strings += [b"", b"\xff", b"a", "é".encode()[:1]]
    yes = no = 0
    for s in strings:
        want = _re_accepts(pattern, s)
        assert g.matches(s) == want, (pattern, s)
        yes, no = yes + want, no + (not want)
    assert all(_re_accepts(pattern, m) for m in members)     # what the DFA generates, `re` accepts
    assert yes >= len(strings) // 2 and no >= 5, (pattern, yes, no)


@pytest.mark.parametrize("pattern", PATTERNS + [G.schema_to_regex(G.layout_schema())])
def test_every_state_reaches_an_accepting_one(pattern):
    g = G.compile_regex(pattern)
    assert g.table.dtype == np.uint16 and g.table.shape == (g.n_states, 256) and g.accepting.dtype == np.uint8
    assert g.n_states <= G.MAX_GUIDE_STATES and 0 <= g.start < g.n_states
    live = g.accepting != 0
    while True:
        nxt = live | np.concatenate([live, [False]])[np.where(g.table == G.DEAD, g.n_states, g.table)].any(axis=1)
        if (nxt == live).all():
            break
        live = nxt
    assert live.all()
    assert (g.distance() < (1 << 30)).all() and g.min_length == len(min((g.sample(np.random.default_rng(k), 0, 1.0) for k in range(40)), key=len))


def test_minimised_equal_languages_give_equal_tables():
    a, b = G.compile_regex(r"(a|b)*abb"), G.compile_regex(r"(a|b)*a(b)(b)|(b|a)*abb")
    assert a.n_states == 4 and np.array_equal(a.table, b.table) and np.array_equal(a.accepting, b.accepting)
    assert G.compile_choice(["yes", "no", "maybe"]).n_states == G.compile_regex("yes|no|maybe").n_states


@pytest.mark.parametrize("bad,word", [(r"^a", "anchor"), (r"a$", "anchor"), (r"\bword", "anchor"), (r"(a)\1", "back-reference"),
                                      (r"(?=a)b", "look-ahead"), (r"(?!a)b", "look-ahead"), (r"(?<=a)b", "look-behind"), (r"(?<!a)b", "look-behind"),
                                      (r"a*?", "lazy"), (r"a+?", "lazy"), (r"a{2,3}?", "lazy"), (r"a*+", "possessive"), (r"a++", "possessive"),
                                      (r"(?i)abc", "flags"), (r"(?P<n>a)", "named group"), (r"\D", "escape"), (r"\pL", "escape"),
                                      (r"a{", "'{'"), (r"*a", "nothing to repeat"), (r"(a", "unbalanced"), (r"a)", "unbalanced"),
                                      (r"[a", "unterminated"), (r"[z-a]", "reversed"), (r"a{3,2}", "n < m"), (r"a**", "repeated")])
def test_unsupported_constructs_raise_naming_the_construct(bad, word):
    with pytest.raises(ValueError) as ei:
        G.compile_regex(bad)
    assert word in str(ei.value), str(ei.value)


def test_state_limit_and_empty_language():
    with pytest.raises(ValueError) as ei:
        G.compile_regex(r"(a|b)*a(a|b){13}")                 # 2^14 states after minimisation
    assert "4096" in str(ei.value) or "DOTS_MAX_GUIDE_STATES" in str(ei.value)
    assert G.compile_regex(r"(a|b)*a(a|b){10}").n_states == 2048
    with pytest.raises(ValueError) as ei:
        G.compile_regex("[^\x00-\U0010ffff]")
    assert "empty language" in str(ei.value)
    for bad in ([], ["a", "a"], [1], "ab"):
        with pytest.raises(ValueError):
            G.compile_choice(bad)
    g = G.compile_choice(["a.b", "c|d", "[x]", 'q"r', "tab\there"])
    assert all(g.matches(s.encode()) for s in ["a.b", "c|d", "[x]", 'q"r', "tab\there"]) and not g.matches(b"axb") and not g.matches(b"c")


# ---------------------------------------------------------------------------------------------------- JSON schema

def _valid(doc, s) -> bool:
    """the subset's meaning, by hand"""
    if "anyOf" in s:
        return any(_valid(doc, x) for x in s["anyOf"])
    if "const" in s:
        return type(doc) is type(s["const"]) and doc == s["const"]
    if "enum" in s:
        return any(type(doc) is type(v) and doc == v for v in s["enum"])
    t = s["type"]
    if isinstance(t, list):
        return any(_valid(doc, {**s, "type": x}) for x in t)
    if t == "string":
        return isinstance(doc, str) and s.get("minLength", 0) <= len(doc) <= s.get("maxLength", 1 << 30) and \
            ("pattern" not in s or re.fullmatch(s["pattern"], doc) is not None)
    if t == "integer":
        return isinstance(doc, int) and not isinstance(doc, bool)
    if t == "number":
        return isinstance(doc, (int, float)) and not isinstance(doc, bool)
    if t == "boolean":
        return isinstance(doc, bool)
    if t == "null":
        return doc is None
    if t == "array":
        return isinstance(doc, list) and s.get("minItems", 0) <= len(doc) <= s.get("maxItems", 1 << 30) and all(_valid(x, s["items"]) for x in doc)
    if t == "object":
        names = list(s["properties"])
        req = s.get("required", names)
        if not isinstance(doc, dict) or list(doc) != names[:len(doc)] or len(doc) < len(req):
            return False
        return all(_valid(doc[k], s["properties"][k]) for k in doc)
    raise AssertionError(t)


SCHEMAS = [
    {"type": "object", "properties": {"name": {"type": "string", "maxLength": 8}, "age": {"type": "integer"},
                                      "tags": {"type": "array", "items": {"enum": ["a", "b", 3, None, True]}, "maxItems": 3}}},
    {"type": "array", "items": {"type": "number"}, "minItems": 1, "maxItems": 4},
    {"anyOf": [{"type": "boolean"}, {"type": "null"}, {"const": "x y"}, {"type": "string", "pattern": "[A-Z]{2}[0-9]+"}]},
    {"type": "object", "properties": {"a": {"type": ["integer", "null"]}, "b": {"type": "string", "minLength": 2}, "c": {"type": "boolean"}},
     "required": ["a"], "additionalProperties": False},
    {"type": "array", "items": {"type": "array", "items": {"type": "integer"}, "minItems": 2, "maxItems": 2}},
    G.layout_schema(),
]


@pytest.mark.parametrize("k", range(len(SCHEMAS)))
def test_schema_language_parses_and_satisfies_the_schema(k):
    schema = SCHEMAS[k]
    rx = G.schema_to_regex(schema)
    g = G.compile_regex(rx)
    assert np.array_equal(G.compile_json_schema(json.dumps(schema)).table, g.table)        # a JSON string is accepted too
    rng = np.random.default_rng(50 + k)
    bad = 0
    for i in range(60):
        text = g.sample(rng, soft_len=int(rng.integers(8, 120)))
        doc = json.loads(text.decode("utf-8"))               # every member parses ...
        assert _valid(doc, schema), (text, doc)              # ... and satisfies the schema
        assert re.fullmatch(rx, text.decode("utf-8"))
        try:                                                 # json.dumps' own spacing is inside the language (1e999 parses to inf, which
            again = json.dumps(doc, ensure_ascii=False, allow_nan=False)       # JSON cannot write: nothing to compare there)
        except ValueError:
            again = None
        assert again is None or g.matches(again.encode()), doc
        broken = _mutate(rng, text)
        try:
            ok = _valid(json.loads(broken.decode("utf-8")), schema)
        except (ValueError, UnicodeDecodeError):
            ok = False
        if not ok:                                           # an invalid document is rejected
            bad += 1
            assert not g.matches(broken), broken
    assert bad >= 20
    tight = G.compile_json_schema(schema, whitespace="")
    assert tight.matches(json.dumps(json.loads(g.sample(rng, 60).decode()), separators=(",", ":"), ensure_ascii=False).encode())


def test_invalid_documents_are_rejected():
    g = G.compile_json_schema(SCHEMAS[0])
    good = '{"name": "ab", "age": -12, "tags": ["a", 3, null]}'
    assert g.matches(good.encode())
    for bad in ('{"name": "ab", "age": 1.5, "tags": []}', '{"age": 1, "name": "ab", "tags": []}', '{"name": "ab", "age": 1}',
                '{"name": "abcdefghi", "age": 1, "tags": []}', '{"name": "ab", "age": 01, "tags": []}', '{"name": "ab", "age": 1, "tags": ["c"]}',
                '{"name": "ab", "age": 1, "tags": ["a","a","a","a"]}', '{"name": "a\nb", "age": 1, "tags": []}', good[:-1], good + "}",
                '{"name": "ab", "age": 1, "tags": [], "x": 1}', '{"name": "a"b", "age": 1, "tags": []}'):
        assert not g.matches(bad.encode()), bad


@pytest.mark.parametrize("schema,word", [({"$ref": "#/defs/a"}, "$ref"), ({"type": "object"}, "free-form"), ({}, "free-form"),
                                         ({"type": "object", "patternProperties": {"a": {}}}, "patternProperties"),
                                         ({"allOf": [{"type": "string"}]}, "allOf"), ({"not": {"type": "string"}}, "not"),
                                         ({"oneOf": [{"type": "string"}]}, "oneOf"), ({"type": "integer", "minimum": 3}, "minimum"),
                                         ({"type": "array"}, "items"), ({"type": "tuple"}, "tuple"), ({"enum": [[1]]}, "scalars"),
                                         ({"type": "object", "properties": {"a": {"type": "null"}, "b": {"type": "null"}}, "required": ["b"]}, "required"),
                                         ({"type": "string", "pattern": "(?=a)"}, "look-ahead")])
def test_unsupported_schema_keywords_raise(schema, word):
    with pytest.raises(ValueError) as ei:
        G.compile_json_schema(schema)
    assert word in str(ei.value), str(ei.value)


def test_layout_schema_takes_real_layout_output_and_refuses_what_the_cleaner_repairs():
    from dots_ocr_amd.guided import layout_categories
    schema = G.layout_schema()
    g = G.compile_json_schema(schema)
    assert "Section-header" in layout_categories() and len(layout_categories()) == 11
    cases = json.loads((GOLDEN / "output_cleaner.json").read_text(encoding="utf-8"))
    yes = no = 0
    for raw, _ in cases:
        if not isinstance(raw, str):
            continue
        try:
            ok = _valid(json.loads(raw), schema)
        except ValueError:
            ok = False
        assert g.matches(raw.encode("utf-8")) == ok, raw[:200]
        yes, no = yes + ok, no + (not ok)
    assert yes >= 3 and no >= 20, (yes, no)                  # the fixture holds both: intact pages and the broken ones the cleaner salvages
    page = [{"bbox": [10, 20, 600, 50], "category": "Section-header", "text": "1. Überblick \"x\" \\ $a^2$\n"}, {"bbox": [0, 0, 1, 1], "category": "Picture"}]
    assert g.matches(json.dumps(page, ensure_ascii=False).encode()) and g.matches(json.dumps(page).encode()) and g.matches(b"[]")
    for broken in ('[{"bbox": [10, 20, 600, 50], "category": "Text", "text": "cut off',              # truncated
                   '[{"bbox": [10, 20, 600], "category": "Text"}]',                                  # a 3-number box
                   '[{"bbox": [10, 20, 600, 50], "category": "Heading"}]',                           # a category outside the list
                   '[{"bbox": [10, 20, 600, 50], "category": "Text}]',                               # a missing quote
                   '[{"bbox": [10, 20, 600, 50], "category": "Text"}{"bbox": [1, 2, 3, 4], "category": "Text"}]',      # a lost comma
                   '[{"bbox": [10, 20.5, 600, 50], "category": "Text"}]'):
        assert not g.matches(broken.encode()), broken
    assert G.compile_json_schema(G.layout_schema(["A", "B"])).matches(b'[{"bbox": [1, 2, 3, 4], "category": "B"}]')


# ---------------------------------------------------------------------------------------------------- mask

def test_mask_equals_a_brute_force_walk():
    rng = np.random.default_rng(3)
    alphabet = [b"0", b"7", b"42", b",", b", ", b"[", b"]", b"{", b'"', b'"bbox"', b"Text", b":", b" ", b"\n", b"a", b"yes", b"ye", b"s",
                "é".encode(), "中".encode()[:1], "中".encode()[1:], "中".encode(), b"\xff"]
    toks = [bytes([i]) for i in range(256)]
    for i in range(256, 3000):
        toks.append(b"" if i % 50 == 0 else b"".join(alphabet[int(j)] for j in rng.integers(0, len(alphabet), int(rng.integers(1, 5)))))
    special = [2990, 2995, 48]                               # a special id that would otherwise be allowed ('0')
    tb = G.TokenBytes(toks, special)
    assert tb.vocab_size == 3000 and tb.token(48) == b"" and tb.token(49) == b"1" and tb.token(300) == toks[300]
    for pattern in (r"-?[0-9]+(, [0-9]+)*", r"yes|no", r"[^a-z]*中", G.schema_to_regex(G.layout_schema())):
        g = G.compile_regex(pattern)
        states = {g.start, G.DEAD} | {int(s) for s in rng.integers(0, g.n_states, 6)}
        some = 0
        for s in states:
            got = g.mask(s, tb)
            want = np.array([len(tb.token(t)) > 0 and g.walk(s, tb.token(t)) != G.DEAD for t in range(tb.vocab_size)])
            assert got.dtype == bool and np.array_equal(got, want), (pattern, s)
            assert not got[special].any() and not got[[t for t in range(256, 3000) if t % 50 == 0]].any()
            some += int(got.any())
        assert some >= 1 and not g.mask(G.DEAD, tb).any()
    assert g.walk(g.start, b"[]") != G.DEAD and g.walk(g.start, b"]") == G.DEAD and g.walk(G.DEAD, b"") == G.DEAD


# ---------------------------------------------------------------------------------------------------- scheduler and server through fakes

def _guide_engine(base):
    """a slot engine that takes guides as Engine does: handles, rows that hold them, refusal to destroy a held one"""
    class E(base):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            self.token_bytes, self.guides, self.row_guides, self.guide_calls = None, {}, {}, []

        def set_token_bytes(self, tb, special_ids=()):
            self.token_bytes = tb

        def create_guide(self, g):
            h = max(self.guides, default=-1) + 1
            self.guides[h] = g
            self.guide_calls.append(("create", g.pattern))
            return h

        def destroy_guide(self, h):
            if h in self.row_guides.values():
                raise RuntimeError("guide is held")
            self.guide_calls.append(("destroy", self.guides.pop(h).pattern))

        def set_row_guide(self, row, h):
            self.guide_calls.append((row, h))
            if h is None:
                self.row_guides.pop(row, None)
            else:
                assert h in self.guides
                self.row_guides[row] = h

        def set_row_logit_rules(self, row, rules):
            pass

        def slot_release(self, s):
            self.row_guides.pop(s, None)
            super().slot_release(s)
    return E


def test_scheduler_sets_the_guide_before_the_prefill_and_clears_it():
    from fakes import FakeSlotEngine
    from dots_ocr_amd.scheduler import ContinuousBatcher, Request
    order = []

    class Eng(_guide_engine(FakeSlotEngine)):
        def slots_prefill(self, slots, ids, lens, caps):
            order.append(("prefill", [self.row_guides.get(int(s)) for s in slots]))
            super().slots_prefill(slots, ids, lens, caps)
    eng = Eng(lambda prompt: [5, 6, 7, 8], max_batch=2, max_prefill_tokens=64)
    h = eng.create_guide(G.compile_regex("a+"))
    cb = ContinuousBatcher(eng, chunk=2)
    out = cb.run([Request(np.array([1 + i, 2], np.int32), max_new_tokens=3, guide=h if i % 2 == 0 else None) for i in range(4)])
    assert [list(o) for o in out] == [[5, 6, 7]] * 4
    assert order[0] == ("prefill", [h, None])                # rows are set before their prefill
    assert eng.row_guides == {} and rows_holding(cb._rows, "guide") == []      # and nothing stays behind
    eng.destroy_guide(h)
    with pytest.raises(ValueError):                          # an engine without the call
        ContinuousBatcher(FakeSlotEngine(lambda p: [5], max_batch=2, max_prefill_tokens=64)).submit(Request(np.array([1, 2], np.int32), guide=0))


class _Model:
    def __init__(self, cfg, proc, guides=True):
        from fakes import FakeSlotEngine

        class Eng(FakeSlotEngine):
            def slots_decode(self, n):
                time.sleep(0.002)
                super().slots_decode(n)
        script = lambda prompt: proc.tokenizer.encode("ok then") + [cfg.eos_token_ids[0]] + proc.tokenizer.encode("more")     # noqa: E731
        self.config = cfg
        self.engine = (_guide_engine(Eng) if guides else Eng)(script, max_batch=2, max_patches=4096, max_prefill_tokens=4096, max_seq_len=2048)


def _payload(**kw):
    body = {"model": "model", "messages": [{"role": "user", "content": "Read this."}], "max_completion_tokens": 32}
    body.update(kw)
    return body


def _app(guides=True, continuous=True):
    pytest.importorskip("fastapi")
    from dots_ocr_amd.processing import DotsOcrProcessor
    from dots_ocr_amd.server import create_app
    cfg = DotsConfig.tiny()
    proc = DotsOcrProcessor(cfg)
    return cfg, proc, create_app(_Model(cfg, proc, guides), proc, model_name="model", max_batch=2, continuous=continuous)


SCHEMA = {"type": "object", "properties": {"a": {"type": "integer"}}}
FIELDS = (dict(guided_regex="[0-9]+"), dict(guided_choice=["yes", "no"]), dict(guided_json=SCHEMA), dict(guided_json=json.dumps(SCHEMA)),
          dict(guided_json=SCHEMA, guided_whitespace_pattern=" ?"), dict(guided_layout=True),
          dict(response_format={"type": "json_schema", "json_schema": {"name": "x", "schema": SCHEMA}}))


def test_server_accepts_each_guided_field_and_caches_the_guides():
    from fastapi.testclient import TestClient
    cfg, proc, app = _app()
    eng = app.state.worker.model.engine
    assert eng.token_bytes is not None and eng.token_bytes.vocab_size == cfg.vocab_size          # uploaded at start-up
    assert eng.token_bytes.token(65) == b"A" and eng.token_bytes.token(cfg.eos_token_ids[0]) == b"" and eng.token_bytes.token(cfg.image_token_id) == b""
    with TestClient(app) as c:
        for f in FIELDS:
            r = c.post("/v1/chat/completions", json=_payload(**f))
            assert r.status_code == 200, (f, r.text)
            assert r.json()["choices"][0]["message"]["content"] == "ok then"
        creates = [x for x in eng.guide_calls if x[0] == "create"]
        assert len(creates) == 5                             # the schema given as object, as string and as response_format is one guide
        assert sum(1 for x in eng.guide_calls if isinstance(x[0], int) and x[1] is not None) == len(FIELDS)      # every request's row was set
        assert c.post("/v1/chat/completions", json=_payload(guided_regex="[0-9]+")).status_code == 200
        assert len([x for x in eng.guide_calls if x[0] == "create"]) == 5                         # served from the cache
        for k in range(app.state.worker.GUIDE_CACHE + 3):    # more patterns than the cache holds: the oldest unused handles go
            assert c.post("/v1/chat/completions", json=_payload(guided_regex=f"x{k}")).status_code == 200
        assert len(eng.guides) <= app.state.worker.GUIDE_CACHE and any(x[0] == "destroy" for x in eng.guide_calls)
        assert eng.row_guides == {}


def test_a_repeated_request_compiles_nothing(monkeypatch):
    """the host-side cache: the pattern -> DFA pipeline runs once per pattern text, however the request spells it"""
    from fastapi.testclient import TestClient
    compiled = []
    real = G._compile_ast
    monkeypatch.setattr(G, "_compile_ast", lambda ast, pattern: (compiled.append(pattern), real(ast, pattern))[1])
    monkeypatch.setattr(G, "_guide_cache", type(G._guide_cache)())               # whatever earlier tests left in it
    schema = {"type": "object", "properties": {"once": {"type": "boolean"}}}
    _, _, app = _app()
    with TestClient(app) as c:
        for f in (dict(guided_layout=True), dict(guided_layout=True), dict(guided_regex="q[0-9]{2}"), dict(guided_regex="q[0-9]{2}"),
                  dict(guided_json=schema), dict(guided_json=json.dumps(schema)), dict(response_format={"type": "json_schema", "json_schema": {"schema": schema}}),
                  dict(guided_choice=["u", "v"]), dict(guided_choice=["u", "v"]), dict(guided_layout=True)):
            assert c.post("/v1/chat/completions", json=_payload(**f)).status_code == 200, f
    assert len(compiled) == 4 and len(set(compiled)) == 4, compiled              # layout, the regex, the schema, the choice: each once
    assert G.compile_cached("q[0-9]{2}") is G.compile_cached("q[0-9]{2}")
    for k in range(G.GUIDE_CACHE_SIZE + 5):                                      # the cache is bounded
        G.compile_cached(f"z{k}")
    assert len(G._guide_cache) == G.GUIDE_CACHE_SIZE


def test_a_hostile_pattern_fails_fast():
    t0 = time.perf_counter()
    for bad in (r"(a|b)*a(a|b){14}", r"(a|b)*a(a|b){30}", r"([a-z]{1,40}){1,4000}"):
        with pytest.raises(ValueError) as ei:
            G.compile_regex(bad)
        assert "DOTS_MAX_GUIDE_STATES" in str(ei.value)
    assert time.perf_counter() - t0 < 5.0                                        # each stops at the build limits, not after minutes


def test_server_rejects_bad_guided_fields():
    from fastapi.testclient import TestClient
    _, _, app = _app()
    eng = app.state.worker.model.engine
    with TestClient(app) as c:
        for bad, word in ((dict(guided_regex="[0-9]+", guided_choice=["a"]), "at most one"), (dict(guided_json=SCHEMA, guided_layout=True), "at most one"),
                          (dict(guided_regex="a", response_format={"type": "json_schema", "json_schema": {"schema": SCHEMA}}), "at most one"),
                          (dict(guided_json=SCHEMA, response_format={"type": "json_schema", "json_schema": {"schema": SCHEMA}}), "at most one"),
                          (dict(guided_regex="^a"), "anchor"), (dict(guided_regex="(a"), "unbalanced"), (dict(guided_regex=5), "string"),
                          (dict(guided_choice=[]), "at least one"), (dict(guided_choice=["a", "a"]), "twice"), (dict(guided_choice="ab"), "list"),
                          (dict(guided_json={"$ref": "#"}), "$ref"), (dict(guided_json="{not json"), "JSON"), (dict(guided_json=[1]), "schema object"),
                          (dict(guided_json=SCHEMA, guided_whitespace_pattern="(?=x)"), "look-ahead"), (dict(guided_whitespace_pattern=" "), "needs"),
                          (dict(guided_regex="a", guided_whitespace_pattern=" "), "needs"), (dict(guided_choice=["a"], guided_whitespace_pattern=" "), "needs"),
                          (dict(guided_regex="a" * (G.MAX_PATTERN_CHARS + 1)), "characters long"),
                          (dict(guided_layout="yes"), "true or false"),
                          (dict(response_format={"type": "json_object"}), "free-form JSON is recursive; give a schema"),
                          (dict(response_format={"type": "json_schema"}), "json_schema.schema"), (dict(response_format={"type": "xml"}), "xml"),
                          (dict(guided_choice=["yes", "no"], min_tokens=3), "shortest match")):
            r = c.post("/v1/chat/completions", json=_payload(**bad))
            assert r.status_code == 400 and word in r.text, (bad, r.text)
        assert c.post("/v1/chat/completions", json=_payload(guided_choice=["yes", "no"], min_tokens=2)).status_code == 200
        assert c.post("/v1/chat/completions", json=_payload(response_format={"type": "text"})).status_code == 200
        assert [x for x in eng.guide_calls if x[0] == "create"] == [("create", "yes|no")]


def test_server_refuses_guides_where_the_worker_cannot_honour_them():
    from fastapi.testclient import TestClient
    _, _, app = _app(continuous=False)                       # static batches through model.generate
    with TestClient(app) as c:
        for f in FIELDS:
            r = c.post("/v1/chat/completions", json=_payload(**f))
            assert r.status_code == 400 and "guided" in r.text, (f, r.text)
    _, _, app = _app(guides=False)                           # slots, but an engine without guides
    with TestClient(app) as c:
        for f in FIELDS:
            assert c.post("/v1/chat/completions", json=_payload(**f)).status_code == 400, f
        assert c.post("/v1/chat/completions", json=_payload()).status_code == 200


def test_responses_without_the_fields_are_unchanged():
    from fastapi.testclient import TestClient
    outs = []
    for guides in (True, False):
        _, _, app = _app(guides=guides)
        with TestClient(app) as c:
            r = c.post("/v1/chat/completions", json=_payload(temperature=0.0))
            assert r.status_code == 200
            body = r.json()
            body.pop("id"), body.pop("created")
            outs.append(body)
        if guides:
            assert app.state.worker.model.engine.guide_calls == []          # no guide call for a request that names none
    assert outs[0] == outs[1]
    assert sorted(outs[0]) == ["choices", "model", "object", "usage"] and sorted(outs[0]["choices"][0]) == ["finish_reason", "index", "message"]


def test_parser_switch_adds_guided_layout_for_the_layout_modes_only():
    from dots_ocr_amd.parser import DotsOCRParser
    from dots_ocr_amd.prompts import dict_promptmode_to_prompt as P
    off, on = DotsOCRParser(), DotsOCRParser(guided=True)
    assert not off.guided and not off._guided_layout([P["prompt_layout_all_en"]])                  # the default is off
    assert on._guided_layout([P["prompt_layout_all_en"]]) and on._guided_layout([P["prompt_layout_only_en"], P["prompt_layout_all_en"]])
    assert not on._guided_layout([P["prompt_ocr"]]) and not on._guided_layout([P["prompt_layout_all_en"], P["prompt_ocr"]])


# ---------------------------------------------------------------------------------------------------- C ABI

def test_new_symbols_are_exported():
    from dots_ocr_amd import _lib, build, engine
    if not build.lib_path().exists():
        build.build(verbose=False)
    lib = _lib.load()
    new = ["dots_set_token_bytes", "dots_guide_create", "dots_guide_destroy", "dots_set_row_guide", "dots_row_guide_state",
           "dots_op_select_tokens_guided", "dots_bench_select_tokens_guided"]
    for sym in new:
        assert hasattr(lib, sym) and sym in engine.EXPORTED_SYMBOLS, sym
    header = (Path(__file__).parent.parent / "include" / "dots_ocr_hip.h").read_text()
    assert all(f"int {sym}(" in header for sym in new) and "#define DOTS_MAX_GUIDE_STATES 4096" in header
    assert G.MAX_GUIDE_STATES == 4096
