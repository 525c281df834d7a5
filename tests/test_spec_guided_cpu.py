"""Speculative decoding of guided rows, the parts that need no GPU: the server's --speculative-guided flag, the generate() /
DotsOCRParser keywords, Engine.set_speculation_guided against a fake library, the header line, the row rule (RowStage::speculates with
the internal bit SPEC_ROWS_GUIDED) against the brute-force statement of tests/spec_guided_model.cpp — a stand-alone program compiled with
-fsanitize=address,undefined and run directly — and the host statement of the state chain (Guide.draft_states) checked by hand."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

from dots_ocr_amd import guided as G
from dots_ocr_amd.engine import SPEC_ROWS, Engine

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "dots_ocr_amd" / "csrc"


# ---------------------------------------------------------------------------------------------------- server flag

def _parse(*argv):
    from dots_ocr_amd.server import build_arg_parser
    return build_arg_parser().parse_args(list(argv))


def test_server_flag_is_off_by_default():
    from dots_ocr_amd.server import speculation_args
    assert _parse().speculative_guided is False
    a = _parse("--speculative-ngram", "3")
    assert a.speculative_guided is False and speculation_args(a) == (3, 2, 4)


def test_server_flag_parses_with_speculation_on():
    from dots_ocr_amd.server import speculation_args
    a = _parse("--speculative-ngram", "3", "--speculative-guided")
    assert a.speculative_guided is True and a.speculative_rows == "greedy" and speculation_args(a) == (3, 2, 4)
    a = _parse("--speculative-ngram", "3", "--speculative-rows", "sampled", "--speculative-guided")      # the stock client's temperature = 0.1
    assert a.speculative_guided is True and a.speculative_rows == "sampled"


def test_server_flag_without_speculation_is_an_error():
    from dots_ocr_amd.server import speculation_args
    with pytest.raises(ValueError, match="--speculative-ngram"):
        speculation_args(_parse("--speculative-guided"))
    with pytest.raises(ValueError, match="--speculative-ngram"):
        speculation_args(_parse("--speculative-ngram", "0", "--speculative-guided"))


# ---------------------------------------------------------------------------------------------------- Engine.set_speculation_guided

class FakeLib:
    def __init__(self, rc=0):
        self.rc, self.calls = rc, []

    def dots_set_speculation_guided(self, h, on):
        self.calls.append((h, on))
        return self.rc

    def dots_last_error(self, h):
        return b"guided speculation cannot change while slot 0 is occupied"


def _engine(lib):
    e = object.__new__(Engine)                  # no library, no GPU
    e.lib, e.h = lib, 1234
    return e


def test_engine_method_passes_the_switch():
    lib = FakeLib()
    e = _engine(lib)
    assert e.spec_guided is False               # the default, before any call
    e.set_speculation_guided()
    assert e.spec_guided is True
    e.set_speculation_guided(False)
    e.set_speculation_guided(on=1)
    assert lib.calls == [(1234, 1), (1234, 0), (1234, 1)] and e.spec_guided is True
    e.h = None                                  # nothing for __del__ to destroy


def test_engine_method_raises_what_the_library_refuses():
    from dots_ocr_amd.engine import DotsEngineError
    e = _engine(FakeLib(rc=-3))
    with pytest.raises(DotsEngineError) as ei:
        e.set_speculation_guided(True)
    assert "(-3)" in str(ei.value) and e.spec_guided is False          # the refused call changed nothing
    e.h = None


def test_header_and_binding():
    from dots_ocr_amd import engine
    hdr = (ROOT / "include" / "dots_ocr_hip.h").read_text()
    assert re.search(r"^int dots_set_speculation_guided\(DotsEngine\* e, int on\);", hdr, re.M)
    assert re.search(r"^int dots_set_speculation_rows\(DotsEngine\* e, int flags\);", hdr, re.M)      # unchanged, and no third bit
    assert not re.search(r"^#define DOTS_SPEC_ROWS_GUIDED", hdr, re.M) and SPEC_ROWS == {"sampled": 1, "stop": 2}
    assert "dots_set_speculation_guided" in engine.EXPORTED_SYMBOLS and "dots_op_spec_guide_masks" in engine.EXPORTED_SYMBOLS
    src = Path(engine.__file__).read_text()
    assert re.search(r'"dots_set_speculation_guided": \(i32, \[vp, i32\]\)', src)


# ---------------------------------------------------------------------------------------------------- generate() / DotsOCRParser keywords

class RecEngine:
    token_bytes = object()

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def rec(*a, **kw):
            self.calls.append((name, a, kw))
        return rec


def _model():
    from dots_ocr_amd.modeling import DotsOcrHipForCausalLM
    m = object.__new__(DotsOcrHipForCausalLM)
    m.generation_config = {}
    m.engine = RecEngine()
    m.seen = []
    m._generate = lambda *a: m.seen.append(a) or "out"
    return m


def test_generate_without_the_keyword_never_touches_the_switch():
    m = _model()
    assert m.generate(speculative_ngram=3, speculative_rows="all") == "out"
    assert "set_speculation_guided" not in [c[0] for c in m.engine.calls]


def test_generate_sets_and_clears_the_switch():
    m = _model()
    m.generate(speculative_ngram=3, speculative_guided=True)
    names = [c[0] for c in m.engine.calls]
    assert [c[1] for c in m.engine.calls if c[0] == "set_speculation_guided"] == [(True,), (False,)]
    assert names.index("slots_reset") < names.index("set_speculation") < names.index("set_speculation_guided")      # while no slot is occupied
    assert "set_speculation_rows" not in names
    m = _model()
    m.generate(speculative_ngram=3, speculative_rows="sampled", speculative_guided=True, do_sample=True, temperature=0.1, seed=7)
    assert m.seen[0][8](1).seed == 8 and [c[1] for c in m.engine.calls if c[0] == "set_speculation_guided"][0] == (True,)


def test_generate_refuses_the_keyword_without_speculation():
    m = _model()
    with pytest.raises(ValueError, match="speculative_ngram"):
        m.generate(speculative_guided=True)
    with pytest.raises(ValueError, match="speculative_ngram"):
        m.generate(speculative_ngram=0, speculative_guided=True)
    assert "set_speculation" not in [c[0] for c in m.engine.calls] and not m.seen


class RecModel:
    def __init__(self):
        self.engine = RecEngine()
        self.kw = None

    def generate(self, **kw):
        self.kw = kw
        raise StopIteration                                           # the keywords are all this test wants


class FakeInputs(dict):
    def to(self, device):
        return self


def _parser(**kw):
    from dots_ocr_amd.parser import DotsOCRParser
    p = DotsOCRParser(model=RecModel(), processor=object(), **kw)
    p._build_inputs = lambda images, prompts: FakeInputs(input_ids=None)
    return p


def test_parser_passes_the_keyword_to_generate():
    p = _parser(speculative_ngram=3, speculative_guided=True)
    with pytest.raises(StopIteration):
        p._inference_batch_with_hf([None], ["x"])
    assert p.model.kw["speculative_ngram"] == 3 and p.model.kw["speculative_guided"] is True
    p = _parser(speculative_ngram=3)
    with pytest.raises(StopIteration):
        p._inference_batch_with_hf([None], ["x"])
    assert "speculative_guided" not in p.model.kw                     # the default: the call is what it was


def test_parser_refuses_the_keyword_without_speculation():
    with pytest.raises(ValueError, match="speculative_ngram"):
        _parser(speculative_guided=True)


# ---------------------------------------------------------------------------------------------------- the row rule

def test_row_rule_matches_the_brute_force_statement(tmp_path):
    cxx = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    assert cxx, "no C++ compiler (c++, g++ or clang++) on PATH"
    max_batch = re.search(r"^#define DOTS_MAX_BATCH (\d+)", (CSRC / "kernels.h").read_text(), re.M).group(1)
    exe = tmp_path / "spec_guided_model"
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", f"-DDOTS_MAX_BATCH={max_batch}",
           f"-I{CSRC}", str(ROOT / "tests" / "spec_guided_model.cpp"), "-o", str(exe)]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    # 3 rows x {alone, beside a full neighbour} x 2^5 feature subsets x {penalty, none} x 8 modes
    assert int(re.search(r"(\d+) cases", p.stdout).group(1)) == 3 * 2 * 32 * 2 * 8, p.stdout


def test_the_engine_derives_the_mode_in_one_place():
    rows = (CSRC / "rows.hip").read_text()
    assert len(re.findall(r"SPEC_ROWS_GUIDED", rows)) == 1             # spec_row_class ORs it in; nothing else knows the bit
    assert re.search(r"flags & ~SPEC_ROWS_ALL", rows)                  # dots_set_speculation_rows still refuses it


# ---------------------------------------------------------------------------------------------------- the state chain on the host

TOKS = [b"a", b"b", b"c", b"ab", b"abc", b"ca", b"", b"bca", b"cab"]     # id 6 has no bytes
TB = G.TokenBytes(TOKS)


def test_draft_states_by_hand():
    g = G.compile_regex(r"(abc)*")
    s0 = g.start
    sa, sab = g.walk(s0, b"a"), g.walk(s0, b"ab")
    assert len({s0, sa, sab}) == 3 and g.walk(s0, b"abc") == s0 and g.accepting[s0] and not g.accepting[sa]
    assert g.draft_states(s0, [], TB) == []
    assert g.draft_states(s0, [0, 1, 2], TB) == [sa, sab, s0]                    # a, b, c: one byte each, back at the start
    assert g.draft_states(s0, [3, 2, 4], TB) == [sab, s0, s0]                    # ab, c, abc
    assert g.draft_states(sa, [7, 4], TB) == [sa, -1]                            # a + bca = abca: alive; then abc from "a": dead
    assert g.draft_states(sab, [5, 1, 2], TB) == [sa, sab, s0]                   # ab + ca, b, c
    # dead: the walk meets DEAD inside the token, and everything behind it is dead too
    assert g.draft_states(s0, [0, 2, 1], TB) == [sa, -1, -1]                     # a, then c where b is due
    assert g.draft_states(s0, [8, 0, 1], TB) == [-1, -1, -1]                     # cab at the start
    # byte-less: never a token of a guided row, true drafts behind it do not revive the chain
    assert g.draft_states(s0, [4, 6, 4], TB) == [s0, -1, -1]
    assert g.draft_states(s0, [6], TB) == [-1]
    # an EOS id finishes the row and is not walked, whatever its bytes and whether or not the state accepts
    assert g.draft_states(s0, [4, 4, 4], TB, eos_ids=[4]) == [-1, -1, -1]
    assert g.draft_states(s0, [0, 1, 2, 4], TB, eos_ids=[2]) == [sa, sab, -1, -1]
    assert g.draft_states(s0, [0, 1, 2, 4], TB, eos_ids=[5]) == [sa, sab, s0, s0]        # an EOS id that is not drafted changes nothing
    # each entry is the walk over the concatenated bytes of the drafts so far
    d = [3, 2, 0, 1, 2, 4]
    assert g.draft_states(s0, d, TB) == [g.walk(s0, b"".join(TOKS[t] for t in d[:j + 1])) for j in range(len(d))]
