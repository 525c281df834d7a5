"""Speculative decoding of sampled and stop-string rows, the parts that need no GPU: the server's --speculative-rows flag,
Engine.set_speculation_rows against a fake library, the generate() / DotsOCRParser keywords, and the row-class rule
(RowStage::speculates, csrc/row_stage.h) against the brute-force statement of tests/spec_rows_model.cpp, a stand-alone program compiled
with -fsanitize=address,undefined and run directly."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

from dots_ocr_amd.engine import SPEC_ROWS, Engine, spec_rows_flags

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "dots_ocr_amd" / "csrc"


# ---------------------------------------------------------------------------------------------------- the setting's spellings

@pytest.mark.parametrize("value,flags", [
    (None, 0), ("greedy", 0), ("sampled", 1), ("stop", 2), ("all", 3), (("sampled", "stop"), 3), (["stop"], 2), ((), 0), (("stop", "all"), 3),
])
def test_spec_rows_flags(value, flags):
    assert spec_rows_flags(value) == flags
    assert SPEC_ROWS == {"sampled": 1, "stop": 2}                      # DOTS_SPEC_ROWS_SAMPLED / DOTS_SPEC_ROWS_STOP


@pytest.mark.parametrize("value", ["penalties", ("sampled", "logprobs"), 3, ("greedy", "stop"), (1,)])
def test_spec_rows_flags_refuses_other_names(value):
    with pytest.raises((ValueError, TypeError)):
        spec_rows_flags(value)


def test_header_and_binding_agree_on_the_bits():
    hdr = (ROOT / "include" / "dots_ocr_hip.h").read_text()
    assert int(re.search(r"^#define DOTS_SPEC_ROWS_SAMPLED (\d+)", hdr, re.M).group(1)) == SPEC_ROWS["sampled"]
    assert int(re.search(r"^#define DOTS_SPEC_ROWS_STOP (\d+)", hdr, re.M).group(1)) == SPEC_ROWS["stop"]
    assert re.search(r"^int dots_set_speculation_rows\(DotsEngine\* e, int flags\);", hdr, re.M)
    assert re.search(r"^int dots_set_speculation\(DotsEngine\* e, int k, int min_n, int max_n\);", hdr, re.M)      # unchanged


# ---------------------------------------------------------------------------------------------------- server flags

def _parse(*argv):
    from dots_ocr_amd.server import build_arg_parser
    return build_arg_parser().parse_args(list(argv))


def test_server_flag_defaults_to_greedy_rows():
    from dots_ocr_amd.server import speculation_args
    a = _parse()
    assert a.speculative_rows == "greedy" and speculation_args(a) is None
    a = _parse("--speculative-ngram", "3")
    assert a.speculative_rows == "greedy" and speculation_args(a) == (3, 2, 4)
    assert spec_rows_flags(a.speculative_rows) == 0


@pytest.mark.parametrize("name,flags", [("greedy", 0), ("sampled", 1), ("stop", 2), ("all", 3)])
def test_server_flag_parses_with_speculation_on(name, flags):
    from dots_ocr_amd.server import speculation_args
    a = _parse("--speculative-ngram", "3", "--speculative-rows", name)
    assert speculation_args(a) == (3, 2, 4)
    assert spec_rows_flags(a.speculative_rows) == flags


@pytest.mark.parametrize("name", ["sampled", "stop", "all"])
def test_server_flag_without_speculation_is_an_error(name):
    from dots_ocr_amd.server import speculation_args
    with pytest.raises(ValueError, match="--speculative-ngram"):
        speculation_args(_parse("--speculative-rows", name))
    assert speculation_args(_parse("--speculative-rows", "greedy")) is None


def test_server_flag_refuses_other_names():
    with pytest.raises(SystemExit):
        _parse("--speculative-ngram", "3", "--speculative-rows", "penalties")


# ---------------------------------------------------------------------------------------------------- Engine.set_speculation_rows

class FakeLib:
    """the two entry points the method and its error path touch"""

    def __init__(self, rc=0):
        self.rc, self.calls = rc, []

    def dots_set_speculation_rows(self, h, flags):
        self.calls.append((h, flags))
        return self.rc

    def dots_last_error(self, h):
        return b"the speculating rows cannot change while slot 0 is occupied"


def _engine(lib):
    e = object.__new__(Engine)                  # no library, no GPU
    e.lib, e.h = lib, 1234
    return e


def test_engine_method_passes_the_bits():
    lib = FakeLib()
    e = _engine(lib)
    e.set_speculation_rows()
    e.set_speculation_rows(sampled=True)
    e.set_speculation_rows(stop=True)
    e.set_speculation_rows(sampled=True, stop=True)
    e.set_speculation_rows(sampled=1, stop=0)
    assert lib.calls == [(1234, 0), (1234, 1), (1234, 2), (1234, 3), (1234, 1)]
    assert e.spec_rows == 1
    e.h = None                                  # nothing for __del__ to destroy


def test_engine_method_raises_what_the_library_refuses():
    from dots_ocr_amd.engine import DotsEngineError
    lib = FakeLib(rc=-3)
    e = _engine(lib)
    e.spec_rows = 0
    with pytest.raises(DotsEngineError) as ei:
        e.set_speculation_rows(sampled=True)
    assert "(-3)" in str(ei.value) and e.spec_rows == 0                # the refused call changed nothing
    e.h = None


def test_the_entry_point_is_registered_with_the_others():
    from dots_ocr_amd import engine
    assert "dots_set_speculation_rows" in engine.EXPORTED_SYMBOLS
    src = Path(engine.__file__).read_text()
    assert re.search(r'"dots_set_speculation_rows": \(i32, \[vp, i32\]\)', src)


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


def _names(m):
    return [c[0] for c in m.engine.calls]


def test_generate_without_the_keyword_is_what_it_was():
    m = _model()
    assert m.generate(speculative_ngram=3) == "out"
    assert "set_speculation_rows" not in _names(m)
    assert [c[1] for c in m.engine.calls if c[0] == "set_speculation"] == [(3, 2, 4), (0,)]
    assert m.seen[0][8] is None                                       # row_sp: a greedy call gives its rows no parameters


def test_generate_sets_and_clears_the_rows():
    m = _model()
    m.generate(speculative_ngram=3, speculative_rows="stop")
    calls = [(c[0], c[2]) for c in m.engine.calls if c[0] == "set_speculation_rows"]
    assert calls == [("set_speculation_rows", dict(sampled=False, stop=True)), ("set_speculation_rows", {})]
    names = _names(m)                                                 # set after speculation is on, both while no slot is occupied
    assert names.index("slots_reset") < names.index("set_speculation") < names.index("set_speculation_rows")
    m = _model()
    m.generate(speculative_ngram=2, speculative_rows=("sampled", "stop"))
    assert [c[2] for c in m.engine.calls if c[0] == "set_speculation_rows"][0] == dict(sampled=True, stop=True)


def test_generate_gives_sampled_sequences_parameters_of_their_own():
    """the engine-wide sampler never speculates: a sampled call under "sampled" draws per row with seed + b, the engine stays greedy"""
    m = _model()
    m.generate(speculative_ngram=3, speculative_rows="all", do_sample=True, temperature=0.1, seed=40)
    row_sp = m.seen[0][8]
    assert row_sp(0).temperature == pytest.approx(0.1) and row_sp(0).seed == 40 and row_sp(2).seed == 42 and row_sp(0).top_k == 0
    sampling = [c[1] for c in m.engine.calls if c[0] == "set_sampling"]
    assert sampling[0][0] == pytest.approx(0.1) and sampling[-1] == (0.0, 1.0, 0)
    # a greedy call under "sampled" and a sampled call under "stop" keep the engine-wide setting
    m = _model()
    m.generate(speculative_ngram=3, speculative_rows="sampled")
    assert m.seen[0][8] is None and len([c for c in m.engine.calls if c[0] == "set_sampling"]) == 1
    m = _model()
    m.generate(speculative_ngram=3, speculative_rows="stop", do_sample=True, temperature=0.5)
    assert m.seen[0][8] is None and len([c for c in m.engine.calls if c[0] == "set_sampling"]) == 1


@pytest.mark.parametrize("value", ["all", "sampled", ("stop",)])
def test_generate_refuses_the_keyword_without_speculation(value):
    m = _model()
    with pytest.raises(ValueError, match="speculative_ngram"):
        m.generate(speculative_rows=value)
    with pytest.raises(ValueError, match="speculative_ngram"):
        m.generate(speculative_ngram=0, speculative_rows=value)
    assert "set_speculation" not in _names(m) and not m.seen


def test_generate_refuses_other_names():
    m = _model()
    with pytest.raises(ValueError):
        m.generate(speculative_ngram=3, speculative_rows="penalties")
    assert not m.seen


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
    p = _parser(speculative_ngram=3, speculative_rows="all")
    with pytest.raises(StopIteration):
        p._inference_batch_with_hf([None], ["x"])
    assert p.model.kw["speculative_ngram"] == 3 and p.model.kw["speculative_rows"] == "all"
    p = _parser(speculative_ngram=3)
    with pytest.raises(StopIteration):
        p._inference_batch_with_hf([None], ["x"])
    assert "speculative_rows" not in p.model.kw                       # the default: the call is what it was
    p = _parser()
    with pytest.raises(StopIteration):
        p._inference_batch_with_hf([None], ["x"])
    assert "speculative_rows" not in p.model.kw and "speculative_ngram" not in p.model.kw


def test_parser_refuses_the_keyword_without_speculation():
    with pytest.raises(ValueError, match="speculative_ngram"):
        _parser(speculative_rows="all")
    with pytest.raises(ValueError):
        _parser(speculative_ngram=3, speculative_rows="penalties")


# ---------------------------------------------------------------------------------------------------- the row-class rule

def test_row_class_rule_matches_the_brute_force_statement(tmp_path):
    cxx = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    assert cxx, "no C++ compiler (c++, g++ or clang++) on PATH"
    max_batch = re.search(r"^#define DOTS_MAX_BATCH (\d+)", (CSRC / "kernels.h").read_text(), re.M).group(1)
    exe = tmp_path / "spec_rows_model"
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", f"-DDOTS_MAX_BATCH={max_batch}",
           f"-I{CSRC}", str(ROOT / "tests" / "spec_rows_model.cpp"), "-o", str(exe)]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    # 3 rows x {alone, beside a full neighbour} x 2^5 feature subsets x {penalty, none} x 4 modes
    assert int(re.search(r"(\d+) cases", p.stdout).group(1)) == 3 * 2 * 32 * 2 * 4, p.stdout


def test_the_kernels_ask_the_class_array_only():
    """spec.hip decides nothing about a row from the stage's tables: the own / logprob tests are gone from it, and the engine derives the
    class in one function"""
    spec = (CSRC / "spec.hip").read_text()
    assert not re.search(r"\bsp\.(own|lp)\b", spec) and not re.search(r"\bown\[b\]|\blp\[b\]", spec)
    assert len(re.findall(r"SPEC_ROW_NONE", spec)) >= 2                # spec_live_drafts and the drafter
    eng = "".join((CSRC / f).read_text() for f in ("engine.h", "engine.hip", "weights.hip", "slots.hip", "rows.hip", "ops.hip"))
    assert len(re.findall(r"stage\.speculates\(", eng)) == 1
