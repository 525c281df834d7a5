"""Speculative decoding of rows with an n-gram rule, logit rules or penalties, the parts that need no GPU: the row rule
(RowStage::speculates with the internal bits 8 / 16 / 32) against the brute-force statement of tests/spec_shaped_model.cpp — a stand-alone
program compiled with -fsanitize=address,undefined and run directly —, the header line, the symbol, the ctypes entry, Engine.
set_speculation_shaped against a fake library, the generate() / DotsOCRParser keywords, the server's --speculative-shaped flag and its
refusals, and the host statements of what a draft row is selected under (draft_row_history, draft_row_counts) checked by hand."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

from dots_ocr_amd import build
from dots_ocr_amd.engine import SPEC_ROWS, SPEC_SHAPED, Engine, banned_ngram_ids, draft_row_counts, draft_row_history, spec_shaped_flags

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "dots_ocr_amd" / "csrc"


# ---------------------------------------------------------------------------------------------------- the row rule

def test_row_rule_matches_the_brute_force_statement(tmp_path):
    cxx = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    assert cxx, "no C++ compiler (c++, g++ or clang++) on PATH"
    max_batch = re.search(r"^#define DOTS_MAX_BATCH (\d+)", (CSRC / "kernels.h").read_text(), re.M).group(1)
    exe = tmp_path / "spec_shaped_model"
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", f"-DDOTS_MAX_BATCH={max_batch}",
           f"-I{CSRC}", str(ROOT / "tests" / "spec_shaped_model.cpp"), "-o", str(exe)]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    # 3 rows x {alone, beside a full neighbour} x 2^5 feature subsets x {penalty, none} x 64 modes
    assert int(re.search(r"(\d+) cases", p.stdout).group(1)) == 3 * 2 * 32 * 2 * 64, p.stdout


def test_the_engine_derives_the_mode_in_one_place():
    rows = (CSRC / "rows.hip").read_text()
    stage = (CSRC / "row_stage.h").read_text()
    assert re.search(r"SPEC_ROWS_NGRAM = 8, SPEC_ROWS_RULES = 16, SPEC_ROWS_PENALTY = 32", stage)
    assert re.search(r"SPEC_ROWS_SAMPLED = 1, SPEC_ROWS_STOP = 2, SPEC_ROWS_ALL = 3, SPEC_ROWS_GUIDED = 4", stage)      # the existing values did not move
    assert len(re.findall(r"SPEC_ROWS_NGRAM", rows)) == 1 and "SPEC_ROWS_RULES" not in rows and "SPEC_ROWS_PENALTY" not in rows      # spec_row_class alone
    assert re.search(r"flags & ~SPEC_ROWS_ALL", rows)                  # dots_set_speculation_rows still refuses every other bit
    assert "history of rejected tokens" not in stage                   # the reason that did not hold is gone
    assert "history of rejected tokens" not in (ROOT / "DESIGN.md").read_text()


def test_the_launches_sit_behind_a_step_key_field():
    eng_h, eng = (CSRC / "engine.h").read_text(), (CSRC / "engine.hip").read_text()
    assert re.search(r"struct StepKey \{\s*int [^;]*\bsspec\b", eng_h)
    assert re.search(r"k\.sspec = spec_shapes\(e\);", eng)
    # the draft rows' ban kernel and the shaped selection are launched only under a guided or shaped speculating step
    body = eng[eng.index("int decode_step_launches("):eng.index("int splits_for_ctx(")]
    guard = body.index("if (spec_k && (sp.gstate || sspec))")
    assert guard < body.index("launch_ngram_ban_drafts(") < body.index("launch_spec_shape_select(") < body.index("RET(select_tokens(e, 1));")
    assert body.count("launch_ngram_ban_drafts(") == 1 and body.count("launch_spec_shape_select(") == 1


def test_one_definition_of_the_shaping_and_of_the_commit():
    """select_partial_kernel and the draft rows' kernel call one shape_logit, select_rows_kernel and the accept walk one commit_row"""
    dec, spec, hdr = ((CSRC / f).read_text() for f in ("decode.hip", "spec.hip", "select_dev.h"))
    for name in ("shape_logit", "commit_row", "penalise"):
        assert len(re.findall(rf"^DEVI \w+ {name}\(", hdr, re.M)) == 1
        assert not re.search(rf"^DEVI \w+ {name}\(", dec + spec, re.M)
    assert dec.count("shape_logit(row[i], i, sh, p)") == 2 and spec.count("shape_logit(row[i], i, sh, p)") == 1
    assert "penalise(" not in dec and "penalise(" not in spec
    assert "commit_row(st, rs, b, V, pen," in dec and "commit_row(st, rs, b, V, pen," in spec
    ng = (CSRC / "ngram.hip").read_text()
    assert len(re.findall(r"\bngram_ban_row\(g, g\.rows\[b\]", ng)) == 2          # the kernel of the step's rows and the draft rows' kernel


def test_the_new_kernels_use_no_scratch():
    build.build(force=not list((build.OBJ).glob("*.resusage.txt")), verbose=False)
    seen = {}
    for f in ("spec.hip", "ngram.hip", "decode.hip"):
        name = None
        for ln in (build.OBJ / (f + ".resusage.txt")).read_text().splitlines():
            m = re.search(r"Function Name: \S*?\d+([a-z_0-9]+_kernel)", ln)
            if m:
                name = m.group(1)
            m = re.search(r"(VGPRs Spill|SGPRs Spill|ScratchSize \[bytes/lane\]): (\d+)", ln)
            if m and name:
                seen.setdefault(name, []).append(int(m.group(2)))
    for k in ("ngram_ban_drafts_kernel", "ngram_ban_kernel", "spec_shape_select_kernel", "spec_guide_chain_kernel", "spec_accept_kernel", "spec_thresh_kernel",
              "spec_draw_kernel", "select_partial_kernel", "select_rows_kernel"):
        assert seen.get(k) == [0, 0, 0], (k, seen.get(k))


# ---------------------------------------------------------------------------------------------------- header, symbol, binding

def test_header_and_binding():
    from dots_ocr_amd import engine
    hdr = (ROOT / "include" / "dots_ocr_hip.h").read_text()
    assert re.search(r"^int dots_set_speculation_shaped\(DotsEngine\* e, int flags\);", hdr, re.M)
    for name, v in (("NGRAM", 1), ("RULES", 2), ("PENALTY", 4)):
        assert re.search(rf"^#define DOTS_SPEC_SHAPED_{name} {v}$", hdr, re.M)
    assert re.search(r"^int dots_set_speculation_rows\(DotsEngine\* e, int flags\);", hdr, re.M) and SPEC_ROWS == {"sampled": 1, "stop": 2}
    assert SPEC_SHAPED == {"ngram": 1, "rules": 2, "penalties": 4}
    assert "dots_set_speculation_shaped" in engine.EXPORTED_SYMBOLS
    src = Path(engine.__file__).read_text()
    assert re.search(r'"dots_set_speculation_shaped": \(i32, \[vp, i32\]\)', src)


def test_the_library_exports_the_symbol():
    from dots_ocr_amd import _lib
    build.build(verbose=False)
    assert hasattr(_lib.load(), "dots_set_speculation_shaped")


def test_flag_names():
    assert spec_shaped_flags(None) == spec_shaped_flags("") == spec_shaped_flags(False) == spec_shaped_flags(()) == 0
    assert spec_shaped_flags("all") == spec_shaped_flags(True) == 7
    assert spec_shaped_flags("ngram") == 1 and spec_shaped_flags("rules") == 2 and spec_shaped_flags("penalties") == 4
    assert spec_shaped_flags("ngram,penalties") == 5 and spec_shaped_flags("rules, ngram") == 3 and spec_shaped_flags(("rules", "penalties")) == 6
    for bad in ("penalty", "ngram,", "greedy", ("ngram", 3), "sampled"):
        with pytest.raises(ValueError, match="speculative_shaped"):
            spec_shaped_flags(bad)


# ---------------------------------------------------------------------------------------------------- Engine.set_speculation_shaped

class FakeLib:
    def __init__(self, rc=0):
        self.rc, self.calls = rc, []

    def dots_set_speculation_shaped(self, h, flags):
        self.calls.append((h, flags))
        return self.rc

    def dots_last_error(self, h):
        return b"shaped speculation cannot change while slot 0 is occupied"


def _engine(lib):
    e = object.__new__(Engine)                  # no library, no GPU
    e.lib, e.h = lib, 1234
    return e


def test_engine_method_passes_the_bits():
    lib = FakeLib()
    e = _engine(lib)
    assert e.spec_shaped == 0                   # the default, before any call
    e.set_speculation_shaped(ngram=True)
    e.set_speculation_shaped(rules=True, penalties=True)
    e.set_speculation_shaped(True, True, True)
    assert e.spec_shaped == 7
    e.set_speculation_shaped()
    assert lib.calls == [(1234, 1), (1234, 6), (1234, 7), (1234, 0)] and e.spec_shaped == 0
    e.h = None                                  # nothing for __del__ to destroy


def test_engine_method_raises_what_the_library_refuses():
    from dots_ocr_amd.engine import DotsEngineError
    e = _engine(FakeLib(rc=-3))
    with pytest.raises(DotsEngineError) as ei:
        e.set_speculation_shaped(ngram=True)
    assert "(-3)" in str(ei.value) and e.spec_shaped == 0               # the refused call changed nothing
    e.h = None


# ---------------------------------------------------------------------------------------------------- server flag

def _parse(*argv):
    from dots_ocr_amd.server import build_arg_parser
    return build_arg_parser().parse_args(list(argv))


def test_server_flag_is_off_by_default():
    from dots_ocr_amd.server import speculation_args
    assert _parse().speculative_shaped == ""
    a = _parse("--speculative-ngram", "3")
    assert a.speculative_shaped == "" and speculation_args(a) == (3, 2, 4)


def test_server_flag_parses_with_speculation_on():
    from dots_ocr_amd.server import speculation_args
    for value, flags in (("ngram", 1), ("rules", 2), ("penalties", 4), ("ngram,rules,penalties", 7), ("all", 7), ("penalties,ngram", 5)):
        a = _parse("--speculative-ngram", "3", "--speculative-shaped", value)
        assert speculation_args(a) == (3, 2, 4) and spec_shaped_flags(a.speculative_shaped) == flags
    a = _parse("--speculative-ngram", "3", "--speculative-rows", "sampled", "--speculative-guided", "--speculative-shaped", "all")
    assert a.speculative_guided is True and a.speculative_rows == "sampled" and speculation_args(a) == (3, 2, 4)


def test_server_flag_refusals():
    from dots_ocr_amd.server import speculation_args
    with pytest.raises(ValueError, match="--speculative-ngram"):
        speculation_args(_parse("--speculative-shaped", "ngram"))
    with pytest.raises(ValueError, match="--speculative-ngram"):
        speculation_args(_parse("--speculative-ngram", "0", "--speculative-shaped", "all"))
    for bad in ("penalty", "ngram;rules", "sampled", "ngram,,rules"):
        with pytest.raises(ValueError, match="--speculative-shaped"):
            speculation_args(_parse("--speculative-ngram", "3", "--speculative-shaped", bad))
        with pytest.raises(ValueError, match="--speculative-shaped"):
            speculation_args(_parse("--speculative-shaped", bad))


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
    assert m.generate(speculative_ngram=3, speculative_rows="all", speculative_guided=True) == "out"
    assert "set_speculation_shaped" not in [c[0] for c in m.engine.calls]


def test_generate_sets_and_clears_the_switch():
    m = _model()
    m.generate(speculative_ngram=3, speculative_shaped="ngram,penalties")
    names = [c[0] for c in m.engine.calls]
    assert [c[2] for c in m.engine.calls if c[0] == "set_speculation_shaped"] == [dict(ngram=True, rules=False, penalties=True), {}]
    assert names.index("slots_reset") < names.index("set_speculation") < names.index("set_speculation_shaped")      # while no slot is occupied
    m = _model()
    m.generate(speculative_ngram=3, speculative_shaped="all")
    assert [c[2] for c in m.engine.calls if c[0] == "set_speculation_shaped"][0] == dict(ngram=True, rules=True, penalties=True)


def test_generate_refuses_the_keyword_without_speculation():
    m = _model()
    with pytest.raises(ValueError, match="speculative_ngram"):
        m.generate(speculative_shaped="all")
    with pytest.raises(ValueError, match="speculative_shaped"):
        m.generate(speculative_ngram=3, speculative_shaped="penalty")
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
    p = _parser(speculative_ngram=3, speculative_shaped="ngram")
    with pytest.raises(StopIteration):
        p._inference_batch_with_hf([None], ["x"])
    assert p.model.kw["speculative_ngram"] == 3 and p.model.kw["speculative_shaped"] == "ngram"
    p = _parser(speculative_ngram=3)
    with pytest.raises(StopIteration):
        p._inference_batch_with_hf([None], ["x"])
    assert "speculative_shaped" not in p.model.kw                     # the default: the call is what it was


def test_parser_refuses_the_keyword_without_speculation():
    with pytest.raises(ValueError, match="speculative_ngram"):
        _parser(speculative_shaped="all")
    with pytest.raises(ValueError, match="speculative_shaped"):
        _parser(speculative_ngram=3, speculative_shaped="penalty")


# ---------------------------------------------------------------------------------------------------- what a draft row is selected under

def test_virtual_history_ban_by_hand():
    out = [7, 8, 9, 7, 8]                                             # L = 5
    drafts = [9, 7, 8]
    assert draft_row_history(out, drafts, 1) == [7, 8, 9, 7, 8, 9]
    assert draft_row_history(out, drafts, 3) == [7, 8, 9, 7, 8, 9, 7, 8]
    # row 0 (no draft): after ... 7 8 the bigram rule bans 9, the successor of the earlier 8
    assert banned_ngram_ids(out, 2) == {9}
    # draft row 1 takes 9 as committed: the last token is 9, its earlier successor is 7
    assert banned_ngram_ids(draft_row_history(out, drafts, 1), 2) == {7}
    # draft row 2: ... 9 7: 7 was followed by 8 twice
    assert banned_ngram_ids(draft_row_history(out, drafts, 2), 2) == {8}
    # draft row 3: ... 7 8: 8 was followed by 9 twice — the second time by a draft, which counts under the row's hypothesis
    assert banned_ngram_ids(draft_row_history(out, drafts, 3), 2) == {9}
    # n = 3: the pair (8, 9) occurred at 1 .. 2 followed by 7, and nothing else matches
    assert banned_ngram_ids(draft_row_history(out, drafts, 1), 3) == {7}
    assert banned_ngram_ids(out, 3) == {9}
    # a draft supplies a ban the output alone does not hold: 5 5 in the drafts bans 5 after the second 5
    assert banned_ngram_ids([1, 2], 2) == set() and banned_ngram_ids(draft_row_history([1, 2], [5, 5, 5], 2), 2) == {5}
    # the window slides with the virtual length: W = 3 at L + j = 7 reaches back to index 4
    assert banned_ngram_ids(draft_row_history(out, drafts, 2), 2, window=3) == set()
    assert banned_ngram_ids(draft_row_history(out, drafts, 3), 2, window=4) == {9}      # 8 9 at 4 .. 5 lies in [4, 8)
    assert banned_ngram_ids(draft_row_history(out, drafts, 3), 2, window=3) == set()
    # the whitelist holds for draft rows too
    assert banned_ngram_ids(draft_row_history(out, drafts, 3), 2, whitelist=(9,)) == set()
    for bad in (0, 4):
        with pytest.raises(ValueError):
            draft_row_history(out, drafts, bad)


def test_draft_adjusted_counts_by_hand():
    counts = {7: 2, 8: 2, 9: 1}
    drafts = [9, 9, 4]
    assert draft_row_counts(counts, drafts, 1) == {7: 2, 8: 2, 9: 2}
    assert draft_row_counts(counts, drafts, 2) == {7: 2, 8: 2, 9: 3}
    assert draft_row_counts(counts, drafts, 3) == {7: 2, 8: 2, 9: 3, 4: 1}
    assert counts == {7: 2, 8: 2, 9: 1}                               # the row's own counts do not move: a rejected draft leaves nothing
    # they are the counts of the virtual history
    out = [7, 8, 9, 7, 8]
    for j in (1, 2, 3):
        h = draft_row_history(out, drafts, j)
        assert draft_row_counts(counts, drafts, j) == {t: h.count(t) for t in set(h)}
    with pytest.raises(ValueError):
        draft_row_counts(counts, drafts, 0)
