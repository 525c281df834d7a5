"""Speculative decoding of rows that return logprobs (dots_set_speculation_logprobs), the parts that need no GPU: the server's
--speculative-logprobs flag, the generate() / DotsOCRParser keywords, Engine.set_speculation_logprobs against a fake library, the C-ABI
declaration, and the places of the engine source that decide a logprob row's class and what a step launches for it."""
import re
from pathlib import Path

import pytest

from dots_ocr_amd.engine import Engine

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "dots_ocr_amd" / "csrc"


# ---------------------------------------------------------------------------------------------------- server flag

def _parse(*argv):
    from dots_ocr_amd.server import build_arg_parser
    return build_arg_parser().parse_args(list(argv))


def test_server_flag_is_off_by_default():
    from dots_ocr_amd.server import speculation_args
    assert _parse().speculative_logprobs is False
    a = _parse("--speculative-ngram", "3")
    assert a.speculative_logprobs is False and speculation_args(a) == (3, 2, 4)


def test_server_flag_parses_with_speculation_on():
    from dots_ocr_amd.server import speculation_args
    a = _parse("--speculative-ngram", "3", "--speculative-logprobs")
    assert a.speculative_logprobs is True and a.speculative_rows == "greedy" and a.speculative_guided is False
    assert speculation_args(a) == (3, 2, 4)
    a = _parse("--speculative-ngram", "7", "--speculative-rows", "all", "--speculative-guided", "--speculative-shaped", "all", "--speculative-logprobs")
    assert a.speculative_logprobs is True and a.speculative_guided is True and speculation_args(a) == (7, 2, 4)


def test_server_flag_without_speculation_is_an_error():
    from dots_ocr_amd.server import speculation_args
    with pytest.raises(ValueError, match="--speculative-logprobs needs --speculative-ngram"):
        speculation_args(_parse("--speculative-logprobs"))
    with pytest.raises(ValueError, match="--speculative-ngram"):
        speculation_args(_parse("--speculative-ngram", "0", "--speculative-logprobs"))


def test_server_main_switches_the_engine_on_only_with_the_flag():
    """main hands the flag to Engine.speculation_on and touches the switch nowhere else; speculation_on calls the setter only when it is set"""
    src = (ROOT / "dots_ocr_amd" / "server.py").read_text()
    assert re.search(r"Engine\.speculation_on\(model\.engine, \*spec,[^\n]*\n[^\n]*\blogprobs=a\.speculative_logprobs\b", src)
    assert "set_speculation_logprobs" not in src
    for flag, calls in ((False, []), (True, [(True,)])):
        e = RecEngine()
        Engine.speculation_on(e, 3, 2, 4, logprobs=flag)
        assert [c[1] for c in e.calls if c[0] == "set_speculation_logprobs"] == calls
        assert [c[1] for c in e.calls if c[0] == "set_speculation"] == [(3, 2, 4)]


# ---------------------------------------------------------------------------------------------------- Engine.set_speculation_logprobs

class FakeLib:
    def __init__(self, rc=0):
        self.rc, self.calls = rc, []

    def dots_set_speculation_logprobs(self, h, on):
        self.calls.append((h, on))
        return self.rc

    def dots_last_error(self, h):
        return b"logprob speculation cannot change while slot 0 is occupied"


def _engine(lib):
    e = object.__new__(Engine)                  # no library, no GPU
    e.lib, e.h = lib, 1234
    return e


def test_engine_method_passes_the_switch():
    lib = FakeLib()
    e = _engine(lib)
    assert e.spec_logprobs is False             # the default, before any call
    e.set_speculation_logprobs()
    assert e.spec_logprobs is True
    e.set_speculation_logprobs(False)
    assert e.spec_logprobs is False
    e.set_speculation_logprobs(on=1)
    assert lib.calls == [(1234, 1), (1234, 0), (1234, 1)] and e.spec_logprobs is True
    e.h = None                                  # nothing for __del__ to destroy


def test_engine_method_raises_what_the_library_refuses():
    from dots_ocr_amd.engine import DotsEngineError
    e = _engine(FakeLib(rc=-3))
    with pytest.raises(DotsEngineError) as ei:
        e.set_speculation_logprobs(True)
    assert "(-3)" in str(ei.value) and e.spec_logprobs is False        # the refused call changed nothing
    e.h = None


def test_header_and_binding():
    from dots_ocr_amd import engine
    hdr = (ROOT / "include" / "dots_ocr_hip.h").read_text()
    assert re.search(r"^int dots_set_speculation_logprobs\(DotsEngine\* e, int on\);", hdr, re.M)
    assert re.search(r"^int dots_set_speculation_guided\(DotsEngine\* e, int on\);", hdr, re.M)       # the neighbours are what they were
    assert re.search(r"^int dots_set_speculation_rows\(DotsEngine\* e, int flags\);", hdr, re.M)
    assert "dots_set_speculation_logprobs" in engine.EXPORTED_SYMBOLS
    src = Path(engine.__file__).read_text()
    assert re.search(r'"dots_set_speculation_logprobs": \(i32, \[vp, i32\]\)', src)
    assert "logprobs always decode one token per step" not in hdr and "Rows with logprobs, and every row" not in hdr


# ---------------------------------------------------------------------------------------------------- the engine source

def test_the_class_of_a_logprob_row_is_decided_in_one_place():
    rows = (CSRC / "rows.hip").read_text()
    body = re.search(r"int spec_row_class\(const DotsEngine\* e, int row\) \{(.*?)\n\}", rows, re.S).group(1)
    assert "e->row_lp[row] >= 0 && !e->spec_logprobs" in body           # NONE only while the switch is off
    # nothing else asks about the switch but the launch predicate and the setter
    uses = [m.start() for m in re.finditer(r"e->spec_logprobs", rows)]
    assert len(uses) == 4, len(uses)                                     # the class, spec_lps, and the setter's compare and store
    setter = re.search(r"int dots_set_speculation_logprobs\(DotsEngine\* e, int on\) \{(.*?)\n\}", rows, re.S).group(1)
    assert "DOTS_E_STATE" in setter and "drop_step_graphs(e)" in setter and "upload_spec_classes(e)" in setter
    assert setter.index("drop_step_graphs(e)") < setter.index("upload_spec_classes(e)")
    create = (CSRC / "engine.hip").read_text()
    assert "sp_acc_tok" not in create                                    # dots_create allocates no accept record: the first switch-on does


def test_a_step_launches_the_draft_row_pair_only_under_the_switch_with_a_logprob_row():
    rows = (CSRC / "rows.hip").read_text()
    pred = re.search(r"bool spec_lps\(const DotsEngine\* e\) \{(.*?)\n\}", rows, re.S).group(1)
    assert "e->spec_k > 0" in pred and "e->spec_logprobs" in pred and "e->n_lp > 0" in pred
    eng = (CSRC / "engine.hip").read_text()
    assert re.search(r"const bool lpspec = spec_k && spec_lps\(e\);", eng)
    assert re.search(r"if \(lpspec\) \{[^}]*launch_spec_logprob_partial", eng, re.S)
    assert re.search(r"if \(lpspec\) CK\(launch_spec_logprob_final", eng)
    assert len(re.findall(r"launch_spec_logprob_(partial|final)\(", eng)) == 2
    # order: the partials before the selection stage, the entries after the accept walk
    i_part, i_sel = eng.index("launch_spec_logprob_partial("), eng.index("RET(select_tokens(e, 1));")
    i_acc, i_fin = eng.index("launch_spec_accept("), eng.index("launch_spec_logprob_final(")
    assert i_part < i_sel < i_acc < i_fin
    assert re.search(r"k\.lpspec = spec_lps\(e\);", eng)                 # the captured-step key tells the two steps apart
    # the accept record reaches the kernels only then
    assert re.search(r"spec_lps\(e\) \? e->sp_acc_n : nullptr, spec_lps\(e\) \? e->sp_acc_tok : nullptr", rows)


def test_the_partial_pass_has_one_definition():
    dev = (CSRC / "logprobs_dev.h").read_text()
    lp = (CSRC / "logprobs.hip").read_text()
    assert len(re.findall(r"DEVI void lp_partial_chunk\(", dev)) == 1
    assert len(re.findall(r"lp_partial_chunk\(L, ", lp)) == 2            # logprob_partial_kernel and the draft-row kernel call it
    assert len(re.findall(r"lp_final_entry\(l, ", lp)) == 2
    assert "expf" not in lp and "lp_wave_best" not in lp                 # no second copy of the arithmetic beside the shared functions


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
    assert "set_speculation_logprobs" not in [c[0] for c in m.engine.calls]


def test_generate_sets_and_clears_the_switch():
    m = _model()
    assert m.generate(speculative_ngram=3, speculative_logprobs=True) == "out"
    names = [c[0] for c in m.engine.calls]
    assert [c[1] for c in m.engine.calls if c[0] == "set_speculation_logprobs"] == [(True,), (False,)]
    assert names.index("slots_reset") < names.index("set_speculation") < names.index("set_speculation_logprobs")      # while no slot is occupied
    assert "set_speculation_rows" not in names and "set_speculation_guided" not in names
    off = [i for i, c in enumerate(m.engine.calls) if c[0] == "set_speculation" and c[1] == (0,)]
    assert off and off[-1] < len(names) - 1 - names[::-1].index("set_speculation_logprobs")      # cleared after speculation went off


def test_generate_refuses_the_keyword_without_speculation():
    m = _model()
    with pytest.raises(ValueError, match="speculative_logprobs needs speculative_ngram"):
        m.generate(speculative_logprobs=True)
    with pytest.raises(ValueError, match="speculative_ngram"):
        m.generate(speculative_ngram=0, speculative_logprobs=True)
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
    p = _parser(speculative_ngram=3, speculative_logprobs=True)
    with pytest.raises(StopIteration):
        p._inference_batch_with_hf([None], ["x"])
    assert p.model.kw["speculative_ngram"] == 3 and p.model.kw["speculative_logprobs"] is True
    p = _parser(speculative_ngram=3)
    with pytest.raises(StopIteration):
        p._inference_batch_with_hf([None], ["x"])
    assert "speculative_logprobs" not in p.model.kw                   # the default: the call is what it was


def test_parser_refuses_the_keyword_without_speculation():
    with pytest.raises(ValueError, match="speculative_logprobs needs speculative_ngram"):
        _parser(speculative_logprobs=True)


# ---------------------------------------------------------------------------------------------------- the scheduler over a fake engine

def test_the_scheduler_asks_nothing_new_of_a_fake_engine():
    """a request with logprobs runs through the ContinuousBatcher over a fake engine that carries the switch: the scheduler itself never
    touches it (the server or generate() set it, engine-wide, before any slot is occupied)"""
    import numpy as np
    from fakes import FakeSlotEngine
    from dots_ocr_amd.scheduler import ContinuousBatcher, Request

    class FakeSpecLpEngine(FakeSlotEngine):
        spec_logprobs = False

        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            self.switch_calls = []

        def set_speculation_logprobs(self, on=True):
            self.switch_calls.append(bool(on))
            self.spec_logprobs = bool(on)

        def set_row_logprobs(self, row, top_n):
            pass

        def row_logprobs(self, row, n, pos0=0):
            return np.zeros((n,), np.float32), np.zeros((n, 20), np.int32), np.zeros((n, 20), np.float32)

    e = FakeSpecLpEngine(lambda p: [int(p[0]) + i for i in range(1, 9)])
    e.set_speculation_logprobs(True)
    cb = ContinuousBatcher(e, eos_ids=[], chunk=4)
    reqs = [Request(np.asarray([10, 11], np.int32), max_new_tokens=5, logprobs=2), Request(np.asarray([20], np.int32), max_new_tokens=3)]
    outs = cb.run(reqs)
    assert [o.tolist() for o in outs] == [[11, 12, 13, 14, 15], [21, 22, 23]]
    assert e.switch_calls == [True] and e.spec_logprobs is True
