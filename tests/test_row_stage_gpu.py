"""Stage membership across features: a row is in the per-row selection stage exactly while it carries own parameters, logit
rules, a guide, an n-gram rule or stop strings, in whatever order they come and go.

Every feature here is chosen so that it cannot change a greedy choice: parameters equal to greedy, one bias of 0.0, a one-state guide
that accepts every byte (every token of the test's table has bytes), an n-gram size above the number of tokens generated, a stop string
the output does not contain.  So whatever is attached to slot 1, in whatever order, both slots must repeat the greedy baseline token for
token; what the engine's counters say is read through the calls they gate (destroy_guide, destroy_stop, set_token_bytes).  One engine
serves the whole file."""
import ctypes as C

import numpy as np
import pytest

from dots_ocr_amd.config import DotsConfig
from dots_ocr_amd.engine import CDotsNgramRule, DotsEngineError, LogitRules, NgramRule, SamplingParams
from dots_ocr_amd.guided import Guide
from dots_ocr_amd.weights import random_state_dict

pytestmark = pytest.mark.gpu

V = 1024
CHUNK = 2
N_CHUNKS = 12                                    # 24 decode steps: 25 tokens with the prefill's
NGRAM_SIZE = 32                                  # > 25: no n-gram of this size is ever complete
FEATURES = ("params", "rules", "guide", "ngram", "stop")
E_STATE, E_INVALID = "(-3)", "(-1)"              # DOTS_E_STATE, DOTS_E_INVALID as DotsEngineError prints them


def _token_table():
    g = np.random.default_rng(31)
    return [bytes(g.choice(list(b"abc"), int(g.integers(1, 4))).astype(np.uint8)) for _ in range(V)]      # every token has bytes


TOKS = _token_table()
PROMPTS = [np.random.default_rng(900 + b).integers(0, V - 8, 7 + b).astype(np.int32) for b in range(2)]
ANY_BYTES = Guide(np.zeros((1, 256), np.uint16), np.ones((1,), np.uint8), 0, "(any bytes)")


def _start(e, slots=(0, 1)):
    e.set_sampling(0.0, 1.0, 0)
    e.slots_reset()
    e.set_eos([])
    e.slots_prefill(list(slots), np.concatenate([PROMPTS[s] for s in slots]), [len(PROMPTS[s]) for s in slots], [2 * CHUNK * N_CHUNKS] * len(slots))


def _chunk_and_compare(e, base, n_chunks, what):
    """one more chunk; both slots equal the baseline at every token so far"""
    e.slots_decode(CHUNK)
    n = 1 + CHUNK * n_chunks
    for s in (0, 1):
        assert e.slot_read(s, n).tolist() == base[s][:n], (what, s)


def _state_refused(call, *args):
    with pytest.raises(DotsEngineError) as ei:
        call(*args)
    assert E_STATE in str(ei.value), ei.value


def _handles(e, base):
    return dict(guide=e.create_guide(ANY_BYTES), stop=e.create_stop([base["stop"]]))


def _attach(e, row, f, h):
    if f == "params":
        e.set_row_sampling(row, SamplingParams())                  # temperature 0, top_p 1, top_k 0, no penalty
    elif f == "rules":
        e.set_row_logit_rules(row, LogitRules(bias={5: 0.0}))
    elif f == "guide":
        e.set_row_guide(row, h["guide"])
    elif f == "ngram":
        e.set_row_ngram(row, NgramRule(NGRAM_SIZE))
    else:
        e.set_row_stop(row, h["stop"], 0)


def _detach(e, row, f):
    {"params": e.set_row_sampling, "rules": e.set_row_logit_rules, "guide": e.set_row_guide, "ngram": e.set_row_ngram,
     "stop": e.set_row_stop}[f](row, None)


def _all_refused(e, h):
    _state_refused(e.destroy_guide, h["guide"])
    _state_refused(e.destroy_stop, h["stop"])
    _state_refused(e.set_token_bytes, TOKS)


def _all_succeed(e, h):
    e.destroy_guide(h["guide"])
    e.destroy_stop(h["stop"])
    e.set_token_bytes(TOKS)


@pytest.fixture(scope="module")
def eng():
    from dots_ocr_amd.engine import Engine
    cfg = DotsConfig.tiny(layers=2, v_layers=2, vocab=V)
    e = Engine(cfg, max_batch=4, max_seq_len=128, max_patches=256, max_prefill_tokens=256)
    e.load_state_dict(random_state_dict(cfg, seed=13))
    e.set_token_bytes(TOKS)
    yield e
    e.close()


@pytest.fixture(scope="module")
def base(eng):
    """the greedy baseline, computed once: two prompts in slots 0 and 1, nothing attached, 12 chunks of 2 steps; and a stop string over
    the table's own alphabet that slot 1's output does not contain"""
    _start(eng)
    for _ in range(N_CHUNKS):
        eng.slots_decode(CHUNK)
    n = 1 + CHUNK * N_CHUNKS
    toks = [eng.slot_read(s, n).tolist() for s in (0, 1)]
    eng.slots_reset()
    assert all(len(t) == n for t in toks) and toks[0] != toks[1]
    data = b"".join(TOKS[t] for t in toks[1])
    g = np.random.default_rng(32)
    stop = next(s for s in (bytes(g.choice(list(b"abc"), 12).astype(np.uint8)) for _ in range(8)) if s not in data)
    return {0: toks[0], 1: toks[1], "bytes": data, "stop": stop.decode()}


def test_the_neutral_features_rely_on_what_the_baseline_shows(base):
    assert len(base[1]) < NGRAM_SIZE                               # no 32-gram can be complete, so none can repeat
    assert base["stop"].encode() not in base["bytes"] and set(base["stop"]) <= set("abc")
    assert base["stop"][:1].encode() in base["bytes"]              # the automaton does leave its root on this output
    assert all(len(t) > 0 for t in TOKS)                           # the guide can allow every token


@pytest.mark.parametrize("reverse", [False, True], ids=["same_order", "reverse_order"])
@pytest.mark.parametrize("rot", range(5))
def test_neutral_features_in_any_order_change_no_token(eng, base, rot, reverse):
    e = eng
    on = FEATURES[rot:] + FEATURES[:rot]
    off = on[::-1] if reverse else on
    h = _handles(e, base)
    _start(e)
    chunks = 1
    _chunk_and_compare(e, base, chunks, "nothing attached")
    for f in on:
        _attach(e, 1, f, h)
        chunks += 1
        _chunk_and_compare(e, base, chunks, f"+{f} of {on}")
    _all_refused(e, h)                                             # slot 1 holds the guide and the automaton
    held = set(on)
    for f in off:
        _detach(e, 1, f)
        held.remove(f)
        chunks += 1
        _chunk_and_compare(e, base, chunks, f"-{f} of {off} after {on}")
        if held & {"guide", "stop"}:                               # either of the two still pins the token bytes
            _state_refused(e.set_token_bytes, TOKS)
    _all_succeed(e, h)                                             # nothing is held any more
    chunks += 1
    assert chunks == N_CHUNKS
    _chunk_and_compare(e, base, chunks, "everything detached")
    e.slots_reset()


@pytest.mark.parametrize("how", ["slot_release", "slots_reset"])
def test_release_and_reset_take_every_feature_off(eng, base, how):
    e = eng
    h = _handles(e, base)
    _start(e)
    for f in FEATURES:
        _attach(e, 1, f, h)
    _chunk_and_compare(e, base, 1, "everything attached")
    _all_refused(e, h)
    if how == "slot_release":
        e.slot_release(1)
    else:
        e.slots_reset()
    _all_succeed(e, h)
    # the row is back with the engine-wide stage: prefilled again with nothing attached it repeats the baseline
    h = _handles(e, base)
    _start(e)
    _chunk_and_compare(e, base, 1, f"after {how}")
    _all_succeed(e, h)
    e.slots_reset()


def test_forked_children_hold_the_automaton_until_the_last_is_released(eng, base):
    e = eng
    h = e.create_stop([base["stop"]])
    e.set_sampling(0.0, 1.0, 0)
    e.slots_reset()
    e.set_eos([])
    e.set_row_stop(0, h, 0)
    e.slots_prefill([0], PROMPTS[0], [len(PROMPTS[0])], [8])
    e.slots_fork(0, [1, 2])
    e.slots_decode(CHUNK)
    parent = e.slot_read(0, 1 + CHUNK).tolist()
    assert len(parent) == 1 + CHUNK and all(e.slot_read(s, 1 + CHUNK).tolist() == parent for s in (1, 2))      # greedy children of one prompt
    e.slot_release(0)
    e.slot_release(1)
    _state_refused(e.destroy_stop, h)
    _state_refused(e.set_token_bytes, TOKS)
    e.slot_release(2)
    e.destroy_stop(h)
    e.set_token_bytes(TOKS)
    e.slots_reset()


def test_a_refused_setter_changes_nothing(eng, base):
    e = eng
    gid = e.create_guide(ANY_BYTES)
    _start(e)
    _chunk_and_compare(e, base, 1, "nothing attached")
    e.set_row_guide(1, gid)
    _chunk_and_compare(e, base, 2, "+guide")

    def ngram_size_0():                                            # NgramRule refuses size 0 itself: the C struct, as a foreign caller would
        rule = CDotsNgramRule(0, 0, 0)
        e._ck(e.lib.dots_set_row_ngram(e.h, 1, C.byref(rule)), "dots_set_row_ngram")

    refused = [("bias id out of range", lambda: e.set_row_logit_rules(1, LogitRules(bias={V: 0.0}))),
               ("n-gram size 0", ngram_size_0),
               ("unknown guide", lambda: e.set_row_guide(1, 999)),
               ("unknown stop handle", lambda: e.set_row_stop(1, 999, 0))]
    for i, (what, call) in enumerate(refused):
        with pytest.raises(DotsEngineError) as ei:
            call()
        assert E_INVALID in str(ei.value), (what, ei.value)
        _state_refused(e.destroy_guide, gid)                       # still held: the refused call took nothing off either
        _chunk_and_compare(e, base, 3 + i, what)
    e.set_row_guide(1, None)
    e.destroy_guide(gid)
    _chunk_and_compare(e, base, 3 + len(refused), "guide cleared")
    e.slots_reset()
