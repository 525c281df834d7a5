"""Predicted outputs on the GPU: a speculating engine drafts from a caller-supplied prediction.  Every comparison is exact:
whatever the prediction holds, the row commits the tokens of the unspeculated engine, and the steps it takes and every counter are those
engine.predicted_run replays on the host.

`ref` is an engine that never speculates: its runs are computed once per request and shared.  `never` speculates and never sees a
prediction; `spec` speculates and takes them."""
import dataclasses

import numpy as np
import pytest

from dots_ocr_amd import guided as G
from dots_ocr_amd.config import DotsConfig
from dots_ocr_amd.engine import SamplingParams, predicted_draft, predicted_run
from dots_ocr_amd.weights import random_state_dict

pytestmark = pytest.mark.gpu

SEQ = 640
V = 1024
K, MIN_N, MAX_N = 3, 2, 4
P_LEN = 61          # the rows of the first speculating step straddle the 64-token page boundary
P_CAP = 43
P_SEED = 3
NO_BYTES = (3, 77, 500, 1001, 1023)


def _token_table():
    g = np.random.default_rng(20)
    toks = [bytes(g.choice(list(b"abc"), int(g.integers(1, 5))).astype(np.uint8)) for _ in range(V)]
    for t in NO_BYTES:
        toks[t] = b""
    return toks


TOKS = _token_table()
GUIDE = G.compile_regex(r"((abc|cab)b?)*")


def _engine(max_batch=16, kv_cache_dtype=None):
    from dots_ocr_amd.engine import Engine
    cfg = DotsConfig.tiny(layers=3, v_layers=3, vocab=V)
    e = Engine(cfg, max_batch=max_batch, max_seq_len=SEQ, max_patches=4096, max_prefill_tokens=2048, kv_cache_dtype=kv_cache_dtype)
    e.load_state_dict(random_state_dict(cfg, seed=11))
    e.set_token_bytes(TOKS)
    e.test_guide = None
    return e


def _prompt(seed, length=P_LEN):
    return np.random.default_rng(seed).integers(0, V - 8, length).astype(np.int32)


@dataclasses.dataclass(frozen=True)
class Row:
    """the features of one request (hashable: the key of the reference cache)"""
    lp: int = None
    sp: SamplingParams = None
    guide: bool = False
    stop: tuple = None                       # (strings, min_tokens)


def _setup_row(e, slot, row):
    if row.sp is not None:
        e.set_row_sampling(slot, row.sp)
    if row.guide:
        if e.test_guide is None:
            e.test_guide = e.create_guide(GUIDE)
        e.set_row_guide(slot, e.test_guide)
    if row.stop is not None:
        e.set_row_stop(slot, e.create_stop(list(row.stop[0])), row.stop[1])
    if row.lp is not None:
        e.set_row_logprobs(slot, row.lp)


def _fresh(e, k=K, min_n=MIN_N, max_n=MAX_N, sampled=False, stop=False, guided=False, lp=False):
    e.set_sampling(0.0, 1.0, 0)
    e.slots_reset()
    e.set_speculation(k, min_n, max_n)
    e.set_speculation_rows(sampled=sampled, stop=stop)
    e.set_speculation_guided(guided)
    e.set_speculation_logprobs(lp)
    e.set_eos([])


def _bits(lp):
    tok, ids, top = lp
    return tok.view(np.uint32).copy(), ids.copy(), top.view(np.uint32).copy()


def _run(e, prompts, caps, preds=None, rows=None, chunk=16):
    """prefill prompts into slots 0 .. (a prediction and the row's features set before the prefill, as the scheduler does), decode in
    chunks of `chunk` steps until every row has finished: per slot dict(toks, st, pst, lp, hit); the slots are released"""
    slots = list(range(len(prompts)))
    preds = preds or [None] * len(prompts)
    rows = rows or [Row()] * len(prompts)
    for s in slots:
        _setup_row(e, s, rows[s])
        if preds[s] is not None:
            e.set_row_prediction(s, preds[s])
    e.slots_prefill(slots, np.concatenate(prompts), [len(p) for p in prompts], caps)
    for _ in range(-(-max(caps) // chunk) + 1):
        fin, lens = e.slots_poll()
        if all(fin[s] == 1 for s in slots):
            break
        e.slots_decode(chunk)
    fin, lens = e.slots_poll()
    assert all(fin[s] == 1 for s in slots), (fin[:4], lens[:4])
    out = []
    for s in slots:
        out.append(dict(toks=e.slot_read(s, int(lens[s])).tolist(), st=e.spec_stats(s), pst=e.row_prediction_stats(s),
                        lp=_bits(e.row_logprobs(s, caps[s])) if rows[s].lp is not None else None,
                        hit=e.row_stop_hit(s) if rows[s].stop is not None else None))
    for s in slots:
        e.slot_release(s)
    return out


@pytest.fixture(scope="module")
def ref():
    """the unspeculated engine and its runs, keyed by the whole request; a run is computed once and never changed"""
    e = _engine()
    cache = {}

    def run(seed, cap=P_CAP, row=Row(), length=P_LEN):
        key = (seed, length, cap, row)
        if key not in cache:
            e.set_sampling(0.0, 1.0, 0)
            e.slots_reset()
            e.set_eos([])
            cache[key] = _run(e, [_prompt(seed, length)], [cap], rows=[row])[0]
        return cache[key]
    yield e, run
    e.close()


@pytest.fixture(scope="module")
def spec():
    e = _engine()
    yield e
    e.close()


@pytest.fixture(scope="module")
def never():
    """speculates, never sees a prediction: what own-output drafting alone does, keyed by (seeds, cap)"""
    e = _engine()
    cache = {}

    def run(seeds, cap=P_CAP, row=Row()):
        key = (tuple(seeds), cap, row)
        if key not in cache:
            _fresh(e, sampled=row.sp is not None)
            cache[key] = _run(e, [_prompt(s) for s in seeds], [cap] * len(seeds), rows=[row] * len(seeds))
        return cache[key]
    yield e, run
    e.close()


# ---------------------------------------------------------------------------------------------------- 1. the kernel equals the host rule

def _planted():
    """name -> (out, pred, cur, at); what each is meant to be is asserted for (k, min_n, max_n) = (3, 2, 4) below"""
    rng = np.random.default_rng(5)
    far = [int(t) for t in rng.integers(4, 1000, 4096)]             # P = 4096: the only match of the output's last 4 tokens ends at 3000,
    key = [1001, 1002, 1003, 1004]                                   # far past the workgroup's first stride
    far[2996:3000] = key
    return {
        "anchor_hit": ([1, 2, 3, 4], [1, 2, 3, 4, 5, 6, 7, 8], 0, 0),
        "anchor_miss_search": ([1, 2, 9, 4, 5], [1, 2, 3, 4, 5, 6, 7, 8], 0, 0),
        "tie_larger_e": ([7, 8], [7, 8, 20, 21, 7, 8, 30, 31], 4, 2),            # e* = 4: candidates 2 and 6, both two away
        "nearest_beats_farther": ([7, 8], [7, 8, 20, 21, 22, 23, 7, 8, 30, 7, 8, 40], 9, 2),   # e* = 9: candidates 2, 8, 11
        "e_star_past_P": ([5, 6, 7, 8, 9, 10], [5, 6, 7, 8], 0, 0),
        "fewer_than_k_left": ([1, 2, 3], [1, 2, 3, 4, 5], 0, 0),
        "empty_prediction": ([1, 2, 3], [], 0, 0),
        "L_below_min_n": ([1], [1, 2, 3], 0, 0),
        "L_below_min_n_miss": ([2], [1, 2, 3], 0, 0),
        "no_match": ([50, 51, 52], [1, 2, 3, 4, 5, 6], 1, 1),
        "far": ([9, 9] + key, far, 0, 0),
    }


@pytest.mark.parametrize("k,min_n,max_n", [(3, 2, 4), (15, 2, 4), (7, 1, 64)])
def test_kernel_equals_the_host_rule(spec, k, min_n, max_n):
    e = spec
    C = _planted()
    names = sorted(C)
    want = {nm: predicted_draft(*C[nm], k, min_n, max_n) for nm in names}
    for nm in names:                                                 # every case as a launch of its own, then all of them in one launch
        out, pred, cur, at = C[nm]
        assert e.predict_draft_op([pred], [out], [cur], [at], k, min_n, max_n) == [want[nm]], nm
    got = e.predict_draft_op([C[nm][1] for nm in names], [C[nm][0] for nm in names], [C[nm][2] for nm in names], [C[nm][3] for nm in names], k, min_n, max_n)
    assert got == [want[nm] for nm in names], [nm for nm, g in zip(names, got) if g != want[nm]]
    if (k, min_n, max_n) == (3, 2, 4):                              # the planted cases are what they are meant to be
        assert want["anchor_hit"] == ([5, 6, 7], 4, 4)
        assert want["anchor_miss_search"] == ([6, 7, 8], 5, 5)
        assert want["tie_larger_e"] == ([30, 31], 6, 2)
        assert want["nearest_beats_farther"] == ([30, 7, 8], 8, 2)
        assert want["e_star_past_P"] == (None, 0, 0)
        assert want["fewer_than_k_left"] == ([4, 5], 3, 3)
        assert want["empty_prediction"] == (None, 0, 0)
        assert want["L_below_min_n"] == ([2, 3], 1, 1) and want["L_below_min_n_miss"] == (None, 0, 0)
        assert want["no_match"] == (None, 1, 1)
        assert want["far"] == (C["far"][1][3000:3003], 3000, 6)


def test_kernel_on_random_rows(spec):
    """64 rows of different lengths and small alphabets (matches and ties everywhere) in one launch: drafts, cur and at"""
    e = spec
    rng = np.random.default_rng(22)
    outs = [[int(t) for t in rng.integers(0, 2 + b % 4, 1 + (37 * b) % 300)] for b in range(64)]
    preds = [[int(t) for t in rng.integers(0, 2 + b % 4, (53 * b) % 640)] for b in range(64)]
    ats = [int(rng.integers(0, len(o) + 1)) for o in outs]
    curs = [int(rng.integers(0, len(p) + 1)) for p in preds]
    for k, lo, hi in ((3, 2, 4), (15, 2, 4), (7, 1, 64)):
        want = [predicted_draft(o, p, c, a, k, lo, hi) for o, p, c, a in zip(outs, preds, curs, ats)]
        got = e.predict_draft_op(preds, outs, curs, ats, k, lo, hi)
        assert got == want, [b for b in range(64) if got[b] != want[b]]
        assert any(w[0] is None for w in want) and any(w[0] is not None for w in want)


# ---------------------------------------------------------------------------------------------------- 2. exactness end to end

def _variants(T):
    free = [t for t in range(V) if t not in T]
    sub = list(T)
    for i in range(6, len(T), 7):
        sub[i] = free[i]
    return {
        "perfect": list(T),
        "every_7th_replaced": sub,
        "span_deleted": T[:15] + T[20:],
        "one_inserted": T[:18] + [free[0]] + T[18:],
        "spans_swapped": T[:8] + T[24:32] + T[16:24] + T[8:16] + T[32:],
        "never_held": free[100:140],
        "empty": [],
    }


def _check_against_replay(got, T, pred, cap, what):
    want = predicted_run(T, pred, K, MIN_N, MAX_N, cap)
    assert got["toks"] == T, what
    assert got["st"] == {"steps": want["n_steps"], "drafted": want["drafted"], "accepted": want["accepted"]}, (what, got["st"], want)
    assert got["pst"] == {"drafted": want["pred_drafted"], "accepted": want["pred_accepted"]}, (what, got["pst"], want)
    return want


@pytest.mark.parametrize("name", ["perfect", "every_7th_replaced", "span_deleted", "one_inserted", "spans_swapped", "never_held", "empty"])
def test_exact_with_every_prediction(ref, spec, name):
    _, run = ref
    T = run(P_SEED)["toks"]
    assert len(T) == P_CAP
    pred = _variants(T)[name]
    got = {}
    for chunk in (1, 16):                                            # eager-sized chunks and the scheduler's captured 16 steps
        _fresh(spec)
        got[chunk] = _run(spec, [_prompt(P_SEED)], [P_CAP], preds=[pred], chunk=chunk)[0]
        want = _check_against_replay(got[chunk], T, pred, P_CAP, (name, chunk))
    assert got[1] == got[16]
    if name == "perfect":
        assert want["pred_accepted"] == P_CAP - want["n_steps"] - 1 and want["n_steps"] <= 1 + -(-(P_CAP - 2) // (K + 1))
    if name in ("never_held", "empty"):
        assert want["pred_drafted"] == 0


# ---------------------------------------------------------------------------------------------------- 3. it helps where it should

HELP_SEEDS = tuple(range(16))
HELP_CAP = 40
# A greedy row of the random tiny model falls into a short cycle within a few tokens: of the prompt seeds 0 .. 1499 none gives 40 greedy
# tokens without a repeated bigram.  The row is therefore a seeded sampled one, which speculates under set_speculation_rows(sampled) and
# whose tokens are as exact, per seed, as a greedy row's
HELP_ROW = Row(sp=SamplingParams(temperature=1.0, seed=4242))


def _has_repeated_bigram(T):
    grams = [tuple(T[i:i + 2]) for i in range(len(T) - 1)]
    return len(set(grams)) < len(grams)


def test_prediction_drafts_where_own_output_cannot(ref, spec, never):
    _, run = ref
    seed = next((s for s in HELP_SEEDS if not _has_repeated_bigram(run(s, HELP_CAP, HELP_ROW)["toks"])), None)
    assert seed is not None, "no seed of HELP_SEEDS gives 40 tokens without a repeated bigram: a test error, change the list"
    T = run(seed, HELP_CAP, HELP_ROW)["toks"]
    assert len(T) == HELP_CAP
    own = never[1]([seed], HELP_CAP, HELP_ROW)[0]
    assert own["toks"] == T and own["st"] == {"steps": HELP_CAP - 1, "drafted": 0, "accepted": 0}
    _fresh(spec, sampled=True)
    got = _run(spec, [_prompt(seed)], [HELP_CAP], preds=[T], rows=[HELP_ROW])[0]
    want = _check_against_replay(got, T, T, HELP_CAP, "perfect")
    assert got["st"]["steps"] == want["n_steps"] <= 1 + -(-(HELP_CAP - 2) // (K + 1))


# ---------------------------------------------------------------------------------------------------- 4. a mixed batch

def test_rows_without_a_prediction_draft_as_before(ref, spec, never):
    _, run = ref
    seeds = [3, 4, 5, 6]
    T = [run(s)["toks"] for s in seeds]
    base = never[1](seeds)
    _fresh(spec)
    got = _run(spec, [_prompt(s) for s in seeds], [P_CAP] * 4, preds=[T[0], None, T[2], None])
    for b in range(4):
        assert got[b]["toks"] == T[b] == base[b]["toks"], b
    for b in (1, 3):
        assert got[b]["st"] == base[b]["st"] and got[b]["pst"] == {"drafted": 0, "accepted": 0}, b
    for b in (0, 2):
        _check_against_replay(got[b], T[b], T[b], P_CAP, b)


# ---------------------------------------------------------------------------------------------------- 5. the other row classes

def _stop_row(T):
    s = (TOKS[T[20]] + TOKS[T[21]]).decode("ascii")
    assert s
    return Row(stop=((s,), 0))


@pytest.mark.parametrize("kind", ["sampled", "stop", "guided", "logprobs"])
def test_other_row_classes_stay_exact(ref, spec, kind):
    _, run = ref
    row = {"sampled": lambda: Row(sp=SamplingParams(temperature=0.8, top_k=40, seed=9003), lp=5),
           "stop": lambda: _stop_row(run(P_SEED)["toks"]),
           "guided": lambda: Row(guide=True, lp=3),
           "logprobs": lambda: Row(lp=20)}[kind]()
    want = run(P_SEED, P_CAP, row)
    _fresh(spec, sampled=kind == "sampled", stop=kind == "stop", guided=kind == "guided", lp=True)
    got = _run(spec, [_prompt(P_SEED)], [P_CAP], preds=[want["toks"]], rows=[row])[0]
    assert got["toks"] == want["toks"] and got["hit"] == want["hit"]
    if row.lp is not None:
        n = len(want["toks"])
        for g, w, what in zip(got["lp"], want["lp"], ("tok_lp", "top_ids", "top_lp")):
            assert (g[:n] == w[:n]).all(), (kind, what)
    assert got["pst"]["drafted"] >= got["pst"]["accepted"] > 0 and got["st"]["steps"] < len(want["toks"]) - 1      # it did speculate from the prediction


# ---------------------------------------------------------------------------------------------------- 6. lifecycle

def test_a_released_slot_holds_no_prediction(ref, spec, never):
    _, run = ref
    T = run(P_SEED)["toks"]
    _fresh(spec)
    first = _run(spec, [_prompt(P_SEED)], [P_CAP], preds=[T])[0]    # _run releases the slot
    assert first["pst"]["accepted"] > 0
    again = _run(spec, [_prompt(P_SEED)], [P_CAP])[0]
    assert again["toks"] == T and again["pst"] == {"drafted": 0, "accepted": 0} and again["st"] == never[1]([P_SEED])[0]["st"]


def test_clearing_mid_run_stops_prediction_drafts(ref, spec):
    _, run = ref
    T = run(P_SEED)["toks"]
    e = spec
    _fresh(e)
    e.set_row_prediction(0, T)
    e.slots_prefill([0], _prompt(P_SEED), [P_LEN], [P_CAP])
    e.slots_decode(3)
    mid = e.row_prediction_stats(0)
    assert mid["accepted"] > 0
    e.set_row_prediction(0, [])
    for _ in range(4):
        e.slots_decode(16)
    fin, lens = e.slots_poll()
    assert fin[0] == 1 and e.slot_read(0, int(lens[0])).tolist() == T
    assert e.row_prediction_stats(0) == mid
    e.slot_release(0)


def test_inert_without_speculation(ref, spec):
    _, run = ref
    T = run(P_SEED)["toks"]
    _fresh(spec, k=0)
    got = _run(spec, [_prompt(P_SEED)], [P_CAP], preds=[T])[0]
    assert got["toks"] == T and got["pst"] == {"drafted": 0, "accepted": 0} and got["st"] == {"steps": 0, "drafted": 0, "accepted": 0}


def test_setter_errors(spec):
    e = spec
    _fresh(e)
    assert e.lib.dots_set_row_prediction(e.h, 0, (np.ctypeslib.as_ctypes(np.asarray([V], np.int32))), 1) == -1       # DOTS_E_INVALID: an id outside the vocabulary
    too_long = np.zeros(SEQ + 1, np.int32)
    assert e.lib.dots_set_row_prediction(e.h, 0, np.ctypeslib.as_ctypes(too_long), SEQ + 1) == -4                  # DOTS_E_CAPACITY
    e.set_row_prediction(0, [0] * SEQ)                               # as long as a sequence can become: stored
    e.set_row_prediction(0, None)


# ---------------------------------------------------------------------------------------------------- 7. the fp8 KV pool

def test_exact_on_the_fp8_kv_pool():
    plain, e = _engine(16, "fp8"), _engine(16, "fp8")
    try:
        plain.set_sampling(0.0, 1.0, 0)
        plain.slots_reset()
        plain.set_eos([])
        T = _run(plain, [_prompt(P_SEED)], [P_CAP])[0]["toks"]
        pred = _variants(T)["every_7th_replaced"]
        _fresh(e)
        _check_against_replay(_run(e, [_prompt(P_SEED)], [P_CAP], preds=[pred])[0], T, pred, P_CAP, "fp8")
    finally:
        plain.close()
        e.close()
