"""The engine calls the scheduler makes for a request's per-row features (dots_ocr_amd/row_features.py), call for call, over a fake engine
that records them.  The expected traces were recorded from the seven hand-written blocks the feature table replaced and are not edited:
the table must reproduce every set, every clear and every release in the same order with the same arguments."""
import numpy as np
import pytest

from dots_ocr_amd.engine import LogitRules, NgramRule, SamplingParams
from dots_ocr_amd.scheduler import ContinuousBatcher, Request, RequestRejected
from test_parallel_sampling_cpu import ForkEngine

EOS = 9
STOP_HANDLE = 11
BAD_GUIDE = 13


def _plain(v):
    """an argument as the literal traces hold it"""
    if isinstance(v, SamplingParams):
        return ("SamplingParams", v.seed)
    if isinstance(v, LogitRules):
        return ("LogitRules", v.min_tokens)
    if isinstance(v, NgramRule):
        return ("NgramRule", v.size)
    if isinstance(v, (list, tuple, np.ndarray)):
        return tuple(_plain(x) for x in v)
    if isinstance(v, (bool, str)) or v is None:
        return v
    return int(v)


class RecordingEngine(ForkEngine):
    """ForkEngine + every per-row setter, recording each set_row_*, create_stop, slots_prefill, slots_fork and slot_release call with its
    arguments in `trace`.  set_row_guide refuses BAD_GUIDE; slots_prefill fails while `fail_prefill` is set."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.trace, self.streams, self.cursor, self.fail_prefill = [], set(), {}, False

    def _rec(self, name, *args):
        self.trace.append((name,) + tuple(_plain(a) for a in args))

    def set_row_sampling(self, *a):
        self._rec("set_row_sampling", *a)
        super().set_row_sampling(*a)

    def set_row_logprobs(self, *a):
        self._rec("set_row_logprobs", *a)

    def set_row_logit_rules(self, *a):
        self._rec("set_row_logit_rules", *a)

    def set_row_guide(self, *a):
        self._rec("set_row_guide", *a)
        if a[1] == BAD_GUIDE:
            raise RuntimeError("no such guide")

    def set_row_ngram(self, *a):
        self._rec("set_row_ngram", *a)

    def create_stop(self, *a):
        self._rec("create_stop", *a)
        return STOP_HANDLE

    def set_row_stop(self, *a):
        self._rec("set_row_stop", *a)

    def set_row_stream(self, *a):
        self._rec("set_row_stream", *a)
        self.streams.add(a[0]) if a[1] else self.streams.discard(a[0])

    def slots_drain(self):
        fin, lens = self.slots_poll()
        deltas = {}
        for s in sorted(self.streams & set(self.slots)):
            a, b = self.cursor.get(s, 0), len(self.slots[s]["out"])
            if b > a:
                deltas[s], self.cursor[s] = (np.asarray(self.slots[s]["out"][a:b], np.int32), None), b
        return fin, lens, deltas

    def row_logprobs(self, row, n, pos0=0):
        t = np.asarray(self.slots[row]["out"][pos0:pos0 + n], np.float32)
        return -t, np.zeros((len(t), 20), np.int32), np.zeros((len(t), 20), np.float32)

    def row_stop_hit(self, row):
        return None

    def slots_prefill(self, slots, ids, lens, caps):
        self._rec("slots_prefill", slots, lens, caps)
        if self.fail_prefill:
            raise RuntimeError("prefill failed")
        super().slots_prefill(slots, ids, lens, caps)

    def slots_fork(self, src, dst):
        self._rec("slots_fork", src, dst)
        super().slots_fork(src, dst)

    def slot_release(self, s):
        self._rec("slot_release", s)
        self.cursor.pop(s, None)
        super().slot_release(s)


def _script(prompt):
    """a prompt of 2s runs to its cap; any other ends after three tokens"""
    return [20] * 64 if prompt[0] == 2 else [int(prompt[0]) + 10] * 3 + [EOS]


def _batcher(max_batch):
    eng = RecordingEngine(_script, 64, max_batch=max_batch, max_prefill_tokens=1024, max_seq_len=1024)
    return eng, ContinuousBatcher(eng, eos_ids=[EOS])


def _req(first, cap=40, **kw):
    return Request(np.full(5, first, np.int32), max_new_tokens=cap, **kw)


def _all_seven(first, streamed, **kw):
    return _req(first, sampling=SamplingParams(temperature=0.8, seed=5), logprobs=3, rules=LogitRules(min_tokens=2), guide=7, ngram=NgramRule(2),
                stop=("ab",), stream=lambda rid, index, toks, lp, fin: streamed.append((index, [int(t) for t in toks], bool(fin))), **kw)


# (a) two slots: A carries all seven features, B none, C reuses A's slot with an n-gram rule only
TRACE_A = [
    ("set_row_sampling", 0, ("SamplingParams", 5)),
    ("set_row_logprobs", 0, 3),
    ("set_row_logit_rules", 0, ("LogitRules", 2)),
    ("set_row_guide", 0, 7),
    ("set_row_ngram", 0, ("NgramRule", 2)),
    ("create_stop", ("ab",)),
    ("set_row_stop", 0, 11, 2),
    ("set_row_stream", 0, True),
    ("slots_prefill", (0, 1), (5, 5), (40, 40)),
    ("set_row_ngram", 0, None),
    ("slot_release", 0),
    ("set_row_sampling", 0, None),
    ("set_row_logprobs", 0, None),
    ("set_row_logit_rules", 0, None),
    ("set_row_ngram", 0, ("NgramRule", 3)),
    ("slots_prefill", (0,), (5,), (40,)),
    ("set_row_ngram", 0, None),
    ("slot_release", 0),
    ("slot_release", 1),
]

# (b) a request whose set_row_guide raises is rejected alone and its rows cleared; the rest of its group is admitted
TRACE_B = [
    ("set_row_sampling", 0, ("SamplingParams", 5)),
    ("set_row_logprobs", 0, 2),
    ("set_row_guide", 0, 13),
    ("set_row_sampling", 0, None),
    ("set_row_logprobs", 0, None),
    ("set_row_guide", 0, None),
    ("set_row_logit_rules", 1, ("LogitRules", 1)),
    ("slots_prefill", (1,), (5,), (40,)),
    ("slot_release", 1),
]

# (c) slots_prefill raises: every row of the group is cleared
TRACE_C = [
    ("set_row_sampling", 0, ("SamplingParams", 5)),
    ("set_row_stream", 0, True),
    ("set_row_logprobs", 1, 0),
    ("create_stop", ("ab", "c")),
    ("set_row_stop", 1, 11, 0),
    ("set_row_logprobs", 2, 0),
    ("create_stop", ("ab", "c")),
    ("set_row_stop", 2, 11, 0),
    ("slots_prefill", (0, 1), (5, 5), (40, 40)),
    ("set_row_sampling", 0, None),
    ("set_row_stream", 0, False),
    ("set_row_logprobs", 1, None),
    ("set_row_stop", 1, None),
    ("set_row_logprobs", 2, None),
    ("set_row_stop", 2, None),
]

# (d) cancel of a running request that carries all seven features
TRACE_D = [
    ("set_row_sampling", 0, ("SamplingParams", 5)),
    ("set_row_logprobs", 0, 3),
    ("set_row_logit_rules", 0, ("LogitRules", 2)),
    ("set_row_guide", 0, 7),
    ("set_row_ngram", 0, ("NgramRule", 2)),
    ("create_stop", ("ab",)),
    ("set_row_stop", 0, 11, 2),
    ("set_row_stream", 0, True),
    ("slots_prefill", (0,), (5,), (40,)),
    ("slot_release", 0),
    ("set_row_sampling", 0, None),
    ("set_row_logprobs", 0, None),
    ("set_row_logit_rules", 0, None),
    ("set_row_ngram", 0, None),
    ("set_row_stream", 0, False),
]

# (e) n = 3 with seed 7: the kids are set with 8 and 9
TRACE_E = [
    ("set_row_sampling", 0, ("SamplingParams", 7)),
    ("set_row_sampling", 1, ("SamplingParams", 8)),
    ("set_row_sampling", 2, ("SamplingParams", 9)),
    ("slots_prefill", (0,), (5,), (40,)),
    ("slots_fork", 0, (1, 2)),
    ("slot_release", 0),
    ("slot_release", 1),
    ("slot_release", 2),
]


def scenario_a():
    eng, cb = _batcher(2)
    streamed = []
    a, b, c = _all_seven(1, streamed), _req(2), _req(3, ngram=NgramRule(3))
    outs = cb.run([a, b, c])
    assert [len(o) for o in outs] == [4, 40, 4] and a.logprobs_out is not None and a.stop_hit is None
    assert [t for _, toks, _ in streamed for t in toks] == outs[0].tolist() and streamed[-1][2]
    return eng.trace


def scenario_b():
    eng, cb = _batcher(3)
    bad = _req(1, sampling=SamplingParams(temperature=0.8, seed=5), logprobs=2, guide=BAD_GUIDE, ngram=NgramRule(2))
    good = _req(3, rules=LogitRules(min_tokens=1))
    ids = [cb.submit(bad), cb.submit(good)]
    done = {}
    while not cb.idle:
        for rid, r, toks in cb.step():
            done[rid] = (r, toks)
    assert isinstance(bad.error, RequestRejected) and str(bad.error) == "no such guide" and len(done[ids[0]][1]) == 0
    assert len(done[ids[1]][1]) == 4 and getattr(good, "error", None) is None
    return eng.trace


def scenario_c():
    eng, cb = _batcher(3)
    streamed = []
    cb.submit(_req(1, sampling=SamplingParams(temperature=0.8, seed=5), stream=lambda *a: streamed.append(a)))
    cb.submit(_req(3, logprobs=0, stop=("ab", "c"), n=2))
    eng.fail_prefill = True
    with pytest.raises(RuntimeError, match="prefill failed"):
        cb.step()
    assert len(cb.pending) == 2 and not cb.running and not eng.slots and not streamed
    return eng.trace


def scenario_d():
    eng, cb = _batcher(2)
    streamed = []
    r = _all_seven(2, streamed)
    rid = cb.submit(r)
    assert cb.step() == [] and cb.running
    assert cb.cancel(rid)
    (got, req, toks), = cb.step()
    assert got == rid and req is r and r.cancelled and len(toks) == 17 and cb.idle and not eng.slots
    return eng.trace


def scenario_e():
    eng, cb = _batcher(4)
    r = _req(1, sampling=SamplingParams(temperature=0.8, seed=7), n=3)
    cb.run([r])
    assert [len(o) for o in r.outputs] == [4, 4, 4]
    return eng.trace


SCENARIOS = {"a": (scenario_a, TRACE_A), "b": (scenario_b, TRACE_B), "c": (scenario_c, TRACE_C), "d": (scenario_d, TRACE_D),
             "e": (scenario_e, TRACE_E)}


@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_the_engine_sees_the_calls_it_saw_before_the_table(name):
    run, want = SCENARIOS[name]
    assert run() == want
