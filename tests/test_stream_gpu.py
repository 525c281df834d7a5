"""Streaming on the GPU: Engine.set_row_stream / Engine.slots_drain against the per-row reads they replace.

The test owns the token-byte table (1 to 4 bytes over {a, b, c}, a few ids without bytes) and samples rows at temperature 1 under fixed
seeds, as tests/test_stop_strings_gpu.py does: a row's tokens depend on nothing but its prompt and seed.  Every assertion on tokens is
exact, every assertion on logprobs compares bits."""
import numpy as np
import pytest

from dots_ocr_amd.config import DotsConfig
from dots_ocr_amd.engine import STREAM_ROW_CAP, DotsEngineError, SamplingParams
from dots_ocr_amd.stop_strings import first_stop
from dots_ocr_amd.weights import random_state_dict

pytestmark = pytest.mark.gpu

V = 1024
NO_BYTES = (3, 77, 500, 1001, 1023)
SEED = 5200
SEQ = 640


def _token_table():
    g = np.random.default_rng(20)
    toks = [bytes(g.choice(list(b"abc"), int(g.integers(1, 5))).astype(np.uint8)) for _ in range(V)]
    for t in NO_BYTES:
        toks[t] = b""
    return toks


TOKS = _token_table()


def _prompt(seed):
    g = np.random.default_rng(seed)
    return g.integers(0, V - 8, 6 + seed % 4).astype(np.int32)


def _sp(seed):
    return SamplingParams(temperature=1.0, seed=seed)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same_lp(a, b):
    return all(x.shape == y.shape and np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))


@pytest.fixture(scope="module")
def eng():
    from dots_ocr_amd.engine import Engine
    cfg = DotsConfig.tiny(layers=3, v_layers=3, vocab=V)
    e = Engine(cfg, max_batch=8, max_seq_len=SEQ, max_patches=4096, max_prefill_tokens=2048)
    e.load_state_dict(random_state_dict(cfg, seed=11))
    e.set_token_bytes(TOKS)
    yield e
    e.close()


def _start(e):
    e.set_sampling(0.0, 1.0, 0)
    e.slots_reset()
    e.set_eos([])


def _plain(e, prompt, cap, seed=None, slot=0, chunk=16):
    """an undisturbed, unstreamed run of one row: its tokens"""
    _start(e)
    if seed is not None:
        e.set_row_sampling(slot, _sp(seed))
    e.slots_prefill([slot], prompt, [len(prompt)], [cap])
    for _ in range(-(-cap // chunk)):
        e.slots_decode(chunk)
    fin, lens = e.slots_poll()
    assert fin[slot] == 1
    toks = e.slot_read(slot, int(lens[slot])).tolist()
    e.slot_release(slot)
    return toks


class Tracker:
    """what the drains delivered per slot, checked against the per-row reads at every drain"""

    def __init__(self, e, streaming, lp=()):
        self.e, self.streaming, self.lp = e, set(streaming), set(lp)
        self.toks = {s: [] for s in streaming}
        self.lps = {s: [] for s in lp}

    def drain(self, occupied):
        e = self.e
        fin, lens, deltas = e.slots_drain()
        fin2, lens2 = e.slots_poll()
        assert np.array_equal(fin, fin2) and np.array_equal(lens, lens2)
        assert set(deltas) <= self.streaming
        for s in occupied:
            if s not in self.streaming:
                assert s not in deltas
                continue
            prev, n = len(self.toks[s]), int(lens[s])
            want = e.slot_read(s, n)[prev:min(n, prev + STREAM_ROW_CAP)].tolist()
            got, entries = deltas.get(s, (np.zeros((0,), np.int32), None))
            assert got.dtype == np.int32 and got.tolist() == want, (s, prev, n)
            self.toks[s] += want
            if s in self.lp and want:
                assert entries is not None
                ref = e.row_logprobs(s, len(want), pos0=prev)
                assert _same_lp(entries, ref), s
                self.lps[s].append(entries)
            else:
                assert entries is None
        return fin, lens, deltas


def test_drain_equals_read(eng):
    e = eng
    _start(e)
    slots, caps = [0, 2, 3, 5], [7, 20, 33, 48]
    prompts = [_prompt(900 + i) for i in range(4)]
    e.set_row_sampling(2, _sp(SEED))
    e.set_row_sampling(3, _sp(SEED + 1))
    e.set_row_logprobs(5, 3)
    for s in (0, 2, 5):                                     # slot 3 does not stream
        e.set_row_stream(s, True)
    e.slots_prefill(slots, np.concatenate(prompts), [len(p) for p in prompts], caps)
    t = Tracker(e, (0, 2, 5), lp=(5,))
    fin, lens, deltas = t.drain(slots)
    assert sorted(deltas) == [0, 2, 5] and all(len(deltas[s][0]) == 1 for s in deltas)      # the first token, before any decode
    done_at = {}
    for i in range(40):
        chunk = (1, 16, 5)[i % 3]
        e.slots_decode(chunk)
        fin, lens, deltas = t.drain(slots)
        for s in (0, 2, 5):
            assert len(t.toks[s]) == int(lens[s])                                              # nothing left behind a drain
            if fin[s] == 1 and s not in done_at:
                done_at[s] = i
                assert s in deltas                                                             # its last tokens come with the report
            elif s in done_at:
                assert s not in deltas
        if all(fin[s] == 1 for s in slots):
            break
    assert all(fin[s] == 1 for s in slots)
    e.slots_decode(3)
    assert t.drain(slots)[2] == {}
    for s, cap in zip(slots, caps):
        if s != 3:
            assert t.toks[s] == e.slot_read(s, cap).tolist() and len(t.toks[s]) == cap
    whole = e.row_logprobs(5, 48)
    got = tuple(np.concatenate([d[k] for d in t.lps[5]]) for k in range(3))
    assert _same_lp(got, whole)
    assert np.array_equal(got[1][:, 3:], np.full((48, 17), -1, np.int32)) and (got[1][:, :3] >= 0).all()
    assert len(set(t.toks[2])) > 8                                                             # the sampled output does vary
    for s in slots:
        e.slot_release(s)


def test_nothing_is_lost_behind_the_cap(eng):
    e = eng
    n = STREAM_ROW_CAP + 44
    _start(e)
    e.set_row_sampling(1, _sp(SEED + 7))
    e.set_row_stream(1, True)
    p = _prompt(911)
    e.slots_prefill([1], p, [len(p)], [n])
    for _ in range(-(-n // 16)):
        e.slots_decode(16)
    t = Tracker(e, (1,))
    fin, lens, deltas = t.drain([1])
    assert fin[1] == 1 and lens[1] == n and len(deltas[1][0]) == STREAM_ROW_CAP
    fin, lens, deltas = t.drain([1])
    assert len(deltas[1][0]) == 44
    assert t.drain([1])[2] == {}
    assert t.toks[1] == e.slot_read(1, n).tolist()
    e.slot_release(1)


def test_speculating_engine(eng):
    """accepted drafts as tests/test_spec_gpu.py obtains them: no built-in drafter (max_n = 0), the host plants the true continuation"""
    e = eng
    p, cap = _prompt(921), 30
    T = _plain(e, p, cap)
    _start(e)
    e.set_speculation(3, 2, 0)
    try:
        e.set_row_stream(0, True)
        e.slots_prefill([0], p, [len(p)], [cap])
        t = Tracker(e, (0,))
        t.drain([0])
        grew = []
        for step in range(cap):
            L = len(t.toks[0])
            if L >= cap:
                break
            e.set_row_drafts(0, T[L:L + 3] if step % 2 == 0 else [])
            e.slots_decode(1)
            fin, lens, _ = t.drain([0])
            grew.append(len(t.toks[0]) - L)
        assert max(grew) > 1                                                                   # a chunk grew the row by more than its steps
        assert fin[0] == 1 and t.toks[0] == T == e.slot_read(0, cap).tolist()
        e.slot_release(0)
    finally:
        e.slots_reset()
        e.set_speculation(0)


def test_fork_children_stream_their_own_tokens(eng):
    e = eng
    _start(e)
    p, cap = _prompt(931), 24
    for i, s in enumerate((0, 1, 2)):
        e.set_row_sampling(s, _sp(SEED + 20 + i))
        e.set_row_stream(s, True)
    e.slots_prefill([0], p, [len(p)], [cap])
    e.slots_fork(0, [1, 2])
    t = Tracker(e, (0, 1, 2))
    _, _, deltas = t.drain([0, 1, 2])
    assert sorted(deltas) == [0, 1, 2] and all(len(d[0]) == 1 for d in deltas.values())
    for chunk in (16, 5, 16):
        e.slots_decode(chunk)
        fin, lens, _ = t.drain([0, 1, 2])
    assert all(fin[s] == 1 for s in (0, 1, 2))
    reads = [e.slot_read(s, cap).tolist() for s in (0, 1, 2)]
    assert [t.toks[s] for s in (0, 1, 2)] == reads and len({tuple(r) for r in reads}) == 3
    for s in (0, 1, 2):
        e.slot_release(s)


def test_suspend_and_resume(eng):
    e = eng
    p, cap = _prompt(941), 40
    want = _plain(e, p, cap, seed=SEED + 30, slot=1)
    _start(e)
    e.kv_swap_reserve(8)
    e.set_row_sampling(1, _sp(SEED + 30))
    e.set_row_stream(1, True)
    q = _prompt(942)
    e.slots_prefill([1, 4], np.concatenate([p, q]), [len(p), len(q)], [cap, 60])      # slot 4 keeps the engine stepping
    e.slots_decode(16)
    e.slot_suspend(1)
    t = Tracker(e, (1,))
    fin, lens, deltas = t.drain([1, 4])
    assert fin[1] == 2 and lens[1] == 17 and len(deltas[1][0]) == 17                   # the backlog it held at the suspend
    e.slots_decode(5)
    fin, lens, deltas = t.drain([1, 4])
    assert fin[1] == 2 and deltas == {}
    e.slot_resume(1)
    for _ in range(3):
        e.slots_decode(16)
        fin, lens, _ = t.drain([1, 4])
    assert fin[1] == 1 and t.toks[1] == want
    e.slots_reset()
    e.kv_swap_reserve(0)


def test_extend_restarts_the_cursor(eng):
    e = eng
    _start(e)
    e.set_row_sampling(0, _sp(SEED + 40))
    e.set_row_stream(0, True)
    p = _prompt(951)
    e.slots_prefill([0], p, [len(p)], [12])
    e.slots_decode(16)
    t = Tracker(e, (0,))
    fin, _, deltas = t.drain([0])
    assert fin[0] == 1 and len(deltas[0][0]) == 12
    e.slots_extend([0], [[5, 6, 7, 8]], keep_pending=True, max_new_tokens=9)
    t2 = Tracker(e, (0,))                                                              # from index 0 of the new output
    _, _, deltas = t2.drain([0])
    assert len(deltas[0][0]) == 1
    e.slots_decode(16)
    fin, lens, _ = t2.drain([0])
    assert fin[0] == 1 and lens[0] == 9 and t2.toks[0] == e.slot_read(0, 9).tolist()
    e.slot_release(0)


def test_stop_string_row_streams_through_the_matching_token(eng):
    e = eng
    p, cap = _prompt(961), 48
    base = _plain(e, p, cap, seed=SEED + 50, slot=2)
    chunks = [TOKS[x] for x in base]
    stop = hit = None
    for i in range(8, cap - 4):                                                       # three tokens' bytes from the row's own output
        s = (chunks[i] + chunks[i + 1] + chunks[i + 2]).decode()
        h = first_stop(chunks, [s])
        if len(s) >= 4 and h is not None and 6 < h[0] < cap - 2:
            stop, hit = s, h
            break
    assert stop is not None, "the seeded row offers no stop string: a test error, choose another seed"
    _start(e)
    e.set_row_sampling(2, _sp(SEED + 50))
    e.set_row_stop(2, e.create_stop([stop]), 0)
    e.set_row_stream(2, True)
    e.slots_prefill([2], p, [len(p)], [cap])
    t = Tracker(e, (2,))
    t.drain([2])
    for chunk in (5, 16, 16, 16):
        before = e.row_stop_hit(2)
        fin, lens, _ = t.drain([2])
        assert e.row_stop_hit(2) == before                                             # draining does not touch the hit record
        e.slots_decode(chunk)
    fin, lens, _ = t.drain([2])
    assert fin[2] == 1 and e.row_stop_hit(2) == hit
    assert t.toks[2] == base[:hit[0] + 1]                                              # up to and including the token that completes the match
    e.slot_release(2)


def test_edges(eng):
    e = eng
    _start(e)
    p = _prompt(971)
    # no streaming row: a drain is a poll
    e.slots_prefill([1], p, [len(p)], [8])
    fin, lens, deltas = e.slots_drain()
    fin2, lens2 = e.slots_poll()
    assert deltas == {} and np.array_equal(fin, fin2) and np.array_equal(lens, lens2) and fin[1] == 0 and lens[1] == 1
    e.slot_release(1)
    # a row of a beam group does not stream
    e.slots_prefill([0], p, [len(p)], [8])
    e.slots_beam(0, [1])
    for s in (0, 1):
        with pytest.raises(DotsEngineError):
            e.set_row_stream(s, True)
    e.slot_release(0)
    # a streaming row cannot join a group
    e.set_row_stream(2, True)
    e.slots_prefill([2], p, [len(p)], [8])
    with pytest.raises(DotsEngineError):
        e.slots_beam(2, [3])
    # release switches the row off: the slot's next occupant, not set to stream, delivers nothing
    e.slots_decode(4)
    assert len(e.slots_drain()[2][2][0]) == 5
    e.slot_release(2)
    e.slots_prefill([2], p, [len(p)], [8])
    e.slots_decode(4)
    fin, lens, deltas = e.slots_drain()
    assert deltas == {} and lens[2] == 5
    # switched on again over the next occupant, the cursor starts at 0
    e.slot_release(2)
    e.set_row_stream(2, True)
    e.slots_prefill([2], p, [len(p)], [8])
    assert [len(d[0]) for d in e.slots_drain()[2].values()] == [1]
    e.slots_reset()
    e.slots_prefill([2], p, [len(p)], [8])
    assert e.slots_drain()[2] == {}                                                    # slots_reset switched it off
    e.slot_release(2)
