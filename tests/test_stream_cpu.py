"""Streaming without a GPU: the text assembly by brute force, the scheduler over a stand-in engine that has slots_drain,
and the SSE wire format event by event."""
import asyncio
import json
from concurrent.futures import Future

import numpy as np
import pytest

from dots_ocr_amd.config import DotsConfig
from dots_ocr_amd.engine import E_CAPACITY, E_STATE, DotsEngineError
from dots_ocr_amd.processing import DotsOcrProcessor
from dots_ocr_amd.scheduler import ContinuousBatcher, Request, RequestRejected
from dots_ocr_amd.stop_strings import first_stop
from dots_ocr_amd.stream_text import IncrementalText
from fakes import FakePagedEngine

# ---------------------------------------------------------------------------------------------------- 1. IncrementalText


class _ByteProcessor:
    """completion_text's stop-less branch for a byte-level vocabulary: the ids' bytes joined, decoded with errors="replace" """

    def __init__(self, table):
        self.table = table

    def batch_decode(self, seqs, skip_special_tokens=True, clean_up_tokenization_spaces=False):
        return [b"".join(self.table[t] for t in s).decode("utf-8", errors="replace") for s in seqs]


def _table(rng):
    """a byte table: 2- to 4-byte characters split across tokens, whole ones, ASCII, invalid bytes, specials without bytes"""
    text = "aébc€d𝄞ab表é€".encode("utf-8")
    toks, at = [], 0
    while at < len(text):
        n = int(rng.integers(1, 4))
        toks.append(text[at:at + n])
        at += n
    toks += [b"a", b"b", b"ab", b"c", "é".encode(), "€".encode(), b"\xff", b"\xc3", b"\x80", b"\xe2\x82", b"", b""]
    return toks


def _cuts(n):
    """every way of cutting n tokens into consecutive pushes"""
    for mask in range(1 << (n - 1)):
        cut, last = [], 0
        for i in range(n - 1):
            if mask >> i & 1:
                cut.append((last, i + 1))
                last = i + 1
        yield cut + [(last, n)]


def _check(table, seq, stops, include, cuts):
    from dots_ocr_amd.server import completion_text
    chunks = [table[t] for t in seq]
    hit = first_stop(chunks, stops) if stops else None
    if hit is not None:
        seq = seq[:hit[0] + 1]                                   # the row ends at the token that completes the match
    want = completion_text(_ByteProcessor(table), seq, hit, lambda t: table[t], include)
    n = 0
    for cut in cuts(len(seq)):
        it = IncrementalText(lambda t: table[t], stops or None, include)
        said = ""
        for a, b in cut:
            said += it.push(seq[a:b])
            assert want.startswith(said), (seq, stops, include, cut, said, want)          # nothing retracted
        said += it.finish(hit)
        assert said == want, (seq, stops, include, cut, said, want)                       # equal to the unstreamed text
        n += 1
    return n, hit


def _stop_lists(rng, table, seq):
    text = b"".join(table[t] for t in seq).decode("utf-8", errors="ignore")
    out = [[]]
    for _ in range(3):
        k = int(rng.integers(1, 4))
        picks = []
        for _ in range(k):
            if text and rng.random() < 0.7:
                a = int(rng.integers(0, len(text)))
                picks.append(text[a:a + int(rng.integers(1, 4))])
            else:
                picks.append(["ab", "é", "b€", "ca", "€d"][int(rng.integers(0, 5))])
        out.append(sorted(set(p for p in picks if p)))
    return out


def test_incremental_text_equals_completion_text_for_every_cut():
    rng = np.random.default_rng(31)
    cases = hits = 0
    for trial in range(36):
        table = _table(rng)
        L = 12 if trial < 4 else int(rng.integers(1, 9))
        seq = [int(t) for t in rng.integers(0, len(table), L)]
        for stops in _stop_lists(rng, table, seq):
            for include in (False, True):
                n, hit = _check(table, seq, stops, include, _cuts)
                cases += n
                hits += hit is not None
    assert cases > 30000 and hits > 20                                                    # the stop branch is exercised too


def test_incremental_text_on_long_sequences_with_sampled_cuts():
    rng = np.random.default_rng(32)

    def sampled(n):
        for _ in range(40):
            marks = sorted(set(int(x) for x in rng.integers(1, n, int(rng.integers(0, 12))))) if n > 1 else []
            edges = [0] + marks + [n]
            yield list(zip(edges[:-1], edges[1:]))
    for _ in range(12):
        table = _table(rng)
        seq = [int(t) for t in rng.integers(0, len(table), 40)]
        for stops in _stop_lists(rng, table, seq):
            for include in (False, True):
                _check(table, seq, stops, include, sampled)


def test_incremental_text_follows_the_given_decoder():
    """with `decode` (the stop-less branch of completion_text itself) the streamed text is that decoder's, whatever the byte table says"""
    cfg = DotsConfig.tiny()
    proc = DotsOcrProcessor(cfg)
    eos = cfg.eos_token_ids[0]
    ids = proc.tokenizer.encode("é€") [:3] + [eos] + proc.tokenizer.encode("€x𝄞")           # a special between the bytes of one character
    dec = lambda s: proc.batch_decode([list(s)], skip_special_tokens=True, clean_up_tokenization_spaces=False)[0]     # noqa: E731
    want = dec(ids)
    for cut in _cuts(len(ids)):
        it = IncrementalText(proc.token_bytes, None, False, decode=dec)
        said = ""
        for a, b in cut:
            said += it.push(ids[a:b])
            assert want.startswith(said)
        assert said + it.finish(None) == want


# ---------------------------------------------------------------------------------------------------- 2. the scheduler

def _err(code, what):
    e = DotsEngineError(f"{what} failed ({code})")
    e.code = code
    return e


class StreamEngine(FakePagedEngine):
    """FakePagedEngine + what the streaming tests need of the real engine: per-row seeds that vary the output, fork, extend, the resumable
    prefill, suspend / resume, logprobs that are a function of the token, and set_row_stream / slots_drain with a cursor per slot."""
    CAP = 5                                                            # tokens a row delivers per drain (the real engine: 256)

    def __init__(self, script, pool_pages, **kw):
        super().__init__(script, pool_pages, **kw)
        self.rows, self.lp, self.streams, self.cursor = {}, {}, set(), {}
        self.fills, self.fresh, self.order, self.cur = {}, set(), 0, None
        self.swap_total = self.swap_free = 0
        self.polls = self.drains = 0
        self.fail_decode = False
        inner = script
        self.script = lambda prompt: inner(prompt, getattr(self.rows.get(self.cur), "seed", 0))

    # row settings
    def set_row_sampling(self, row, params):
        if params is not None and getattr(params, "top_k", 0) == 13:
            raise ValueError("top_k = 13 is refused by this engine")
        self.rows.pop(row, None) if params is None else self.rows.__setitem__(row, params)

    def set_row_logprobs(self, row, top_n):
        self.lp.pop(row, None) if top_n is None else self.lp.__setitem__(row, top_n)

    def set_row_stream(self, row, on=True):
        self.streams.add(row) if on else self.streams.discard(row)

    @staticmethod
    def _lp_of(toks):
        t = np.asarray(toks, np.float32)
        return -t / 100, np.repeat(np.asarray(toks, np.int32)[:, None], 20, 1), np.repeat((-t / 100)[:, None], 20, 1)

    def row_logprobs(self, row, n, pos0=0):
        return self._lp_of(self.slots[row]["out"][pos0:pos0 + n])

    # admission
    def _need(self, n, c):
        return (min(n + min(c, 64), self.max_seq_len) + 63) // 64

    def _live(self, s):
        self.cur = s
        st = self.slots[s]
        st.update(plan=list(self.script(st["prompt"])), out=[], done=False)
        self.cursor[s] = 0
        self._advance(st)

    def slots_reset(self):
        super().slots_reset()
        self.fills, self.fresh = {}, set()
        self.swap_free = self.swap_total
        self.streams.clear()

    def slots_prefill(self, slots, ids, lens, caps):
        assert not set(slots) & set(self.fills)
        super().slots_prefill(slots, ids, lens, caps)
        for s in slots:
            self._live(s)
        self.fresh = set(slots)

    def slots_prefill_begin(self, slots, ids, lens, caps):
        need = [self._need(n, c) for n, c in zip(lens, caps)]
        if sum(need) > self.free:
            raise RuntimeError("KV pool exhausted")
        off = 0
        for s, n, c, p in zip(slots, lens, caps, need):
            assert s not in self.slots and s not in self.fills
            self.order += 1
            self.fills[s] = dict(prompt=np.asarray(ids[off:off + n]).copy(), cap=int(c), cursor=0, pages=p, order=self.order)
            self.free -= p
            off += n

    def slots_prefill_advance(self, n):
        budget, done = n, []
        for s in sorted(self.fills, key=lambda k: self.fills[k]["order"]):
            f = self.fills[s]
            left = len(f["prompt"]) - f["cursor"]
            take = min(left, budget)
            if take < left:
                take = take // 64 * 64
            if take <= 0:
                break
            f["cursor"] += take
            budget -= take
            if f["cursor"] == len(f["prompt"]):
                done.append(s)
        for s in done:
            f = self.fills.pop(s)
            L = len(f["prompt"])
            self.slots[s] = dict(prompt=f["prompt"], cap=f["cap"], pages=f["pages"], limit=L + f["cap"], ctx=L)
            self._live(s)
        self.fresh = set(done)
        return sum(len(f["prompt"]) - f["cursor"] for f in self.fills.values())

    def slots_fork(self, src, dst):
        assert src in self.fresh and src in self.slots
        p = self.slots[src]
        L = len(p["prompt"])
        own = self._need(L, p["limit"] - L)
        if own * len(dst) > self.free:
            raise RuntimeError("KV pool exhausted")
        for d in dst:
            assert d not in self.slots and d not in self.fills
            self.slots[d] = dict(prompt=p["prompt"].copy(), cap=p["cap"], pages=own, limit=p["limit"], ctx=L)
            self.free -= own
            self._live(d)

    def slots_extend(self, slots, ids_list, keep_pending=False, max_new_tokens=1):
        lacking = [max(0, self._need(len(self.slots[s]["prompt"]) + len(x), max_new_tokens) - self.slots[s]["pages"]) for s, x in zip(slots, ids_list)]
        if sum(lacking) > self.free:
            raise RuntimeError("KV pool exhausted")
        for s, x, more in zip(slots, ids_list, lacking):
            st = self.slots[s]
            st["prompt"] = np.concatenate([st["prompt"], np.asarray(x, st["prompt"].dtype)])
            st.update(pages=st["pages"] + more, cap=int(max_new_tokens), limit=len(st["prompt"]) + int(max_new_tokens), ctx=len(st["prompt"]))
            self.free -= more
            self._live(s)
        self.fresh = set()

    # steps
    def _parked(self):
        return {s: st for s, st in self.slots.items() if st.get("parked") is not None}

    def slots_decode(self, n):
        if self.fail_decode:
            self.fail_decode = False
            raise RuntimeError("the device fell over")
        self.fresh = set()
        parked = self._parked()
        for s in parked:
            del self.slots[s]
        try:
            super().slots_decode(n)
        finally:
            self.slots.update(parked)

    def slots_poll(self):
        self.polls += 1
        return self._poll()

    def _poll(self):
        fin, lens = super().slots_poll()
        for s in self._parked():
            fin[s] = 2
        for s in self.fills:
            fin[s] = 3
        return fin, lens

    def slots_drain(self):
        self.drains += 1
        fin, lens = self._poll()
        deltas = {}
        for s in sorted(self.slots):
            if s not in self.streams:
                continue
            a = self.cursor[s]
            b = min(len(self.slots[s]["out"]), a + self.CAP)
            if b > a:
                toks = self.slots[s]["out"][a:b]
                deltas[s] = (np.asarray(toks, np.int32), self._lp_of(toks) if s in self.lp else None)
                self.cursor[s] = b
        return fin, lens, deltas

    def slot_release(self, s):
        self.streams.discard(s)
        self.lp.pop(s, None)
        if s in self.fills:
            self.free += self.fills.pop(s)["pages"]
            return
        if self.slots[s].get("parked") is not None:
            self.swap_free += self.slots[s]["parked"]
        super().slot_release(s)

    # suspend / resume
    def kv_swap_reserve(self, pages):
        self.swap_total = self.swap_free = int(pages)

    def kv_swap_info(self):
        return self.swap_total, self.swap_free

    def slot_suspend(self, s):
        st = self.slots.get(s)
        if st is None or st["done"] or st.get("parked") is not None:
            raise _err(E_STATE, "dots_slot_suspend")
        data = (st["ctx"] + 63) // 64
        if data > self.swap_free:
            raise _err(E_CAPACITY, "dots_slot_suspend")
        self.swap_free -= data
        self.free += st["pages"]
        st.update(parked=data, pages=0)

    def slot_resume(self, s):
        st = self.slots.get(s)
        if st is None or st.get("parked") is None:
            raise _err(E_STATE, "dots_slot_resume")
        if st["parked"] > self.free:
            raise _err(E_CAPACITY, "dots_slot_resume")
        self.free -= st["parked"]
        self.swap_free += st["parked"]
        st.update(pages=st["parked"], parked=None)

    def slots_pages_short(self, n):
        lack = 0
        for st in self.slots.values():
            if st["done"] or st.get("parked") is not None:
                continue
            lack += max(0, (min(st["ctx"] + n, st["limit"] - 1) + 63) // 64 - st["pages"])
        return max(0, lack - self.free)


def _script(prompt, seed):
    return [1 + (int(prompt[-1]) + seed * 11 + 3 * i) % 90 for i in range(1000)]


def _engine(pool_pages=40, **kw):
    args = dict(max_batch=4, max_patches=100, max_prefill_tokens=128, max_seq_len=640)
    args.update(kw)
    return StreamEngine(_script, pool_pages, **args)


def _req(L=20, cap=23, first=0, **kw):
    ids = np.full(L, 3, np.int32)
    ids[0] = first
    return Request(ids, max_new_tokens=cap, **kw)


class _Sink:
    def __init__(self):
        self.events = []

    def __call__(self, rid, index, toks, lp, finished):
        self.events.append((rid, int(index), [int(t) for t in toks], lp, bool(finished)))

    def tokens(self, rid, index):
        return [t for r, i, toks, _, _ in self.events if (r, i) == (rid, index) for t in toks]


def _sampling(seed):
    from dots_ocr_amd.engine import SamplingParams
    return SamplingParams(temperature=1.0, seed=seed)


def _run(cb, sink):
    """run to idle: {rid: request}; every callback for a request comes before its report"""
    out = {}
    while not cb.idle:
        for rid, req, toks in cb.step():
            assert rid not in out
            out[rid] = (req, toks, len(sink.events))
    return out


def test_one_sequence_streams_in_order_and_polls_only_while_nothing_streams():
    e = _engine()
    cb = ContinuousBatcher(e, chunk=4)
    sink = _Sink()
    plain = cb.submit(_req(cap=9, first=1))
    out = _run(cb, sink)
    assert e.drains == 0 and e.polls > 0 and not sink.events                              # nothing streams: the plain poll, as before
    polls = e.polls
    rid = cb.submit(_req(cap=23, first=2, stream=sink, logprobs=2))
    out = _run(cb, sink)
    req, toks, seen = out[rid]
    assert e.polls == polls and e.drains >= 6                                             # one drain per collect while the request streams
    assert seen == len(sink.events)                                                       # every callback came before the report
    assert sink.tokens(rid, 0) == toks.tolist() == _script(req.input_ids, 0)[:23]
    assert sink.events[0][2] == toks.tolist()[:1] and sink.events[0][4] is False          # the first token, after the prefill
    assert [ev[4] for ev in sink.events] == [False] * (len(sink.events) - 1) + [True]
    assert all(len(ev[2]) <= 4 for ev in sink.events[1:])
    lp = [np.concatenate([ev[3][k] for ev in sink.events if len(ev[2])]) for k in range(3)]
    assert all(np.array_equal(a, b) for a, b in zip(lp, req.logprobs_out))
    assert not e.slots and e.free == e.pool_pages and not e.streams


def test_a_row_that_finishes_behind_the_drain_cap_still_delivers_everything():
    e = _engine()
    cb = ContinuousBatcher(e, chunk=16)                                                   # 16 tokens per chunk, 5 per drain
    sink = _Sink()
    rid = cb.submit(_req(cap=40, stream=sink, logprobs=0))
    req, toks, _ = _run(cb, sink)[rid]
    assert sink.tokens(rid, 0) == toks.tolist() and len(toks) == 40
    lp = np.concatenate([ev[3][0] for ev in sink.events if len(ev[2])])
    assert np.array_equal(lp, req.logprobs_out[0])


def test_n_sequences_and_suffixes_stream_by_index():
    e = _engine()
    cb = ContinuousBatcher(e, chunk=4)
    sink = _Sink()
    a = cb.submit(_req(cap=11, n=3, sampling=_sampling(5), stream=sink))
    req, _, seen = _run(cb, sink)[a]
    assert seen == len(sink.events) and len({tuple(o.tolist()) for o in req.outputs}) == 3
    for i in range(3):
        assert sink.tokens(a, i) == req.outputs[i].tolist() == _script(req.input_ids, 5 + i)[:11]
        assert [ev[4] for ev in sink.events if ev[1] == i][-1] is True
    sink.events.clear()
    b = cb.submit(_req(cap=7, suffixes=[[40, 41], [50], [60, 61, 62]], stream=sink))
    req, _, _ = _run(cb, sink)[b]
    for i, last in enumerate((41, 50, 62)):
        assert sink.tokens(b, i) == req.outputs[i].tolist() == _script([last], 0)[:7]      # the prompt index
    assert not e.slots and e.free == e.pool_pages


def test_submit_refuses_what_cannot_stream():
    cb = ContinuousBatcher(_engine(), chunk=4)
    with pytest.raises(RequestRejected, match="beam"):
        cb.submit(_req(stream=_Sink(), num_beams=2))
    with pytest.raises(RequestRejected, match="score"):
        cb.submit(_req(stream=_Sink(), score=[[1, 2]]))
    with pytest.raises(ValueError, match="callable"):
        cb.submit(_req(stream=True))
    plain = ContinuousBatcher(FakePagedEngine(lambda p: [1] * 100, 40, max_batch=4, max_seq_len=640), chunk=4)
    with pytest.raises(ValueError, match="slots_drain"):
        plain.submit(_req(stream=_Sink()))


def _state(e):
    return dict(slots=dict(e.slots), fills=dict(e.fills), free=e.free, swap=e.swap_free, streams=set(e.streams))


def _cancelled(cb, rid):
    got = [(r, req, toks) for r, req, toks in cb.step() if r == rid]
    assert len(got) == 1 and got[0][1].cancelled is True
    return got[0]


def test_cancel_pending_running_and_group():
    e = _engine()
    cb = ContinuousBatcher(e, chunk=4)
    sink = _Sink()
    before = _state(e)
    # pending: it leaves the queue
    rid = cb.submit(_req(cap=30, stream=sink))
    assert cb.cancel(rid) and not cb.pending
    _, req, toks = _cancelled(cb, rid)
    assert len(toks) == 0 and _state(e) == before and cb.idle
    assert not cb.cancel(rid)                                                             # reported once, then unknown
    # running: its slot, pages and row handles go back, with the tokens it had
    rid = cb.submit(_req(cap=30, first=4, stream=sink, logprobs=1, sampling=_sampling(3)))
    keep = cb.submit(_req(cap=30, first=5))
    cb.step()
    cb.step()
    assert cb.cancel(rid)
    _, req, toks = _cancelled(cb, rid)
    assert toks.tolist() == _script(req.input_ids, 3)[:9] == sink.tokens(rid, 0)           # 1 + 2 chunks of 4
    assert list(cb.running) == [1] and 0 not in e.slots and not e.streams and not e.lp and 0 not in e.rows
    out = _run(cb, sink)
    assert len(out[keep][1]) == 30 and _state(e) == before                                 # the neighbour finishes undisturbed
    # one member of an n group cancels the group, sequences that had finished included
    sink.events.clear()
    rid = cb.submit(_req(cap=6, n=3, sampling=_sampling(1), stream=sink))
    cb.step()
    assert cb.cancel(rid)
    _, req, toks = _cancelled(cb, rid)
    assert [o.tolist() for o in req.outputs] == [_script(req.input_ids, 1 + i)[:5] for i in range(3)]
    assert _state(e) == before and cb.idle and not cb._seq_index and not cb._streamed


def test_cancel_suspended_filling_and_prefetched():
    sink = _Sink()
    # suspended: the parked host pages go back too
    e = _engine(pool_pages=8)
    e.CAP = 64                                                                            # a chunk fits a drain, as on the real engine
    cb = ContinuousBatcher(e, chunk=16, preemption="swap", headroom_pages=0)
    before = _state(e)
    a = cb.submit(_req(L=100, cap=300, first=1, stream=sink))
    b = cb.submit(_req(L=100, cap=300, first=2, stream=sink))
    for _ in range(40):
        cb.step()
        if cb.suspended:
            break
    assert cb.suspended, "the pool never ran short: a test error"
    s = cb.suspended[0]
    rid = cb.running[s][0]
    assert e.swap_free < e.swap_total
    assert cb.cancel(rid)
    _, req, toks = _cancelled(cb, rid)
    assert toks.tolist() == sink.tokens(rid, 0) and len(toks) > 16
    assert not cb.suspended and not cb._parked_pages and e.swap_free == e.swap_total and s not in e.slots
    other = b if rid == a else a
    assert cb.cancel(other)
    _cancelled(cb, other)
    assert _state(e) == before and cb.idle
    # inside a chunked fill: flagged, cancelled by the first collect that sees it running
    e = _engine()
    cb = ContinuousBatcher(e, chunk=4, prefill_chunk=64)
    before = _state(e)
    rid = cb.submit(_req(L=200, cap=30, stream=sink))
    assert cb.step() == [] and cb.filling and e.fills
    assert cb.cancel(rid) and rid in cb._cancel
    got = []
    for _ in range(6):
        got += [x for x in cb.step() if x[0] == rid]
        if got:
            break
    assert len(got) == 1 and got[0][1].cancelled and len(got[0][2]) == 1                   # its first token was all it had
    assert _state(e) == before and cb.idle and not cb._cancel
    # in a prefetched group: likewise
    e = _engine(max_patches=400)
    cb = ContinuousBatcher(e, chunk=4, prefetch=1, admit_group=1)
    before = _state(e)

    def page(first):
        r = _req(L=20, cap=12, first=first, stream=sink)
        r.pixel_values, r.grid_thw = np.zeros((16, 4), np.float32), np.asarray([[1, 4, 4]])
        return r
    first, second = cb.submit(page(1)), cb.submit(page(2))
    cb.step()
    assert [rid for rid, _ in cb._ahead] == [second]
    assert cb.cancel(second) and second in cb._cancel
    out = {}
    for _ in range(12):
        for rid, req, toks in cb.step():
            out[rid] = (req, toks)
        if cb.idle:
            break
    assert getattr(out[first][0], "cancelled", False) is False and len(out[first][1]) == 12
    assert out[second][0].cancelled and _state(e) == before and cb.idle


# ---------------------------------------------------------------------------------------------------- 3. the server

fastapi = pytest.importorskip("fastapi")
from fastapi.testclient import TestClient  # noqa: E402

TEXT = "héllo wörld — 表格 ✓ done"


class _StreamModel:
    def __init__(self, proc, cfg, engine=None):
        self.config = cfg

        def script(prompt, seed):
            return proc.tokenizer.encode(TEXT + "!" * (seed % 5)) + [cfg.eos_token_ids[0]]
        self.engine = engine or StreamEngine(script, 4096, max_batch=4, max_patches=4096, max_prefill_tokens=4096, max_seq_len=2048)


def _payload(**kw):
    body = {"model": "model", "messages": [{"role": "user", "content": "read"}], "max_completion_tokens": 64, "temperature": 0}
    body.update(kw)
    return body


def _events(r):
    """the SSE body as a list of (event name or None, parsed data or "[DONE]")"""
    out = []
    for block in r.text.split("\n\n"):
        if not block.strip():
            continue
        name, data = None, None
        for ln in block.split("\n"):
            if ln.startswith("event: "):
                name = ln[7:]
            elif ln.startswith("data: "):
                data = ln[6:]
        out.append((name, data if data == "[DONE]" else json.loads(data)))
    return out


@pytest.fixture()
def served():
    from dots_ocr_amd.server import create_app
    cfg = DotsConfig.tiny()
    proc = DotsOcrProcessor(cfg)
    model = _StreamModel(proc, cfg)
    app = create_app(model, proc, model_name="model", max_batch=4, look_ahead=0)
    with TestClient(app) as c:
        app.state.worker.chunk = 3                                                        # cuts inside the multi-byte characters
        yield c, model, app


def test_sse_wire_format_event_by_event(served):
    c, model, app = served
    plain = c.post("/v1/chat/completions", json=_payload()).json()
    r = c.post("/v1/chat/completions", json=_payload(stream=True, stream_options={"include_usage": True}))
    assert r.status_code == 200 and r.headers["content-type"].startswith("text/event-stream")
    ev = _events(r)
    assert all(name is None for name, _ in ev) and ev[-1][1] == "[DONE]"
    chunks = [d for _, d in ev[:-1]]
    assert all(d["object"] == "chat.completion.chunk" and d["id"] == chunks[0]["id"] and d["model"] == "model" for d in chunks)
    assert chunks[0]["choices"] == [{"index": 0, "delta": {"role": "assistant", "content": ""}, "finish_reason": None}]
    body, last, usage = chunks[1:-2], chunks[-2], chunks[-1]
    assert len(body) > 3 and all(list(d["choices"][0]["delta"]) == ["content"] and d["choices"][0]["finish_reason"] is None for d in body)
    assert "".join(d["choices"][0]["delta"]["content"] for d in body) == plain["choices"][0]["message"]["content"] == TEXT
    assert last["choices"] == [{"index": 0, "delta": {}, "finish_reason": "stop"}]
    assert usage["choices"] == [] and usage["usage"] == plain["usage"]
    # without include_usage: no usage chunk; every other event as before
    ev2 = _events(c.post("/v1/chat/completions", json=_payload(stream=True)))
    assert len(ev2) == len(ev) - 1 and ev2[-1][1] == "[DONE]" and "usage" not in ev2[-2][1]
    assert not model.engine.slots and model.engine.free == model.engine.pool_pages


def test_sse_n_choices_and_logprobs(served):
    c, model, app = served
    kw = dict(n=2, temperature=1.0, seed=3, logprobs=True, top_logprobs=2)
    plain = c.post("/v1/chat/completions", json=_payload(**kw)).json()
    ev = _events(c.post("/v1/chat/completions", json=_payload(stream=True, **kw)))
    chunks = [d for _, d in ev[:-1]]
    assert [d["choices"][0]["index"] for d in chunks[:2]] == [0, 1] and all(d["choices"][0]["delta"].get("role") == "assistant" for d in chunks[:2])
    for i in (0, 1):
        mine = [d["choices"][0] for d in chunks[2:] if d["choices"][0]["index"] == i]
        assert "".join(ch["delta"].get("content", "") for ch in mine) == plain["choices"][i]["message"]["content"]
        assert mine[-1]["delta"] == {} and mine[-1]["finish_reason"] == plain["choices"][i]["finish_reason"]
        entries = [x for ch in mine if "logprobs" in ch for x in ch["logprobs"]["content"]]
        assert entries == plain["choices"][i]["logprobs"]["content"]
    assert plain["choices"][0]["message"]["content"] != plain["choices"][1]["message"]["content"]


def test_sse_error_events_and_400s(served):
    c, model, app = served
    # refused at admission: the engine's last word on the request's own parameters
    ev = _events(c.post("/v1/chat/completions", json=_payload(stream=True, temperature=1.0, top_k=13)))
    assert ev[0][1]["choices"][0]["delta"]["role"] == "assistant"
    assert ev[-2][0] == "error" and ev[-2][1]["error"]["code"] == 400 and "refused" in ev[-2][1]["error"]["message"] and ev[-1][1] == "[DONE]"
    # an engine failure ends the stream, it does not hang it
    model.engine.fail_decode = True
    ev = _events(c.post("/v1/chat/completions", json=_payload(stream=True)))
    assert ev[-2][0] == "error" and ev[-2][1]["error"]["code"] == 500 and "fell over" in ev[-2][1]["error"]["message"]
    assert _events(c.post("/v1/chat/completions", json=_payload(stream=True)))[-1][1] == "[DONE]"      # and the server goes on
    for bad in (dict(use_beam_search=True, n=2), dict(score_candidates=["a"]), dict(stream_options={"include_usage": "yes"}),
                dict(stream_options=[1])):
        r = c.post("/v1/chat/completions", json=_payload(stream=True, **bad))
        assert r.status_code == 400 and "streaming" in r.json()["detail"], bad


def test_streaming_is_a_400_without_a_draining_engine():
    from dots_ocr_amd.server import create_app
    from fakes import FakeSlotEngine
    cfg = DotsConfig.tiny()
    proc = DotsOcrProcessor(cfg)
    plain = FakeSlotEngine(lambda p: [65, cfg.eos_token_ids[0]], max_batch=3, max_patches=4096, max_prefill_tokens=4096, max_seq_len=2048)
    for kw in (dict(continuous=True), dict(continuous=False)):                            # an engine without slots_drain; static batching
        app = create_app(_StreamModel(proc, cfg, engine=plain), proc, **kw)
        with TestClient(app) as c:
            r = c.post("/v1/chat/completions", json=_payload(stream=True))
            assert r.status_code == 400 and "streaming" in r.json()["detail"]


def test_closing_the_response_cancels_the_request():
    """the generator closed before the request finished: the worker is told; a worker told so releases the request's slot"""
    from dots_ocr_amd.server import ContinuousWorker, RequestCancelled, _Job, sse_events
    cfg = DotsConfig.tiny()
    proc = DotsOcrProcessor(cfg)

    class _Worker:
        def __init__(self):
            self.cancelled = []

        def cancel(self, job):
            self.cancelled.append(job)

    async def closed_early():
        w, job, fut, q = _Worker(), _Job(None, "read", 64, 0.0, 1.0), Future(), asyncio.Queue()
        q.put_nowait(("delta", 0, proc.tokenizer.encode("ab"), None, False))
        gen = sse_events(w, job, fut, q, proc, proc.token_bytes, "model", False)
        first, second = await gen.__anext__(), await gen.__anext__()
        assert '"role": "assistant"' in first and '"content": "ab"' in second
        await gen.aclose()
        return w.cancelled == [job]
    assert asyncio.run(closed_early())

    async def finished():
        w, job, fut, q = _Worker(), _Job(None, "read", 64, 0.0, 1.0), Future(), asyncio.Queue()
        fut.set_result({"text": "ab", "prompt_tokens": 3, "completion_tokens": 2, "finish_reason": "stop"})
        q.put_nowait(("done", fut))
        out = [x async for x in sse_events(w, job, fut, q, proc, proc.token_bytes, "model", False)]
        return out[-1] == "data: [DONE]\n\n" and not w.cancelled
    assert asyncio.run(finished())

    # the real worker: a sink that hangs up at the first delta
    model = _StreamModel(proc, cfg)
    model.engine.script = lambda prompt: [66] * 500                                        # never an EOS: only the cap or a cancel ends it
    w = ContinuousWorker(model, proc, max_batch=4, look_ahead=0, chunk=2)
    try:
        job = _Job(None, proc.apply_chat_template([{"role": "user", "content": "read"}]), 400, 0.0, 1.0)
        seen = []

        def sink(ev):
            seen.append(ev)
            if len(seen) == 1:
                w.cancel(job)
        job.sink = sink
        with pytest.raises(RequestCancelled):
            w.submit(job).result(timeout=30)
        assert 1 <= sum(len(ev[2]) for ev in seen) < 400
        done = _Job(None, job.text, 5, 0.0, 1.0)                                           # the worker goes on, on a clean engine
        assert w.submit(done).result(timeout=30)["completion_tokens"] == 5
        assert not model.engine.slots and model.engine.free == model.engine.pool_pages and not model.engine.streams
    finally:
        w.close()
