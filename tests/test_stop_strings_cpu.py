"""Stop strings without a GPU: the host compiler against the rule restated with bytes.find, the named cases of the rule,
the limits, and the server's `stop` field over a fake engine that walks the automaton as the device does."""
import numpy as np
import pytest
import torch

from dots_ocr_amd.config import DotsConfig
from dots_ocr_amd.engine import MAX_STOP_BYTES, MAX_STOP_IDS, MAX_STOP_STRINGS
from dots_ocr_amd.row_features import rows_holding
from dots_ocr_amd.stop_strings import StopAutomaton, compile_stop, cut_text, first_stop, stopped_text
from test_parallel_sampling_cpu import ForkEngine


# ---------------------------------------------------------------------------------------------------- the automaton

OVERLAPPING = [("abab", "bab", "ba"), ("a", "aa", "aaa"), ("abc", "bc", "c"), ("abca", "ca", "aab"), ("ab", "ba"), ("cab", "abcab", "b"),
               ("aabaab", "abaa", "baab", "aa"), ("ccc",), ("abcabcab", "cabc", "bca")]


def _tokens(g, data):
    """the stream cut at random into "tokens" of 0 to 4 bytes"""
    out, i = [], 0
    while i < len(data):
        n = int(g.integers(0, 5))
        out.append(data[i:i + n])
        i += n
    return out + [b""] * int(g.integers(0, 2))


def test_the_automaton_gives_exactly_the_restatement_on_random_overlapping_cases():
    g = np.random.default_rng(5)
    hits = 0
    for case in range(4000):
        if case % 2:
            strings = list(OVERLAPPING[int(g.integers(len(OVERLAPPING)))])
        else:                                          # random sets over {a, b, c}: short strings overlap themselves and each other
            strings = ["".join("abc"[int(k)] for k in g.integers(0, 3, int(g.integers(1, 5)))) for _ in range(int(g.integers(1, 5)))]
        g.shuffle(strings)
        data = bytes(g.choice(list(b"abc"), int(g.integers(0, 40))).astype(np.uint8))
        chunks = _tokens(g, data)
        m = int(g.integers(0, 4)) * int(g.integers(0, 2)) * 3
        a = compile_stop(strings)
        want = first_stop(chunks, strings, min_tokens=m)
        assert a.walk(chunks, m) == want, (strings, chunks, m)
        hits += want is not None
    assert 1000 < hits < 3990                          # both outcomes are exercised


def test_the_table_is_dense_and_the_limits_hold():
    a = compile_stop(["abab", "bab", "ba", "abab"])    # the duplicate is dropped
    assert a.strings == ("abab", "bab", "ba") and isinstance(a, StopAutomaton)
    assert a.table.dtype == np.uint16 and a.table.shape == (a.n_states, 256) and int(a.table.max()) < a.n_states      # no dead state
    assert a.match_len.dtype == np.uint16 and a.match_len.shape == (a.n_states,) and a.match_id.shape == (a.n_states,)
    assert a.match_len[0] == 0 and set(a.match_len.tolist()) == {0, 2, 3, 4}
    assert (MAX_STOP_IDS, MAX_STOP_STRINGS, MAX_STOP_BYTES) == (16, 16, 64)
    big = compile_stop([chr(ord("A") + i) * 64 for i in range(16)])
    assert big.n_states == 16 * 64 + 1 == 1025         # the most states the limits allow
    assert big.walk([b"zz", b"C" * 63, b"C", b"C"]) == (2, 1, 64, 2)


@pytest.mark.parametrize("bad", [[""], ["ok", ""], [], ["x" * 65], ["é" * 33], [f"s{i}" for i in range(17)], [b"bytes"], ["ok", 3], 7, [None]])
def test_bad_input_is_a_value_error_at_the_call(bad):
    with pytest.raises(ValueError):
        compile_stop(bad)
    with pytest.raises(ValueError):
        first_stop([b"abc"], bad)


def test_limits_are_inclusive():
    assert compile_stop(["x" * 64]).n_states == 65 and compile_stop("é" * 32).strings == ("é" * 32,)
    assert len(compile_stop([f"s{i}" for i in range(16)]).strings) == 16
    assert len(compile_stop([f"s{i % 16}" for i in range(40)]).strings) == 16       # duplicates do not count


def _both(chunks, strings, m=0):
    got = compile_stop(strings).walk(chunks, m)
    assert got == first_stop(chunks, strings, min_tokens=m)
    return got


def test_the_named_cases():
    # a match inside one token
    assert _both([b"xx", b"a</t>b", b"yy"], ["</t>"]) == (1, 5, 4, 0)
    # begins and ends mid-token across three tokens
    assert _both([b"12", b"3</", b"tab", b"le>9"], ["</table>"]) == (3, 3, 8, 0)
    # two strings end at the same byte: the longest wins (it has the earliest start), whatever the order of the list
    assert _both([b"ab", b"ab", b"c"], ["bab", "abab"]) == (1, 2, 4, 1)
    assert _both([b"ab", b"ab", b"c"], ["abab", "bab", "b"]) == (0, 2, 1, 2)        # an earlier END beats a longer string
    # a match wholly below min_tokens is ignored: the row stops at the next one
    assert _both([b"$$", b"x", b"y", b"$", b"$z"], ["$$"], 1) == (4, 1, 2, 0)
    assert _both([b"$$", b"x", b"y"], ["$$"], 1) is None
    # a match that straddles the min_tokens boundary is taken: the automaton advanced below it
    assert _both([b"a$", b"$b"], ["$$"], 1) == (1, 1, 2, 0)
    # a token without bytes in the middle of a match leaves the state alone
    assert _both([b"..", b"", b"..", b"", b"..x"], ["......"]) == (4, 2, 6, 0)
    # a three-byte UTF-8 character split across tokens
    euro = "€".encode()
    assert _both([b"1" + euro[:1], euro[1:2], euro[2:] + b"2"], ["€"]) == (2, 1, 3, 0)
    assert _both([b"1" + euro[:1], euro[1:2], euro[2:] + b"2"], ["€2", "1€"]) == (2, 1, 4, 1)


def test_the_text_is_cut_where_the_match_starts_or_ends():
    chunks = [b"12", b"3</", b"tab", b"le>9"]
    hit = first_stop(chunks, ["</table>"])
    assert cut_text(chunks, hit) == b"123" and cut_text(chunks, hit, include_stop_str=True) == b"123</table>"
    tb = {i: c for i, c in enumerate(chunks)}.__getitem__
    assert stopped_text([0, 1, 2, 3], hit, tb) == "123" and stopped_text([0, 1, 2, 3], hit, tb, True) == "123</table>"
    # a cut in the middle of a multi-byte character: errors="replace"
    broken = ["€".encode()[:2], b"]"]
    assert stopped_text([0, 1], first_stop(broken, ["]"]), {0: broken[0], 1: broken[1]}.__getitem__) == "�"


# ---------------------------------------------------------------------------------------------------- scheduler and server

class StopEngine(ForkEngine):
    """ForkEngine + stop strings as the engine defines them: the commit of a token walks the row's automaton over the token's bytes and
    finishes the row at a match; prefill and fork start the automaton at the root, a fork hands the source's automaton to its children,
    release and reset clear the row."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.token_bytes, self.automata, self.stops, self.uploads = None, {}, {}, 0

    def set_token_bytes(self, tb):
        self.token_bytes = tb

    def create_stop(self, strings):
        key = tuple(strings)
        if key not in self.automata:
            self.uploads += 1
            self.automata[key] = (len(self.automata) + 1, compile_stop(list(key)))
        return self.automata[key][0]

    def set_row_stop(self, row, handle, min_tokens=0):
        if not handle:
            self.stops.pop(row, None)
            return
        a = next(a for h, a in self.automata.values() if h == handle)
        self.stops[row] = dict(a=a, min=min_tokens, state=0, hit=None)

    def set_row_logit_rules(self, row, rules):         # accepted and recorded: min_tokens reaches the stop strings through the batcher
        self.rules = getattr(self, "rules", {})
        self.rules[row] = rules

    def row_stop_hit(self, row):
        return self.stops[row]["hit"] if row in self.stops else None

    def _advance(self, st):
        was = st["done"]
        super()._advance(st)
        slot = next((s for s, v in self.slots.items() if v is st), None)
        rs = self.stops.get(slot)
        if was or rs is None or st["out"][-1] in self.eos:
            return
        n = len(st["out"]) - 1
        for j, b in enumerate(self.token_bytes.token(st["out"][-1])):
            rs["state"] = int(rs["a"].table[rs["state"], b])
            if rs["a"].match_len[rs["state"]] and n >= rs["min"]:
                rs["hit"] = (n, j + 1, int(rs["a"].match_len[rs["state"]]), int(rs["a"].match_id[rs["state"]]))
                st["done"] = True
                break

    def _restart(self, s):
        if s in self.stops:
            self.stops[s].update(state=0, hit=None)
        super()._restart(s)

    def slots_fork(self, src, dst):
        for d in dst:
            if src in self.stops:
                self.stops[d] = dict(self.stops[src], state=0, hit=None)
        super().slots_fork(src, dst)

    def slot_release(self, s):
        self.stops.pop(s, None)
        super().slot_release(s)

    def slots_reset(self):
        super().slots_reset()
        self.stops = {}


TEXTS = {0: "row one</table>tail]", 1: "right$$y]z</table>"}


class _StopModel:
    """a completion spells TEXTS[seed % 2] and ends by EOS; generate() is the static path's (it ignores stop_strings, as a model object
    without engine rows would)"""

    def __init__(self, proc, cfg):
        self.config, self.proc = cfg, proc
        model = self

        def script(prompt):
            e = model.engine
            p = e.rows.get(e.cur)
            return proc.tokenizer.encode(TEXTS[(0 if p is None else p.seed) % 2]) + [cfg.eos_token_ids[0]]
        self.engine = StopEngine(script, 256, max_batch=3, max_patches=4096, max_prefill_tokens=4096, max_seq_len=2048)
        self.generate_kw = []

    def generate(self, input_ids=None, seed=0, **kw):
        self.generate_kw.append(kw)
        new = torch.tensor(self.proc.tokenizer.encode(TEXTS[seed % 2]) + [self.config.eos_token_ids[0]])
        return torch.cat([input_ids, new[None].repeat(input_ids.shape[0], 1)], dim=1)


def _payload(**kw):
    body = {"model": "model", "messages": [{"role": "user", "content": "Read this."}], "max_completion_tokens": 40, "temperature": 0.8, "seed": 10}
    body.update(kw)
    return body


def _app(**kw):
    pytest.importorskip("fastapi")
    from dots_ocr_amd.processing import DotsOcrProcessor
    from dots_ocr_amd.server import create_app
    cfg = DotsConfig.tiny()
    proc = DotsOcrProcessor(cfg)
    model = _StopModel(proc, cfg)
    return model, proc, create_app(model, proc, model_name="model", max_batch=3, **kw)


def _post(c, **kw):
    r = c.post("/v1/chat/completions", json=_payload(**kw))
    assert r.status_code == 200, r.text
    return r.json()


@pytest.mark.parametrize("continuous", [True, False])
def test_server_cuts_the_text_and_reports_the_reason(continuous):
    from fastapi.testclient import TestClient
    model, proc, app = _app(continuous=continuous)
    with TestClient(app) as c:
        d = _post(c, stop="</table>")                                               # a string
        ch = d["choices"][0]
        assert ch["message"]["content"] == "row one" and ch["finish_reason"] == "stop" and ch["stop_reason"] == "</table>"
        assert d["usage"]["completion_tokens"] == len("row one</table>")            # the token that completed the match included
        d = _post(c, stop=["]", "</table>"], include_stop_str_in_output=True)       # a list; the earliest end wins
        ch = d["choices"][0]
        assert ch["message"]["content"] == "row one</table>" and ch["stop_reason"] == "</table>"
        d = _post(c, stop=["nowhere"])                                              # no match: the EOS ends it, nothing is cut
        ch = d["choices"][0]
        assert ch["message"]["content"] == TEXTS[0] and ch["finish_reason"] == "stop" and ch["stop_reason"] is None
        assert d["usage"]["completion_tokens"] == len(TEXTS[0]) + 1
        if continuous:                                                              # the cap comes first: no hit, nothing cut
            ch = _post(c, stop="</table>", max_completion_tokens=4)["choices"][0]
            assert (ch["message"]["content"], ch["finish_reason"], ch["stop_reason"]) == ("row ", "length", None)
        plain = _post(c)                                                            # without the field: today's keys
        assert sorted(plain["choices"][0]) == ["finish_reason", "index", "message"] and plain["choices"][0]["message"]["content"] == TEXTS[0]
        assert sorted(_post(c, stop=[])["choices"][0]) == ["finish_reason", "index", "message"]
        for bad in ("", [""], ["x" * 65], [f"s{i}" for i in range(17)], 5, ["a", 1], {"a": 1}):
            assert c.post("/v1/chat/completions", json=_payload(stop=bad)).status_code == 400, bad
        assert c.post("/v1/chat/completions", json=_payload(stop="a", include_stop_str_in_output="yes")).status_code == 400
        r = c.post("/v1/chat/completions", json=_payload(stop="</table>", stream=True))
        assert r.status_code == 400 and "stream" in r.text                          # stop together with stream is still a 400
    if continuous:
        assert not model.engine.slots and model.engine.stops == {} and model.engine.kv_pool_info() == (256, 256)
        assert model.engine.uploads == 3                                            # one automaton per distinct list
    else:
        assert model.generate_kw[0]["stop_strings"] == ["</table>"] and "stop_strings" not in model.generate_kw[-1]


def test_server_n_2_reports_each_choices_own_hit():
    from fastapi.testclient import TestClient
    model, proc, app = _app()
    with TestClient(app) as c:
        d = _post(c, stop=["]", "$$"], n=2, logprobs=None)                          # seeds 10 and 11: two texts, two different matches
        a, b = d["choices"]
        assert (a["message"]["content"], a["stop_reason"], a["finish_reason"]) == ("row one</table>tail", "]", "stop")
        assert (b["message"]["content"], b["stop_reason"], b["finish_reason"]) == ("right", "$$", "stop")
        assert d["usage"]["completion_tokens"] == len(TEXTS[0]) + len("right$$")
        d = _post(c, stop=["</table>"], n=2, include_stop_str_in_output=True, min_tokens=12)
        assert [ch["message"]["content"] for ch in d["choices"]] == ["row one</table>", TEXTS[1]]
    assert not model.engine.slots and model.engine.stops == {}


def test_the_batcher_sets_reads_and_clears_the_row():
    from dots_ocr_amd.engine import LogitRules, SamplingParams
    from dots_ocr_amd.processing import DotsOcrProcessor
    from dots_ocr_amd.scheduler import ContinuousBatcher, Request, RequestRejected
    cfg = DotsConfig.tiny()
    proc = DotsOcrProcessor(cfg)
    model = _StopModel(proc, cfg)
    eng = model.engine
    eng.set_token_bytes(proc.guide_token_bytes())
    cb = ContinuousBatcher(eng, eos_ids=cfg.eos_token_ids, chunk=4)
    ids = np.full(5, 65, np.int32)
    a = Request(ids, max_new_tokens=40, sampling=SamplingParams(temperature=1.0, seed=2), stop=["one", "one"])
    b = Request(ids, max_new_tokens=40, sampling=SamplingParams(temperature=1.0, seed=2), stop=("row",),
                rules=LogitRules(min_tokens=3, vocab_size=cfg.vocab_size, eos_ids=cfg.eos_token_ids))
    plain = Request(ids, max_new_tokens=40, sampling=SamplingParams(temperature=1.0, seed=2))
    outs = cb.run([a, b, plain])
    assert a.stop == ("one",) and a.stop_hit == (6, 1, 3, 0) and proc.tokenizer.decode(outs[0].tolist()) == "row one"
    assert b.stop_hit is None and not hasattr(plain, "stop_hit")                    # "row" lies wholly below min_tokens = 3
    assert proc.tokenizer.decode(outs[2].tolist()) == TEXTS[0] and eng.stops == {} and rows_holding(cb._rows, "stop") == []
    with pytest.raises(RequestRejected):
        cb.submit(Request(ids, stop=[""]))
    from fakes import FakePagedEngine
    with pytest.raises(ValueError, match="set_row_stop"):
        ContinuousBatcher(FakePagedEngine(lambda p: [1], 8), chunk=2).submit(Request(ids, stop=["a"]))
