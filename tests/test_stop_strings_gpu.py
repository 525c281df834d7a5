"""Stop strings on the GPU: a row ends at the token that completes one of its strings, inside captured chunks, in the static
batch, in any slot, beside any neighbour.

The test owns the token-byte table: token i has 1 to 4 bytes over {a, b, c} from a seeded generator and a few ids have none.  Rows are
sampled at temperature 1 under fixed seeds (the draw of a row is hash(seed, position) over its own logits, so a row's tokens depend on
nothing but its prompt and seed).  A baseline of 48 tokens per row is taken once without stop strings; the stop strings are picked from
each row's own baseline bytes, the properties of what was picked are asserted, and every check compares a stopped run against the baseline
and against stop_strings.first_stop, the rule restated with bytes.find.

The context length of a row is not readable from the host; it advances under the same "not finished" test as the output length
(csrc/step_dev.h commit_token), so "stops growing" is checked on the output length over further decode chunks."""
import numpy as np
import pytest

from dots_ocr_amd.config import DotsConfig
from dots_ocr_amd.engine import DotsEngineError, SamplingParams
from dots_ocr_amd.stop_strings import first_stop
from dots_ocr_amd.weights import random_state_dict

pytestmark = pytest.mark.gpu

CAP = 48
V = 1024
NO_BYTES = (3, 77, 500, 1001, 1023)
SEED = 4100


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


PROMPTS = [_prompt(700 + b) for b in range(4)]


def _sp(seed):
    return SamplingParams(temperature=1.0, seed=seed)


def _chunks(toks):
    return [TOKS[t] for t in toks]


def _run(e, prompts, slots=None, seeds=None, stops=None, cap=CAP, chunk=16, lp=None, extra=0):
    """prefill `prompts` into `slots` and decode to the end in captured chunks.  seeds[i]: the row samples at temperature 1 under it (None:
    a plain greedy row); stops[i]: (strings, min_tokens) or None.  -> per prompt dict(toks, hit, fin, lp); extra: decode steps issued
    after every row has finished, to see that nothing grows."""
    slots = list(range(len(prompts))) if slots is None else slots
    e.set_sampling(0.0, 1.0, 0)
    e.slots_reset()
    e.set_eos([])
    for i, s in enumerate(slots):
        if seeds and seeds[i] is not None:
            e.set_row_sampling(s, _sp(seeds[i]))
        if stops and stops[i] is not None:
            e.set_row_stop(s, e.create_stop(list(stops[i][0])), stops[i][1])
        if lp and lp[i] is not None:
            e.set_row_logprobs(s, lp[i])
    e.slots_prefill(slots, np.concatenate(prompts), [len(p) for p in prompts], [cap] * len(prompts))
    steps = 0
    while steps < cap + 2 * chunk:
        fin, lens = e.slots_poll()
        if all(fin[s] == 1 for s in slots):
            break
        e.slots_decode(chunk)
        steps += chunk
    fin, lens = e.slots_poll()
    if extra:
        e.slots_decode(extra)
        fin2, lens2 = e.slots_poll()
        assert np.array_equal(fin, fin2) and np.array_equal(lens, lens2)
    out = []
    for i, s in enumerate(slots):
        n = int(lens[s])
        out.append(dict(toks=e.slot_read(s, n).tolist(), hit=e.row_stop_hit(s), fin=int(fin[s]),
                        lp=e.row_logprobs(s, n) if lp and lp[i] is not None else None))
    for s in slots:
        e.slot_release(s)
    return out


def _pos(chunks):
    """byte position -> (token index, bytes into it), and each token's first byte position"""
    owner, start = [], []
    for n, c in enumerate(chunks):
        start.append(len(owner))
        owner += [(n, j + 1) for j in range(len(c))]
    return owner, start


def _pick(chunks, want):
    """A stop list from the row's own bytes whose first_stop has the wanted property; (strings, hit).  Candidates are the bytes of three
    consecutive tokens (long enough to be unlikely earlier in a stream over three letters), trimmed as the property asks."""
    for i in range(6, len(chunks) - 3):
        a, b, c = chunks[i], chunks[i + 1], chunks[i + 2]
        if min(len(a), len(c)) < 2 or not b:
            continue
        if want == "mid":
            strings = [(a[1:] + b + c[:-1]).decode()]
        elif want == "token_end":
            strings = [(a[1:] + b + c).decode()]
        else:
            full = (a[1:] + b + c[:-1]).decode()
            strings = [full[1:], full]                # both end at the same byte; the longer one starts earlier
        hit = first_stop(chunks, strings)
        if hit is None:
            continue
        tok, used, length, mid = hit
        owner, start = _pos(chunks)
        end = start[tok] + used - 1
        first_tok, first_used = owner[end - length + 1]
        if want == "mid" and first_used > 1 and used < len(chunks[tok]) and tok - first_tok >= 1:
            return strings, hit
        if want == "token_end" and used == len(chunks[tok]) and tok - first_tok >= 1:
            return strings, hit
        if want == "same_byte" and length == len(full) and mid == 1 and first_stop(chunks, strings[:1])[:2] == hit[:2]:
            return strings, hit
    raise AssertionError(f"the seeded rows offer no '{want}' case: a test error, choose another seed")


@pytest.fixture(scope="module")
def eng():
    from dots_ocr_amd.engine import Engine
    cfg = DotsConfig.tiny(layers=3, v_layers=3, vocab=V)
    e = Engine(cfg, max_batch=8, max_seq_len=640, max_patches=4096, max_prefill_tokens=2048)
    e.load_state_dict(random_state_dict(cfg, seed=11))
    early = None
    try:
        e.create_stop(["ab"])
    except DotsEngineError as err:
        early = err
    e.set_token_bytes(TOKS)
    yield e, early
    e.close()


@pytest.fixture(scope="module")
def base(eng):
    """the baselines, computed once: four sampled rows and the same prompts greedy, 48 tokens each, no stop strings; the stop lists picked
    from the rows' own bytes"""
    e, _ = eng
    seeds = [SEED + b for b in range(4)]
    sampled = _run(e, PROMPTS, seeds=seeds, lp=[0, None, None, None])
    greedy = _run(e, PROMPTS[:2])
    assert all(len(r["toks"]) == CAP and r["hit"] is None and r["fin"] == 1 for r in sampled + greedy)
    chunks = [_chunks(r["toks"]) for r in sampled]
    picks = [_pick(chunks[0], "mid"), _pick(chunks[1], "token_end"), _pick(chunks[2], "same_byte")]
    return dict(seeds=seeds, sampled=sampled, greedy=greedy, chunks=chunks, picks=picks)


def test_the_picked_cases_have_their_properties(base):
    (s0, h0), (s1, h1), (s2, h2) = base["picks"]
    c = base["chunks"]
    assert 0 < h0[1] < len(c[0][h0[0]]) and h0[2] > h0[1]                          # ends mid-token, began in an earlier token
    assert h1[1] == len(c[1][h1[0]])                                               # ends exactly at its token's last byte
    assert len(s2) == 2 and s2[1].endswith(s2[0]) and h2[2] == len(s2[1]) and h2[3] == 1      # two end at one byte: the longest is the match
    assert all(h[0] < CAP - 1 for h in (h0, h1, h2))                               # the stop, not the cap, ends the row
    assert len({t for r in base["sampled"] for t in r["toks"]}) > 40              # the tiny model's sampled output does vary


def test_rows_stop_exactly_at_the_matching_token(eng, base):
    e, _ = eng
    stops = [(s, 0) for s, _ in base["picks"]] + [None]
    got = _run(e, PROMPTS, seeds=base["seeds"], stops=stops, extra=16)
    for b in range(3):
        want = base["picks"][b][1]
        assert got[b]["hit"] == want == first_stop(base["chunks"][b], stops[b][0]), b
        assert got[b]["toks"] == base["sampled"][b]["toks"][:want[0] + 1], b       # through the hit token and nothing more
        assert got[b]["fin"] == 1
    assert got[3]["toks"] == base["sampled"][3]["toks"] and got[3]["hit"] is None


def test_chunk_size_does_not_matter_and_a_hit_inside_a_chunk_stops_there(eng, base):
    e, _ = eng
    stops = [(s, 0) for s, _ in base["picks"]]
    runs = {c: _run(e, PROMPTS[:3], seeds=base["seeds"][:3], stops=stops, chunk=c) for c in (1, 5, 16)}
    for c in (1, 5):
        assert [(r["toks"], r["hit"]) for r in runs[c]] == [(r["toks"], r["hit"]) for r in runs[16]], c
    # tokens 1 .. 16 are the first captured chunk of 16 steps, and so on: a hit at index h ends its chunk only when h % 16 == 0
    inside = [b for b in range(3) if runs[16][b]["hit"][0] % 16 != 0]
    assert inside
    for b in inside:
        assert len(runs[16][b]["toks"]) == runs[16][b]["hit"][0] + 1 == base["picks"][b][1][0] + 1


def test_the_static_batch_ends_the_row_at_the_same_token(eng, base):
    e, _ = eng
    e.set_sampling(0.0, 1.0, 0)
    try:
        for b in range(3):
            e.set_row_sampling(b, _sp(base["seeds"][b]))
            e.set_row_stop(b, e.create_stop(base["picks"][b][0]), 0)
        e.set_row_sampling(3, _sp(base["seeds"][3]))
        out, lens = e.generate(np.concatenate(PROMPTS), np.array([len(p) for p in PROMPTS], np.int32), max_new_tokens=CAP, eos_ids=[])
        hits = [e.row_stop_hit(b) for b in range(4)]
    finally:
        for b in range(4):
            e.set_row_sampling(b, None)
            e.set_row_stop(b, None)
    for b in range(3):
        h = base["picks"][b][1]
        assert int(lens[b]) == h[0] + 1 and out[b, :lens[b]].tolist() == base["sampled"][b]["toks"][:h[0] + 1] and hits[b] == h, b
    assert int(lens[3]) == CAP and out[3].tolist() == base["sampled"][3]["toks"] and hits[3] is None


def test_a_stopping_request_is_the_same_alone_in_a_batch_and_in_any_slot(eng, base):
    e, _ = eng
    strings, hit = base["picks"][0]
    want = (base["sampled"][0]["toks"][:hit[0] + 1], hit)
    alone = _run(e, PROMPTS[:1], seeds=base["seeds"][:1], stops=[(strings, 0)])[0]
    moved = _run(e, PROMPTS[:1], slots=[5], seeds=base["seeds"][:1], stops=[(strings, 0)])[0]
    batch = _run(e, PROMPTS, slots=[2, 0, 1, 3], seeds=base["seeds"], stops=[(strings, 0), None, None, None])
    for r in (alone, moved, batch[0]):
        assert (r["toks"], r["hit"]) == want
    for b in (1, 2, 3):                                                            # the neighbours: bit for bit their own baselines
        assert batch[b]["toks"] == base["sampled"][b]["toks"] and batch[b]["hit"] is None


def test_a_greedy_row_stops_on_its_greedy_baseline(eng, base):
    e, _ = eng
    toks = base["greedy"][0]["toks"]
    c = _chunks(toks)
    strings = [b"".join(c[7:10]).decode()]
    hit = first_stop(c, strings)
    assert hit is not None and 0 < hit[0] < CAP - 1
    got = _run(e, PROMPTS[:2], stops=[(strings, 0), None])
    assert got[0]["toks"] == toks[:hit[0] + 1] and got[0]["hit"] == hit
    assert got[1]["toks"] == base["greedy"][1]["toks"]


def _two_matches(chunks):
    """(strings, min_tokens): the string's first match lies wholly below min_tokens and a later one ends at or after it"""
    owner, start = _pos(chunks)
    data = b"".join(chunks)
    for n in (4, 3, 2):
        for at in range(len(data) - n):
            s = data[at:at + n]
            first = first_stop(chunks, [s.decode()])
            m = first[0] + 1
            if m >= CAP - 2:
                continue
            second = first_stop(chunks, [s.decode()], min_tokens=m)
            if second is not None and second[0] < CAP - 1:
                return [s.decode()], m, first, second
    raise AssertionError("no string of the row matches twice: a test error, choose another seed")


def test_no_match_is_taken_below_min_tokens(eng, base):
    e, _ = eng
    strings, m, first, second = _two_matches(base["chunks"][3])
    assert first[0] < m <= second[0]
    got = _run(e, PROMPTS[3:], seeds=base["seeds"][3:], stops=[(strings, m)])[0]
    assert got["hit"] == second == first_stop(base["chunks"][3], strings, min_tokens=m)
    assert got["toks"] == base["sampled"][3]["toks"][:second[0] + 1]
    assert _run(e, PROMPTS[3:], seeds=base["seeds"][3:], stops=[(strings, 0)])[0]["hit"] == first


def test_release_prefill_and_reset_return_the_row_to_the_root(eng, base):
    e, _ = eng
    strings, hit = base["picks"][0]
    assert _run(e, PROMPTS[:1], seeds=base["seeds"][:1], stops=[(strings, 0)])[0]["hit"] == hit      # ... and releases slot 0
    # the same slot, no stop strings: the row runs to its cap (no reset in between: the release alone cleared the row)
    e.set_row_sampling(0, _sp(base["seeds"][0]))
    e.slots_prefill([0], PROMPTS[0], [len(PROMPTS[0])], [CAP])
    e.slots_decode(CAP)
    fin, lens = e.slots_poll()
    assert fin[0] == 1 and e.slot_read(0, int(lens[0])).tolist() == base["sampled"][0]["toks"] and e.row_stop_hit(0) is None
    e.slot_release(0)
    # a second prefill of a row that keeps its stop strings starts over: same hit again, not a stale state or record
    e.slots_reset()
    e.set_row_sampling(1, _sp(base["seeds"][0]))
    e.set_row_stop(1, e.create_stop(strings), 0)
    e.slots_prefill([1], PROMPTS[0], [len(PROMPTS[0])], [CAP])
    e.slots_decode(CAP)
    assert e.row_stop_hit(1) == hit
    e.slots_reset()
    assert e.row_stop_hit(1) is None


def test_fork_children_inherit_the_stop_strings_at_the_root(eng, base):
    e, _ = eng
    seeds = [SEED + 50 + i for i in range(3)]
    same = [PROMPTS[0]] * 3
    free = _run(e, same, seeds=seeds)
    chunks = [_chunks(r["toks"]) for r in free]
    strings = [b"".join(c[9:12]).decode() for c in chunks]                          # one string from each sequence's own bytes
    hits = [first_stop(c, strings) for c in chunks]
    assert all(h is not None and h[0] < CAP - 1 for h in hits)
    independent = _run(e, same, seeds=seeds, stops=[(strings, 0)] * 3)
    e.set_sampling(0.0, 1.0, 0)
    e.slots_reset()
    e.set_eos([])
    for i in range(3):
        e.set_row_sampling(i, _sp(seeds[i]))
    e.set_row_stop(0, e.create_stop(strings), 0)                                    # the parent only: the fork hands it on
    e.slots_prefill([0], PROMPTS[0], [len(PROMPTS[0])], [CAP])
    e.slots_fork(0, [1, 2])
    e.slots_decode(CAP)
    fin, lens = e.slots_poll()
    for i in range(3):
        toks = e.slot_read(i, int(lens[i])).tolist()
        assert fin[i] == 1 and e.row_stop_hit(i) == hits[i] == independent[i]["hit"], i
        assert toks == free[i]["toks"][:hits[i][0] + 1] == independent[i]["toks"], i
    e.slots_reset()


def test_with_speculation_on_the_stop_row_and_a_greedy_neighbour_are_unchanged(eng, base):
    e, _ = eng
    strings, hit = base["picks"][0]
    e.slots_reset()
    e.set_speculation(3)
    try:
        got = _run(e, PROMPTS[:2], seeds=[base["seeds"][0], None], stops=[(strings, 0), None], chunk=4)
        stats = e.spec_stats()
    finally:
        e.slots_reset()
        e.set_speculation(0)
    assert got[0]["toks"] == base["sampled"][0]["toks"][:hit[0] + 1] and got[0]["hit"] == hit
    assert got[1]["toks"] == base["greedy"][1]["toks"]
    assert stats["steps"] > 0


def test_logprobs_cover_every_token_through_the_hit(eng, base):
    e, _ = eng
    strings, hit = base["picks"][0]
    got = _run(e, PROMPTS[:1], seeds=base["seeds"][:1], stops=[(strings, 0)], lp=[0])[0]
    ref = base["sampled"][0]["lp"]
    n = hit[0] + 1
    assert got["lp"][0].shape[0] == n and not np.isnan(got["lp"][0]).any()
    assert got["lp"][0].tobytes() == ref[0][:n].tobytes()                           # bitwise the baseline's


def test_refusals(eng):
    e, early = eng
    assert isinstance(early, DotsEngineError) and "token bytes" in str(early)       # created before set_token_bytes
    with pytest.raises(ValueError):
        e.create_stop([f"s{i}" for i in range(17)])
    with pytest.raises(ValueError):
        e.create_stop(["x" * 65])
    with pytest.raises(DotsEngineError):
        e.set_row_stop(0, 999)
