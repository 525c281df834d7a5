"""N-gram speculative decoding, the parts that need no GPU: the drafting rule as the host states it, the server's flags and
the slot arithmetic of a speculating engine."""
import argparse

import numpy as np
import pytest

from dots_ocr_amd.engine import MAX_SPEC_DRAFTS, ngram_draft, spec_usable_slots


# ---------------------------------------------------------------------------------------------------- the drafting rule

def test_longest_n_wins():
    #        0  1  2  3  4  5  6  7  8  9 10 11 12
    hist = [1, 2, 3, 4, 50, 9, 3, 4, 60, 1, 2, 3, 4]
    # n = 4: key 1 2 3 4 matches at i = 0 -> 50 ...; the bigram 3 4 also matches at i = 6 (-> 60), more recently, but the longer key decides
    assert ngram_draft(hist, 3, 2, 4) == [50, 9, 3]
    assert ngram_draft(hist, 3, 2, 2) == [60, 1, 2]
    # n = 3 has a match of its own (2 3 4 at i = 1) and is tried before n = 2
    assert ngram_draft(hist, 1, 2, 3) == [50]


def test_most_recent_match_with_a_full_continuation_is_preferred():
    #        0  1  2  3  4  5  6  7  8  9 10 11
    hist = [7, 8, 11, 12, 13, 7, 8, 21, 22, 23, 7, 8]
    assert ngram_draft(hist, 3, 2, 2) == [21, 22, 23]           # i = 5 over i = 0: both have 3 tokens behind them
    #        0  1  2  3  4  5  6  7  8  9
    hist = [7, 8, 11, 12, 13, 7, 8, 21, 7, 8]
    # i = 5 is more recent but only 21, 7, 8 ... lies behind it: i + n + k = 5 + 2 + 4 = 11 > L = 10; i = 0 has the full 4
    assert ngram_draft(hist, 4, 2, 2) == [11, 12, 13, 7]
    assert ngram_draft(hist, 3, 2, 2) == [21, 7, 8]             # with k = 3 the recent one is full again


def test_falls_back_to_the_earliest_match_without_a_full_continuation():
    assert ngram_draft([5, 5, 5, 5], 3, 2, 2) == [5, 5]          # matches at i = 0 (2 tokens behind it) and i = 1 (1): none full, earliest
    assert ngram_draft([5, 5, 5, 5], 3, 1, 3) == [5]             # n = 3: the only match is i = 0, one token behind it
    assert ngram_draft([5, 5, 5, 5], 1, 2, 2) == [5]             # k = 1: i = 1 is full (1 + 2 + 1 <= 4) and the most recent
    #        0  1  2  3  4  5  6
    hist = [1, 2, 9, 1, 2, 8, 1, 2]
    assert ngram_draft(hist, 7, 2, 2) == [9, 1, 2, 8, 1, 2]      # nothing is full with k = 7: the earliest match gives the most


def test_short_histories_draft_nothing():
    assert ngram_draft([], 3, 2, 4) == []
    assert ngram_draft([4], 3, 2, 4) == []
    assert ngram_draft([4, 4], 3, 2, 4) == []                    # L = min_n: n + 1 <= L fails for every n
    assert ngram_draft([4, 4, 4], 3, 2, 4) == [4]                # L = min_n + 1: the first history that can match
    assert ngram_draft([4, 4], 3, 1, 4) == [4]


def test_no_match_drafts_nothing():
    assert ngram_draft(list(range(100, 140)), 3, 1, 4) == []
    assert ngram_draft([1, 2, 3, 1, 3, 2, 2, 1], 3, 2, 4) == []   # every unigram repeats, no bigram does


def test_k_larger_than_what_remains():
    #        0  1  2  3  4
    hist = [1, 2, 3, 1, 2]
    assert ngram_draft(hist, 15, 2, 4) == [3, 1, 2]              # three tokens lie behind the match, whatever k asks for
    assert ngram_draft(hist, 2, 2, 4) == [3, 1]
    assert len(ngram_draft(hist, MAX_SPEC_DRAFTS, 2, 2)) == 3


def test_the_rule_against_a_brute_force_restatement():
    """every (history, k, min_n, max_n) of a small random family: the list comprehension of engine.ngram_draft against explicit loops"""
    def brute(out, k, lo, hi):
        L = len(out)
        for n in range(hi, lo - 1, -1):
            if n + 1 > L:
                continue
            best_full, first = None, None
            for i in range(0, L - n):
                if all(out[i + j] == out[L - n + j] for j in range(n)):
                    if first is None:
                        first = i
                    if i + n + k <= L:
                        best_full = i
            i = best_full if best_full is not None else first
            if i is not None:
                return out[i + n:min(i + n + k, L)]
        return []
    rng = np.random.default_rng(5)
    for _ in range(400):
        L = int(rng.integers(0, 40))
        out = [int(t) for t in rng.integers(0, 4, L)]
        k, lo = int(rng.integers(1, 8)), int(rng.integers(1, 4))
        hi = lo + int(rng.integers(0, 4))
        assert ngram_draft(out, k, lo, hi) == brute(out, k, lo, hi), (out, k, lo, hi)


def test_bad_arguments_raise():
    for k, lo, hi in ((0, 2, 4), (3, 0, 4), (3, 3, 2)):
        with pytest.raises(ValueError):
            ngram_draft([1, 2, 3], k, lo, hi)


# ---------------------------------------------------------------------------------------------------- server flags

def _parse(*argv):
    from dots_ocr_amd.server import build_arg_parser
    return build_arg_parser().parse_args(list(argv))


def test_server_flags_default_to_no_speculation():
    from dots_ocr_amd.server import speculation_args
    a = _parse()
    assert a.speculative_ngram == 0 and a.prompt_lookup_min == 2 and a.prompt_lookup_max == 4
    assert speculation_args(a) is None
    assert speculation_args(_parse("--prompt-lookup-max", "9")) is None          # the lookup sizes alone switch nothing on


def test_server_flags_parse_to_the_engine_setting():
    from dots_ocr_amd.server import speculation_args
    assert speculation_args(_parse("--speculative-ngram", "3")) == (3, 2, 4)
    assert speculation_args(_parse("--speculative-ngram", "7", "--prompt-lookup-min", "1", "--prompt-lookup-max", "6", "--max-batch", "16")) == (7, 1, 6)
    assert speculation_args(_parse("--speculative-ngram", "7", "--max-batch", "8")) == (7, 2, 4)      # one request at a time


@pytest.mark.parametrize("argv", [
    ("--speculative-ngram", "16"),                                        # above DOTS_MAX_SPEC_DRAFTS
    ("--speculative-ngram", "-1"),
    ("--speculative-ngram", "3", "--prompt-lookup-min", "0"),
    ("--speculative-ngram", "3", "--prompt-lookup-min", "5", "--prompt-lookup-max", "4"),
    ("--speculative-ngram", "3", "--prompt-lookup-max", "65"),             # above DOTS_MAX_NGRAM_SIZE
    ("--speculative-ngram", "3", "--static-batching"),
    ("--speculative-ngram", "8", "--max-batch", "8"),                      # 9 rows per request
])
def test_server_flags_refuse_what_the_engine_would(argv):
    from dots_ocr_amd.server import speculation_args
    with pytest.raises(ValueError):
        speculation_args(_parse(*argv))


def test_server_flag_needs_an_integer():
    with pytest.raises(SystemExit):
        _parse("--speculative-ngram", "many")


# ---------------------------------------------------------------------------------------------------- slot arithmetic

class FakeEngine:
    """what ContinuousBatcher's constructor touches, plus the slot rule of a speculating engine"""
    max_patches, max_prefill_tokens, max_seq_len = 64, 4096, 640

    def __init__(self, max_batch, k=None):
        self.max_batch = max_batch
        if k is not None:
            self.usable_slots = spec_usable_slots(max_batch, k)
        self.prefills = []

    def set_eos(self, ids):
        pass

    def slots_reset(self):
        pass

    def kv_pool_info(self):
        return 1000, 1000

    def slots_prefill(self, slots, ids, lens, caps):
        assert all(s < getattr(self, "usable_slots", self.max_batch) for s in slots)
        self.prefills.append(list(slots))


@pytest.mark.parametrize("max_batch,k,slots", [(16, 0, 16), (16, 1, 8), (16, 3, 4), (40, 4, 8), (64, 15, 4), (8, 7, 1), (64, 2, 21), (10, 3, 2), (3, 3, 0)])
def test_usable_slots_is_max_batch_over_rows_per_slot(max_batch, k, slots):
    assert spec_usable_slots(max_batch, k) == slots == max_batch // (k + 1)


def test_batcher_follows_the_engines_usable_slots():
    from dots_ocr_amd.scheduler import ContinuousBatcher, Request
    assert ContinuousBatcher(FakeEngine(16)).n_slots == 16             # an engine without the attribute: every slot, as before
    assert ContinuousBatcher(FakeEngine(16, 0)).n_slots == 16
    eng = FakeEngine(16, 3)
    cb = ContinuousBatcher(eng)
    assert cb.n_slots == 4 and cb.free_slots() == [0, 1, 2, 3]
    for i in range(6):
        cb.submit(Request(np.arange(5, dtype=np.int32) + i, max_new_tokens=8))
    group = cb.plan_admission()
    assert [s for s, _, _ in group] == [0, 1, 2, 3] and len(cb.pending) == 2      # two requests wait for a slot although 12 rows are idle
    cb._prefill(group)
    assert eng.prefills == [[0, 1, 2, 3]] and cb.free_slots() == []


def test_engine_property_uses_the_same_arithmetic():
    from dots_ocr_amd.engine import Engine
    e = object.__new__(Engine)                  # no library, no GPU: the property reads two attributes
    e.max_batch = 40
    assert e.usable_slots == 40
    e.spec_k = 4
    assert e.usable_slots == 8
    e.h = None                                  # nothing for __del__ to destroy
