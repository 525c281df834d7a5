"""The inputs of test_sampling_exact_gpu.py judged WITHOUT a GPU (tests/sampling_reference.py): on every case the definition of DESIGN
§6.1 is decisive (the nucleus boundary is 1e-3 of the mass away from top_p on both sides), a kept set wrong by one key group sends at
least 8 of the 256 draws outside the accepted sets, the case takes the code path it is named for, and the accepted sets stay small."""
import functools

import numpy as np
import pytest

import sampling_reference as sr

CASES = {c.name: c for c in sr.cases()}
DRAWS = sr.draws()


@functools.lru_cache(maxsize=None)
def judged(name):
    c = CASES[name]
    K = c.kept()
    cdf = sr.cdf_of(K.w, K.mask())
    us = [sr.row_u(s, n) for s, n in DRAWS]
    return c, K, cdf, us, [set(cdf.accepted(u, sr.DELTA).tolist()) for u in us]


def test_splitmix64_matches_hand_computed_values():
    # x = 0: z = 0x9E3779B97F4A7C15; (z ^ z >> 30) * 0xBF58476D1CE4E5B9, (z ^ z >> 27) * 0x94D049BB133111EB, z ^ z >> 31 (mod 2^64):
    # the first output of the published SplitMix64 generator seeded with 0, and its second (state 2 * 0x9E37...: x = the golden gamma)
    assert sr.splitmix64(0) == 0xE220A8397B1DCDAF
    assert sr.splitmix64(0x9E3779B97F4A7C15) == 0x6E789E6AA1B965F4
    assert sr.row_u(0, 0) == sr.splitmix64(0 ^ 0xE220A8397B1DCDAF) / 2.0 ** 64
    assert sr.step_u(5, 3, 7) == (sr.splitmix64(5 ^ sr.splitmix64((3 << 32) | 7)) >> 40) / 2.0 ** 24


def test_draws_cover_the_seed_corners_and_every_counter():
    seeds = [s for s, _ in DRAWS]
    assert len(DRAWS) == 256 and len(set(seeds)) == 256 and {0, 2 ** 63, 2 ** 64 - 1} <= set(seeds)
    assert {n for _, n in DRAWS} == set(sr.COUNTERS)
    # two rows that differ only in n draw different u: the counter is live in every call
    assert len({sr.row_u(7, n) for n in sr.COUNTERS}) == len(sr.COUNTERS)


def test_reference_arithmetic_is_fp32_and_monotone():
    row = np.array([3.0, 1.0, 3.0, -40.0, -np.inf, 2.9999998], np.float32)
    t = sr.tempered(row, 0.7)
    inv = np.float32(1.0) / np.float32(0.7)
    assert t.dtype == np.float32 and t[0] == 0 and t[1] == np.float32(-2.0) * inv and t[4] == -np.inf
    k = sr.keys_of(t)
    assert k[0] == k[2] == 0 and k[5] > 0 and k[1] > k[5] and k[3] > k[1]
    w = sr.weights_of(t)
    assert w[0] == 2 ** 40 and w[3] == 0 and w[4] == 0 and w[1] == int(np.floor(np.exp(np.float64(t[1])) * 2.0 ** 40))
    assert sr.bins_of(np.array([0.0, -27.0, -0.0132, -0.0131], np.float32)).tolist() == [0, 2047, 1, 0]


@pytest.mark.parametrize("name", list(CASES))
def test_case_keeps_what_it_is_named_for(name):
    c, K, cdf, us, acc = judged(name)
    kept = int(K.mask().sum())
    assert kept >= 1 and kept == len(cdf.idx)
    if c.keeps is not None:
        assert kept == c.keeps, (kept, c.keeps)
    assert not np.any(K.mask() & ~(K.t >= -sr.TCUT))
    # what is out of range is never accepted, under any u
    assert all(K.t[j] >= -sr.TCUT for a in acc for j in a)


@pytest.mark.parametrize("name", list(CASES))
def test_case_nucleus_is_decisive(name):
    c, K, *_ = judged(name)
    if not np.float32(c.top_p) < 1:
        assert K.frac_incl is None
        return
    assert K.frac_incl is not None
    p = float(np.float32(c.top_p))
    assert K.frac_incl - p >= sr.DECISIVE, (K.frac_before, K.frac_incl)
    assert p - K.frac_before >= sr.DECISIVE or K.frac_before == 0.0, (K.frac_before, K.frac_incl)


@pytest.mark.parametrize("name", list(CASES))
def test_case_shows_a_kept_set_wrong_by_one_key_group(name):
    c, K, cdf, us, acc = judged(name)
    muts = K.mutants()
    filtered = c.top_k > 0 or np.float32(c.top_p) < 1
    if filtered and int(K.mask().sum()) >= 2 and c.V > 2:
        assert muts, "a filtered case with two kept tokens must have a mutant"
    for kind, mask in muts.items():
        m = sr.cdf_of(K.w, mask)
        caught = sum(m.exact(u) not in a for u, a in zip(us, acc))
        assert caught >= sr.MIN_CAUGHT, (kind, caught)


@pytest.mark.parametrize("name", list(CASES))
def test_case_takes_its_path(name):
    c, K, *_ = judged(name)
    assert K.path == c.path, (K.path, K.info)
    e, i = c.expect, K.info
    if "kb" in e:
        assert i["kb"] is None
    if e.get("p_bin_is_kb"):
        assert i["kb"] is not None and i["p_bin"] == i["kb"] and K.k_groups is not None
    if e.get("far_bin"):
        assert i["p_bin"] >= 16
    if e.get("pb_below_kb"):
        assert i["pb_lo"] < i["kb"]
    if e.get("boundary_bins_over_cap"):
        assert all(n > sr.CAP for n in (i["count_kb"], i["count_pb"]) if n is not None)
    if "n_boundary" in e:
        assert i["n_boundary"] == e["n_boundary"] and i["g_lo"] == i["g_hi"]
        assert K.gcount[3:7].tolist() == [2048, 2048, 2048, e["n_boundary"] - 3 * 2048]           # 4 tied groups behind the head
        assert K.k_groups == 5                                                                   # k ends in the second of them


@pytest.mark.parametrize("name", list(CASES))
def test_case_accepted_sets_are_sharp(name):
    c, K, cdf, us, acc = judged(name)
    sizes = [len(a) for a in acc]
    assert min(sizes) >= 1
    assert np.mean(sizes) <= sr.MAX_MEAN_ACCEPTED, np.mean(sizes)
    exact = [cdf.exact(u) for u in us]
    assert all(x in a for x, a in zip(exact, acc))
    if len(cdf.idx) >= 2:
        assert len(set(exact)) >= 2


def test_ragged_cases_draw_from_the_first_and_the_last_wave():
    for V in (63, 64, 65, 1000, 1025, 1087):
        for kind in ("kp", "all"):
            c, K, cdf, us, acc = judged(f"ragged_{V}_{kind}")
            seg = -(-V // 16)
            waves = {cdf.exact(u) // seg for u in us}
            assert 0 in waves and (V - 1) // seg in waves, (V, kind, sorted(waves))


def test_step_sampler_reference_accepts_its_own_draws():
    rng = np.random.default_rng(3)
    row = rng.normal(0.0, 2.0, 1024).astype(np.float32)
    cdf = sr.step_cdf(row, 0.8)
    assert len(cdf.idx) == 1024 and cdf.hi[-1] == 1.0
    sizes = []
    for slot in range(2):
        for pos in range(16):
            u = sr.step_u(11, slot, pos)
            a = cdf.accepted(u, sr.STEP_DELTA)
            assert cdf.exact(u) in a
            sizes.append(len(a))
    assert np.mean(sizes) <= sr.MAX_MEAN_ACCEPTED
