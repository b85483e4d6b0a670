"""CPU checks of tests/sample_ref.py, the numpy restatement of the sampling
definition that the GPU tests compare against row by row: the reference's own
test properties (tests/golden/sample.json), the Poisson tables, the
distributions, and the algebra between sample and random_split."""
import json
import math
import os

import numpy as np
import pytest

import sample_ref as sr

HERE = os.path.dirname(os.path.abspath(__file__))
LAMBDAS = [1e-6, 0.1, 1.0, 3.5, 16.0]


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(HERE, "golden", "sample.json")) as f:
        g = json.load(f)
    # every fixture names its op: the golden tests that walk tests/golden/*.json
    # dispatch on it and pass over the ones that are not theirs
    assert g["op"] == "sample"
    return g


def elements(g):
    lo, hi = g["range_inclusive"]
    return np.arange(lo, hi + 1, dtype=np.int64)


def test_draw_is_53_bits_and_indexed_globally():
    d = sr.draw53(42, np.arange(0, 10_000, dtype=np.uint64))
    assert d.dtype == np.uint64 and int(d.max()) < sr.ONE
    # a shard sees the slice of the global stream
    assert np.array_equal(sr.draw53(42, np.arange(7_000, 10_000, dtype=np.uint64)), d[7_000:])
    # scalar and vector hash agree
    assert int(sr.rand_u64_np(sr.hash_u64(42), [3])[0]) >> 11 == int(d[3])
    assert not np.array_equal(d, sr.draw53(43, np.arange(0, 10_000, dtype=np.uint64)))


def test_thresholds():
    assert sr.thresholds(0.0) == 0 and sr.thresholds(-1.0) == 0
    assert sr.thresholds(float("nan")) == 0
    assert sr.thresholds(1.0) == sr.ONE and sr.thresholds(1.5) == sr.ONE
    assert sr.thresholds(0.5) == 1 << 52
    assert sr.thresholds(2.0 ** -53) == 1


def test_golden_take_sample(golden):
    assert len(golden["take_sample"]) == 3
    for g in golden["take_sample"]:
        k = elements(g)
        v = np.zeros(len(k), np.int64)
        info = {}
        tk, tv = sr.take_sample_ref(k, v, g["with_replacement"], g["num"], g["seed"], info=info)
        assert len(tk) == len(tv) == g["expected_len"], g["source"]
        assert set(tk.tolist()) <= set(k.tolist())
        if g["property"] == "permutation":
            assert sorted(tk.tolist()) == k.tolist()
            assert info["attempts"] == 0
        elif g["property"] == "distinct_subset":
            assert len(set(tk.tolist())) == len(tk)
        else:
            assert g["property"] == "subset"
    # the first attempt oversamples: 145 and 33 candidates for the 100-row cases
    info = {}
    k = np.arange(100, dtype=np.int64)
    sr.take_sample_ref(k, k, True, 80, 5, info=info)
    assert info == {"attempts": 1, "candidates": 145}
    sr.take_sample_ref(k, k, False, 10, 5, info=info)
    assert info == {"attempts": 1, "candidates": 33}


def test_golden_random_split(golden):
    (g,) = golden["random_split"]
    k = elements(g)
    assert len(k) == g["expected_total"]
    sizes_by_seed = {}
    for seed in g["seeds"]:
        parts = sr.random_split_ref(k, np.zeros(len(k), np.int64), g["weights"], seed)
        assert len(parts) == g["expected_splits"]
        sizes = [len(pk) for pk, _ in parts]
        sizes_by_seed[seed] = sizes
        assert sum(sizes) == g["expected_total"]
        for got, want in zip(sizes, g["expected_sizes"]):
            assert abs(got - want) < g["size_tolerance_exclusive"], (seed, sizes)
        sets = [set(pk.tolist()) for pk, _ in parts]
        assert not (sets[0] & sets[1]) and not (sets[0] & sets[2]) and not (sets[1] & sets[2])
    assert sizes_by_seed[123] == [90, 206, 304]


@pytest.mark.parametrize("lam", LAMBDAS)
def test_poisson_table(lam):
    t = sr.poisson_table(lam).astype(np.int64)
    assert 1 <= len(t) <= 255
    assert len(t) <= 60
    assert np.all(np.diff(t) >= 0)
    assert 0 <= sr.ONE - int(t[-1]) <= 2
    assert int(t[0]) == sr.thresholds(math.exp(-lam))


def test_poisson_table_edges():
    # lambda = 0: one entry at 2^53, no draw reaches it -> the empty sample
    t = sr.poisson_table(0.0)
    assert t.tolist() == [sr.ONE]
    assert sr.sample_counts(5000, True, 0.0, 1).sum() == 0
    with pytest.raises(ValueError):
        sr.poisson_table(-0.5)
    with pytest.raises(ValueError):
        sr.poisson_table(float("nan"))
    with pytest.raises(NotImplementedError):
        sr.poisson_table(16.5)


@pytest.mark.parametrize("lam", LAMBDAS)
def test_poisson_mean_and_variance(lam):
    # fixed seed: deterministic. At 1e6 rows the standard error of the mean is
    # sqrt(lam / 1e6) — for lam = 1e-6 the 1 % window holds only because this
    # seed draws exactly one copy; the four larger lambdas sit inside it with
    # room (0.3 % standard error at lam = 0.1).
    c = sr.sample_counts(1_000_000, True, lam, 3)
    assert abs(c.mean() - lam) <= 0.01 * lam
    assert abs(c.var() - lam) <= 0.01 * lam


@pytest.mark.parametrize("n,f,seed", [(4096, 0.5, 1), (100_000, 1e-4, 1), (1_000_000, 0.3, 1)])
def test_bernoulli_counts_within_4_sigma(n, f, seed):
    kept = int(sr.sample_counts(n, False, f, seed).sum())
    sigma = math.sqrt(n * f * (1.0 - f))
    z = (kept - n * f) / sigma
    print(f"n={n} f={f} kept={kept} z={z:+.2f}")
    assert abs(z) < 4.0


def test_bernoulli_edges():
    assert sr.sample_counts(5000, False, 0.0, 9).sum() == 0
    assert sr.sample_counts(5000, False, 1.0, 9).sum() == 5000
    assert sr.sample_counts(5000, False, 1.0 + 5e-7, 9).sum() == 5000
    assert sr.sample_counts(5000, False, -5e-7, 9).sum() == 0
    with pytest.raises(ValueError):
        sr.sample_counts(10, False, 1.5, 9)
    with pytest.raises(ValueError):
        sr.sample_counts(10, False, float("nan"), 9)


def test_sample_keeps_order_and_adjacent_copies():
    k = np.arange(20_000, dtype=np.int64)
    v = k * 7
    sk, sv = sr.sample_ref(k, v, False, 0.3, 11)
    assert np.all(np.diff(sk) > 0) and np.array_equal(sv, sk * 7)
    pk, pv = sr.sample_ref(k, v, True, 2.5, 11)
    assert len(pk) > len(k) and np.all(np.diff(pk) >= 0) and np.array_equal(pv, pk * 7)
    assert np.array_equal(np.bincount(pk, minlength=len(k)),
                          sr.sample_counts(len(k), True, 2.5, 11))


@pytest.mark.parametrize("weights", [[1.0], [1, 1], [1, 2, 3], [0.2, 0.0, 0.8], [1.0] * 256,
                                     [3, 0, 0], [0, 0, 5]])
def test_splits_complete_and_disjoint(weights):
    n = 50_000
    k = np.arange(n, dtype=np.int64)
    parts = sr.random_split_ref(k, -k, weights, 77)
    assert len(parts) == len(weights)
    allk = np.concatenate([pk for pk, _ in parts])
    assert len(allk) == n and np.array_equal(np.sort(allk), k)
    for (pk, pv), w in zip(parts, weights):
        assert np.all(np.diff(pk) > 0) and np.array_equal(pv, -pk)
        if w == 0:
            assert len(pk) == 0


@pytest.mark.parametrize("weights", [[1, 2, 3], [0.25, 0.75], [5.0], [1.0] * 7])
def test_split_zero_is_the_bernoulli_sample(weights):
    k = np.arange(30_000, dtype=np.int64)
    (p0k, p0v) = sr.random_split_ref(k, k, weights, 2024)[0]
    s = 0.0
    for w in weights:
        s += float(w)
    sk, sv = sr.sample_ref(k, k, False, float(weights[0]) / s, 2024)
    assert np.array_equal(p0k, sk) and np.array_equal(p0v, sv)


def test_split_invalid_weights():
    for bad in ([], [1.0] * 257, [1.0, -0.5], [0.0, 0.0], [1.0, float("nan")]):
        with pytest.raises(ValueError):
            sr.split_bounds(bad)


def test_fraction_for_sample_size():
    # utils/random.rs:331-358
    assert sr.fraction_for_sample_size(80, 100, True) == (80 + 6 * math.sqrt(80)) / 100
    assert sr.fraction_for_sample_size(5, 100, True) == (5 + 12 * math.sqrt(5)) / 100
    assert sr.fraction_for_sample_size(10, 100, True) == (10 + 9 * math.sqrt(10)) / 100
    f = sr.fraction_for_sample_size(10, 100, False)
    gamma = -math.log(1e-4) / 100
    assert f == 0.1 + gamma + math.sqrt(gamma * gamma + 0.2 * gamma)
    assert sr.fraction_for_sample_size(99, 100, False) == 1.0


def test_take_sample_resamples_until_enough():
    """The device loop is not reachable by a real draw (undershoot probability
    below 1e-4), so the re-sample logic is exercised here with an injected
    too-small fraction."""
    k = np.arange(1000, dtype=np.int64)
    want = 60
    frac = 0.05  # mean 50 kept rows: most attempts fall short of 60
    sizes = [int(sr.sample_counts(1000, False, frac, 31 + t).sum()) for t in range(100)]
    first_ok = next(t for t, s in enumerate(sizes) if s >= want)
    assert first_ok >= 1, "seed must make the first attempt undershoot"
    info = {}
    tk, tv = sr.take_sample_ref(k, k, False, want, 31, fraction=frac, info=info)
    assert info == {"attempts": first_ok + 1, "candidates": sizes[first_ok]}
    assert len(tk) == want and len(set(tk.tolist())) == want
    # the candidates are those of sample(seed + attempt)
    ck, _ = sr.sample_ref(k, k, False, frac, 31 + first_ok)
    assert set(tk.tolist()) <= set(ck.tolist())
    # never enough: gives up after 100 attempts
    with pytest.raises(NotImplementedError):
        sr.take_sample_ref(k, k, False, 900, 31, fraction=0.05)


def test_take_sample_trivia():
    k = np.arange(50, dtype=np.int64)
    assert len(sr.take_sample_ref(k, k, False, 0, 1)[0]) == 0
    assert len(sr.take_sample_ref(k[:0], k[:0], True, 5, 1)[0]) == 0
    tk, _ = sr.take_sample_ref(k, k, False, 50, 1)
    assert sorted(tk.tolist()) == k.tolist() and tk.tolist() != k.tolist()
    # deterministic in the seed, different across seeds
    assert np.array_equal(tk, sr.take_sample_ref(k, k, False, 50, 1)[0])
    assert not np.array_equal(tk, sr.take_sample_ref(k, k, False, 50, 2)[0])
