"""The rows-per-bucket estimate behind the automatic route of the grouping
sort (vega_diag_bucket_rows; host arithmetic, no GPU): route 0 takes the
bucket finish only from GATE rows per bucket. Inputs with chosen bucket ids
come from tests/bucket_keys.py."""
import numpy as np
import pytest

import bucket_keys as bk

GATE = 24.0      # FIN_MIN_BUCKET_ROWS
NS = bk.NSAMPLE


def estimate(keys, n):
    from vega_amd import gpu
    return gpu.diag_bucket_rows(np.ascontiguousarray(keys, dtype=np.int64), n)


def sample_from_buckets(nbuckets, seed, ns=NS):
    """ns keys whose buckets are drawn evenly from nbuckets ids"""
    rng = np.random.RandomState(seed)
    ids = np.unique(rng.randint(0, 1 << 24, size=2 * nbuckets))[:nbuckets]
    assert len(ids) == nbuckets
    return bk.keys_for_hashes(bk.make_h64(ids[rng.randint(0, nbuckets, size=ns)],
                                          rng.randint(0, 256, size=ns),
                                          rng.randint(0, 1 << 32, size=ns, dtype=np.uint64)))


def test_spread_keys_count_all_buckets():
    """fewer than 8 coinciding bucket ids: all 2^24 buckets assumed, so the
    verdict is n alone and the gate opens at 24 * 2^24 rows"""
    k = bk.keys_for_hashes(np.random.RandomState(1).randint(0, 2**64, size=NS, dtype=np.uint64))
    assert NS - len(np.unique(bk.bucket_of(k))) < 8
    for n in (10**8, 4 * 10**8, 10**9, 1 << 30):
        assert estimate(k, n) == n / 2.0**24
    assert estimate(k, 4 * 10**8) < GATE <= estimate(k, 24 << 24)


@pytest.mark.parametrize("nbuckets", [500, 5000, 50_000])
def test_bisection_recovers_the_bucket_count(nbuckets):
    """d distinct ids among ns draws from B buckets: B (1 - exp(-ns / B)) = d.
    The estimate rests on the c = ns - d coinciding draws, a count with
    relative scatter 1 / sqrt(c); the bound is three of those, c taken at its
    expectation."""
    k = sample_from_buckets(nbuckets, seed=nbuckets)
    c = NS - nbuckets * (1.0 - np.exp(-NS / nbuckets))
    assert c >= 8 and NS - len(np.unique(bk.bucket_of(k))) >= 8
    n = 60 * nbuckets
    assert abs(estimate(k, n) / 60.0 - 1.0) < 3.0 / np.sqrt(c)


def test_narrow_miss_below_the_gate():
    """enough coinciding ids for the bisection, yet too few rows per bucket:
    15 rows in each of 50000 buckets stays on the four-pass route, 40 does not"""
    k = sample_from_buckets(50_000, seed=3)
    assert estimate(k, 15 * 50_000) < GATE < estimate(k, 40 * 50_000)


def test_benchmark_like_input_passes_the_gate():
    lay = bk.poisson()
    est = estimate(lay.k[bk.sampled_positions(lay.n)], lay.n)
    assert GATE < est and abs(est / 60.0 - 1.0) < 3.0 / np.sqrt(368)   # c for 5000 buckets


def test_short_samples():
    assert estimate(np.array([5], dtype=np.int64), 1) == 1 / 2.0**24
    k = np.full(NS, 7, dtype=np.int64)      # one bucket: d = 1
    assert estimate(k, 1000) > 100
