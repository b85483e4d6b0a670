"""Strategy switches of group_sort_u64 (and pass skipping in radix_sort_u64)
that uniform / Zipf data never reaches:

  - the strided 2048-row sample sees narrow keys, the exact histogram does
    not: exact_hists runs twice and the hash path takes over;
  - active key bytes that are not contiguous: the pass list is sparse, and
    gbase_d + p*256 / the packed-unpacked pass chain are indexed through it;
  - six active bytes: one too many for the narrow strategy;
  - keys in [-8, 8): all eight bytes active with only 16 runs, and a signed
    top byte with two live digits for sort_by_key.

Each case runs reduce_by_key(SUM_I64) and group_count against the numpy
reducers of tests/seg_layout.py and asserts, through the kernel statistics,
which strategy ran.
"""
import numpy as np
import pytest

import seg_layout as sl

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from vega_amd import gpu
    with gpu.VegaContext() as c:
        yield c


def profiled(ctx, fn):
    ctx.set_profiling(True)
    try:
        out = fn()
        stats = ctx.kernel_stats()
    finally:
        ctx.set_profiling(False)
    return out, stats


def check_reduce_and_count(ctx, k, seed, check_stats):
    from vega_amd import gpu
    v = np.random.RandomState(seed).randint(sl.I64_MIN, sl.I64_MAX, size=len(k), dtype=np.int64)
    rdd = ctx.make_rdd(k, v)
    for op, fn in ((sl.OP_SUM_I64, lambda: rdd.reduce_by_key(gpu.OP_SUM_I64)),
                   (sl.OP_COUNT, rdd.group_count)):
        red, stats = profiled(ctx, fn)
        check_stats(set(stats))
        gk, gv = red.collect()
        rk, rv = sl.reduce_ref(op, k, v)
        assert len(gk) == len(rk)
        assert sl.sorted_pairs(gk, gv) == sl.sorted_pairs(rk, rv)
        red.free()
    rdd.free()


def check_sort(ctx, k):
    """stable signed order, values = row index"""
    rdd = ctx.make_rdd(k, np.arange(len(k), dtype=np.int64))
    srt = rdd.sort_by_key()
    gk, gv = srt.collect()
    o = np.argsort(k, kind="stable")
    assert (gk == k[o]).all(), "keys not in signed ascending order"
    assert (gv == o).all(), "stability violated (values out of row order)"
    rdd.free(); srt.free()


def narrow_ran(names):
    assert "hist8" in names and not ({"ghist", "group_cleanup"} & names), names


def hash_ran(names):
    assert {"ghist", "group_cleanup"} <= names and "hist8" not in names, names


def keys_with_bytes(positions, n, seed, pool=3000):
    """n rows drawn from `pool` keys whose bytes are random at `positions`
    and zero elsewhere (so runs have ~n/pool rows)"""
    rng = np.random.RandomState(seed)
    u = np.zeros(pool, dtype=np.uint64)
    for p in positions:
        u |= rng.randint(0, 256, size=pool).astype(np.uint64) << np.uint64(8 * p)
    k = u.view(np.int64)[rng.randint(0, pool, size=n)]
    assert sl.active_bytes(k) == sorted(positions)
    return k


def test_sample_says_narrow_exact_says_wide(ctx):
    n = 2048 * 40 + 17
    rng = np.random.RandomState(41)
    pool = sl.draw_wide_keys(5000, rng)
    k = pool[rng.randint(0, len(pool), size=n)]
    sampled = np.arange(2048) * (n // 2048)      # the rows k_sample_keys reads
    assert n // 2048 == 40
    k[sampled] = rng.randint(0, 1 << 16, size=2048)
    assert len(sl.active_bytes(k[sampled])) <= 5 and len(sl.active_bytes(k)) == 8

    def both_ran(names):   # narrow attempt (exact key hist), then the hash path
        assert {"hist8", "ghist", "group_cleanup"} <= names, names
    check_reduce_and_count(ctx, k, 42, both_ran)


@pytest.mark.parametrize("positions", [(1, 6), (0, 3, 7), (0, 2, 4, 6, 7)],
                         ids=lambda p: "bytes" + "".join(map(str, p)))
def test_noncontiguous_active_bytes(ctx, positions):
    k = keys_with_bytes(positions, 50_021, seed=sum(positions))
    if 7 in positions:
        assert (k < 0).any() and (k >= 0).any()
    check_reduce_and_count(ctx, k, 43, narrow_ran)
    check_sort(ctx, k)


def test_six_active_bytes_takes_hash_path(ctx):
    k = keys_with_bytes((0, 1, 2, 4, 6, 7), 50_021, seed=6)
    check_reduce_and_count(ctx, k, 44, hash_ran)
    check_sort(ctx, k)


def test_small_negative_keys(ctx):
    k = np.random.RandomState(8).randint(-8, 8, size=40_003).astype(np.int64)
    assert sl.active_bytes(k) == list(range(8)) and len(np.unique(k)) == 16
    check_reduce_and_count(ctx, k, 45, hash_ran)
    check_sort(ctx, k)
