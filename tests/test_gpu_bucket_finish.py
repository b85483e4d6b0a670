"""The finish route of the hash grouping sort (three hash passes, then
k_bucket_finish) must leave exactly the rows the four-pass route leaves, row
for row: vega_dev_group_rows_i64 runs either route on inputs from
tests/bucket_keys.py whose buckets sit against the kernel's tile edges, exceed
its caps, or look like the benchmark's. Values are the input row index, so a
stability slip shows as well.
"""
import numpy as np
import pytest

import bucket_keys as bk
import seg_layout as sl

pytestmark = pytest.mark.gpu

FT = bk.FT


def group_rows(k, v, route):
    import torch
    from vega_amd import gpu
    kt = torch.from_numpy(np.ascontiguousarray(k)).cuda()
    vt = torch.from_numpy(np.ascontiguousarray(v).view(np.int64)).cuda()
    ok, ov = torch.empty_like(kt), torch.empty_like(vt)
    taken = gpu.dev_group_rows(kt, vt, route, ok, ov, gpu.alloc_ws(len(k)))
    return ok.cpu().numpy(), ov.cpu().numpy(), taken


def assert_same_rows(a, b):
    assert (a[0] == b[0]).all(), f"keys differ at rows {np.flatnonzero(a[0] != b[0])[:8]}"
    assert (a[1] == b[1]).all(), f"values differ at rows {np.flatnonzero(a[1] != b[1])[:8]}"


def assert_grouped(lay, gk, gv):
    """a permutation of the input with equal keys adjacent"""
    assert (lay.k[gv] == gk).all() and (np.sort(gv) == lay.v).all()
    heads = 1 + int((gk[1:] != gk[:-1]).sum()) if len(gk) else 0
    assert heads == len(np.unique(lay.k))


def test_crafted_buckets_match_four_pass_route():
    lay = bk.crafted()
    r1 = group_rows(lay.k, lay.v, 1)
    r2 = group_rows(lay.k, lay.v, 2)
    assert r1[2] == 1 and r2[2] == 2
    assert_same_rows(r2, r1)
    assert_grouped(lay, r2[0], r2[1])
    # hash order: the order tests/seg_layout.py predicts runs in
    assert (np.diff(sl.h32(r2[0]).astype(np.int64)) >= 0).all()


def test_oversized_buckets_fall_back():
    lay = bk.oversized()
    r1 = group_rows(lay.k, lay.v, 1)
    r2 = group_rows(lay.k, lay.v, 2)
    assert r1[2] == 1 and r2[2] == 1
    assert_same_rows(r2, r1)
    assert_grouped(lay, r2[0], r2[1])


def test_dirty_run_of_65_takes_the_key_sort():
    lay = bk.dirty_run()
    r1 = group_rows(lay.k, lay.v, 1)
    r2 = group_rows(lay.k, lay.v, 2)
    assert r2[2] == 1
    assert_same_rows(r2, r1)
    assert_grouped(lay, r2[0], r2[1])
    # the fallback is the full unsigned key sort, stable
    o = np.argsort(lay.k.view(np.uint64), kind="stable")
    assert (r2[0] == lay.k[o]).all() and (r2[1] == o).all()


@pytest.mark.parametrize("n", [1, 2, 63, FT - 1, FT, FT + 1, 2 * FT + 255])
def test_sizes(n):
    lay = bk.distinct(n, seed=n)
    r1 = group_rows(lay.k, lay.v, 1)
    r2 = group_rows(lay.k, lay.v, 2)
    assert r2[2] == (2 if n >= 2 else 0)
    assert_same_rows(r2, r1)
    assert_grouped(lay, r2[0], r2[1])


def test_persistent_blocks_walk_several_tiles():
    """more tiles than blocks (the grid is 512), a count that is no multiple
    of 8 and a ragged last tile: every block restages LDS for a second and a
    third tile from its prefetched registers"""
    n = 1100 * FT + 77
    rng = np.random.RandomState(11)
    k = bk.keys_for_hashes(bk.make_h64(rng.randint(0, 1 << 15, size=n),
                                       rng.randint(0, 256, size=n), rng.permutation(n)))
    lay = bk.Layout(k, [], [])
    assert len(np.unique(k)) == n and np.bincount(bk.bucket_of(k)).max() <= bk.BUCKET_CAP
    r1 = group_rows(lay.k, lay.v, 1)
    r2 = group_rows(lay.k, lay.v, 2)
    assert r1[2] == 1 and r2[2] == 2
    assert_same_rows(r2, r1)
    assert_grouped(lay, r2[0], r2[1])


# ---- through the public entry, benchmark-like buckets ----

@pytest.fixture(scope="module")
def poisson():
    """the input, f64 values for SUM_F64, and route 1's grouped rows"""
    lay = bk.poisson()
    vf = np.random.RandomState(7).uniform(-1.0, 1.0, size=lay.n)
    gk, gv, taken = group_rows(lay.k, lay.v, 1)
    assert taken == 1
    return lay, vf, gk, gv


def reduce_in_order(op, gk, vals):
    """segmented reduce of grouped rows, output in their order"""
    starts = np.flatnonzero(np.concatenate([[True], gk[1:] != gk[:-1]]))
    lens = np.diff(np.concatenate([starts, [len(gk)]]))
    if op == sl.OP_COUNT:
        return gk[starts], lens.astype(np.int64)
    if op == sl.OP_SUM_I64:
        return gk[starts], np.add.reduceat(vals.view(np.uint64), starts).view(np.int64)
    if op == sl.OP_MIN_I64:
        return gk[starts], np.minimum.reduceat(vals, starts)
    if op == sl.OP_MAX_I64:
        return gk[starts], np.maximum.reduceat(vals, starts)
    assert (lens == 1).all()     # f64: one row per key, the sum is the row
    return gk[starts], vals[starts]


def sort_reduce_profiled(k, v, op):
    import torch
    from vega_amd import gpu
    kt = torch.from_numpy(k).cuda()
    vt = torch.from_numpy(v).cuda()
    out_k, out_v = torch.empty_like(kt), torch.empty_like(vt)
    ws = gpu.alloc_ws(len(k))
    gpu.prof_stats()
    gpu.prof_enable(True)
    try:
        nout = gpu.dev_sort_reduce(kt, vt, op, out_k, out_v, ws)
        torch.cuda.synchronize()
        stats = gpu.prof_stats()
    finally:
        gpu.prof_enable(False)
    return out_k[:nout].cpu().numpy(), out_v[:nout].cpu().numpy(), stats


@pytest.mark.parametrize("op", ["SUM_I64", "COUNT", "MIN_I64", "MAX_I64", "SUM_F64"])
def test_sort_reduce_takes_finish_route(poisson, op):
    lay, vf, gk, gv = poisson
    f64 = op == "SUM_F64"
    v = vf if f64 else lay.v
    out_k, out_v, stats = sort_reduce_profiled(lay.k, v, sl.OPS[op])
    assert "bucket_finish" in stats and stats["bucket_finish"]["n"] == 1, stats
    assert stats["radix_scatter"]["n"] == 3, stats
    for name in ("ghist", "group_cleanup", "head_count", "seg_emit"):
        assert stats[name]["n"] == 1, stats
    assert "hist8" not in stats
    ek, ev = reduce_in_order(sl.OPS[op], gk, v[gv])
    assert (out_k == ek).all(), "keys are not in the four-pass route's order"
    assert (out_v.view(np.int64) == ev.view(np.int64)).all()


def test_sampled_repeat_takes_four_pass_route(poisson):
    lay = bk.with_sampled_repeat(poisson[0])
    out_k, out_v, stats = sort_reduce_profiled(lay.k, lay.v, sl.OP_SUM_I64)
    assert "bucket_finish" not in stats, stats
    assert stats["radix_scatter"]["n"] == 4 and stats["group_cleanup"]["n"] == 1, stats
    gk, gv, taken = group_rows(lay.k, lay.v, 1)
    ek, ev = reduce_in_order(sl.OP_SUM_I64, gk, lay.v[gv])
    assert (out_k == ek).all() and (out_v == ev).all()


def test_sparse_buckets_take_four_pass_route():
    """3e5 keys spread over all 2^24 buckets: far below one row per bucket, so
    the automatic route keeps the four passes"""
    rng = np.random.RandomState(12)
    k = bk.keys_for_hashes(rng.randint(0, 2**64, size=300_000, dtype=np.uint64))
    v = np.arange(len(k), dtype=np.int64)
    assert len(np.unique(k[bk.sampled_positions(len(k))])) == 2048
    out_k, out_v, stats = sort_reduce_profiled(k, v, sl.OP_SUM_I64)
    assert "bucket_finish" not in stats and stats["radix_scatter"]["n"] == 4, stats
    gk, gv, taken = group_rows(k, v, 0)
    assert taken == 1
    ek, ev = reduce_in_order(sl.OP_SUM_I64, gk, v[gv])
    assert (out_k == ek).all() and (out_v == ev).all()
