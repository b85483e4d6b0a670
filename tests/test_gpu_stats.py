"""stats_by_key: combine_by_key with C = (count, sum, min, max) in one grouping
sort and one segmented pass (k_head_count<PK> + k_seg_stats<PK>).

The edge inputs are those of test_gpu_segreduce.py (tests/seg_layout.py puts
runs on every chunk / wave / tile edge the kernel distinguishes; k_seg_stats
keeps k_seg_emit's geometry). All four columns are integer, so every
comparison is bit for bit.
"""
import ctypes
import functools

import numpy as np
import pytest

import oracle_ctypes as oc
import seg_layout as sl
from vega_amd import datagen

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_UNSUPPORTED, ERR_CAP = -1, -4, -5
STAT_OPS = (sl.OP_COUNT, sl.OP_SUM_I64, sl.OP_MIN_I64, sl.OP_MAX_I64)

LAYOUTS = {"soa0": (lambda: sl.soa_layout(0), "narrow"),
           "soa3": (lambda: sl.soa_layout(3), "narrow"),
           "hash_minus1": (lambda: sl.hash_layout(True), "hash"),
           "hash_plain": (lambda: sl.hash_layout(False), "hash")}
VALUES = {"minmax": (sl.values_minmax, 11), "sum": (sl.values_sum_i64, 12)}


@pytest.fixture(scope="module")
def ctx():
    from vega_amd import gpu
    with gpu.VegaContext() as c:
        yield c


# ---- inputs and references: built once, shared, never modified ----

@functools.lru_cache(maxsize=None)
def layout(name):
    lay = LAYOUTS[name][0]()
    lay.k.setflags(write=False)
    return lay


@functools.lru_cache(maxsize=None)
def values(name, what):
    gen, seed = VALUES[what]
    v = gen(layout(name), np.random.RandomState(seed))
    v.setflags(write=False)
    return v


def stats_ref(k, v):
    """(keys ascending, count, sum, min, max): the four numpy reducers of
    seg_layout on the SAME value column"""
    cols = [sl.reduce_ref(op, k, v) for op in STAT_OPS]
    for rk, _ in cols[1:]:
        assert (rk == cols[0][0]).all()
    return (cols[0][0],) + tuple(c[1] for c in cols)


@functools.lru_cache(maxsize=None)
def layout_ref(name, what):
    return stats_ref(layout(name).k, values(name, what))


def by_key(cols):
    o = np.argsort(cols[0], kind="stable")
    return tuple(np.asarray(c)[o] for c in cols)


def assert_stats_equal(got, ref):
    got = by_key(got)
    assert len(got[0]) == len(ref[0])
    for name, g, r in zip(("key", "count", "sum", "min", "max"), got, ref):
        assert g.dtype == np.int64
        bad = np.flatnonzero(g != r)
        assert len(bad) == 0, (name, len(bad), got[0][bad][:5], g[bad][:5], r[bad][:5])


def assert_kernels(stats, strategy):
    """one head count, one fused pass, no single-op pass; and the grouping
    strategy that hands over packed (hash) or SoA (narrow) rows"""
    names = set(stats)
    assert stats["seg_stats"]["n"] == 1 and stats["head_count"]["n"] == 1, stats
    assert "seg_emit" not in names, names
    if strategy == "hash":
        assert {"ghist", "group_cleanup"} <= names and "hist8" not in names, names
    else:
        assert "hist8" in names and not ({"ghist", "group_cleanup"} & names), names


def profiled(ctx, fn):
    ctx.set_profiling(True)
    try:
        out = fn()
        stats = ctx.kernel_stats()
    finally:
        ctx.set_profiling(False)
    return out, stats


def wrap64(x):
    return ((int(x) + (1 << 63)) % (1 << 64)) - (1 << 63)


def still_answers(ctx):
    """the context computes a normal reduce_by_key correctly"""
    from vega_amd import gpu
    k = np.arange(1000, dtype=np.int64) % 37
    v = np.arange(1000, dtype=np.int64) * 3 - 500
    rdd = ctx.make_rdd(k, v)
    red = rdd.reduce_by_key(gpu.OP_SUM_I64)
    assert sl.sorted_pairs(*red.collect()) == sl.sorted_pairs(*sl.reduce_ref(sl.OP_SUM_I64, k, v))
    rdd.free(); red.free()


# ---- 1. edges, both layouts ----

@pytest.mark.parametrize("what", sorted(VALUES))
@pytest.mark.parametrize("name", sorted(LAYOUTS))
def test_stats_edges(ctx, name, what):
    lay = layout(name)
    rdd = ctx.make_rdd(lay.k, values(name, what))
    st, kstats = profiled(ctx, rdd.stats_by_key)
    assert_kernels(kstats, LAYOUTS[name][1])
    got = st.collect()
    assert len(got) == 5 and len(got[0]) == len(lay.run_lens)
    assert st.count() == len(lay.run_lens)
    assert_stats_equal(got, layout_ref(name, what))
    gk, gv = rdd.collect()          # input untouched
    assert (gk == lay.k).all() and (gv == values(name, what)).all()
    rdd.free(); st.free()


# ---- 2. hot key ----

def test_stats_hot_key(ctx):
    """one key over three tiles and five rows: tiles without any head, so the
    wave-combined tail flush carries all four fields"""
    n = 3 * 4096 + 5
    key = (1 << 45) + 7
    rng = np.random.RandomState(21)
    v = rng.randint(-(1 << 40), 1 << 40, size=n, dtype=np.int64)
    v[-1] = sl.I64_MIN
    v[5000] = sl.I64_MAX
    k = np.full(n, key, dtype=np.int64)
    rk, sums = sl.exact_int_sums(k, v)
    assert rk.tolist() == [key]
    rdd = ctx.make_rdd(k, v)
    st = rdd.stats_by_key()
    gk, gc, gs, gmn, gmx = st.collect()
    assert gk.tolist() == [key]
    assert gc.tolist() == [12293]
    assert gs.tolist() == [wrap64(sums[0])]
    assert gmn.tolist() == [sl.I64_MIN] and gmx.tolist() == [sl.I64_MAX]
    rdd.free(); st.free()


# ---- 3. reference parity ----

@pytest.mark.parametrize("n,key_bits", [(200_000, 16), (100_000, 63)])
def test_stats_reference_parity(ctx, n, key_bits):
    seed = 0xC0FFEE + key_bits
    hk, hv = datagen.uniform_pairs(seed, n, key_bits=key_bits)
    if key_bits == 63:
        assert len(np.unique(hk)) == n      # all distinct: the fast path
    rdd = ctx.make_rdd(hk, hv, nparts=16)
    st = rdd.stats_by_key(nparts=16)
    gk, gc, gs, gmn, gmx = by_key(st.collect())
    ok, ov = oc.reduce_by_key_i64(hk, hv, 16, 16)
    assert sl.sorted_pairs(gk, gs) == sl.sorted_pairs(ok, ov)
    ok, ov = oc.group_count_i64(hk, hv, 16, 16)
    assert sl.sorted_pairs(gk, gc) == sl.sorted_pairs(ok, ov)
    rk, rmn = sl.reduce_ref(sl.OP_MIN_I64, hk, hv)
    assert (gk == rk).all() and (gmn == rmn).all()
    rk, rmx = sl.reduce_ref(sl.OP_MAX_I64, hk, hv)
    assert (gk == rk).all() and (gmx == rmx).all()
    rdd.free(); st.free()


# ---- 4. small and empty ----

def test_stats_empty(ctx):
    e = np.empty(0, dtype=np.int64)
    rdd = ctx.make_rdd(e, e)
    st = rdd.stats_by_key()
    assert st.count() == 0
    got = st.collect()
    assert len(got) == 5
    for col in got:
        assert col.dtype == np.int64 and len(col) == 0
    rdd.free(); st.free()


def test_stats_one_row(ctx):
    rdd = ctx.make_rdd(np.array([-5], dtype=np.int64), np.array([sl.I64_MIN], dtype=np.int64))
    st = rdd.stats_by_key()
    assert [c.tolist() for c in st.collect()] == [[-5], [1], [sl.I64_MIN], [sl.I64_MIN],
                                                  [sl.I64_MIN]]
    rdd.free(); st.free()


def test_stats_nine_rows_two_keys(ctx):
    """a full chunk plus a guarded tail chunk; the second run crosses them"""
    k = np.array([3, 8, 3, 8, 8, 3, 8, 3, 8], dtype=np.int64)
    v = np.array([5, -1, sl.I64_MAX, 7, 0, 1, sl.I64_MIN, -4, 2], dtype=np.int64)
    assert (k == 3).sum() == 4 and (k == 8).sum() == 5
    rdd = ctx.make_rdd(k, v)
    st = rdd.stats_by_key()
    assert_stats_equal(st.collect(), stats_ref(k, v))
    rdd.free(); st.free()


# ---- 5. device-pointer entry ----

def test_dev_sort_stats(ctx):
    import torch
    from vega_amd import gpu
    name, what = "hash_minus1", "sum"
    lay = layout(name)
    n = lay.n
    k = torch.from_numpy(lay.k.copy()).cuda()
    v = torch.from_numpy(values(name, what).copy()).cuda()
    k0, v0 = k.clone(), v.clone()
    outs = [torch.empty_like(k) for _ in range(5)]
    ws = gpu.alloc_ws(n)
    gpu.prof_enable(True)
    try:
        nout = gpu.dev_sort_stats(k, v, *outs, ws)
        torch.cuda.synchronize()
        kstats = gpu.prof_stats()
    finally:
        gpu.prof_enable(False)
    assert_kernels(kstats, "hash")
    assert torch.equal(k, k0), "dev_sort_stats modified in_k"
    assert torch.equal(v, v0), "dev_sort_stats modified in_v"
    assert nout == len(lay.run_lens)
    assert_stats_equal(tuple(o[:nout].cpu().numpy() for o in outs), layout_ref(name, what))
    # a workspace one byte short is refused before anything runs
    with pytest.raises(gpu.VegaGpuError) as ei:
        gpu.dev_sort_stats(k, v, *outs, ws[:gpu.ws_bytes(n) - 1])
    assert ei.value.rc == ERR_CAP
    # a misaligned output column is refused (the fast path stores 16-B pairs)
    odd = torch.empty(n + 1, dtype=torch.int64, device="cuda")[1:]
    assert odd.data_ptr() % 16 == 8
    with pytest.raises(gpu.VegaGpuError) as ei:
        gpu.dev_sort_stats(k, v, outs[0], outs[1], odd, outs[3], outs[4], ws)
    assert ei.value.rc == ERR_INVALID
    assert torch.equal(k, k0) and torch.equal(v, v0)


# ---- 6. composition ----

def test_stats_column_composes(ctx):
    from vega_amd import gpu
    hk, hv = datagen.uniform_pairs(77, 50_000, key_bits=10)
    rdd = ctx.make_rdd(hk, hv, nparts=16)
    st = rdd.stats_by_key(nparts=16)
    ref = stats_ref(hk, hv)
    nk = len(ref[0])
    assert st.count() == nk
    col = st.column(gpu.STAT_SUM)
    ok, ov = oc.reduce_by_key_i64(hk, hv, 16, 16)
    assert sl.sorted_pairs(*col.collect()) == sl.sorted_pairs(ok, ov)
    assert col.count() == nk
    # same row order as the stats rdd
    sk, _, ss, _, _ = st.collect()
    ck, cv = col.collect()
    assert (ck == sk).all() and (cv == ss).all()
    # an existing op and an existing action on the plain handle
    srt = col.sort_by_key()
    gk, gv = srt.collect()
    assert (gk == ref[0]).all() and (gv == ref[2]).all()
    mx = st.column(gpu.STAT_MAX)
    top = max(zip(ref[0].tolist(), ref[4].tolist()))
    assert mx.max() == top
    for which, r in ((gpu.STAT_COUNT, ref[1]), (gpu.STAT_MIN, ref[3])):
        c = st.column(which)
        assert sl.sorted_pairs(*c.collect()) == sl.sorted_pairs(ref[0], r)
        c.free()
    rdd.free(); st.free(); col.free(); srt.free(); mx.free()


# ---- 7. guards ----

def refused(rc, fn):
    from vega_amd import gpu
    with pytest.raises(gpu.VegaGpuError) as ei:
        fn()
    assert ei.value.rc == rc, ei.value
    return ei.value


def test_stats_guards(ctx):
    from vega_amd import gpu
    k = np.arange(100, dtype=np.int64) % 7
    v = np.arange(100, dtype=np.int64)
    plain = ctx.make_rdd(k, v)
    f64 = ctx.make_rdd(k, v.astype(np.float64))
    err = refused(ERR_UNSUPPORTED, f64.stats_by_key)
    assert "f64" in str(err)
    still_answers(ctx)

    h = ctypes.c_uint64()
    assert gpu.lib().vega_gpu_group_by_key(ctx._c, ctypes.c_uint64(plain.h),
                                           ctypes.c_uint32(4), ctypes.byref(h)) == 0
    grouped = gpu.Rdd(ctx, h.value, np.int64)
    refused(ERR_INVALID, grouped.stats_by_key)
    still_answers(ctx)

    joined = plain.join(plain)
    refused(ERR_INVALID, joined.stats_by_key)
    still_answers(ctx)

    st = plain.stats_by_key()
    as_plain = gpu.Rdd(ctx, st.h, np.int64)
    for fn in (lambda: as_plain.reduce(gpu.OP_SUM_I64), lambda: as_plain.take_ordered(3),
               as_plain.stats_by_key):
        refused(ERR_INVALID, fn)
        still_answers(ctx)

    as_stats = gpu.StatsRdd(ctx, plain.h)
    for fn in (as_stats.collect, lambda: as_stats.column(gpu.STAT_SUM),
               lambda: st.column(4)):
        refused(ERR_INVALID, fn)
        still_answers(ctx)

    # the stats handle itself is still intact
    assert_stats_equal(st.collect(), stats_ref(k, v))
    for r in (plain, f64, grouped, joined, st):
        r.free()
