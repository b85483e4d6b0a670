"""Segmented reduce at run / chunk / wave / tile edges, for every op on both
row layouts.

seg_reduce = k_head_count<PK> + k_seg_emit<OP,PK> (+ k_f64_seg_combine): five
ops x two layouts. PK (interleaved 16-byte rows) is what the hash grouping
strategy of group_sort_u64 hands over, SoA what the narrow-key strategy does;
each test asserts through the kernel statistics which of the two ran.

The inputs come from tests/seg_layout.py, whose CPU test proves that they put
runs on every edge the kernel distinguishes (fast chunk at an even / odd output
slot, a distinct chunk whose last run goes on, runs that are exactly a chunk,
a wave or a tile, runs over a tile edge, a tile without any head, a guarded
tail chunk, key -1 as the very last run). Integer ops are compared bit for bit
with the numpy reducers there, SUM_F64 against math.fsum.
"""
import functools

import numpy as np
import pytest

import seg_layout as sl

pytestmark = pytest.mark.gpu

OP_NAMES = ["SUM_I64", "COUNT", "SUM_F64", "MIN_I64", "MAX_I64"]


@pytest.fixture(scope="module")
def ctx():
    from vega_amd import gpu
    with gpu.VegaContext() as c:
        yield c


# ---- inputs and references: built once, shared, never modified ----

@functools.lru_cache(maxsize=None)
def layout(kind, variant):
    lay = sl.soa_layout(variant) if kind == "soa" else sl.hash_layout(variant)
    lay.k.setflags(write=False)
    return lay


@functools.lru_cache(maxsize=None)
def values(kind, variant, what):
    lay = layout(kind, variant)
    gen = {"minmax": (sl.values_minmax, 11), "sum": (sl.values_sum_i64, 12),
           "f64int": (sl.values_f64_integral, 13), "f64mix": (sl.values_f64_mixed, 14)}[what]
    v = gen[0](lay, np.random.RandomState(gen[1]))
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def int_ref(kind, variant, op):
    lay = layout(kind, variant)
    what = {sl.OP_SUM_I64: "sum", sl.OP_COUNT: "sum"}.get(op, "minmax")
    rk, rv = sl.reduce_ref(op, lay.k, values(kind, variant, what))
    return what, sl.sorted_pairs(rk, rv)


@functools.lru_cache(maxsize=None)
def f64_ref(kind, variant, what):
    return sl.sum_f64_ref(layout(kind, variant).k, values(kind, variant, what))


# ---- which grouping strategy ran ----

def assert_strategy(stats, strategy):
    """hash strategy: hashed histogram + cleanup, rows stay packed (an exact
    key histogram would mean the fall-back key sort, which unpacks them);
    narrow strategy: exact key histogram, no hashing, SoA rows"""
    names = set(stats)
    if strategy == "hash":
        assert {"ghist", "group_cleanup"} <= names and "hist8" not in names, names
    else:
        assert "hist8" in names and not ({"ghist", "group_cleanup"} & names), names
    assert stats["seg_emit"]["n"] == 1 and stats["head_count"]["n"] == 1


def profiled(ctx, fn):
    ctx.set_profiling(True)
    try:
        out = fn()
        stats = ctx.kernel_stats()
    finally:
        ctx.set_profiling(False)
    return out, stats


def by_key(gk, gv):
    o = np.argsort(gk, kind="stable")
    return gk[o], gv[o]


def check_f64_exact(gk, gv, ref):
    rk, fs, sabs, _ = ref
    assert sabs.max() < 2.0 ** 53        # premise: exact in any order
    gk, gv = by_key(gk, gv)
    assert len(gk) == len(rk) and (gk == rk).all()
    bad = np.flatnonzero(gv.view(np.int64) != fs.view(np.int64))
    assert len(bad) == 0, (gk[bad][:5], gv[bad][:5], fs[bad][:5])


def check_f64_bound(gk, gv, ref):
    """any-order summation bound, with a factor 2 of slack:
    |got - fsum| <= len * 2^-52 * sum|v| per key"""
    rk, fs, sabs, lens = ref
    gk, gv = by_key(gk, gv)
    assert len(gk) == len(rk) and (gk == rk).all()
    err = np.abs(gv - fs)
    bound = lens * 2.0 ** -52 * sabs
    bad = np.flatnonzero(~(err <= bound))
    assert len(bad) == 0, (gk[bad][:5], gv[bad][:5], fs[bad][:5], bound[bad][:5])


def run_op(ctx, kind, variant, op, strategy):
    from vega_amd import gpu
    assert (gpu.OP_SUM_I64, gpu.OP_COUNT, gpu.OP_SUM_F64, gpu.OP_MIN_I64, gpu.OP_MAX_I64) \
        == (sl.OP_SUM_I64, sl.OP_COUNT, sl.OP_SUM_F64, sl.OP_MIN_I64, sl.OP_MAX_I64)
    lay = layout(kind, variant)
    nruns = len(lay.run_lens)
    if op != sl.OP_SUM_F64:
        what, exp = int_ref(kind, variant, op)
        rdd = ctx.make_rdd(lay.k, values(kind, variant, what))
        red, stats = profiled(ctx, lambda: rdd.reduce_by_key(op))
        assert_strategy(stats, strategy)
        gk, gv = red.collect()
        assert len(gk) == nruns
        assert sl.sorted_pairs(gk, gv) == exp
        red.free()
        if op == sl.OP_COUNT:       # the group_count entry: same path
            red, stats = profiled(ctx, rdd.group_count)
            assert_strategy(stats, strategy)
            assert sl.sorted_pairs(*red.collect()) == exp
            red.free()
        rdd.free()
        return
    # SUM_F64, 1: integer-valued doubles -> exact in any order -> bit equality
    rdd = ctx.make_rdd(lay.k, values(kind, variant, "f64int"))
    red, stats = profiled(ctx, lambda: rdd.reduce_by_key(op))
    assert_strategy(stats, strategy)
    gk, gv = red.collect()
    assert len(gk) == nruns
    check_f64_exact(gk, gv, f64_ref(kind, variant, "f64int"))
    rdd.free(); red.free()
    # SUM_F64, 2: mixed sign and magnitude -> derived bound, and run-to-run
    # bit identity (the f64 path promises a fixed summation shape)
    rdd = ctx.make_rdd(lay.k, values(kind, variant, "f64mix"))
    red1, stats = profiled(ctx, lambda: rdd.reduce_by_key(op))
    assert_strategy(stats, strategy)
    red2 = rdd.reduce_by_key(op)
    k1, v1 = red1.collect()
    k2, v2 = red2.collect()
    assert len(k1) == nruns
    check_f64_bound(k1, v1, f64_ref(kind, variant, "f64mix"))
    assert (k1 == k2).all() and (v1.view(np.int64) == v2.view(np.int64)).all()
    rdd.free(); red1.free(); red2.free()


@pytest.mark.parametrize("tail", [0, 3])
@pytest.mark.parametrize("op", OP_NAMES)
def test_seg_ops_exact_layout_soa(ctx, op, tail):
    """k_seg_emit<op,false>: narrow keys (key = run index), runs placed by
    hand on every chunk / wave / tile edge; n % 8 == 0 and n % 8 == 3"""
    run_op(ctx, "soa", tail, sl.OPS[op], "narrow")


@pytest.mark.parametrize("with_minus1", [True, False])
@pytest.mark.parametrize("op", OP_NAMES)
def test_seg_ops_hash_layout_packed(ctx, op, with_minus1):
    """k_seg_emit<op,true>: 155,365 rows of wide keys in h32 order, n % 8 == 5;
    with_minus1 ends the grouped rows with a run of key -1 (the pad value)"""
    run_op(ctx, "hash", with_minus1, sl.OPS[op], "hash")


@pytest.mark.parametrize("op", ["SUM_I64", "SUM_F64"])
def test_dev_sort_reduce_packed_keeps_inputs(ctx, op):
    """the device-pointer entry on the packed case; in_k / in_v must come
    back unchanged (vega_gpu.h: "not modified")"""
    import torch
    from vega_amd import gpu
    lay = layout("hash", True)
    n = lay.n
    f64 = op == "SUM_F64"
    hv = values("hash", True, "f64mix" if f64 else "sum")
    k = torch.from_numpy(lay.k.copy()).cuda()
    v = torch.from_numpy(hv.copy()).cuda()
    k0, v0 = k.clone(), v.clone()
    out_k = torch.empty_like(k)
    out_v = torch.empty_like(v)
    ws = gpu.alloc_ws(n)
    gpu.prof_enable(True)
    try:
        nout = gpu.dev_sort_reduce(k, v, sl.OPS[op], out_k, out_v, ws)
        torch.cuda.synchronize()
        stats = gpu.prof_stats()
    finally:
        gpu.prof_enable(False)
    assert_strategy(stats, "hash")
    assert torch.equal(k, k0), "dev_sort_reduce modified in_k"
    assert torch.equal(v.view(torch.int64), v0.view(torch.int64)), "dev_sort_reduce modified in_v"
    assert nout == len(lay.run_lens)
    gk = out_k[:nout].cpu().numpy()
    gv = out_v[:nout].cpu().numpy()
    if f64:
        check_f64_bound(gk, gv, f64_ref("hash", True, "f64mix"))
    else:
        assert sl.sorted_pairs(gk, gv) == int_ref("hash", True, sl.OP_SUM_I64)[1]


@pytest.mark.parametrize("kind,variant,strategy", [("soa", 3, "narrow"),
                                                   ("hash", True, "hash")])
def test_count_by_value_and_distinct_reuse_layouts(ctx, kind, variant, strategy):
    """count_by_value groups the VALUE column (pointer roles swapped),
    distinct zeroes the counts: same sort + segmented count underneath"""
    lay = layout(kind, variant)
    exp = int_ref(kind, variant, sl.OP_COUNT)[1]
    other = np.arange(lay.n, dtype=np.int64)
    rdd = ctx.make_rdd(other, lay.k)
    cbv, stats = profiled(ctx, rdd.count_by_value)
    assert_strategy(stats, strategy)
    assert sl.sorted_pairs(*cbv.collect()) == exp
    rdd.free(); cbv.free()
    rdd = ctx.make_rdd(lay.k, other)
    dis, stats = profiled(ctx, rdd.distinct)
    assert_strategy(stats, strategy)
    gk, gv = dis.collect()
    assert sorted(gk.tolist()) == [key for key, _ in exp]
    assert (gv == 0).all()
    rdd.free(); dis.free()
