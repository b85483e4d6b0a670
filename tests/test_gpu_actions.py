"""Device-side actions through the RDD-handle API — reduce, fold, min, max,
take, first, is_empty, take_ordered, top (rdd.rs:274-322, :534-620,
:1073-1153) — against the pure-Python restatement in actions_ref."""
import json
import math
import os
import sys

import numpy as np
import pytest

import actions_ref as ar
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vega_amd import datagen

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
SIZES = [0, 1, 63, 64, 65, 4095, 4096, 4097, 300_001]
OPS = [ar.OP_SUM_I64, ar.OP_MIN_I64, ar.OP_MAX_I64]


@pytest.fixture(scope="module")
def ctx():
    from vega_amd import gpu
    with gpu.VegaContext() as c:
        yield c


def pairs(k, v):
    return list(zip(np.asarray(k).tolist(), np.asarray(v).tolist()))


def mixed_rows(seed, n, key_bits=63):
    """mixed-sign keys; values of magnitude near 2^62 so column sums wrap"""
    k, v = datagen.uniform_pairs(seed, n, key_bits=64 if key_bits == 63 else key_bits)
    if key_bits != 63:
        k = k - (1 << (key_bits - 1))  # narrow but still mixed-sign
    # |v| in [2^62, 2^63): two of one sign already wrap
    v = ((v.view(np.uint64) >> np.uint64(2)) | np.uint64(1 << 62)).view(np.int64)
    v[::3] = -v[::3]
    return k, v


# ---------------- golden vectors ----------------

def test_actions_golden(ctx):
    from vega_amd import gpu
    with open(os.path.join(HERE, "golden", "actions.json")) as f:
        entries = json.load(f)["entries"]
    assert len(entries) == 12
    for g in entries:
        if "range" in g:
            k = np.arange(g["range"][0], g["range"][1], dtype=np.int64)
        else:
            k = np.asarray(g["elements"], dtype=np.int64)
        rdd = ctx.make_rdd(k, np.zeros(len(k), np.int64), nparts=g["nparts"])
        op = g["op"]
        if op == "fold":
            assert rdd.fold(gpu.OP_SUM_I64, g["init"], 0) == (g["expected"], 0)
        elif op == "max":
            assert rdd.max() == (g["expected"], 0)
        elif op == "min":
            assert rdd.min() == (g["expected"], 0)
        elif op == "top":
            tk, tv = rdd.top(g["num"])
            assert tk.tolist() == g["expected"] and tv.tolist() == [0] * g["num"]
        elif op == "take_ordered":
            tk, tv = rdd.take_ordered(g["num"])
            assert tk.tolist() == g["expected"] and tv.tolist() == [0] * g["num"]
        elif op == "take":
            tk, tv = rdd.take(g["num"])
            assert len(tk) == len(tv) == g["expected_len"]
            assert tk.tolist() == k[:g["expected_len"]].tolist()
        elif op == "first":
            if g["expected_ok"]:
                assert rdd.first() == (int(k[0]), 0)
            else:
                with pytest.raises(gpu.VegaGpuError, match="rc=-4.*empty collection"):
                    rdd.first()
        elif op == "is_empty":
            assert rdd.is_empty() is g["expected"]
        else:
            raise AssertionError(op)
        rdd.free()


# ---------------- reduce / min / max ----------------

@pytest.mark.parametrize("n", SIZES)
def test_reduce_min_max_sizes(ctx, n):
    k, v = mixed_rows(1000 + n, n)
    if n >= 2:
        k[n // 3], v[n // 3] = I64_MIN, I64_MAX
        k[n // 2], v[n // 2] = I64_MAX, I64_MIN
    rdd = ctx.make_rdd(k, v, nparts=3)
    for op in OPS:
        assert rdd.reduce(op) == ar.reduce(k, v, op), op
    assert rdd.min() == ar.lex_min(k, v)
    assert rdd.max() == ar.lex_max(k, v)
    if n == 0:
        assert rdd.reduce(ar.OP_SUM_I64) is None and rdd.min() is None and rdd.max() is None
    gk, gv = rdd.collect()
    assert (gk == k).all() and (gv == v).all()  # input untouched
    rdd.free()


@pytest.mark.parametrize("n", [65, 4097, 300_001])
def test_lex_min_max_break_key_ties_on_value(ctx, n):
    # key_bits=2: a quarter of the rows tie on the extreme key
    k, v = mixed_rows(2000 + n, n, key_bits=2)
    rdd = ctx.make_rdd(k, v)
    assert rdd.min() == ar.lex_min(k, v)
    assert rdd.max() == ar.lex_max(k, v)
    rdd.free()
    # all keys equal: the value column alone decides
    k[:] = -7
    rdd = ctx.make_rdd(k, v)
    assert rdd.min() == (-7, int(v.min()))
    assert rdd.max() == (-7, int(v.max()))
    rdd.free()


@pytest.mark.parametrize("n", SIZES)
def test_reduce_sum_f64_sizes(ctx, n):
    """the fourth op over the same size sweep: f64 values (dyadic [0,1)),
    mixed-sign full-range keys whose i64 sum wraps"""
    from vega_amd import gpu
    k, v = datagen.uniform_pairs_f64(3000 + n, n, key_bits=64)
    if n >= 2:
        k[n // 3], k[n // 2] = I64_MIN, I64_MAX
    rdd = ctx.make_rdd(k, v, nparts=3)
    assert rdd.vdtype == np.float64
    got = rdd.reduce(gpu.OP_SUM_F64)
    exp = ar.reduce(k, v, ar.OP_SUM_F64)
    if n == 0:
        assert got is None and exp is None
    else:
        assert got[0] == exp[0]  # key column: exact wrapping i64 sum
        err = abs(got[1] - exp[1])
        print(f"f64 reduce n={n}: got {got[1]!r} fsum {exp[1]!r} abs err {err:.3e}")
        # 1e-6 relative of math.fsum; all values >= 0, so no cancellation
        assert err <= 1e-6 * exp[1]
        again = rdd.reduce(gpu.OP_SUM_F64)
        assert np.float64(got[1]).tobytes() == np.float64(again[1]).tobytes()
    gk, gv = rdd.collect()
    assert (gk == k).all() and (gv == v).all()  # input untouched
    rdd.free()


def test_reduce_f64(ctx):
    from vega_amd import gpu
    n = 300_001
    k, v = datagen.uniform_pairs_f64(31, n, key_bits=64)
    rdd = ctx.make_rdd(k, v)
    exp_k, exp_v = ar.reduce(k, v, ar.OP_SUM_F64)
    got = rdd.reduce(gpu.OP_SUM_F64)
    again = rdd.reduce(gpu.OP_SUM_F64)
    assert got[0] == exp_k  # key column: wrapping i64 even under SUM_F64
    rel = abs(got[1] - exp_v) / exp_v
    print(f"f64 reduce n={n}: got {got[1]!r} fsum {exp_v!r} rel {rel:.3e}")
    assert rel <= 1e-6
    # no atomics, fixed summation shape: bit-identical run to run
    assert np.float64(got[1]).tobytes() == np.float64(again[1]).tobytes()
    assert got[0] == again[0]
    # i64 ops on f64 values / COUNT are type errors, like reduce_by_key
    for op in (gpu.OP_SUM_I64, gpu.OP_MIN_I64, gpu.OP_MAX_I64, gpu.OP_COUNT):
        with pytest.raises(gpu.VegaGpuError, match="rc=-1 "):
            rdd.reduce(op)
    # f64 is not Ord: the ordered actions refuse
    for call in (rdd.min, rdd.max, lambda: rdd.top(3), lambda: rdd.take_ordered(3)):
        with pytest.raises(gpu.VegaGpuError, match="rc=-1 "):
            call()
    # take / first still serve f64 rows
    tk, tv = rdd.take(5)
    assert (tk == k[:5]).all() and (tv == v[:5]).all() and tv.dtype == np.float64
    assert rdd.first() == (int(k[0]), float(v[0]))
    rdd.free()
    i64 = ctx.make_rdd(k[:10], np.arange(10))
    with pytest.raises(gpu.VegaGpuError, match="rc=-1 "):
        i64.reduce(gpu.OP_SUM_F64)
    i64.free()


# ---------------- fold ----------------

@pytest.mark.parametrize("nparts", [1, 10])
def test_fold_init_counts_every_partition(ctx, nparts):
    k, v = mixed_rows(77, 4097)
    rdd = ctx.make_rdd(k, v, nparts=nparts)
    for op in OPS:
        exp = ar.fold(k, v, op, 5, 5, nparts)
        assert rdd.fold(op, 5, 5) == exp, op
    rk, rv = ar.reduce(k, v, ar.OP_SUM_I64)
    add = 5 * (nparts + 1)
    assert rdd.fold(ar.OP_SUM_I64, 5, 5) == (ar.wrap_i64(rk + add), ar.wrap_i64(rv + add))
    rdd.free()


def test_fold_empty_rdd(ctx):
    from vega_amd import gpu
    e = np.zeros(0, dtype=np.int64)
    rdd = ctx.make_rdd(e, e, nparts=4)
    assert rdd.fold(gpu.OP_SUM_I64, 5, -2) == (25, -10)  # (P+1) * init
    assert rdd.fold(gpu.OP_MIN_I64, 5, -2) == (5, -2)
    assert rdd.fold(gpu.OP_MAX_I64, 5, -2) == (5, -2)
    rdd.free()
    f = ctx.make_rdd(e, np.zeros(0, dtype=np.float64), nparts=4)
    assert f.fold(gpu.OP_SUM_F64, 1, 0.25) == (5, 1.25)
    f.free()


def test_fold_f64(ctx):
    from vega_amd import gpu
    k, v = datagen.uniform_pairs_f64(32, 4097, key_bits=20)
    rdd = ctx.make_rdd(k, v, nparts=10)
    fk, fv = rdd.fold(gpu.OP_SUM_F64, 3, 0.5)
    ek, ev = ar.fold(k, v, ar.OP_SUM_F64, 3, 0.5, 10)
    assert fk == ek and abs(fv - ev) <= 1e-6 * ev
    rdd.free()


# ---------------- take / first / is_empty ----------------

@pytest.mark.parametrize("n", [0, 1, 4097])
def test_take_first_is_empty(ctx, n):
    from vega_amd import gpu
    k, v = mixed_rows(500 + n, n)
    rdd = ctx.make_rdd(k, v, nparts=4)
    for num in (0, 1, n, n + 1):
        tk, tv = rdd.take(num)
        ek, ev = ar.take(k, v, num)
        assert (tk == ek).all() and (tv == ev).all() and len(tk) == min(num, n)
    assert rdd.is_empty() is (n == 0)
    if n:
        assert rdd.first() == ar.first(k, v)
    else:
        with pytest.raises(gpu.VegaGpuError, match="rc=-4.*empty collection"):
            rdd.first()
    rdd.free()


def test_take_after_filter_is_the_stable_prefix(ctx):
    from vega_amd import gpu
    k, v = datagen.uniform_pairs(62, 100_000, key_bits=12)
    rdd = ctx.make_rdd(k, v)
    f = rdd.filter(gpu.PRED_KEY_MOD_EQ, 5, 2)
    mask = (k % 5) == 2
    tk, tv = f.take(1000)
    assert (tk == k[mask][:1000]).all() and (tv == v[mask][:1000]).all()
    assert f.first() == (int(k[mask][0]), int(v[mask][0]))
    none = rdd.filter(gpu.PRED_KEY_IN_RANGE, -5, -1)  # keeps nothing
    assert none.is_empty() and len(none.take(3)[0]) == 0 and none.reduce() is None
    rdd.free(); f.free(); none.free()


# ---------------- take_ordered / top ----------------

def test_top_take_ordered_handle_level(ctx):
    n = 300_000
    k, v = datagen.uniform_pairs(90, n, key_bits=63)
    rdd = ctx.make_rdd(k, v)
    tk, tv = rdd.take_ordered(1000)
    assert pairs(tk, tv) == pairs(*ar.take_ordered(k, v, 1000))
    tk, tv = rdd.top(1000)
    assert pairs(tk, tv) == pairs(*ar.top(k, v, 1000))
    gk, gv = rdd.collect()
    assert (gk == k).all() and (gv == v).all()  # input untouched
    rdd.free()


def test_ordered_guards(ctx):
    from vega_amd import gpu
    k, v = mixed_rows(91, 1000, key_bits=4)
    rdd = ctx.make_rdd(k, v)
    for fn, ref in ((rdd.take_ordered, ar.take_ordered), (rdd.top, ar.top)):
        tk, tv = fn(0)
        assert len(tk) == 0 and len(tv) == 0
        for num in (1000, 1001, 1 << 40):  # num >= n: all rows, sorted
            tk, tv = fn(num)
            assert pairs(tk, tv) == pairs(*ref(k, v, num))
    grouped = ctypes_group_handle(ctx, rdd)
    few = rdd.filter(gpu.PRED_KEY_IN_RANGE, 0, 2)
    join = rdd.join(few)
    for h in (grouped, join):
        for call in (h.reduce, h.min, h.max, h.is_empty, h.first,
                     lambda: h.fold(gpu.OP_SUM_I64, 0, 0), lambda: h.take(1),
                     lambda: h.take_ordered(1), lambda: h.top(1)):
            with pytest.raises(gpu.VegaGpuError, match="rc=-1 "):
                call()
    rdd.free(); grouped.free(); few.free(); join.free()


def ctypes_group_handle(ctx, rdd):
    """a grouped handle (vega_gpu_group_by_key) kept alive as an Rdd"""
    import ctypes
    from vega_amd import gpu
    out = ctypes.c_uint64()
    rc = gpu.lib().vega_gpu_group_by_key(ctx._c, ctypes.c_uint64(rdd.h),
                                         ctypes.c_uint32(4), ctypes.byref(out))
    assert rc == 0
    return gpu.Rdd(ctx, out.value, np.int64)
