"""CPU checks of the f64 combiner's reference (tests/stats_f64_ref.py) on
hand-written vectors, and of the exported order key vega_f64_order_key (pure
host code in libvega_gpu.so: needs no GPU and no context)."""
import ctypes
import math
import os
import struct

import numpy as np
import pytest

import stats_f64_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "vega_amd", "csrc", "libvega_gpu.so")

INF = math.inf
NAN = math.nan
DEN = 5e-324   # the smallest denormal
NEG_NAN_PAYLOAD = struct.unpack("<d", struct.pack("<Q", 0xFFF0000000000123))[0]

# ascending under the order the issue fixes; written out by hand
ASCENDING = [-INF, -1.7976931348623157e308, -1.0, -2.2250738585072014e-308, -DEN, -0.0,
             0.0, DEN, 2.2250738585072014e-308, 1.0, 1.7976931348623157e308, INF]


def bits(x):
    return struct.unpack("<q", struct.pack("<d", x))[0]


def test_order_key_formula_on_hand_values():
    v = np.array(ASCENDING, dtype=np.float64)
    o = sr.order_key(v)
    assert o.dtype == np.int64
    for x, got in zip(ASCENDING, o.tolist()):
        b = bits(x)
        exp = b ^ ((b >> 63) & 0x7FFFFFFFFFFFFFFF)   # Python ints: >> is arithmetic
        assert got == exp, x
    assert (np.diff(o) > 0).all(), "strictly ascending, -0.0 below +0.0"
    # non-negative doubles keep their bits; -0.0 maps to -1, just below +0.0's 0
    assert bits(ASCENDING[5]) == -(1 << 63) and bits(ASCENDING[6]) == 0   # -0.0, +0.0
    assert o[4:8].tolist() == [-2, -1, 0, 1]   # -DEN, -0.0, +0.0, DEN


def test_order_key_involution():
    rng = np.random.RandomState(5)
    pats = rng.randint(sr.I64_MIN, sr.I64_MAX, size=10_000, dtype=np.int64)
    pats = np.concatenate([pats, [0, -1, sr.I64_MIN, sr.I64_MAX, bits(NAN), bits(-0.0)]])
    assert (sr.order_key(sr.order_key(pats)) == pats).all()
    v = np.array(ASCENDING + [NAN, NEG_NAN_PAYLOAD], dtype=np.float64)
    assert sr.same_bits(sr.un_key(sr.order_key(v)), v).all()


def test_identities_unmap_to_nan():
    assert np.isnan(sr.un_key(np.array([sr.I64_MAX, sr.I64_MIN]))).all()
    # and no non-NaN double has an identity as its key
    o = sr.order_key(np.array(ASCENDING, dtype=np.float64))
    assert sr.I64_MIN < o.min() and o.max() < sr.I64_MAX


def test_order_equals_value_then_sign():
    """on non-NaN values, sorting by order_key equals sorting by (value, not signbit)"""
    rng = np.random.RandomState(6)
    v = np.concatenate([
        rng.standard_normal(4000) * 10.0 ** rng.randint(-300, 300, size=4000),
        np.array(ASCENDING * 5, dtype=np.float64), np.zeros(50), -np.zeros(50)])
    v = v[rng.permutation(len(v))]
    assert not np.isnan(v).any()
    by_key = np.argsort(sr.order_key(v), kind="stable")
    by_val = np.lexsort((~np.signbit(v), v))   # primary v, then -0.0 before +0.0
    assert sr.same_bits(v[by_key], v[by_val]).all()


def test_is_nan_bits():
    v = np.array([NAN, -NAN, NEG_NAN_PAYLOAD, INF, -INF, 0.0, -0.0, DEN, 1.0], dtype=np.float64)
    assert sr.is_nan_bits(v).tolist() == [True, True, True] + [False] * 6


def test_reference_on_hand_written_rows():
    #        key 1: zeros      key 2: NaN skipped      key 3: all NaN   key 4: infinities
    k = [1, 1,                 2, 2, 2, 2,             3, 3,            4, 4, 4,
         5, 5, 5,              6,                      7, 7]
    v = [0.0, -0.0,            1.5, NAN, -2.5, NEG_NAN_PAYLOAD, NAN, NEG_NAN_PAYLOAD, INF, 3.0, -INF,
         DEN, -DEN, 0.0,       -7.25,                  -0.0, 0.0]
    perm = np.random.RandomState(7).permutation(len(k))
    k = np.array(k, dtype=np.int64)[perm]
    v = np.array(v, dtype=np.float64)[perm]
    rk, cnt, fs, mn, mx, sabs, lens = sr.stats_f64_ref(k, v)
    assert rk.tolist() == [1, 2, 3, 4, 5, 6, 7]
    assert cnt.tolist() == [2, 4, 2, 3, 3, 1, 2] and (lens == cnt).all()
    # -0.0 < +0.0, in both input orders (keys 1 and 7)
    for i in (0, 6):
        assert bits(mn[i]) == bits(-0.0) and bits(mx[i]) == bits(0.0)
    # NaN skipped by min and max, counted by count, propagated by sum
    assert (mn[1], mx[1]) == (-2.5, 1.5) and math.isnan(fs[1])
    # an all-NaN key gives NaN
    assert math.isnan(mn[2]) and math.isnan(mx[2]) and math.isnan(fs[2])
    # +-inf: extremes are the infinities, inf + -inf is NaN
    assert (mn[3], mx[3]) == (-INF, INF) and math.isnan(fs[3])
    # the denormal and its negative around zero
    assert (mn[4], mx[4]) == (-DEN, DEN) and fs[4] == 0.0
    assert (mn[5], mx[5], fs[5], sabs[5]) == (-7.25, -7.25, -7.25, 7.25)
    rk2, mn2, mx2 = sr.minmax_f64_ref(k, v)
    assert (rk2 == rk).all() and sr.extremes_match(mn2, mn).all() and sr.extremes_match(mx2, mx).all()


def test_reference_empty():
    e = np.empty(0, dtype=np.int64)
    out = sr.stats_f64_ref(e, np.empty(0, dtype=np.float64))
    assert len(out) == 7 and all(len(c) == 0 for c in out)


def test_extremes_match_helper():
    ref = np.array([1.0, NAN, -0.0])
    assert sr.extremes_match(np.array([1.0, NEG_NAN_PAYLOAD, -0.0]), ref).all()
    assert sr.extremes_match(np.array([1.0, 2.0, 0.0]), ref).tolist() == [True, False, False]


# ---- the exported key ----

@pytest.fixture(scope="module")
def order_key_fn():
    so = ctypes.CDLL(SO)
    fn = so.vega_f64_order_key
    fn.restype = ctypes.c_uint64
    fn.argtypes = [ctypes.c_uint64]
    return fn


def test_exported_order_key(order_key_fn):
    hand = np.array(ASCENDING + [NAN, -NAN, NEG_NAN_PAYLOAD], dtype=np.float64).view(np.uint64)
    rng = np.random.RandomState(8)
    rand = rng.randint(sr.I64_MIN, sr.I64_MAX, size=10_000, dtype=np.int64).view(np.uint64)
    pats = np.concatenate([hand, rand, np.array([0, 2 ** 64 - 1, 2 ** 63, 2 ** 63 - 1],
                                                dtype=np.uint64)])
    got = np.array([order_key_fn(int(p)) for p in pats], dtype=np.uint64).view(np.int64)
    assert (got == sr.order_key(pats)).all()


def test_python_order_key_wrapper():
    from vega_amd import gpu
    v = np.array(ASCENDING + [NAN], dtype=np.float64)
    got = gpu.f64_order_key(v)
    assert got.dtype == np.int64 and (got == sr.order_key(v)).all()
    assert (gpu.f64_order_key(v.view(np.uint64)) == got).all()
    assert (gpu.f64_order_key(v.view(np.int64)) == got).all()   # sign bit set included
    with pytest.raises(TypeError):
        gpu.f64_order_key(np.arange(3, dtype=np.int32))
