"""numpy reference for the f64 combiner (stats_by_key_f64) and the f64 order
ops (OP_MIN_F64 / OP_MAX_F64).

Order of doubles: for the bit pattern b of a double,
    ord(b) = b ^ (((int64)b >> 63) & 0x7FFFFFFFFFFFFFFF)   read as a signed i64
is strictly monotone on non-NaN doubles (-inf < ... < -0.0 < +0.0 < ... <
+inf) and an involution. min / max are min / max under ord with NaN values
(either sign, any payload) skipped; a key whose values are all NaN gets a NaN.

Pure numpy: used by test_stats_f64_ref.py (CPU) and test_gpu_stats_f64.py.
"""
import math

import numpy as np

I64_MIN = np.iinfo(np.int64).min
I64_MAX = np.iinfo(np.int64).max
_MASK = np.int64(0x7FFFFFFFFFFFFFFF)


def bits_of(v):
    """the int64 view of doubles (or of uint64 / int64 bit patterns)"""
    a = np.ascontiguousarray(v)
    if a.dtype == np.float64:
        return a.view(np.int64)
    if a.dtype == np.uint64:
        return a.view(np.int64)
    assert a.dtype == np.int64, a.dtype
    return a


def order_key(v):
    """ord of every double (or 64-bit pattern) in v, as int64"""
    b = bits_of(v)
    return b ^ ((b >> np.int64(63)) & _MASK)


def un_key(o):
    """the doubles whose order keys are o (ord is an involution)"""
    return order_key(np.ascontiguousarray(o, dtype=np.int64)).view(np.float64)


def is_nan_bits(v):
    b = bits_of(v)
    return (b & _MASK) > np.int64(0x7FF0000000000000)


def _runs(k):
    k = np.asarray(k, dtype=np.int64)
    order = np.argsort(k, kind="stable")
    ks = k[order]
    starts = np.flatnonzero(np.concatenate([[True], ks[1:] != ks[:-1]])) \
        if len(ks) else np.empty(0, dtype=np.int64)
    return order, ks, starts


def minmax_f64_ref(k, v):
    """(keys ascending, min, max): through order_key with NaN mapped to the
    op's identity, reduceat, then un-mapped — an identity that survives (an
    all-NaN key) un-maps to a NaN"""
    order, ks, starts = _runs(k)
    if len(ks) == 0:
        e = np.empty(0, dtype=np.float64)
        return ks, e, e.copy()
    vs = np.asarray(v, dtype=np.float64)[order]
    o = order_key(vs)
    nan = is_nan_bits(vs)
    mn = np.minimum.reduceat(np.where(nan, I64_MAX, o), starts)
    mx = np.maximum.reduceat(np.where(nan, I64_MIN, o), starts)
    return ks[starts], un_key(mn), un_key(mx)


def stats_f64_ref(k, v):
    """(keys ascending, count, math.fsum per key, min, max, sum|v| per key,
    rows per key). fsum of a key holding NaN or both infinities is NaN (what
    IEEE addition gives in any order); sum|v| is then inf or NaN."""
    order, ks, starts = _runs(k)
    vs = np.asarray(v, dtype=np.float64)[order]
    lens = np.diff(np.concatenate([starts, [len(ks)]])).astype(np.int64)
    parts = np.split(vs, starts[1:]) if len(ks) else []

    def fsum(p):
        p = p.tolist()
        if any(math.isnan(x) for x in p) or (math.inf in p and -math.inf in p):
            return math.nan
        if math.inf in p or -math.inf in p:
            return math.inf if math.inf in p else -math.inf
        return math.fsum(p)

    fs = np.array([fsum(p) for p in parts], dtype=np.float64)
    sabs = np.array([fsum(np.abs(p)) for p in parts], dtype=np.float64)
    rk, mn, mx = minmax_f64_ref(k, v)
    return ks[starts], lens.copy(), fs, mn, mx, sabs, lens


def same_bits(a, b):
    """element-wise bit equality of two double arrays"""
    return bits_of(np.asarray(a, dtype=np.float64)) == bits_of(np.asarray(b, dtype=np.float64))


def extremes_match(got, ref):
    """bit-equal where the reference is a number, NaN where it is NaN"""
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    rn = np.isnan(ref)
    return np.where(rn, np.isnan(got), same_bits(got, ref))
