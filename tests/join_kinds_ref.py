"""Expected results of vega_gpu_join_kind, restated in numpy.

Kinds 0-3: the matched rows are the oracle's inner join (oracle_ctypes.join_i64,
the reference's own cogroup cross product, pair_rdd.rs:104-155); the rows of a
side without a partner come from np.isin and carry 0 in the absent slot. The
result is a multiset, returned in sorted_rows order. Semi and anti are masks
over A that keep A's row order."""
import numpy as np

import oracle_ctypes as oc

INNER, LEFT_OUTER, RIGHT_OUTER, FULL_OUTER, LEFT_SEMI, LEFT_ANTI = range(6)
HAS_A, HAS_B = 1, 2
KINDS = (INNER, LEFT_OUTER, RIGHT_OUTER, FULL_OUTER, LEFT_SEMI, LEFT_ANTI)
OUTER_KINDS = (INNER, LEFT_OUTER, RIGHT_OUTER, FULL_OUTER)


def _i64(a):
    return np.ascontiguousarray(a, dtype=np.int64)


def sorted_rows(k, va, vb, present):
    """the four columns ordered by (k, va, vb, present): the multiset's
    canonical form"""
    k, va, vb = _i64(k), _i64(va), _i64(vb)
    present = np.ascontiguousarray(present, dtype=np.uint8)
    idx = np.lexsort((present, vb, va, k))
    return k[idx], va[idx], vb[idx], present[idx]


def inner_rows(ak, av, bk, bv):
    """the oracle's inner join (computed once per input and shared)"""
    ak, av, bk, bv = _i64(ak), _i64(av), _i64(bk), _i64(bv)
    if len(ak) == 0 or len(bk) == 0:
        z = np.empty(0, dtype=np.int64)
        return z, z.copy(), z.copy()
    return oc.join_i64(ak, av, bk, bv, 4, 4)


def outer(ak, av, bk, bv, kind, inner=None):
    """(k, va, vb, present) of kinds 0-3 in sorted_rows order"""
    assert kind in OUTER_KINDS
    ak, av, bk, bv = _i64(ak), _i64(av), _i64(bk), _i64(bv)
    ik, iva, ivb = inner if inner is not None else inner_rows(ak, av, bk, bv)
    ks, vas, vbs = [ik], [iva], [ivb]
    ps = [np.full(len(ik), HAS_A | HAS_B, dtype=np.uint8)]
    if kind in (LEFT_OUTER, FULL_OUTER):
        m = ~np.isin(ak, bk)
        ks.append(ak[m]); vas.append(av[m]); vbs.append(np.zeros(int(m.sum()), dtype=np.int64))
        ps.append(np.full(int(m.sum()), HAS_A, dtype=np.uint8))
    if kind in (RIGHT_OUTER, FULL_OUTER):
        m = ~np.isin(bk, ak)
        ks.append(bk[m]); vas.append(np.zeros(int(m.sum()), dtype=np.int64)); vbs.append(bv[m])
        ps.append(np.full(int(m.sum()), HAS_B, dtype=np.uint8))
    return sorted_rows(np.concatenate(ks), np.concatenate(vas), np.concatenate(vbs),
                       np.concatenate(ps))


def member(ak, av, bk, kind):
    """(k, v) of LEFT_SEMI / LEFT_ANTI: rows of A in A's row order"""
    assert kind in (LEFT_SEMI, LEFT_ANTI)
    ak = _i64(ak)
    av = np.ascontiguousarray(av)
    m = np.isin(ak, _i64(bk))
    if kind == LEFT_ANTI:
        m = ~m
    return ak[m], av[m]
