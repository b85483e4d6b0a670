"""join_kinds_ref against an independent restatement of "cogroup, then
flat-map per key" (Spark's definition over pair_rdd.rs:123-155) and against
hand-written expectations. CPU only."""
import numpy as np
import pytest

import join_kinds_ref as jr

LIT_A = [(1, 10), (1, 11), (2, 20), (3, 30)]
LIT_B = [(1, 0), (3, 300), (3, 301), (4, 400)]   # B value 0: only the presence byte tells
LIT_INNER = [(1, 10, 0, 3), (1, 11, 0, 3), (3, 30, 300, 3), (3, 30, 301, 3)]
LIT_EXPECT = {
    jr.INNER: LIT_INNER,
    jr.LEFT_OUTER: sorted(LIT_INNER + [(2, 20, 0, 1)]),
    jr.RIGHT_OUTER: sorted(LIT_INNER + [(4, 0, 400, 2)]),
    jr.FULL_OUTER: sorted(LIT_INNER + [(2, 20, 0, 1), (4, 0, 400, 2)]),
    jr.LEFT_SEMI: [(1, 10), (1, 11), (3, 30)],
    jr.LEFT_ANTI: [(2, 20)],
}


def cols(pairs):
    k = np.array([p[0] for p in pairs], dtype=np.int64)
    v = np.array([p[1] for p in pairs], dtype=np.int64)
    return k, v


def cogroup_flat_map(a, b, kind):
    """dict-of-lists cogroup, then Spark's per-key flat map; sorted tuples"""
    groups = {}
    for k, v in a:
        groups.setdefault(k, ([], []))[0].append(v)
    for k, w in b:
        groups.setdefault(k, ([], []))[1].append(w)
    out = []
    for k, (vs, ws) in groups.items():
        if vs and ws:
            out += [(k, v, w, 3) for v in vs for w in ws]
        elif vs and kind in (jr.LEFT_OUTER, jr.FULL_OUTER):
            out += [(k, v, 0, 1) for v in vs]
        elif ws and kind in (jr.RIGHT_OUTER, jr.FULL_OUTER):
            out += [(k, 0, w, 2) for w in ws]
    return sorted(out)


def as_tuples(cols4):
    return list(zip(*[c.tolist() for c in cols4]))


@pytest.mark.parametrize("kind", jr.KINDS)
def test_literal(kind):
    ak, av = cols(LIT_A)
    bk, bv = cols(LIT_B)
    if kind in jr.OUTER_KINDS:
        assert as_tuples(jr.outer(ak, av, bk, bv, kind)) == LIT_EXPECT[kind]
    else:
        assert as_tuples(jr.member(ak, av, bk, kind)) == LIT_EXPECT[kind]


@pytest.mark.parametrize("seed,na,nb,bits", [(1, 200, 150, 5), (2, 1, 300, 6), (3, 257, 0, 4),
                                             (4, 0, 64, 4), (5, 500, 500, 9), (6, 0, 0, 3)])
@pytest.mark.parametrize("kind", jr.KINDS)
def test_random_against_cogroup(kind, seed, na, nb, bits):
    rng = np.random.default_rng(seed)
    ak = rng.integers(-(1 << bits) // 2, (1 << bits) // 2, na)
    bk = rng.integers(-(1 << bits) // 2, (1 << bits) // 2, nb)
    av = rng.integers(-5, 5, na)     # zeros and repeats among the values
    bv = rng.integers(-5, 5, nb)
    a = list(zip(ak.tolist(), av.tolist()))
    b = list(zip(bk.tolist(), bv.tolist()))
    if kind in jr.OUTER_KINDS:
        assert as_tuples(jr.outer(ak, av, bk, bv, kind)) == cogroup_flat_map(a, b, kind)
    else:
        bset = set(bk.tolist())
        want = kind == jr.LEFT_SEMI
        exp = [(k, v) for k, v in a if (k in bset) == want]
        assert as_tuples(jr.member(ak, av, bk, kind)) == exp


def test_semi_and_anti_partition_a():
    ak, av = cols(LIT_A)
    bk, _ = cols(LIT_B)
    sk, _ = jr.member(ak, av, bk, jr.LEFT_SEMI)
    tk, _ = jr.member(ak, av, bk, jr.LEFT_ANTI)
    assert len(sk) + len(tk) == len(ak)
    assert not set(sk.tolist()) & set(tk.tolist())


def test_member_keeps_f64_values():
    ak = np.array([5, 6, 5], dtype=np.int64)
    av = np.array([0.5, -0.0, np.nan])
    k, v = jr.member(ak, av, [5], jr.LEFT_SEMI)
    assert v.dtype == np.float64 and k.tolist() == [5, 5]
    assert v.view(np.int64).tolist() == av[[0, 2]].view(np.int64).tolist()
