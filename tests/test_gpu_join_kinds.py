"""Outer, semi and anti joins on the GPU (vega_gpu_join_kind,
vega_gpu_collect_join_outer, vega_dev_join_grouped_kind) against
join_kinds_ref: results as sorted multisets of (k, va, vb, present), plus the
row order the header specifies."""
import ctypes
import os
import sys

import numpy as np
import pytest

import join_kinds_ref as jr
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vega_amd import datagen

pytestmark = pytest.mark.gpu

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
SPAN = 4096            # rows per block span of k_join_count / k_join_unmatched
GRID_CAP = 2048        # both kernels launch at most this many blocks
ERR_INVALID, ERR_CAP = -1, -5

LIT_A = ([1, 1, 2, 3], [10, 11, 20, 30])
LIT_B = ([1, 3, 3, 4], [0, 300, 301, 400])   # B value 0: only the presence byte tells
LIT_INNER = [(1, 10, 0, 3), (1, 11, 0, 3), (3, 30, 300, 3), (3, 30, 301, 3)]
LIT_EXPECT = {
    jr.INNER: LIT_INNER,
    jr.LEFT_OUTER: sorted(LIT_INNER + [(2, 20, 0, 1)]),
    jr.RIGHT_OUTER: sorted(LIT_INNER + [(4, 0, 400, 2)]),
    jr.FULL_OUTER: sorted(LIT_INNER + [(2, 20, 0, 1), (4, 0, 400, 2)]),
    jr.LEFT_SEMI: [(1, 10), (1, 11), (3, 30)],
    jr.LEFT_ANTI: [(2, 20)],
}


@pytest.fixture(scope="module")
def gpu():
    from vega_amd import gpu as g
    return g


@pytest.fixture(scope="module")
def ctx(gpu):
    with gpu.VegaContext() as c:
        yield c


def i64(a):
    return np.ascontiguousarray(a, dtype=np.int64)


def keys(seed, n, bits):
    if n == 0:
        return np.empty(0, dtype=np.int64)
    return datagen.uniform_pairs(seed, n, key_bits=bits)[0]


def assert_cols_equal(got, exp):
    assert len(got) == len(exp)
    for g, e in zip(got, exp):
        assert g.shape == e.shape, (g.shape, e.shape)
        assert np.array_equal(g, e)


def assert_lex_within_key(k, x, y):
    """within each key, in output order, the (x, y) pairs ascend"""
    idx = np.argsort(k, kind="stable")
    ks, xs, ys = k[idx], x[idx], y[idx]
    same = ks[1:] == ks[:-1]
    ok = (xs[1:] > xs[:-1]) | ((xs[1:] == xs[:-1]) & (ys[1:] >= ys[:-1]))
    assert bool((~same | ok).all())


def check_outer(a, b, cols, kind, inner_ref, inner_gpu, row_index_values=False):
    """one of the kinds 0-3 on the rdds a, b built from cols"""
    ak, av, bk, bv = cols
    r = a.join_kind(b, kind)
    try:
        k, va, vb, p = r.collect_join_outer()
        assert r.count() == len(k)
        assert_cols_equal(r.collect_join(), (k, va, vb))
    finally:
        r.free()
    # absent slots are exactly 0, presence bytes only ever 1, 2 or 3
    assert bool(np.isin(p, (1, 2, 3)).all())
    assert not vb[p == jr.HAS_A].any() and not va[p == jr.HAS_B].any()
    assert_cols_equal(jr.sorted_rows(k, va, vb, p),
                      jr.outer(ak, av, bk, bv, kind, inner=inner_ref))
    both = p == 3
    if kind == jr.INNER:
        assert bool(both.all())
    if kind in (jr.INNER, jr.LEFT_OUTER, jr.FULL_OUTER):
        # the matched rows, in order, are the inner join's rows
        assert_cols_equal((k[both], va[both], vb[both]), inner_gpu)
    if kind == jr.LEFT_OUTER:
        assert not (p == jr.HAS_B).any()
    if kind == jr.RIGHT_OUTER:
        assert not (p == jr.HAS_A).any()
    if kind == jr.FULL_OUTER:
        tail = np.flatnonzero(p == jr.HAS_B)
        assert len(tail) == 0 or tail[0] == len(p) - len(tail)   # after every other row
    if row_index_values:
        head = p != jr.HAS_B if kind == jr.FULL_OUTER else np.ones(len(p), dtype=bool)
        if kind == jr.RIGHT_OUTER:
            assert_lex_within_key(k, vb, va)
        else:
            assert_lex_within_key(k[head], va[head], vb[head])
            tail = ~head   # FULL's appended B rows keep B's row order within a key
            assert_lex_within_key(k[tail], vb[tail], va[tail])
    return k, va, vb, p


def check_member(a, b, cols):
    """semi and anti: the numpy masks in order, and a partition of A"""
    ak, av, bk, _ = cols
    got = {}
    for kind in (jr.LEFT_SEMI, jr.LEFT_ANTI):
        r = a.join_kind(b, kind)
        try:
            got[kind] = r.collect()
            assert r.count() == len(got[kind][0])
        finally:
            r.free()
        assert_cols_equal(got[kind], jr.member(ak, av, bk, kind))
    assert len(got[jr.LEFT_SEMI][0]) + len(got[jr.LEFT_ANTI][0]) == len(ak)


def run_case(ctx, ak, av, bk, bv, kinds=jr.KINDS, row_index_values=False):
    cols = (i64(ak), i64(av), i64(bk), i64(bv))
    a = ctx.make_rdd(cols[0], cols[1])
    b = ctx.make_rdd(cols[2], cols[3])
    try:
        outer_kinds = [kd for kd in kinds if kd in jr.OUTER_KINDS]
        if outer_kinds:
            inner_ref = jr.inner_rows(*cols)
            j = a.join(b)
            inner_gpu = j.collect_join()
            j.free()
            for kind in outer_kinds:
                check_outer(a, b, cols, kind, inner_ref, inner_gpu, row_index_values)
        if jr.LEFT_SEMI in kinds or jr.LEFT_ANTI in kinds:
            check_member(a, b, cols)
        # inputs unchanged after every kind
        assert_cols_equal(a.collect(), cols[:2])
        assert_cols_equal(b.collect(), cols[2:])
    finally:
        a.free()
        b.free()


def test_literal(ctx):
    a = ctx.make_rdd(*LIT_A)
    b = ctx.make_rdd(*LIT_B)
    for kind in jr.OUTER_KINDS:
        r = a.join_kind(b, kind)
        got = sorted(zip(*[c.tolist() for c in r.collect_join_outer()]))
        r.free()
        assert got == LIT_EXPECT[kind], kind
    for kind in (jr.LEFT_SEMI, jr.LEFT_ANTI):
        r = a.join_kind(b, kind)
        got = list(zip(*[c.tolist() for c in r.collect()]))   # A's row order
        r.free()
        assert got == LIT_EXPECT[kind], kind
    a.free(); b.free()
    run_case(ctx, *LIT_A, *LIT_B)


def test_wrappers_name_the_kinds(ctx, gpu):
    a = ctx.make_rdd(*LIT_A)
    b = ctx.make_rdd(*LIT_B)
    for fn, kind in ((a.left_outer_join, jr.LEFT_OUTER), (a.right_outer_join, jr.RIGHT_OUTER),
                     (a.full_outer_join, jr.FULL_OUTER)):
        r = fn(b)
        assert sorted(zip(*[c.tolist() for c in r.collect_join_outer()])) == LIT_EXPECT[kind]
        r.free()
    for fn, kind in ((a.semi_join, jr.LEFT_SEMI), (a.subtract_by_key, jr.LEFT_ANTI)):
        r = fn(b)
        assert list(zip(*[c.tolist() for c in r.collect()])) == LIT_EXPECT[kind]
        r.free()
    assert (gpu.JOIN_INNER, gpu.JOIN_LEFT_OUTER, gpu.JOIN_RIGHT_OUTER, gpu.JOIN_FULL_OUTER,
            gpu.JOIN_LEFT_SEMI, gpu.JOIN_LEFT_ANTI) == jr.KINDS
    a.free(); b.free()


@pytest.mark.parametrize("na,nb", [(0, 0), (1000, 0), (0, 1000)])
def test_empty_sides(ctx, na, nb):
    run_case(ctx, keys(11, na, 9), np.arange(na), keys(12, nb, 9), np.arange(nb))


# 13 key bits against 5000 rows: exp(-5000/8192) = 54 % of the varied side's
# rows find no partner
@pytest.mark.parametrize("n", [1, SPAN - 1, SPAN, SPAN + 1, 2 * SPAN + 1])
def test_span_edges_on_a(ctx, n):
    run_case(ctx, keys(21, n, 13), np.arange(n), keys(22, 5000, 13), np.arange(5000),
             kinds=(jr.LEFT_OUTER, jr.FULL_OUTER, jr.LEFT_SEMI, jr.LEFT_ANTI),
             row_index_values=True)


@pytest.mark.parametrize("n", [1, SPAN - 1, SPAN, SPAN + 1, 2 * SPAN + 1])
def test_span_edges_on_b(ctx, n):
    run_case(ctx, keys(23, 5000, 13), np.arange(5000), keys(24, n, 13), np.arange(n),
             kinds=(jr.RIGHT_OUTER, jr.FULL_OUTER), row_index_values=True)


def test_all_matched(ctx):
    n = 6000
    k = keys(31, n, 11)
    rng = np.random.default_rng(31)
    run_case(ctx, k, np.arange(n), rng.permutation(k), np.arange(n), row_index_values=True)


def test_none_matched(ctx):
    na, nb = 5000, 4500
    ak = keys(32, na, 12) * 2          # A even, B odd
    bk = keys(33, nb, 12) * 2 + 1
    run_case(ctx, ak, np.arange(na), bk, np.arange(nb))
    a = ctx.make_rdd(ak, np.arange(na))
    b = ctx.make_rdd(bk, np.arange(nb))
    r = a.full_outer_join(b)
    _, _, _, p = r.collect_join_outer()
    assert len(p) == na + nb and int((p == 1).sum()) == na and int((p == 2).sum()) == nb
    r.free(); a.free(); b.free()


def test_heavy_duplicates(ctx):
    # 8 shared keys of ~250 rows a side: cross products of ~60k rows per key,
    # each written by one thread; keys 100 (A) and 200 (B) occur on one side only
    n = 2000
    rng = np.random.default_rng(41)
    ak = rng.integers(0, 8, n)
    bk = rng.integers(0, 8, n)
    ak[rng.choice(n, 5, replace=False)] = 100
    bk[rng.choice(n, 7, replace=False)] = 200
    run_case(ctx, ak, np.arange(n), bk, np.arange(n), row_index_values=True)


def test_mixed_order_tags(ctx):
    """the shapes of test_join_mixed_order_tags: a narrow-key side (tag 0)
    against a wide-key side with negatives (tag 4)"""
    na, nb = 300_000, 200_000
    ak, av = datagen.uniform_pairs(51, na, key_bits=8)     # narrow: tag 0
    bk_w, bv = datagen.uniform_pairs(52, nb, key_bits=64)  # wide (negatives): tag 4
    # overlap: every 200th row of b falls into a's narrow range (~4 rows a
    # key against ~1170 of a's: an inner join of ~1.2e6 rows; the ~2 % of the
    # 256 keys that b misses leave a few thousand rows of a unmatched)
    bk = np.where(np.arange(nb) % 200 == 0, bk_w & 0xFF, bk_w)
    run_case(ctx, ak, av, bk, bv, kinds=(jr.LEFT_OUTER, jr.FULL_OUTER, jr.LEFT_ANTI))


def test_extreme_keys(ctx):
    ak = [I64_MIN, -1, 0, 5, I64_MIN, I64_MAX, 9]
    bk = [I64_MIN, 0, 0, I64_MAX, 7, 9, 9]
    run_case(ctx, ak, np.arange(len(ak)), bk, np.arange(len(bk)), row_index_values=True)
    # and with each extreme on one side only
    ak = [I64_MIN, -1, 3, 3]
    bk = [I64_MAX, 0, 3]
    run_case(ctx, ak, np.arange(len(ak)), bk, np.arange(len(bk)), row_index_values=True)


# ---- more spans than the grid cap: a block loops over spans only above
# GRID_CAP * SPAN rows, for k_join_count and k_join_unmatched alike ----

@pytest.fixture(scope="module")
def big():
    """one big and one small side; values are row index + 1, so a row is
    named by (va, vb) and 0 can only be an absent slot"""
    nbig, nsmall = GRID_CAP * SPAN + SPAN + 1, 1 << 20
    kb = keys(61, nbig, 23)
    ks = keys(62, nsmall, 23)
    vb_, vs = np.arange(1, nbig + 1), np.arange(1, nsmall + 1)
    # rows without a partner add nothing to the inner join: the oracle gets
    # only the rows whose key occurs on the other side (an eighth of the big one)
    mb, ms = np.isin(kb, ks), np.isin(ks, kb)
    ik, iv_big, iv_small = jr.inner_rows(kb[mb], vb_[mb], ks[ms], vs[ms])
    return dict(kb=kb, vb=i64(vb_), ks=ks, vs=i64(vs), inner=(ik, iv_big, iv_small))


def canon(k, vbig, vsmall, p):
    """order rows by the injective code (vbig, vsmall): vsmall <= 2^20"""
    idx = np.argsort(vbig * (1 << 21) + vsmall, kind="stable")
    return k[idx], vbig[idx], vsmall[idx], p[idx]


def big_expected(big, big_unmatched, small_unmatched):
    ik, ivb, ivs = big["inner"]
    cols = [[ik], [ivb], [ivs], [np.full(len(ik), 3, dtype=np.uint8)]]
    if big_unmatched:
        m = ~np.isin(big["kb"], big["ks"])
        z = np.zeros(int(m.sum()), dtype=np.int64)
        for c, x in zip(cols, (big["kb"][m], big["vb"][m], z, np.full(len(z), 1, dtype=np.uint8))):
            c.append(x)
    if small_unmatched:
        m = ~np.isin(big["ks"], big["kb"])
        z = np.zeros(int(m.sum()), dtype=np.int64)
        for c, x in zip(cols, (big["ks"][m], z, big["vs"][m], np.full(len(z), 2, dtype=np.uint8))):
            c.append(x)
    return [np.concatenate(c) for c in cols]


def test_more_spans_than_grid_full_and_anti(ctx, big):
    a = ctx.make_rdd(big["kb"], big["vb"])      # A is the big side: the driving pass loops
    b = ctx.make_rdd(big["ks"], big["vs"])
    r = a.full_outer_join(b)
    k, va, vb, p = r.collect_join_outer()
    r.free()
    ek, ebig, esmall, ep = big_expected(big, True, True)
    assert_cols_equal(canon(k, va, vb, p), canon(ek, ebig, esmall, ep))
    tail = np.flatnonzero(p == jr.HAS_B)
    assert len(tail) and tail[0] == len(p) - len(tail)
    r = a.subtract_by_key(b)
    assert_cols_equal(r.collect(), jr.member(big["kb"], big["vb"], big["ks"], jr.LEFT_ANTI))
    r.free(); a.free(); b.free()


def test_more_spans_than_grid_right_and_full_mirrored(ctx, big):
    a = ctx.make_rdd(big["ks"], big["vs"])      # B is the big side: RIGHT's driving pass
    b = ctx.make_rdd(big["kb"], big["vb"])      # and FULL's unmatched pass loop
    r = a.right_outer_join(b)
    k, va, vb, p = r.collect_join_outer()
    r.free()
    ek, ebig, esmall, ep = big_expected(big, True, False)
    ep = np.where(ep == 1, 2, ep).astype(np.uint8)       # the big side is B here
    assert_cols_equal(canon(k, vb, va, p), canon(ek, ebig, esmall, ep))
    r = a.full_outer_join(b)
    k, va, vb, p = r.collect_join_outer()
    r.free()
    ek, ebig, esmall, ep = big_expected(big, True, True)
    ep = np.where(ep == 3, 3, 3 - ep).astype(np.uint8)   # swap HAS_A and HAS_B
    assert_cols_equal(canon(k, vb, va, p), canon(ek, ebig, esmall, ep))
    a.free(); b.free()


def test_semi_anti_keep_f64_values(ctx):
    n = 5000
    ak = keys(71, n, 12)
    bits = datagen.uniform_pairs(72, n, key_bits=64)[0]        # arbitrary bit patterns,
    av = bits.view(np.float64).copy()                          # NaNs and -0.0 included
    av[:3] = [-0.0, np.nan, np.inf]
    bk = keys(73, 3000, 12)
    a = ctx.make_rdd(ak, av)
    b = ctx.make_rdd(bk, np.arange(3000))
    for kind in (jr.LEFT_SEMI, jr.LEFT_ANTI):
        r = a.join_kind(b, kind)
        gk, gv = r.collect()
        r.free()
        ek, ev = jr.member(ak, av, bk, kind)
        assert gv.dtype == np.float64
        assert np.array_equal(gk, ek) and np.array_equal(gv.view(np.int64), ev.view(np.int64))
    a.free(); b.free()


def test_member_result_feeds_other_ops(ctx, gpu):
    """a semi-join result is a plain rdd: an op and an action take it"""
    a = ctx.make_rdd(*LIT_A)
    b = ctx.make_rdd(*LIT_B)
    s = a.semi_join(b)
    red = s.reduce_by_key(gpu.OP_SUM_I64)
    assert sorted(zip(*[c.tolist() for c in red.collect()])) == [(1, 21), (3, 30)]
    assert s.reduce(gpu.OP_SUM_I64) == (5, 51)
    red.free(); s.free(); a.free(); b.free()


def test_device_entry(ctx, gpu):
    import torch
    na, nb = 2 * SPAN + 77, 5000
    spread = 0x9E3779B97F4A7C15 - (1 << 64)          # wide keys with negatives
    with np.errstate(over="ignore"):
        ak = keys(81, na, 13) * np.int64(spread)
        bk = keys(82, nb, 13) * np.int64(spread)
    av, bv = np.arange(na, dtype=np.int64), np.arange(nb, dtype=np.int64)
    dev = "cuda"
    t = [torch.from_numpy(x).to(dev) for x in (ak, av, bk, bv)]
    ws = gpu.alloc_ws(max(na, nb), dev)
    ta = gpu.dev_group_pairs(t[0], t[1], ws)
    tb = gpu.dev_group_pairs(t[2], t[3], ws)
    if ta == 4 and tb == 4:
        mode = 2
    elif ta == 0 and tb == 0:
        mode = 1
    else:
        gpu.dev_sort_pairs(t[0], t[1], ws)
        gpu.dev_sort_pairs(t[2], t[3], ws)
        mode = 0
    torch.cuda.synchronize()
    before = [x.clone() for x in t]
    a = ctx.make_rdd(ak, av)
    b = ctx.make_rdd(bk, bv)
    for kind in jr.OUTER_KINDS:
        r = a.join_kind(b, kind)
        exp = r.collect_join_outer()
        r.free()
        # count-only: the handle path's row count, nothing needed for output
        n = ctypes.c_uint64(0)
        rc = gpu.lib().vega_dev_join_grouped_kind(
            gpu._stream(), gpu._t(t[0]), gpu._t(t[1]), ctypes.c_uint64(na), gpu._t(t[2]),
            gpu._t(t[3]), ctypes.c_uint64(nb), ctypes.c_int(mode), ctypes.c_int(kind),
            None, None, None, None, ctypes.c_uint64(0), ctypes.byref(n), gpu._t(ws),
            ctypes.c_size_t(ws.numel()))
        assert rc == 0 and n.value == len(exp[0])
        # too small a cap: VEGA_ERR_CAP, the needed count, untouched buffers
        small = tuple(torch.full((n.value - 1,), -7, dtype=torch.int64, device=dev)
                      for _ in range(3)) + (torch.full((n.value - 1,), 9, dtype=torch.uint8,
                                                       device=dev),)
        with pytest.raises(gpu.VegaGpuError) as ei:
            gpu.dev_join_grouped_kind(*t, mode, kind, out=small, ws_t=ws)
        assert ei.value.rc == ERR_CAP and ei.value.needed == n.value
        torch.cuda.synchronize()
        assert all(bool((x == -7).all()) for x in small[:3]) and bool((small[3] == 9).all())
        # the full call
        k, va, vb, p, m = gpu.dev_join_grouped_kind(*t, mode, kind, ws_t=ws)
        got = tuple(x.cpu().numpy() for x in (k, va, vb, p))
        assert m == n.value
        if mode == 2:       # the comparator the handle path used: same row order
            assert_cols_equal(got, exp)
        assert_cols_equal(jr.sorted_rows(*got), jr.sorted_rows(*exp))
    # the grouped inputs were not modified by the joins
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(t, before))
    a.free(); b.free()


def test_errors(ctx, gpu):
    a = ctx.make_rdd(*LIT_A)
    b = ctx.make_rdd(*LIT_B)
    for bad in (-1, 6, 99):
        with pytest.raises(gpu.VegaGpuError) as ei:
            a.join_kind(b, bad)
        assert ei.value.rc == ERR_INVALID
    outer = a.left_outer_join(b)
    inner = a.join(b)
    grouped_stats = a.stats_by_key()
    for bad_input in (outer, inner, grouped_stats):
        for kind in (jr.LEFT_OUTER, jr.LEFT_ANTI):
            with pytest.raises(gpu.VegaGpuError) as ei:
                a.join_kind(bad_input, kind)
            assert ei.value.rc == ERR_INVALID
            with pytest.raises(gpu.VegaGpuError) as ei:
                gpu.Rdd(ctx, bad_input.h, np.int64).join_kind(b, kind)
            assert ei.value.rc == ERR_INVALID
    # a device-side action rejects an outer result like any join result
    for act in (lambda: outer.reduce(gpu.OP_SUM_I64), lambda: outer.take(1),
                lambda: outer.sample(False, 0.5, seed=1)):
        with pytest.raises(gpu.VegaGpuError) as ei:
            act()
        assert ei.value.rc == ERR_INVALID
    # an inner result collects through the outer entry with presence 3
    k, va, vb, p = inner.collect_join_outer()
    assert sorted(zip(k.tolist(), va.tolist(), vb.tolist(), p.tolist())) == LIT_INNER
    # f64 values are refused by the kinds 0-3
    f = ctx.make_rdd([1, 2], np.array([0.5, 1.5]))
    with pytest.raises(gpu.VegaGpuError) as ei:
        f.join_kind(b, jr.FULL_OUTER)
    assert ei.value.rc == ERR_INVALID
    for r in (outer, inner, grouped_stats, f, a, b):
        r.free()
