"""stats_by_key_f64 (count, sum, min, max over f64 values in one grouping sort
and one segmented pass, k_seg_stats_f64<PK> + k_stats_f64_fold +
k_f64_seg_combine) and the f64 order ops OP_MIN_F64 / OP_MAX_F64 through
reduce_by_key, reduce, fold and the device-pointer entries.

The edge inputs are the project's hand-placed layouts (tests/seg_layout.py,
tests/finish_heads_keys.py); the reference is tests/stats_f64_ref.py. count,
min and max are compared bit for bit (NaN: isnan). The sum is compared
  - bit for bit with the reference where the values make every order exact,
  - bit for bit with reduce_by_key(OP_SUM_F64) of the same handle (same
    grouped rows, same summation shape),
  - within len * 2^-52 * sum|v| of math.fsum otherwise
    (test_gpu_segreduce.check_f64_bound's any-order bound).
"""
import ctypes
import functools

import numpy as np
import pytest

import finish_heads_keys as fh
import seg_layout as sl
import stats_f64_ref as sr

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_UNSUPPORTED, ERR_CAP = -1, -4, -5
SENT_I = -0x0123456789ABCDEF
SENT_F = -1.2345678901234567e-123   # a double no test input or result holds

LAYOUTS = {"soa0": (lambda: sl.soa_layout(0), "narrow"),
           "soa3": (lambda: sl.soa_layout(3), "narrow"),
           "hash_minus1": (lambda: sl.hash_layout(True), "hash"),
           "hash_plain": (lambda: sl.hash_layout(False), "hash")}
ONE_EACH = ("soa3", "hash_minus1")   # one SoA and one packed layout


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


def nan_of(i):
    """NaNs of both signs and several payloads"""
    pats = (0x7FF8000000000000, 0xFFF8000000000000, 0x7FF0000000000001, 0xFFFFFFFFFFFFFFFF)
    return np.array([pats[i % 4]], dtype=np.uint64).view(np.float64)[0]


(SP_PLAIN, SP_NAN_FIRST, SP_NAN_LAST, SP_NAN_LATER, SP_ZEROS_PM, SP_ZEROS_MP, SP_INFS, SP_DENORM,
 SP_ALL_NAN) = range(9)


def special_classes(lay):
    """class per run: cycles through the classes; then one run of length 1, one
    of length 9 and the shortest run that crosses a tile edge are made all-NaN,
    and the longest crossing run carries its NaN in a later chunk"""
    nr = len(lay.run_lens)
    cls = (np.arange(nr) * 5 + 1) % 9
    crossing = np.flatnonzero(lay.gstart // sl.TILE != (lay.gstart + lay.run_lens - 1) // sl.TILE)
    crossing = crossing[np.argsort(lay.run_lens[crossing], kind="stable")]
    assert len(crossing) >= 2
    cls[crossing[-1]] = SP_NAN_LATER
    forced = [int(np.flatnonzero(lay.run_lens == 1)[0]), int(np.flatnonzero(lay.run_lens == 9)[0]),
              int(crossing[0])]
    cls[forced] = SP_ALL_NAN
    return cls, forced


def values_special(lay, rng):
    v = rng.standard_normal(lay.n) * 10.0 ** rng.randint(-3, 6, size=lay.n)
    rcls, _ = special_classes(lay)
    cls = rcls[lay.row_run]
    p = lay.pos_in_run
    ln = lay.run_lens[lay.row_run]
    later = sl.later_chunk_pos(lay)[lay.row_run]
    nans = np.array([nan_of(i) for i in range(4)])[np.arange(lay.n) % 4]
    even = (p % 2) == 0

    def put(mask, vals):
        v[mask] = vals[mask] if isinstance(vals, np.ndarray) else vals

    put((cls == SP_NAN_FIRST) & (p == 0), nans)
    put((cls == SP_NAN_LAST) & (p == ln - 1), nans)
    put((cls == SP_NAN_LATER) & (p == later), nans)
    put((cls == SP_ZEROS_PM) & even, 0.0)
    put((cls == SP_ZEROS_PM) & ~even, -0.0)
    put((cls == SP_ZEROS_MP) & even, -0.0)
    put((cls == SP_ZEROS_MP) & ~even, 0.0)
    put((cls == SP_INFS) & (p == 0), np.inf)
    put((cls == SP_INFS) & (p == ln - 1) & (ln > 1), -np.inf)
    put((cls == SP_DENORM) & even, 5e-324)
    put((cls == SP_DENORM) & ~even, -5e-324)
    put(cls == SP_ALL_NAN, nans)
    return v


VALUES = {"integral": (sl.values_f64_integral, 31),
          "mixed": (sl.values_f64_mixed, 32),
          "extremes": (lambda lay, rng: sl.values_minmax(lay, rng).astype(np.float64), 33),
          "special": (values_special, 34)}


@functools.lru_cache(maxsize=None)
def values(name, what):
    gen, seed = VALUES[what]
    v = np.ascontiguousarray(gen(layout(name), np.random.RandomState(seed)), dtype=np.float64)
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def layout_ref(name, what):
    return sr.stats_f64_ref(layout(name).k, values(name, what))


def by_key(cols):
    o = np.argsort(cols[0], kind="stable")
    return tuple(np.asarray(c)[o] for c in cols)


def check_dtypes(got):
    assert len(got) == 5
    assert [c.dtype for c in got] == [np.int64, np.int64, np.float64, np.float64, np.float64]


def check_exact_columns(got, ref):
    """key, count, min, max: bit for bit (NaN where the reference is NaN)"""
    assert len(got[0]) == len(ref[0])
    for name, g, r in (("key", got[0], ref[0]), ("count", got[1], ref[1])):
        bad = np.flatnonzero(g != r)
        assert len(bad) == 0, (name, len(bad), got[0][bad][:5], g[bad][:5], r[bad][:5])
    for name, g, r in (("min", got[3], ref[3]), ("max", got[4], ref[4])):
        bad = np.flatnonzero(~sr.extremes_match(g, r))
        assert len(bad) == 0, (name, len(bad), got[0][bad][:5], g[bad][:5], r[bad][:5])


def check_sum_bits(got, ref):
    bad = np.flatnonzero(~sr.same_bits(got[2], ref[2]))
    assert len(bad) == 0, ("sum", len(bad), got[0][bad][:5], got[2][bad][:5], ref[2][bad][:5])


def check_sum_bound(got, ref):
    """NaN exactly where the reference is; +-inf equal; else the any-order
    bound |sum - fsum| <= len * 2^-52 * sum|v|"""
    g, fs, sabs, lens = got[2], ref[2], ref[5], ref[6]
    assert (np.isnan(g) == np.isnan(fs)).all(), got[0][np.isnan(g) != np.isnan(fs)][:5]
    inf = np.isinf(fs)
    assert (g[inf] == fs[inf]).all()
    fin = np.isfinite(fs)
    err = np.abs(g[fin] - fs[fin])
    bound = lens[fin] * 2.0 ** -52 * sabs[fin]
    bad = np.flatnonzero(~(err <= bound))
    assert len(bad) == 0, (got[0][fin][bad][:5], g[fin][bad][:5], fs[fin][bad][:5], bound[bad][:5])


def assert_kernels(stats, strategy):
    """one head count, one fused f64 pass, no single-op pass and no i64 stats
    pass; and the grouping strategy test_gpu_stats.assert_kernels expects"""
    names = set(stats)
    assert stats["seg_stats_f64"]["n"] == 1 and stats["head_count"]["n"] == 1, stats
    assert "seg_emit" not in names and "seg_stats" not in names, names
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


def still_answers(ctx):
    """the context computes a normal reduce_by_key correctly"""
    from vega_amd import gpu
    k = np.arange(1000, dtype=np.int64) % 37
    v = np.arange(1000, dtype=np.int64) * 3 - 500
    rdd = ctx.make_rdd(k, v)
    red = rdd.reduce_by_key(gpu.OP_SUM_I64)
    assert sl.sorted_pairs(*red.collect()) == sl.sorted_pairs(*sl.reduce_ref(sl.OP_SUM_I64, k, v))
    rdd.free(); red.free()


def refused(rc, fn):
    from vega_amd import gpu
    with pytest.raises(gpu.VegaGpuError) as ei:
        fn()
    assert ei.value.rc == rc, ei.value
    return ei.value


def reduce_both(rdd):
    """((keys, min) by key, (keys, max) by key) through reduce_by_key"""
    from vega_amd import gpu
    out = []
    for op in (gpu.OP_MIN_F64, gpu.OP_MAX_F64):
        red = rdd.reduce_by_key(op)
        assert red.vdtype == np.float64
        out.append(by_key(red.collect()))
        red.free()
    return out


def check_reduce_both(rdd, ref):
    (kn, mn), (kx, mx) = reduce_both(rdd)
    assert len(kn) == len(ref[0]) and (kn == ref[0]).all() and (kx == ref[0]).all()
    for name, g, r in (("min", mn, ref[3]), ("max", mx, ref[4])):
        assert g.dtype == np.float64
        bad = np.flatnonzero(~sr.extremes_match(g, r))
        assert len(bad) == 0, (name, len(bad), kn[bad][:5], g[bad][:5], r[bad][:5])


# ---- 1. edges, both row forms ----

@pytest.mark.parametrize("name", sorted(LAYOUTS))
def test_edges_integral(ctx, name):
    """sums exact in any order: all five columns bit-equal to the reference"""
    lay = layout(name)
    rdd = ctx.make_rdd(lay.k, values(name, "integral"))
    st, kstats = profiled(ctx, rdd.stats_by_key_f64)
    assert_kernels(kstats, LAYOUTS[name][1])
    got = st.collect()
    check_dtypes(got)
    assert st.count() == len(lay.run_lens) == len(got[0])
    got = by_key(got)
    ref = layout_ref(name, "integral")
    check_exact_columns(got, ref)
    check_sum_bits(got, ref)
    rdd.free(); st.free()


@pytest.mark.parametrize("name", sorted(LAYOUTS))
def test_edges_mixed(ctx, name):
    lay = layout(name)
    rdd = ctx.make_rdd(lay.k, values(name, "mixed"))
    st = rdd.stats_by_key_f64()
    first = st.collect()
    got = by_key(first)
    ref = layout_ref(name, "mixed")
    check_exact_columns(got, ref)
    check_sum_bound(got, ref)
    st2 = rdd.stats_by_key_f64()
    second = st2.collect()
    for a, b in zip(first, second):   # same rows, same order, same bits
        assert a.dtype == b.dtype and (a.view(np.int64) == b.view(np.int64)).all()
    gk, gv = rdd.collect()            # input untouched
    assert (gk == lay.k).all() and sr.same_bits(gv, values(name, "mixed")).all()
    rdd.free(); st.free(); st2.free()


# ---- 2. sum shape ----

@pytest.mark.parametrize("name", sorted(LAYOUTS))
def test_sum_shape_is_reduce_by_key(ctx, name):
    from vega_amd import gpu
    lay = layout(name)
    rdd = ctx.make_rdd(lay.k, values(name, "mixed"))
    st = rdd.stats_by_key_f64()
    got = by_key(st.collect())
    red = rdd.reduce_by_key(gpu.OP_SUM_F64)
    rk, rv = by_key(red.collect())
    assert (rk == got[0]).all()
    bad = np.flatnonzero(~sr.same_bits(got[2], rv))
    assert len(bad) == 0, (len(bad), rk[bad][:5], got[2][bad][:5], rv[bad][:5])
    cnt = rdd.group_count()
    ck, cv = by_key(cnt.collect())
    assert (ck == got[0]).all() and (cv == got[1]).all()
    (kn, mn), (kx, mx) = reduce_both(rdd)
    assert (kn == got[0]).all() and (kx == got[0]).all()
    assert sr.same_bits(mn, got[3]).all() and sr.same_bits(mx, got[4]).all()
    for r in (rdd, st, red, cnt):
        r.free()


# ---- 3. extremes in every position ----

@pytest.mark.parametrize("name", ONE_EACH)
def test_extremes_in_every_position(ctx, name):
    lay = layout(name)
    v = values(name, "extremes")
    assert v.min() == -2.0 ** 63 and v.max() == 2.0 ** 63   # the planted extremes stay extreme
    ref = layout_ref(name, "extremes")
    rdd = ctx.make_rdd(lay.k, v)
    st = rdd.stats_by_key_f64()
    got = by_key(st.collect())
    check_exact_columns(got, ref)
    check_sum_bound(got, ref)
    check_reduce_both(rdd, ref)
    rdd.free(); st.free()


# ---- 4. special values ----

@pytest.mark.parametrize("name", ONE_EACH)
def test_special_values(ctx, name):
    lay = layout(name)
    v = values(name, "special")
    rcls, forced = special_classes(lay)
    ref = layout_ref(name, "special")
    # what the planting promises, seen through the reference
    pos = {int(k): i for i, k in enumerate(ref[0].tolist())}
    crossing = forced[2]
    assert lay.gstart[crossing] // sl.TILE != (lay.gstart[crossing] + lay.run_lens[crossing] - 1) // sl.TILE
    for run, ln in zip(forced, (1, 9, int(lay.run_lens[crossing]))):
        i = pos[int(lay.keys[run])]
        assert ref[1][i] == ln and np.isnan(ref[3][i]) and np.isnan(ref[4][i]) and np.isnan(ref[2][i])
    for c in range(9):
        assert (rcls == c).any(), c
    zeros = np.flatnonzero(((rcls == SP_ZEROS_PM) | (rcls == SP_ZEROS_MP)) & (lay.run_lens > 1))
    zi = [pos[int(lay.keys[r])] for r in zeros]
    assert len(zi) > 1
    assert (np.signbit(ref[3][zi])).all() and not np.signbit(ref[4][zi]).any()
    assert (ref[3][zi] == 0).all() and (ref[4][zi] == 0).all()

    rdd = ctx.make_rdd(lay.k, v)
    st = rdd.stats_by_key_f64()
    got = by_key(st.collect())
    check_exact_columns(got, ref)   # count includes the NaN rows
    check_sum_bound(got, ref)       # NaN exactly where the reference is
    check_reduce_both(rdd, ref)
    rdd.free(); st.free()


# ---- 5. bucket-finish route ----

@functools.lru_cache(maxsize=None)
def finish_input(n):
    lay = fh.build(n, seed=n)
    rng = np.random.RandomState(n)
    v = rng.randint(-(1 << 30), (1 << 30) + 1, size=n).astype(np.float64)   # sums exact
    v[rng.randint(0, n, size=16)] = np.nan
    lay.k.setflags(write=False)
    v.setflags(write=False)
    return lay, v, sr.stats_f64_ref(lay.k, v)


def dev_profiled(fn):
    import torch
    from vega_amd import gpu
    gpu.prof_stats()
    gpu.prof_enable(True)
    try:
        out = fn()
        torch.cuda.synchronize()
        stats = gpu.prof_stats()
    finally:
        gpu.prof_enable(False)
    return out, stats


def assert_finish_route(stats):
    assert stats["bucket_finish"]["n"] == 1 and stats["radix_scatter"]["n"] == 3, stats
    assert stats["head_count"]["n"] == 1, stats


@pytest.mark.parametrize("n", fh.SIZES)
def test_finish_route(n):
    import torch
    from vega_amd import gpu
    lay, v, ref = finish_input(n)
    kt = torch.from_numpy(np.array(lay.k)).cuda()
    vt = torch.from_numpy(np.array(v)).cuda()
    oi = [torch.full((n,), SENT_I, dtype=torch.int64, device="cuda") for _ in range(2)]
    of = [torch.full((n,), SENT_F, dtype=torch.float64, device="cuda") for _ in range(3)]
    ws = gpu.alloc_ws(n)
    nout, stats = dev_profiled(lambda: gpu.dev_sort_stats_f64(kt, vt, *oi, *of, ws))
    assert_finish_route(stats)
    assert stats["seg_stats_f64"]["n"] == 1 and "seg_stats" not in stats and "seg_emit" not in stats
    assert nout == len(ref[0])
    got = by_key(tuple(o[:nout].cpu().numpy() for o in oi + of))
    check_exact_columns(got, ref)
    nonan = ~np.isnan(ref[2])
    assert (np.isnan(got[2]) == ~nonan).all() and (~nonan).sum() >= 1
    assert sr.same_bits(got[2][nonan], ref[2][nonan]).all()
    for o in oi:
        assert (o[nout:] == SENT_I).all()
    for o in of:
        assert (o[nout:] == SENT_F).all()
    # and in the grouped order, like the single-op reduce
    assert (oi[0][:nout].cpu().numpy() == lay.final_k[lay.run_start]).all()

    for op, col in ((gpu.OP_MIN_F64, 3), (gpu.OP_MAX_F64, 4)):
        ok = torch.full((n,), SENT_I, dtype=torch.int64, device="cuda")
        ov = torch.full((n,), SENT_F, dtype=torch.float64, device="cuda")
        nout2, stats = dev_profiled(lambda: gpu.dev_sort_reduce(kt, vt, op, ok, ov, ws))
        assert_finish_route(stats)
        assert stats["seg_emit"]["n"] == 1
        assert nout2 == nout
        gk, gv = by_key((ok[:nout].cpu().numpy(), ov[:nout].cpu().numpy()))
        assert (gk == ref[0]).all() and sr.extremes_match(gv, ref[col]).all()
        assert (ok[nout:] == SENT_I).all() and (ov[nout:] == SENT_F).all()


# ---- 5b. sizes at which the lead arrays no longer fit the workspace's slack ----
# count / min / max leads (20 B per chunk) live in the grouping sort's idle
# ping-pong buffer, next to the buffer that holds the grouped rows; past ~4e5
# rows they can live nowhere else. A wrong choice of buffer would overwrite the
# rows under the pass. 1,000,003 rows (245 tiles, n % 8 == 3), runs that cross
# chunks so that every lead array is written, on the SoA (narrow) route, on the
# packed four-pass hash route and, keys all distinct, on the packed route with
# no lead at all. (The bucket-finish route takes its idle buffer through the
# same report; the automatic route picks it only from ~4e8 rows, and the
# layouts of section 5 already keep their leads there.)

BIG_N = 1_000_003


@functools.lru_cache(maxsize=None)
def big_input(kind):
    rng = np.random.RandomState(77)
    if kind == "narrow":
        k = rng.randint(0, 1 << 16, size=BIG_N, dtype=np.int64)          # runs of ~15
    elif kind == "hash_runs":
        pool = rng.randint(1 << 40, 1 << 62, size=50_000, dtype=np.int64)
        k = pool[rng.randint(0, len(pool), size=BIG_N)]                   # runs of ~20
    else:
        k = rng.permutation(BIG_N).astype(np.int64) * 4_000_000_007 + (1 << 40)   # < 2^52, no overflow
        assert len(np.unique(k)) == BIG_N
    v = rng.standard_normal(BIG_N) * 10.0 ** rng.randint(-3, 6, size=BIG_N)
    v[rng.randint(0, BIG_N, size=64)] = np.nan
    order = np.argsort(k, kind="stable")
    ks = k[order]
    starts = np.flatnonzero(np.concatenate([[True], ks[1:] != ks[:-1]]))
    cnt = np.diff(np.concatenate([starts, [BIG_N]])).astype(np.int64)
    rk, mn, mx = sr.minmax_f64_ref(k, v)
    for a in (k, v):
        a.setflags(write=False)
    return k, v, (rk, cnt, None, mn, mx)


@pytest.mark.parametrize("kind", ("narrow", "hash_runs", "hash_distinct"))
def test_leads_in_the_idle_sort_buffer(ctx, kind):
    import torch
    from vega_amd import gpu
    k, v, ref = big_input(kind)
    assert 20 * 512 * ((BIG_N + 4095) // 4096) > (1 << 20)   # more than the workspace's slack
    rdd = ctx.make_rdd(k, v)
    st, kstats = profiled(ctx, rdd.stats_by_key_f64)
    assert_kernels(kstats, "narrow" if kind == "narrow" else "hash")
    assert "bucket_finish" not in kstats
    got = by_key(st.collect())
    check_exact_columns(got, ref)
    red = rdd.reduce_by_key(gpu.OP_SUM_F64)
    rk, rv = by_key(red.collect())
    assert (rk == got[0]).all()
    bad = np.flatnonzero(~sr.same_bits(got[2], rv))
    assert len(bad) == 0, (len(bad), rk[bad][:5], got[2][bad][:5], rv[bad][:5])
    assert np.isnan(got[2]).sum() >= 1
    rdd.free(); st.free(); red.free()

    # the device entry on a workspace of exactly vega_dev_ws_bytes(n)
    kt = torch.from_numpy(np.array(k)).cuda()
    vt = torch.from_numpy(np.array(v)).cuda()
    oi = [torch.full((BIG_N,), SENT_I, dtype=torch.int64, device="cuda") for _ in range(2)]
    of = [torch.full((BIG_N,), SENT_F, dtype=torch.float64, device="cuda") for _ in range(3)]
    ws = gpu.alloc_ws(BIG_N)
    assert ws.numel() == gpu.ws_bytes(BIG_N)
    nout = gpu.dev_sort_stats_f64(kt, vt, *oi, *of, ws)
    assert nout == len(ref[0])
    dgot = by_key(tuple(o[:nout].cpu().numpy() for o in oi + of))
    check_exact_columns(dgot, ref)
    assert sr.same_bits(dgot[2], rv).all()
    for o, s in zip(oi + of, (SENT_I, SENT_I, SENT_F, SENT_F, SENT_F)):
        assert (o[nout:] == s).all()


# ---- 6. sizes ----

SIZES = (0, 1, 2, 7, 8, 9, 511, 512, 513, 4095, 4096, 4097)


@pytest.mark.parametrize("kind", ("distinct", "single"))
@pytest.mark.parametrize("n", SIZES)
def test_sizes(ctx, n, kind):
    import torch
    from vega_amd import gpu
    rng = np.random.RandomState(1000 + n)
    if kind == "distinct":
        k = (rng.permutation(n).astype(np.int64) * 7919) - 3
    else:
        k = np.full(n, (1 << 45) + 7, dtype=np.int64)
    v = rng.randint(-(1 << 30), (1 << 30) + 1, size=n).astype(np.float64)   # sums exact
    ref = sr.stats_f64_ref(k, v)

    rdd = ctx.make_rdd(k, v)
    st = rdd.stats_by_key_f64()
    got = st.collect()
    check_dtypes(got)
    assert st.count() == len(ref[0])
    got = by_key(got)
    check_exact_columns(got, ref)
    check_sum_bits(got, ref)
    check_reduce_both(rdd, ref)
    rdd.free(); st.free()

    kt = torch.from_numpy(k).cuda()
    vt = torch.from_numpy(v).cuda()
    m = max(n, 1)
    oi = [torch.full((m,), SENT_I, dtype=torch.int64, device="cuda") for _ in range(2)]
    of = [torch.full((m,), SENT_F, dtype=torch.float64, device="cuda") for _ in range(3)]
    ws = gpu.alloc_ws(n)
    nout = gpu.dev_sort_stats_f64(kt, vt, *oi, *of, ws)
    assert nout == len(ref[0])
    got = by_key(tuple(o[:nout].cpu().numpy() for o in oi + of))
    check_exact_columns(got, ref)
    check_sum_bits(got, ref)
    for o, s in zip(oi + of, (SENT_I, SENT_I, SENT_F, SENT_F, SENT_F)):
        assert (o[nout:] == s).all()


# ---- 7. actions ----

def col_ref(op_is_max, k, v):
    """column-wise reduce: i64 extreme of the keys, f64 extreme of the values"""
    _, mn, mx = sr.minmax_f64_ref(np.zeros(len(v), dtype=np.int64), v)
    return (int(k.max()), mx[0]) if op_is_max else (int(k.min()), mn[0])


def same_row(got, exp):
    return got[0] == exp[0] and bool(sr.extremes_match(np.array([got[1]]), np.array([exp[1]]))[0])


@pytest.mark.parametrize("n", (1, 4097, 100_003))
def test_reduce_and_fold(ctx, n):
    import torch
    from vega_amd import gpu
    rng = np.random.RandomState(n)
    k = rng.randint(-(1 << 50), 1 << 50, size=n, dtype=np.int64)
    v = rng.standard_normal(n) * 10.0 ** rng.randint(-3, 6, size=n)
    v[n // 2] = np.nan                       # a NaN present (the only row when n == 1)
    if n > 2:
        v[0], v[n - 1] = -0.0, 0.0
    rdd = ctx.make_rdd(k, v, nparts=5)
    kt = torch.from_numpy(k).cuda()
    vt = torch.from_numpy(v).cuda()
    for op, is_max in ((gpu.OP_MIN_F64, False), (gpu.OP_MAX_F64, True)):
        exp = col_ref(is_max, k, v)
        assert np.isnan(exp[1]) == (n == 1)
        got = rdd.reduce(op)
        assert isinstance(got[1], float) and same_row(got, exp), (got, exp)
        assert same_row(gpu.dev_reduce_pairs(kt, vt, op), exp)
        # an init that loses, one that wins, and a NaN init (skipped)
        far = 1e300 if not is_max else -1e300
        near = -1e300 if not is_max else 1e300
        kfar = (1 << 60) if not is_max else -(1 << 60)
        assert same_row(rdd.fold(op, kfar, far), exp if n > 1 else (exp[0], far))
        assert same_row(rdd.fold(op, -kfar, near), (-kfar, near))
        assert same_row(rdd.fold(op, kfar, float("nan")), exp)
    rdd.free()


def test_reduce_and_fold_empty(ctx):
    from vega_amd import gpu
    rdd = ctx.make_rdd(np.empty(0, dtype=np.int64), np.empty(0, dtype=np.float64), nparts=4)
    for op in (gpu.OP_MIN_F64, gpu.OP_MAX_F64):
        assert rdd.reduce(op) is None
        assert rdd.fold(op, 12, -3.5) == (12, -3.5)   # init combined P+1 times is init
        got = rdd.fold(op, 0, -0.0)
        assert got[0] == 0 and np.signbit(got[1]) and got[1] == 0
    rdd.free()


def test_ordered_actions_still_refuse_f64(ctx):
    k = np.arange(50, dtype=np.int64)
    rdd = ctx.make_rdd(k, k.astype(np.float64))
    for fn in (rdd.min, rdd.max, lambda: rdd.top(3), lambda: rdd.take_ordered(3)):
        refused(ERR_INVALID, fn)
        still_answers(ctx)
    rdd.free()


# ---- 8. guards and composition ----

def test_guards(ctx):
    import torch
    from vega_amd import gpu
    k = np.arange(100, dtype=np.int64) % 7
    v = np.arange(100, dtype=np.int64)
    plain = ctx.make_rdd(k, v)
    f64 = ctx.make_rdd(k, v.astype(np.float64))

    err = refused(ERR_INVALID, plain.stats_by_key_f64)
    assert "i64" in str(err)
    still_answers(ctx)
    for fn in (lambda: plain.reduce_by_key(gpu.OP_MIN_F64), lambda: plain.reduce_by_key(gpu.OP_MAX_F64),
               lambda: plain.reduce(gpu.OP_MIN_F64), lambda: plain.fold(gpu.OP_MAX_F64, 0, 0.0)):
        refused(ERR_INVALID, fn)
        still_answers(ctx)

    h = ctypes.c_uint64()
    assert gpu.lib().vega_gpu_group_by_key(ctx._c, ctypes.c_uint64(f64.h),
                                           ctypes.c_uint32(4), ctypes.byref(h)) == 0
    grouped = gpu.Rdd(ctx, h.value, np.float64)
    refused(ERR_INVALID, grouped.stats_by_key_f64)
    still_answers(ctx)

    joined = plain.join(plain)
    refused(ERR_INVALID, joined.stats_by_key_f64)
    still_answers(ctx)

    st_i = plain.stats_by_key()
    st_f = f64.stats_by_key_f64()
    for st in (st_i, st_f):
        refused(ERR_INVALID, gpu.Rdd(ctx, st.h, np.float64).stats_by_key_f64)
        still_answers(ctx)
    # each collect entry refuses the other kind, and a plain handle
    for fn in (gpu.StatsRdd(ctx, st_f.h).collect, gpu.StatsF64Rdd(ctx, st_i.h).collect,
               gpu.StatsF64Rdd(ctx, f64.h).collect, lambda: st_f.column(4)):
        refused(ERR_INVALID, fn)
        still_answers(ctx)
    # the actions reject the f64 stats handle like the i64 one
    as_plain = gpu.Rdd(ctx, st_f.h, np.float64)
    for fn in (lambda: as_plain.reduce(gpu.OP_SUM_F64), lambda: as_plain.take(3)):
        refused(ERR_INVALID, fn)
        still_answers(ctx)
    # the old entry still refuses f64
    err = refused(ERR_UNSUPPORTED, f64.stats_by_key)
    assert "f64" in str(err)
    still_answers(ctx)

    # both handles are intact
    ref = sr.stats_f64_ref(k, v.astype(np.float64))
    got = by_key(st_f.collect())
    check_exact_columns(got, ref)
    check_sum_bits(got, ref)
    assert len(st_i.collect()[0]) == 7

    # device entry: mis-aligned output, short workspace
    n = 100
    kt = torch.from_numpy(k).cuda()
    vt = torch.from_numpy(v.astype(np.float64)).cuda()
    oi = [torch.empty(n, dtype=torch.int64, device="cuda") for _ in range(2)]
    of = [torch.empty(n, dtype=torch.float64, device="cuda") for _ in range(3)]
    ws = gpu.alloc_ws(n)
    odd = torch.empty(n + 1, dtype=torch.float64, device="cuda")[1:]
    assert odd.data_ptr() % 16 == 8
    refused(ERR_INVALID, lambda: gpu.dev_sort_stats_f64(kt, vt, oi[0], oi[1], of[0], odd, of[2], ws))
    still_answers(ctx)
    refused(ERR_CAP, lambda: gpu.dev_sort_stats_f64(kt, vt, *oi, *of, ws[:gpu.ws_bytes(n) - 1]))
    still_answers(ctx)
    assert gpu.dev_sort_stats_f64(kt, vt, *oi, *of, ws) == 7
    still_answers(ctx)
    for r in (plain, f64, grouped, joined, st_i, st_f):
        r.free()


def test_columns_compose(ctx):
    from vega_amd import gpu
    rng = np.random.RandomState(9)
    n = 50_000
    k = rng.randint(0, 1 << 10, size=n, dtype=np.int64)
    v = rng.standard_normal(n)
    ref = sr.stats_f64_ref(k, v)
    rdd = ctx.make_rdd(k, v, nparts=16)
    st = rdd.stats_by_key_f64(nparts=16)
    sk, sc, ss, smn, smx = st.collect()

    mn = st.column(gpu.STAT_MIN)
    assert mn.vdtype == np.float64 and mn.count() == len(ref[0])
    ck, cv = mn.collect()
    assert cv.dtype == np.float64 and (ck == sk).all() and sr.same_bits(cv, smn).all()  # same row order
    tk, tv = mn.take(5)
    assert (tk == sk[:5]).all() and sr.same_bits(tv, smn[:5]).all()
    again = mn.reduce_by_key(gpu.OP_MIN_F64)      # keys are distinct: the same rows
    ak, av = by_key(again.collect())
    assert (ak == ref[0]).all() and sr.same_bits(av, ref[3]).all()
    assert same_row(mn.reduce(gpu.OP_MIN_F64), (int(k.min()), v.min()))

    for which, col in ((gpu.STAT_SUM, ss), (gpu.STAT_MAX, smx)):
        c = st.column(which)
        assert c.vdtype == np.float64
        ck, cv = c.collect()
        assert (ck == sk).all() and sr.same_bits(cv, col).all()
        c.free()

    cnt = st.column(gpu.STAT_COUNT)
    assert cnt.vdtype == np.int64
    ck, cv = cnt.collect()
    assert cv.dtype == np.int64 and (ck == sk).all() and (cv == sc).all()
    assert cnt.reduce(gpu.OP_SUM_I64)[1] == n
    for r in (rdd, st, mn, again, cnt):
        r.free()


# ---- 9. inputs unchanged ----

def test_device_entries_leave_inputs_alone():
    import torch
    from vega_amd import gpu
    name = "hash_minus1"
    lay = layout(name)
    n = lay.n
    kt = torch.from_numpy(lay.k.copy()).cuda()
    vt = torch.from_numpy(values(name, "special").copy()).cuda()
    k0, v0 = kt.clone(), vt.clone()
    oi = [torch.empty(n, dtype=torch.int64, device="cuda") for _ in range(2)]
    of = [torch.empty(n, dtype=torch.float64, device="cuda") for _ in range(3)]
    ws = gpu.alloc_ws(n)
    nout, stats = dev_profiled(lambda: gpu.dev_sort_stats_f64(kt, vt, *oi, *of, ws))
    assert_kernels(stats, "hash")
    assert nout == len(lay.run_lens)
    # bit comparison: the values hold NaN
    assert torch.equal(kt, k0) and torch.equal(vt.view(torch.int64), v0.view(torch.int64))
    ref = layout_ref(name, "special")
    check_exact_columns(by_key(tuple(o[:nout].cpu().numpy() for o in oi + of)), ref)
    assert gpu.dev_sort_reduce(kt, vt, gpu.OP_MIN_F64, oi[0], of[0], ws) == nout
    assert torch.equal(kt, k0) and torch.equal(vt.view(torch.int64), v0.view(torch.int64))
    gk, gv = by_key((oi[0][:nout].cpu().numpy(), of[0][:nout].cpu().numpy()))
    assert (gk == ref[0]).all() and sr.extremes_match(gv, ref[3]).all()
