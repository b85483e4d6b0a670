"""sample / random_split / take_sample / dev_sample on the GPU, row-exact
against the numpy restatement in sample_ref. The Poisson cases feed sample_ref
the table that vega_sample_poisson_table returns, so the kernel is checked
exactly here and the table separately (test_sample_abi.py)."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest

import oracle_ctypes as oc
import sample_ref as sr
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vega_amd import datagen

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SIZES = [0, 1, 4095, 4096, 4097, 3 * 4096 + 5, 300_000]
FRACTIONS = [0.0, 1e-4, 0.5, 0.999, 1.0]
LAMBDAS = [1e-6, 0.1, 1.0, 3.5, 16.0]
NMAX = 300_000


@pytest.fixture(scope="module")
def ctx():
    from vega_amd import gpu
    with gpu.VegaContext() as c:
        yield c


@pytest.fixture(scope="module")
def rows():
    """one shared host input; the cases use its prefixes (never modified)"""
    k, v = datagen.uniform_pairs(0x5A17, NMAX, key_bits=40)
    k.setflags(write=False)
    v.setflags(write=False)
    return k, v


def same(got, want):
    gk, gv = got
    wk, wv = want
    assert len(gk) == len(wk) and len(gv) == len(wv)
    assert np.array_equal(gk, wk)
    assert np.array_equal(np.asarray(gv).view(np.int64), np.asarray(wv).view(np.int64))


def collect_free(rdd):
    out = rdd.collect()
    rdd.free()
    return out


# ---------------- Bernoulli ----------------

@pytest.mark.parametrize("n", SIZES)
def test_bernoulli_exact(ctx, rows, n):
    k, v = rows[0][:n], rows[1][:n]
    rdd = ctx.make_rdd(k, v, nparts=7)
    for i, f in enumerate(FRACTIONS):
        seed = 1000 + i
        s = rdd.sample(False, f, seed)
        assert s.vdtype == np.int64
        same(collect_free(s), sr.sample_ref(k, v, False, f, seed))
    same(rdd.collect(), (k, v))  # the source is unchanged
    rdd.free()


def test_bernoulli_slop_and_guards(ctx, rows):
    from vega_amd import gpu
    k, v = rows[0][:5000], rows[1][:5000]
    rdd = ctx.make_rdd(k, v)
    same(collect_free(rdd.sample(False, 1.0 + 5e-7, 3)), (k, v))
    assert collect_free(rdd.sample(False, -5e-7, 3))[0].size == 0
    for bad in (1.5, -0.1, float("nan")):
        with pytest.raises(gpu.VegaGpuError, match="rc=-1 "):
            rdd.sample(False, bad, 3)
    for bad in (-0.1, float("nan")):
        with pytest.raises(gpu.VegaGpuError, match="rc=-1 "):
            rdd.sample(True, bad, 3)
    # seed=None draws a seed: two calls almost surely differ, both are subsets
    a = collect_free(rdd.sample(False, 0.5))
    b = collect_free(rdd.sample(False, 0.5))
    assert not np.array_equal(a[0], b[0])
    rdd.free()


def test_f64_values_keep_bits_and_type(ctx):
    from vega_amd import gpu
    n = 3 * 4096 + 5
    k, v = datagen.uniform_pairs_f64(77, n, key_bits=20)
    v = v.copy()
    v[5] = -0.0
    v[6] = np.float64("nan")
    v[7] = np.float64("inf")
    rdd = ctx.make_rdd(k, v, nparts=3)
    s = rdd.sample(False, 0.5, 42)
    assert s.vdtype == np.float64
    # an f64 op accepts the result and an i64 op refuses it: the engine, not
    # only the Python wrapper, kept the value type
    s.reduce_by_key(gpu.OP_SUM_F64).free()
    with pytest.raises(gpu.VegaGpuError):
        s.reduce_by_key(gpu.OP_SUM_I64)
    same(collect_free(s), sr.sample_ref(k, v, False, 0.5, 42))
    p = rdd.sample(True, 1.0, 42)
    assert p.vdtype == np.float64
    same(collect_free(p), sr.sample_ref(k, v, True, 1.0, 42, table=gpu.sample_poisson_table(1.0)))
    parts = rdd.random_split([1, 1], 42)
    assert all(q.vdtype == np.float64 for q in parts)
    for q, want in zip(parts, sr.random_split_ref(k, v, [1, 1], 42)):
        same(collect_free(q), want)
    rdd.free()


def test_bernoulli_two_level_scan(ctx):
    """4097 tiles: more than one k_scan_tile block scans, so the tile bases
    come from the two-level scan path"""
    n = 4096 * 4096 + 17
    seed = 0xC0FFEE
    rdd = ctx.gen_rdd_uniform(n, seed, key_bits=63, nparts=16)
    s = rdd.sample(False, 0.01, 2025)
    got = collect_free(s)
    rdd.free()
    hk, hv = datagen.uniform_pairs(seed, n, key_bits=63)
    same(got, sr.sample_ref(hk, hv, False, 0.01, 2025))


# ---------------- Poisson ----------------

@pytest.mark.parametrize("n", [1, 4097, 300_000])
def test_poisson_exact(ctx, rows, n):
    from vega_amd import gpu
    k, v = rows[0][:n], rows[1][:n]
    rdd = ctx.make_rdd(k, v, nparts=5)
    for i, lam in enumerate(LAMBDAS):
        # at lam = 1 the mean output equals n, so "longer than the input" is a
        # property of the seed there: 2004 gives 4176 and 300353 rows
        # (sample_ref on the CPU); above 1 any seed does
        seed = 2004 if lam == 1.0 else 2000 + i
        table = gpu.sample_poisson_table(lam)
        want = sr.sample_ref(k, v, True, lam, seed, table=table)
        got = collect_free(rdd.sample(True, lam, seed))
        same(got, want)  # order exact, copies adjacent
        if lam >= 1.0 and n >= 4097:
            assert len(got[0]) > n  # the expanding narrow op
    assert collect_free(rdd.sample(True, 0.0, 1))[0].size == 0
    same(rdd.collect(), (k, v))
    rdd.free()


def test_poisson_unsupported_mean(ctx, rows):
    from vega_amd import gpu
    rdd = ctx.make_rdd(rows[0][:100], rows[1][:100])
    with pytest.raises(gpu.VegaGpuError, match="rc=-4 .*16") as ei:
        rdd.sample(True, 16.5, 1)
    assert ei.value.rc == -4
    rdd.free()


# ---------------- results compose ----------------

def test_sample_feeds_reduce_by_key(ctx):
    from vega_amd import gpu
    n = 200_000
    k, v = datagen.uniform_pairs(99, n, key_bits=12)
    rdd = ctx.make_rdd(k, v, nparts=16)
    for repl, f in ((False, 0.3), (True, 1.5)):
        s = rdd.sample(repl, f, 8)
        red = s.reduce_by_key(gpu.OP_SUM_I64, nparts=16)
        gk, gv = collect_free(red)
        s.free()
        table = gpu.sample_poisson_table(f) if repl else None
        hk, hv = sr.sample_ref(k, v, repl, f, 8, table=table)
        ok, ov = oc.reduce_by_key_i64(hk, hv, 16, 16)
        assert sorted(zip(gk.tolist(), gv.tolist())) == sorted(zip(ok.tolist(), ov.tolist()))
        same(rdd.collect(), (k, v))
    rdd.free()


# ---------------- random_split ----------------

def split_weights(w):
    if w == 256:
        return [1.0 + (j % 5) for j in range(256)]
    return {1: [2.0], 2: [1.0, 3.0], 3: [1.0, 2.0, 3.0]}[w]


@pytest.mark.parametrize("n", [600, 4097, 300_000])
@pytest.mark.parametrize("w", [1, 2, 3, 256])
def test_random_split_exact(ctx, rows, n, w):
    k, v = rows[0][:n], rows[1][:n]
    weights = split_weights(w)
    rdd = ctx.make_rdd(k, v, nparts=3)
    parts = rdd.random_split(weights, 555)
    want = sr.random_split_ref(k, v, weights, 555)
    assert len(parts) == w == len(want)
    # each handle is freed on its own, in an order of our choosing
    for j in list(range(1, w, 2)) + list(range(0, w, 2)):
        assert parts[j].count() == len(want[j][0])
        same(collect_free(parts[j]), want[j])
    same(rdd.collect(), (k, v))
    rdd.free()


def test_random_split_zero_weight_and_split0(ctx, rows):
    k, v = rows[0][:20_000], rows[1][:20_000]
    rdd = ctx.make_rdd(k, v)
    parts = rdd.random_split([0.2, 0.0, 0.8], 31)
    want = sr.random_split_ref(k, v, [0.2, 0.0, 0.8], 31)
    assert parts[1].count() == 0
    got = [collect_free(p) for p in parts]
    for g, wnt in zip(got, want):
        same(g, wnt)
    assert sum(len(g[0]) for g in got) == len(k)
    # split 0 is the Bernoulli sample of its share
    same(got[0], collect_free(rdd.sample(False, 0.2 / (0.2 + 0.0 + 0.8), 31)))
    rdd.free()


def test_random_split_invalid_weights(ctx, rows):
    from vega_amd import gpu
    rdd = ctx.make_rdd(rows[0][:100], rows[1][:100])
    before = len(_handles(ctx))
    for bad in ([], [1.0] * 257, [1.0, -0.5], [0.0, 0.0], [1.0, float("nan")]):
        with pytest.raises(gpu.VegaGpuError, match="rc=-1 "):
            rdd.random_split(bad, 1)
    assert len(_handles(ctx)) == before  # nothing was left allocated
    rdd.free()


def _handles(ctx):
    """live handles, probed through vega_gpu_count on a window of ids"""
    from vega_amd import gpu
    n = ctypes.c_uint64()
    return [h for h in range(1, 1 << 14)
            if gpu.lib().vega_gpu_count(ctx._c, ctypes.c_uint64(h), ctypes.byref(n)) == 0]


# ---------------- take_sample ----------------

def test_take_sample_golden(ctx):
    with open(os.path.join(HERE, "golden", "sample.json")) as f:
        golden = json.load(f)
    assert len(golden["take_sample"]) == 3
    for g in golden["take_sample"]:
        lo, hi = g["range_inclusive"]
        k = np.arange(lo, hi + 1, dtype=np.int64)
        z = np.zeros(len(k), np.int64)
        rdd = ctx.make_rdd(k, z, nparts=g["nparts"])
        tk, tv = rdd.take_sample(g["with_replacement"], g["num"], g["seed"])
        assert len(tk) == len(tv) == g["expected_len"], g["source"]
        assert set(tk.tolist()) <= set(k.tolist()) and not tv.any()
        if g["property"] == "permutation":
            assert sorted(tk.tolist()) == k.tolist()
        if g["property"] == "distinct_subset":
            assert len(set(tk.tolist())) == len(tk)
        same((tk, tv), sr.take_sample_ref(k, z, g["with_replacement"], g["num"], g["seed"]))
        rdd.free()
    (g,) = golden["random_split"]
    lo, hi = g["range_inclusive"]
    k = np.arange(lo, hi + 1, dtype=np.int64)
    rdd = ctx.make_rdd(k, np.zeros(len(k), np.int64), nparts=g["nparts"])
    for seed in g["seeds"]:
        got = [collect_free(p)[0] for p in rdd.random_split(g["weights"], seed)]
        assert len(got) == g["expected_splits"]
        assert sum(len(a) for a in got) == g["expected_total"]
        for a, want in zip(got, g["expected_sizes"]):
            assert abs(len(a) - want) < g["size_tolerance_exclusive"]
        assert len(set(np.concatenate(got).tolist())) == g["expected_total"]  # disjoint
    rdd.free()


def test_take_sample_exact(ctx):
    k, v = datagen.uniform_pairs(4242, 1_000_000, key_bits=63)
    rdd = ctx.make_rdd(k, v, nparts=8)
    got = rdd.take_sample(False, 1000, 17)
    same(got, sr.take_sample_ref(k, v, False, 1000, 17))  # order included
    assert len(got[0]) == 1000
    same(rdd.collect(), (k, v))
    rdd.free()
    k, v = k[:20_000], v[:20_000]
    rdd = ctx.make_rdd(k, v, nparts=8)
    got = rdd.take_sample(True, 5000, 18)
    same(got, sr.take_sample_ref(k, v, True, 5000, 18))
    assert len(got[0]) == 5000
    # num >= n without replacement: every row, shuffled
    for num in (20_000, 20_001, 1 << 40):
        got = rdd.take_sample(False, num, 19)
        same(got, sr.take_sample_ref(k, v, False, num, 19))
        assert len(got[0]) == 20_000
    assert rdd.take_sample(False, 0, 1)[0].size == 0
    assert rdd.take_sample(True, 0, 1)[0].size == 0
    rdd.free()
    empty = ctx.make_rdd(k[:0], v[:0])
    assert empty.take_sample(False, 5, 1)[0].size == 0
    assert empty.take_sample(True, 5, 1)[0].size == 0
    empty.free()


# ---------------- dev_sample ----------------

def test_dev_sample_shards_and_cap():
    import torch
    from vega_amd import gpu
    n = 100_000 + 6
    half = n // 2
    k, v = datagen.uniform_pairs(808, n, key_bits=30)
    dk = torch.from_numpy(k).cuda()
    dv = torch.from_numpy(v).cuda()
    for repl, f in ((False, 0.37), (True, 2.25)):
        table = gpu.sample_poisson_table(f) if repl else None
        want = sr.sample_ref(k, v, repl, f, 64, table=table)
        wk, wv, need = gpu.dev_sample(dk, dv, repl, f, 64)
        assert need == len(want[0])
        same((wk.cpu().numpy(), wv.cpu().numpy()), want)
        # two shards with their global offsets concatenate to the whole sample
        ak, av, na = gpu.dev_sample(dk[:half], dv[:half], repl, f, 64, start=0)
        bk, bv, nb = gpu.dev_sample(dk[half:], dv[half:], repl, f, 64, start=half)
        assert na + nb == need
        same((torch.cat([ak, bk]).cpu().numpy(), torch.cat([av, bv]).cpu().numpy()), want)
        # cap too small: VEGA_ERR_CAP, the needed count, and nothing written
        cap = need - 1
        ok = torch.full((need + 64,), -7, dtype=torch.int64, device="cuda")
        ov = torch.full((need + 64,), -7, dtype=torch.int64, device="cuda")
        with pytest.raises(gpu.VegaGpuError) as ei:
            gpu.dev_sample(dk, dv, repl, f, 64, out_k=ok[:cap], out_v=ov[:cap])
        assert ei.value.rc == -5 and ei.value.needed == need
        torch.cuda.synchronize()
        assert bool((ok == -7).all()) and bool((ov == -7).all())
        # exactly enough: rows beyond the sample keep their sentinel fill
        gk, gv, _ = gpu.dev_sample(dk, dv, repl, f, 64, out_k=ok[:need], out_v=ov[:need])
        same((gk.cpu().numpy(), gv.cpu().numpy()), want)
        assert bool((ok[need:] == -7).all()) and bool((ov[need:] == -7).all())


# ---------------- guards ----------------

def test_guards_on_other_handle_kinds(ctx, rows):
    from vega_amd import gpu
    k, v = rows[0][:1000] % 16, rows[1][:1000]
    rdd = ctx.make_rdd(k, v)
    out = ctypes.c_uint64()
    assert gpu.lib().vega_gpu_group_by_key(ctx._c, ctypes.c_uint64(rdd.h), ctypes.c_uint32(4),
                                           ctypes.byref(out)) == 0
    grouped = gpu.Rdd(ctx, out.value, np.int64)  # a grouped handle kept alive
    few = rdd.filter(gpu.PRED_KEY_IN_RANGE, 0, 2)
    join = rdd.join(few)
    stats = rdd.stats_by_key()
    as_rdd = gpu.Rdd(ctx, stats.h, np.int64)
    for h in (grouped, join, as_rdd):
        for call in (lambda: h.sample(False, 0.5, 1), lambda: h.sample(True, 0.5, 1),
                     lambda: h.random_split([1, 1], 1), lambda: h.take_sample(False, 3, 1)):
            with pytest.raises(gpu.VegaGpuError, match="rc=-1 "):
                call()
    with pytest.raises(gpu.VegaGpuError, match="rc=-1 "):
        rdd.sample(False, 1.5, 1)
    rdd.free(); grouped.free(); few.free(); join.free(); stats.free()
