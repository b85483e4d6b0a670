"""GPU parity tests: the HIP path (through the C ABI) vs the CPU oracle.

All tests marked gpu; run on the MI355X box with `pytest tests -m gpu`.
Comparison discipline follows the reference's own tests: collected output is
sorted, then compared exactly (test_pair_rdd.rs:30-36). Integer paths are
bit-exact; f64 sums use the 1e-6 relative tolerance BASELINE.json names.
"""
import glob
import json
import os

import numpy as np
import pytest

import oracle_ctypes as oc
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vega_amd import datagen

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def ctx():
    from vega_amd import gpu
    with gpu.VegaContext() as c:
        yield c


def sorted_pairs(k, v):
    return sorted(zip(np.asarray(k).tolist(), np.asarray(v).tolist()))


# ---------------- generation parity ----------------

def test_device_gen_matches_host(ctx):
    n = 100_003
    rdd = ctx.gen_rdd_uniform(n, seed=42, key_bits=63)
    gk, gv = rdd.collect()
    hk, hv = datagen.uniform_pairs(42, n, key_bits=63)
    assert (gk == hk).all() and (gv == hv).all()
    rdd.free()


# ---------------- reduce_by_key ----------------

@pytest.mark.parametrize("n,bits,seed", [
    (100_000, 20, 1),     # C0-like
    (1_000_000, 63, 2),   # C1 shape (mostly distinct)
    (1_000_000, 8, 3),    # heavy combine (256 keys)
    (4097, 63, 4),        # tile edge +1
    (4096, 63, 5),        # exact tile
    (4095, 10, 6),        # tile edge -1
    (1, 63, 7),
    (2, 1, 8),
    (100_000, 0, 9),      # all keys == 0 (zero active radix passes)
    (65536, 2, 10),       # 4 distinct keys
    (500_000, 64, 11),    # full i64 keys incl. negatives
])
def test_reduce_by_key_i64(ctx, n, bits, seed):
    from vega_amd import gpu
    rdd = ctx.gen_rdd_uniform(n, seed=seed, key_bits=bits)
    red = rdd.reduce_by_key(gpu.OP_SUM_I64)
    gk, gv = red.collect()
    hk, hv = datagen.uniform_pairs(seed, n, key_bits=bits)
    ok, ov = oc.reduce_by_key_i64(hk, hv, 256, 256)
    assert sorted_pairs(gk, gv) == sorted_pairs(ok, ov)
    rdd.free(); red.free()


def test_reduce_wrapping_overflow_gpu(ctx):
    from vega_amd import gpu
    k = np.zeros(4, dtype=np.int64)
    v = np.array([2**62] * 4, dtype=np.int64)
    rdd = ctx.make_rdd(k, v)
    red = rdd.reduce_by_key(gpu.OP_SUM_I64)
    gk, gv = red.collect()
    assert gk.tolist() == [0] and gv.tolist() == [0]
    rdd.free(); red.free()


def test_reduce_by_key_empty(ctx):
    from vega_amd import gpu
    rdd = ctx.make_rdd(np.empty(0, np.int64), np.empty(0, np.int64))
    red = rdd.reduce_by_key(gpu.OP_SUM_I64)
    gk, gv = red.collect()
    assert len(gk) == 0 and len(gv) == 0
    rdd.free(); red.free()


def test_dev_gen_f64_matches_host(ctx):
    import torch
    from vega_amd import gpu
    n = 50_000
    k = torch.empty(n, dtype=torch.int64, device="cuda")
    v = torch.empty(n, dtype=torch.float64, device="cuda")
    gpu.dev_gen_uniform_f64(k, v, seed=19, key_bits=20)
    hk, hv = datagen.uniform_pairs_f64(19, n, key_bits=20)
    assert (k.cpu().numpy() == hk).all()
    assert (v.cpu().numpy() == hv).all()  # exact dyadic conversion: bit-equal


def test_reduce_by_key_f64(ctx):
    from vega_amd import gpu
    n = 500_000
    hk, hv = datagen.uniform_pairs_f64(11, n, key_bits=10)
    rdd = ctx.make_rdd(hk, hv)
    red = rdd.reduce_by_key(gpu.OP_SUM_F64)
    gk, gv = red.collect()
    ok, ov = oc.reduce_by_key_f64(hk, hv, 256, 256)
    assert sorted(gk.tolist()) == sorted(ok.tolist())
    ref = dict(zip(ok.tolist(), ov.tolist()))
    for k, v in zip(gk.tolist(), gv.tolist()):
        assert abs(v - ref[k]) <= 1e-6 * max(1.0, abs(ref[k]))
    rdd.free(); red.free()


def test_min_max_ops(ctx):
    from vega_amd import gpu
    n = 300_000
    hk, hv = datagen.uniform_pairs(13, n, key_bits=8)
    rdd = ctx.make_rdd(hk, hv)
    for op, npop in [(gpu.OP_MIN_I64, np.minimum), (gpu.OP_MAX_I64, np.maximum)]:
        red = rdd.reduce_by_key(op)
        gk, gv = red.collect()
        got = dict(zip(gk.tolist(), gv.tolist()))
        for key in np.unique(hk):
            sel = hv[hk == key]
            exp = sel.min() if op == gpu.OP_MIN_I64 else sel.max()
            assert got[int(key)] == exp
        red.free()
    rdd.free()


# ---------------- group_count (C2 semantics) ----------------

def test_reduce_hash_collisions(ctx):
    """Keys whose splitmix64 hashes collide in the low 32 bits land in one
    hash-sort run with >1 distinct key — exercises k_group_cleanup."""
    from vega_amd import gpu, shuffle
    cand = np.arange(1_500_000, dtype=np.int64)
    h32 = (shuffle.hash_u64_np(cand) & np.uint64(0xFFFFFFFF)).astype(np.uint64)
    order = np.argsort(h32, kind="stable")
    hs = h32[order]
    dup = hs[1:] == hs[:-1]
    pairs = order[:-1][dup], order[1:][dup]
    coll = np.unique(np.concatenate([cand[pairs[0]], cand[pairs[1]]]))
    assert len(coll) >= 20, "expected some 32-bit hash collisions in 1.5M keys"
    # each colliding key appears 3x with distinct values + filler rows
    keys = np.concatenate([np.repeat(coll, 3),
                           np.arange(10_000, 20_000, dtype=np.int64)])
    vals = np.arange(len(keys), dtype=np.int64)
    rng = np.random.RandomState(7)
    perm = rng.permutation(len(keys))
    keys, vals = keys[perm], vals[perm]
    rdd = ctx.make_rdd(keys, vals)
    red = rdd.reduce_by_key(gpu.OP_SUM_I64)
    gk, gv = red.collect()
    ok, ov = oc.reduce_by_key_i64(keys, vals, 8, 8)
    assert sorted_pairs(gk, gv) == sorted_pairs(ok, ov)
    rdd.free(); red.free()


def test_group_count_zipf(ctx):
    n = 1_000_000
    hk, hv = datagen.zipf_pairs(21, n, s=1.1, keyspace=100_000)
    rdd = ctx.make_rdd(hk, hv)
    red = rdd.group_count()
    gk, gv = red.collect()
    ok, ov = oc.group_count_i64(hk, hv, 256, 256)
    assert sorted_pairs(gk, gv) == sorted_pairs(ok, ov)
    rdd.free(); red.free()


def test_group_count_on_f64_values(ctx):
    # group_by_key->count must work for f64-valued RDDs (values ignored)
    hk, hv = datagen.uniform_pairs_f64(23, 200_000, key_bits=8)
    rdd = ctx.make_rdd(hk, hv)
    red = rdd.group_count()
    gk, gv = red.collect()
    ok, ov = oc.group_count_i64(hk, np.zeros_like(hk), 8, 8)
    assert sorted_pairs(gk, gv) == sorted_pairs(ok, ov)
    rdd.free(); red.free()


def test_count_by_value_golden(ctx):
    # test_pair_rdd.rs:85-109 via the dedicated API entry
    vals = np.array([1, 2, 1, 3, 2, 3, 3, 2, 3], dtype=np.int64)
    keys = np.zeros(len(vals), dtype=np.int64)
    for parts in (4, 2):
        rdd = ctx.make_rdd(keys, vals, nparts=parts)
        cbv = rdd.count_by_value(nparts=parts)
        gk, gv = cbv.collect()
        assert sorted_pairs(gk, gv) == [(1, 2), (2, 3), (3, 4)]
        rdd.free(); cbv.free()


# ---------------- sort_by_key ----------------

@pytest.mark.parametrize("n,bits,seed", [
    (1_000_000, 64, 31),  # full i64 incl. negatives -> signed order
    (100_000, 12, 32),
    (4097, 64, 33),
    (3, 64, 34),
])
def test_sort_by_key(ctx, n, bits, seed):
    hk, hv = datagen.uniform_pairs(seed, n, key_bits=bits)
    rdd = ctx.make_rdd(hk, hv)
    srt = rdd.sort_by_key()
    gk, gv = srt.collect()
    ok, ov = oc.sort_by_key_i64(hk, hv)
    assert (gk == ok).all(), "keys not in signed ascending stable order"
    assert (gv == ov).all(), "stability violated (values out of row order)"
    rdd.free(); srt.free()


def test_group_by_key_full_values(ctx):
    k, v = datagen.uniform_pairs(71, 50_000, key_bits=8)
    rdd = ctx.make_rdd(k, v)
    gk, off, gv = rdd.group_by_key()
    import pyref
    ref = pyref.group_by_key(k, v)
    got = {int(gk[i]): gv[off[i]:off[i + 1]].tolist() for i in range(len(gk))}
    assert got == ref  # per-group value ORDER = row order (stable sort)
    rdd.free()


# ---------------- golden vectors through the GPU ----------------

def test_golden_through_gpu(ctx):
    from vega_amd import gpu
    for path in sorted(glob.glob(os.path.join(HERE, "golden", "*.json"))):
        g = json.load(open(path))
        if g["op"] == "reduce_by_key":
            rdd = ctx.make_rdd(g["keys"], g["vals"], nparts=g["nparts_in"])
            red = rdd.reduce_by_key(gpu.OP_SUM_I64, nparts=g["nparts_out"])
            gk, gv = red.collect()
            assert sorted_pairs(gk, gv) == [tuple(x) for x in g["expected_sorted"]], path
            rdd.free(); red.free()
        elif g["op"] == "group_by_key":
            rdd = ctx.make_rdd(g["keys"], g["vals"], nparts=g["nparts_in"])
            red = rdd.group_count(nparts=g["nparts_out"])
            gk, gv = red.collect()
            exp = sorted((int(k), len(v)) for k, v in g["expected_groups"].items())
            assert sorted_pairs(gk, gv) == exp, path
            # full groups: sort_by_key of the pairs reproduces each group's
            # value multiset; value order within groups = row order (stable)
            srt = rdd.sort_by_key()
            sk, sv = srt.collect()
            got = {}
            for k, v in zip(sk.tolist(), sv.tolist()):
                got.setdefault(str(k), []).append(v)
            assert got == g["expected_groups"], path
            rdd.free(); red.free(); srt.free()
        elif g["op"] == "distinct":
            keys = np.asarray(g["keys"], dtype=np.int64)
            rdd = ctx.make_rdd(keys, np.zeros(len(keys), np.int64), nparts=g["nparts_in"])
            red = rdd.group_count(nparts=g["nparts_out"])
            gk, _ = red.collect()
            assert sorted(gk.tolist()) == g["expected_sorted"], path
            rdd.free(); red.free()


# ---------------- device-pointer API (torch plumbing) ----------------

def test_dev_partition_torch(ctx):
    import torch
    from vega_amd import gpu
    n = 1_000_000
    k = torch.empty(n, dtype=torch.int64, device="cuda")
    v = torch.empty(n, dtype=torch.int64, device="cuda")
    gpu.dev_gen_uniform(k, v, seed=77, key_bits=63)
    ok = torch.empty_like(k)
    ov = torch.empty_like(v)
    ws = gpu.alloc_ws(n)
    counts = gpu.dev_partition(k, v, 8, ok, ov, ws)
    assert counts.sum() == n
    # bucket property: every row in bucket p hashes to p
    hk = ok.cpu().numpy()
    off = 0
    for p, c in enumerate(counts.tolist()):
        seg = hk[off:off + int(c)]
        if len(seg):
            hashes = np.array([oc.partition_of(int(x), 8) for x in seg[:100]])
            assert (hashes == p).all()
        off += int(c)
    # multiset preserved
    assert gpu.dev_checksum(ok, ov, ws) == gpu.dev_checksum(k, v, ws)
    torch.cuda.synchronize()


def test_dev_sort_reduce_torch(ctx):
    import torch
    from vega_amd import gpu
    n = 500_000
    k = torch.empty(n, dtype=torch.int64, device="cuda")
    v = torch.empty(n, dtype=torch.int64, device="cuda")
    gpu.dev_gen_uniform(k, v, seed=88, key_bits=16)
    out_k = torch.empty_like(k)
    out_v = torch.empty_like(v)
    ws = gpu.alloc_ws(n)
    nout = gpu.dev_sort_reduce(k, v, gpu.OP_SUM_I64, out_k, out_v, ws)
    torch.cuda.synchronize()
    hk, hv = datagen.uniform_pairs(88, n, key_bits=16)
    ok, ov = oc.reduce_by_key_i64(hk, hv, 8, 8)
    assert nout == len(ok)
    got = sorted_pairs(out_k[:nout].cpu().numpy(), out_v[:nout].cpu().numpy())
    assert got == sorted_pairs(ok, ov)


def test_dev_partition_range_torch(ctx):
    import torch
    from vega_amd import gpu, shuffle
    n = 500_000
    k = torch.empty(n, dtype=torch.int64, device="cuda")
    v = torch.empty(n, dtype=torch.int64, device="cuda")
    gpu.dev_gen_uniform(k, v, seed=171, key_bits=64)
    spl_np = np.sort(np.random.RandomState(0).randint(-2**62, 2**62, size=7))
    spl = torch.from_numpy(spl_np).cuda()
    ok = torch.empty_like(k)
    ov = torch.empty_like(v)
    ws = gpu.alloc_ws(n)
    counts = gpu.dev_partition_range(k, v, spl, ok, ov, ws)
    assert counts.sum() == n
    hk = ok.cpu().numpy()
    # matches the CPU reference partition exactly (stable + same buckets)
    rk, rv, rcounts = shuffle.partition_range_cpu(k.cpu().numpy(), v.cpu().numpy(), spl_np)
    assert (counts.astype(np.int64) == rcounts).all()
    assert (hk == rk).all()
    assert (ov.cpu().numpy() == rv).all()


# ---- partition edges: small, ragged n; exact keys, values (= row index, so
# ---- within-bucket order is pinned) and counts against the CPU reference

PART_N = 12_289  # three tiles and one row


def _partition_input():
    rng = np.random.RandomState(301)
    pool = rng.randint(-2**63, 2**63 - 1, size=2000, dtype=np.int64)
    k = pool[rng.randint(0, len(pool), size=PART_N)]  # ~6 rows per key
    return k, np.arange(PART_N, dtype=np.int64)


@pytest.mark.parametrize("nparts", [1, 2, 3, 255, 256])
def test_dev_partition_nparts_edges(ctx, nparts):
    import torch
    from vega_amd import gpu, shuffle
    hk, hv = _partition_input()
    k = torch.from_numpy(hk).cuda()
    v = torch.from_numpy(hv).cuda()
    ok = torch.empty_like(k)
    ov = torch.empty_like(v)
    counts = gpu.dev_partition(k, v, nparts, ok, ov, gpu.alloc_ws(PART_N))
    rk, rv, rcounts = shuffle.partition_cpu(hk, hv, nparts)
    assert (counts.astype(np.int64) == rcounts).all()
    assert (ok.cpu().numpy() == rk).all()
    assert (ov.cpu().numpy() == rv).all(), "rows of a bucket out of row order"


@pytest.mark.parametrize("nparts", [0, 257])
def test_dev_partition_rejects_bad_nparts(ctx, nparts):
    """an error, and neither the device outputs nor the counts are touched"""
    import ctypes
    import torch
    from vega_amd import gpu
    hk, hv = _partition_input()
    k = torch.from_numpy(hk).cuda()
    v = torch.from_numpy(hv).cuda()
    ok = torch.full_like(k, -77)
    ov = torch.full_like(v, -78)
    counts = np.full(512, 0xABCD, dtype=np.uint64)
    ws = gpu.alloc_ws(PART_N)
    rc = gpu.lib().vega_dev_partition_i64(
        gpu._stream(), gpu._t(k), gpu._t(v), ctypes.c_uint64(PART_N),
        ctypes.c_uint32(nparts), gpu._t(ok), gpu._t(ov), gpu._pp(counts),
        gpu._t(ws), ctypes.c_size_t(ws.numel()))
    torch.cuda.synchronize()
    assert rc != 0
    assert (counts == 0xABCD).all()
    assert (ok == -77).all().item() and (ov == -78).all().item()
    with pytest.raises(gpu.VegaGpuError):
        gpu.dev_partition(k, v, nparts, ok, ov, ws)


I64_LO, I64_HI = -2**63, 2**63 - 1

RANGE_CASES = {
    # duplicate splitters (empty buckets between them), one of them (10)
    # equal to a third of all keys, and the extreme keys on both sides
    "duplicate_splitters": (
        [-5, 10, 10, 10, 1000, 1000, 2**40],
        [I64_LO, -6, -5, -4, 9, 10, 10, 10, 10, 10, 10, 11, 999, 1000, 1001,
         2**40 - 1, 2**40, I64_HI]),
    "extreme_splitters": ([I64_LO, 0, I64_HI], [I64_LO, I64_LO + 1, -1, 0, 1, I64_HI - 1, I64_HI]),
    "all_in_first_bucket": ([1000, 2000, 3000], list(range(-100, 100)) + [I64_LO]),
    "all_in_last_bucket": ([-3000, -2000, -1000], list(range(-100, 100)) + [-1000, I64_HI]),
}


@pytest.mark.parametrize("case", sorted(RANGE_CASES))
def test_dev_partition_range_edges(ctx, case):
    import torch
    from vega_amd import gpu, shuffle
    spl_list, key_pool = RANGE_CASES[case]
    spl_np = np.asarray(spl_list, dtype=np.int64)
    pool = np.asarray(key_pool, dtype=np.int64)
    hk = pool[np.random.RandomState(302).randint(0, len(pool), size=PART_N)]
    hv = np.arange(PART_N, dtype=np.int64)
    k = torch.from_numpy(hk).cuda()
    v = torch.from_numpy(hv).cuda()
    ok = torch.empty_like(k)
    ov = torch.empty_like(v)
    counts = gpu.dev_partition_range(k, v, torch.from_numpy(spl_np).cuda(), ok, ov,
                                     gpu.alloc_ws(PART_N))
    rk, rv, rcounts = shuffle.partition_range_cpu(hk, hv, spl_np)
    if case == "all_in_first_bucket":
        assert rcounts[0] == PART_N
    if case == "all_in_last_bucket":
        assert rcounts[-1] == PART_N
    assert (counts.astype(np.int64) == rcounts).all()
    assert (ok.cpu().numpy() == rk).all()
    assert (ov.cpu().numpy() == rv).all(), "rows of a bucket out of row order"


def test_checksum_matches_oracle(ctx):
    import torch
    from vega_amd import gpu
    n = 123_457
    k = torch.empty(n, dtype=torch.int64, device="cuda")
    v = torch.empty(n, dtype=torch.int64, device="cuda")
    gpu.dev_gen_uniform(k, v, seed=99, key_bits=63)
    ws = gpu.alloc_ws(n)
    dsum = gpu.dev_checksum(k, v, ws)
    hk, hv = datagen.uniform_pairs(99, n, key_bits=63)
    assert dsum == oc.checksum_pairs(hk, hv) % (1 << 64)
