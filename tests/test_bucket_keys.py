"""tests/bucket_keys.py says what it builds: the hash inverse is exact and the
crafted layouts have the buckets, tile-edge positions, planted runs and
distinct key samples that test_gpu_bucket_finish.py relies on. No GPU."""
from collections import Counter

import numpy as np
import pytest

import bucket_keys as bk
from vega_amd.shuffle import hash_u64_np

FT = bk.FT


def hash_order_lens(lay):
    """bucket lengths of the layout's keys, in ascending bucket order"""
    ids, lens = np.unique(bk.bucket_of(lay.k), return_counts=True)
    return lens.tolist()


def h32_runs(lay):
    """equal-h32 runs of length >= 2 in (h32, input position) order: list of
    key lists"""
    h = (bk.hash_u64(lay.k) & np.uint64(0xFFFFFFFF)).astype(np.int64)
    o = np.argsort(h, kind="stable")
    hs, ks = h[o], lay.k[o]
    cut = np.flatnonzero(np.concatenate([[True], hs[1:] != hs[:-1], [True]]))
    return [ks[a:b].tolist() for a, b in zip(cut[:-1], cut[1:]) if b - a >= 2]


def shape_of(keys):
    """['x','y','x'] -> 'ABA' up to renaming: letters in order of first use"""
    names = {}
    return "".join(names.setdefault(k, chr(ord("A") + len(names))) for k in keys)


def canon(shape):
    return shape_of(list(shape))


def test_hash_matches_the_library_mirror():
    k = np.random.RandomState(1).randint(-2**63, 2**63 - 1, size=10_000, dtype=np.int64)
    assert (bk.hash_u64(k) == hash_u64_np(k)).all()


def test_inverse_is_exact():
    rng = np.random.RandomState(2)
    h = rng.randint(0, 2**64, size=10_000, dtype=np.uint64)
    h[:4] = [0, 1, 2**64 - 1, 2**63]
    assert (bk.hash_u64(bk.keys_for_hashes(h)) == h).all()
    k = rng.randint(-2**63, 2**63 - 1, size=10_000, dtype=np.int64)
    assert (bk.keys_for_hashes(bk.hash_u64(k)) == k).all()
    # the two multipliers really are inverses mod 2^64
    assert (0xBF58476D1CE4E5B9 * int(bk.INV_M1)) % 2**64 == 1
    assert (0x94D049BB133111EB * int(bk.INV_M2)) % 2**64 == 1


def test_make_h64_fields():
    k = bk.keys_for_hashes(bk.make_h64([0xABCDEF, 5], [0x12, 0xFF], [7, 2**32 - 1]))
    h = bk.hash_u64(k)
    assert bk.bucket_of(k).tolist() == [0xABCDEF, 5]
    assert (h & np.uint64(0xFF)).tolist() == [0x12, 0xFF]
    assert (h >> np.uint64(32)).tolist() == [7, 2**32 - 1]


def sample_is_distinct(lay):
    s = lay.k[bk.sampled_positions(lay.n)]
    return len(np.unique(s)) == len(s)


def test_crafted_layout():
    lay = bk.crafted()
    assert lay.n == 3 * FT + 37
    assert hash_order_lens(lay) == lay.lens
    assert set(bk.CYCLE) <= set(lay.lens) and max(lay.lens) == bk.BUCKET_CAP
    st = bk.bucket_starts(lay.lens)
    en = st + np.asarray(lay.lens)
    span = dict(zip(st.tolist(), lay.lens))
    assert FT in en and FT in st                         # ends on / starts on an edge
    assert span[FT - 1] == 1                             # 1-row bucket, tile's last row
    assert span[2 * FT - 1] > 1                          # 1 row left of an edge
    assert (3 * FT + 1) in en and span[3 * FT + 1 - 255] == 255   # 1 row right of one
    assert en[-1] == lay.n and st[-1] > 3 * FT           # last bucket ends the data
    # planted runs: every shape, as built, and in a bucket across a tile edge
    # (free rows may add runs of their own where byte 0 happens to repeat)
    got = Counter(shape_of(r) for r in h32_runs(lay))
    want = Counter(canon(s) for _, s in lay.runs)
    assert not (want - got), want - got
    assert {canon(s) for s in bk.SHAPES} <= {canon(s) for _, s in lay.runs}
    edge = {bi for bi in range(len(st)) if st[bi] // FT != (en[bi] - 1) // FT}
    assert edge & {bi for bi, _ in lay.runs}
    assert -1 in lay.k
    assert len(np.unique(lay.k)) < lay.n                 # keys repeat across the input
    assert sample_is_distinct(lay)


def test_oversized_layout():
    lay = bk.oversized()
    assert hash_order_lens(lay) == lay.lens
    span = dict(zip(bk.bucket_starts(lay.lens).tolist(), lay.lens))
    assert span[500] == 257 and span[2 * FT - 100] == 257
    assert sorted(lay.lens)[-3] <= bk.BUCKET_CAP   # only those two are over
    assert 500 + 257 < FT and 2 * FT - 100 < 2 * FT < 2 * FT - 100 + 257
    assert sample_is_distinct(lay)


def test_dirty_run_layout():
    lay = bk.dirty_run()
    assert hash_order_lens(lay) == lay.lens and max(lay.lens) <= bk.BUCKET_CAP
    long = [r for r in h32_runs(lay) if len(r) > bk.RUN_CAP]
    assert len(long) == 1 and len(long[0]) == 65
    assert shape_of(long[0]) == "ABC" * 21 + "AB"
    assert sample_is_distinct(lay)


def test_poisson_layout():
    lay = bk.poisson()
    assert lay.n == 300_000 and len(np.unique(lay.k)) == lay.n
    lens = np.asarray(lay.lens)
    assert len(lens) == 5000 and abs(lens.mean() - 60) < 1e-9
    assert 25 < lens.min() and lens.max() < 110 and abs(lens.var() - 60) < 6
    assert sample_is_distinct(lay)
    rep = bk.with_sampled_repeat(lay)
    s = rep.k[bk.sampled_positions(rep.n)]
    assert len(np.unique(s)) == len(s) - 1
    assert (rep.k != lay.k).sum() == 1


@pytest.mark.parametrize("n", [1, 2, 63, FT - 1, FT, FT + 1, 2 * FT + 255])
def test_distinct_layout(n):
    lay = bk.distinct(n, seed=n)
    assert lay.n == n and len(np.unique(lay.k)) == n
    assert hash_order_lens(lay) == lay.lens
    assert sample_is_distinct(lay)
