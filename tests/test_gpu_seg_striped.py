"""k_seg_emit loads a wave's 512-row span striped (lane-contiguous) and emits
a full span of 512 heads straight from those registers (the fast wave); any
other wave hands its rows over through LDS to the per-chunk code. The layouts
here sit on the edges of that split: tail spans next to fast waves, an odd slot
base under every fast wave, one equal pair across a load round, a wave, a tile
and at the very end, runs that leave a wave with few or no heads.

Both row formats (narrow keys: SoA, wide keys: packed) and all five ops. The
outputs are pre-filled with a sentinel. f64 values are small integers, so the
sums are exact in any order and compare bit for bit with numpy; every f64 case
runs twice and must give the same bits. Reference: seg_layout.reduce_ref.
"""
import functools
import zlib

import numpy as np
import pytest

import seg_layout as sl
from test_gpu_seg_fold import SENTINEL, assert_matches_ref

pytestmark = pytest.mark.gpu

N3 = 2 * sl.TILE + 5          # three tiles, the last one a 5-row tail span
SIZES = [1, 7, 8, 9, 511, 512, 513, 1024, 4095, 4096, 4097, N3]


def _pair_at(p, n=N3):
    """all distinct but rows (p, p + 1)"""
    assert 0 <= p <= n - 2
    return [1] * p + [2] + [1] * (n - p - 2)


def _run_at(start, length, n=N3):
    return [1] * start + [length] + [1] * (n - start - length)


LAYOUTS = {"distinct_%d" % n: (lambda n=n: [1] * n) for n in SIZES}
LAYOUTS.update({
    "pair_0_1": lambda: _pair_at(0),                  # odd slot base from wave 1 on
    "pair_255_256": lambda: _pair_at(255),            # lane 63 -> lane 0 of the next load round
    "pair_511_512": lambda: _pair_at(511),            # across waves
    "pair_4095_4096": lambda: _pair_at(4095),         # across tiles
    "pair_last": lambda: _pair_at(N3 - 2),
    "run512_aligned": lambda: _run_at(512, 512),      # wave 1: one head, 63 lead chunks
    "run512_shift3": lambda: _run_at(515, 512),
    "run1030_from_509": lambda: _run_at(509, 1030),   # wave 1 holds no head at all
    "run8_chunk": lambda: _run_at(520, 8),            # one chunk of a distinct wave
})
INT_OPS = ["SUM_I64", "COUNT", "MIN_I64", "MAX_I64"]


@functools.lru_cache(maxsize=None)
def layout(name, strategy):
    """(Layout or None, k): run i is the i-th grouped run. A single row has no
    varying key byte, so it is sorted as narrow whatever the key: no Layout."""
    lens = np.asarray(LAYOUTS[name](), dtype=np.int64)
    rng = np.random.RandomState(zlib.crc32((name + strategy).encode()) & 0x7FFFFFFF)
    if strategy == "narrow":
        keys = np.arange(len(lens), dtype=np.int64)
    else:
        keys = sl.draw_wide_keys(len(lens), rng)
        keys = keys[np.argsort(sl.h32(keys), kind="stable")]
    if len(lens) == 1:
        k = np.repeat(keys, lens)
        k.setflags(write=False)
        return None, k
    lay = sl.build(lens, keys, rng, strategy)
    assert (lay.order == np.arange(len(lens))).all()
    lay.k.setflags(write=False)
    return lay, lay.k


@functools.lru_cache(maxsize=None)
def values(name, strategy, op):
    _, k = layout(name, strategy)
    rng = np.random.RandomState(53 + op)
    n = len(k)
    if op == sl.OP_SUM_F64:
        v = rng.randint(-(1 << 30), (1 << 30) + 1, size=n).astype(np.float64)
        v[rng.randint(0, n)] = -0.0
    elif op == sl.OP_SUM_I64:
        v = rng.randint(sl.I64_MIN, sl.I64_MAX, size=n, dtype=np.int64)
    else:
        v = rng.randint(-(1 << 40), 1 << 40, size=n, dtype=np.int64)
        v[rng.randint(0, n)] = sl.I64_MIN
        v[rng.randint(0, n)] = sl.I64_MAX
    v.setflags(write=False)
    return v


def sort_reduce_sentinel(k, v, op):
    """dev_sort_reduce into sentinel-filled outputs; v int64 or float64"""
    import torch
    from vega_amd import gpu
    kt = torch.from_numpy(np.array(k)).cuda()
    vt = torch.from_numpy(np.array(v)).cuda()
    out_k = torch.full_like(kt, SENTINEL)
    out_v = torch.full_like(kt, SENTINEL)
    if v.dtype == np.float64:
        out_v = out_v.view(torch.float64)
    ws = gpu.alloc_ws(len(k))
    gpu.prof_stats()
    gpu.prof_enable(True)
    try:
        nout = gpu.dev_sort_reduce(kt, vt, op, out_k, out_v, ws)
        torch.cuda.synchronize()
        stats = gpu.prof_stats()
    finally:
        gpu.prof_enable(False)
    ok, ov = out_k.cpu().numpy(), out_v.cpu().numpy().view(np.int64)
    assert (ok[nout:] == SENTINEL).all() and (ov[nout:] == SENTINEL).all()
    return ok[:nout], ov[:nout], stats


def check_order_and_scopes(name, strategy, out_k, stats):
    lay, k = layout(name, strategy)
    assert stats["seg_emit"]["n"] == 1, stats
    if lay is None:
        assert (out_k == k[:1]).all()
        return
    assert ("hist8" in stats) == (strategy == "narrow"), stats
    # grouped order: narrow rows come out in key order, hash rows in h32 order
    assert len(out_k) == len(lay.keys) and (out_k == lay.keys).all()


@pytest.mark.parametrize("op", INT_OPS)
@pytest.mark.parametrize("strategy", ["narrow", "hash"])
@pytest.mark.parametrize("name", list(LAYOUTS))
def test_int_ops(name, strategy, op):
    opn = sl.OPS[op]
    _, k = layout(name, strategy)
    v = values(name, strategy, opn)
    out_k, out_v, stats = sort_reduce_sentinel(k, v, opn)
    assert stats["seg_fold"]["n"] == 1, stats
    assert_matches_ref(k, v, opn, out_k, out_v)
    check_order_and_scopes(name, strategy, out_k, stats)


@pytest.mark.parametrize("strategy", ["narrow", "hash"])
@pytest.mark.parametrize("name", list(LAYOUTS))
def test_sum_f64_exact_and_stable(name, strategy):
    _, k = layout(name, strategy)
    v = values(name, strategy, sl.OP_SUM_F64)
    out_k, out_v, stats = sort_reduce_sentinel(k, v, sl.OP_SUM_F64)
    # numpy reference, bit for bit: the sums are integers below 2^53, exact in
    # any order; a run of the single value -0.0 sums to +0.0 (0.0 + -0.0)
    order = np.argsort(k, kind="stable")
    ks = k[order]
    starts = np.flatnonzero(np.concatenate([[True], ks[1:] != ks[:-1]]))
    ref = np.add.reduceat(v[order], starts) + 0.0
    o = np.argsort(out_k, kind="stable")
    assert len(out_k) == len(starts) and (out_k[o] == ks[starts]).all()
    assert (out_v[o] == ref.view(np.int64)).all()
    check_order_and_scopes(name, strategy, out_k, stats)
    again_k, again_v, _ = sort_reduce_sentinel(k, v, sl.OP_SUM_F64)
    assert (again_k == out_k).all() and (again_v == out_v).all()
