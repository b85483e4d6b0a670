"""Integer segmented reduce without accumulator init: k_seg_emit plain-stores
every slot and k_seg_lead_fold adds each chunk's lead (the rows of the run
open at the chunk's start).

Layouts put leads across tiles, whole waves and partial waves, on narrow keys
(SoA rows, key-ordered) and wide keys (packed rows, h32-ordered); the outputs
are pre-filled with a sentinel, so a slot that is only added into, or never
stored, shows. Reference: seg_layout.reduce_ref.
"""
import functools

import numpy as np
import pytest

import seg_layout as sl

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A5A5A5A5A
INT_OPS = ["SUM_I64", "COUNT", "MIN_I64", "MAX_I64"]
LONG = 3 * sl.TILE + 5


def _lens_one_long():
    # starts at row 13 (mid-chunk), ends at row 13 + LONG - 1 = 12305 (mid-chunk)
    return [1] * 13 + [LONG] + [1] * 11


def _lens_two_long():
    # rows 14..12306, one row, rows 12308..24600: all four ends are mid-chunk
    return [1] * 14 + [LONG, 1, LONG] + [2, 1, 1]


def _lens_head_at_row3():
    # every chunk's only head is its row 3 (chunk 0 also holds row 0's):
    # each has a 3-row lead and starts a run; 2 tiles and a partial wave
    return [3] + [8] * (2 * sl.TILE // 8 + 70) + [5]


RUNS = {"one_long": _lens_one_long, "two_long": _lens_two_long, "head_at_row3": _lens_head_at_row3}


@functools.lru_cache(maxsize=None)
def layout(name, strategy):
    lens = np.asarray(RUNS[name](), dtype=np.int64)
    rng = np.random.RandomState(len(lens) + (7 if strategy == "hash" else 0))
    if strategy == "narrow":
        keys = np.arange(len(lens), dtype=np.int64)
    else:   # wide keys handed out in ascending h32: run i is the i-th grouped run
        keys = sl.draw_wide_keys(len(lens), rng)
        keys = keys[np.argsort(sl.h32(keys), kind="stable")]
    lay = sl.build(lens, keys, rng, strategy)
    assert (lay.order == np.arange(len(lens))).all()
    if name != "head_at_row3":
        s = lay.gstart[lens == LONG]
        assert (s % sl.CHUNK != 0).all() and ((s + LONG) % sl.CHUNK != 0).all()
    else:
        assert (lay.gstart[1:] % sl.CHUNK == 3).all()
    lay.k.setflags(write=False)
    return lay


def values_with_extremes(lay, rng):
    """+-2^40 noise; in every run longer than a tile INT64_MIN and INT64_MAX
    sit in leads: the chunk after the head's, and one 4096 + 100 rows in"""
    v = rng.randint(-(1 << 40), 1 << 40, size=lay.n, dtype=np.int64)
    at = np.full(lay.n, -1, dtype=np.int64)     # grouped position -> input row
    at[lay.gpos] = np.arange(lay.n)
    for s in lay.gstart[lay.run_lens > sl.TILE]:
        v[at[s + sl.CHUNK]] = sl.I64_MIN
        v[at[s + sl.TILE + 100]] = sl.I64_MAX
        v[at[s + 2 * sl.TILE + 7]] = sl.I64_MIN
    return v


@functools.lru_cache(maxsize=None)
def values(name, strategy, op):
    lay = layout(name, strategy)
    rng = np.random.RandomState(31 + op)
    if op == sl.OP_SUM_I64:
        v = sl.values_sum_i64(lay, rng)
    elif name == "head_at_row3":
        v = sl.values_minmax(lay, rng)
    else:
        v = values_with_extremes(lay, rng)
    v.setflags(write=False)
    return v


def sort_reduce_sentinel(k, v, op):
    import torch
    from vega_amd import gpu
    kt = torch.from_numpy(np.array(k)).cuda()
    vt = torch.from_numpy(np.array(v)).cuda()
    out_k = torch.full_like(kt, SENTINEL)
    out_v = torch.full_like(kt, SENTINEL)
    ws = gpu.alloc_ws(len(k))
    gpu.prof_stats()
    gpu.prof_enable(True)
    try:
        nout = gpu.dev_sort_reduce(kt, vt, op, out_k, out_v, ws)
        torch.cuda.synchronize()
        stats = gpu.prof_stats()
    finally:
        gpu.prof_enable(False)
    ok, ov = out_k.cpu().numpy(), out_v.cpu().numpy()
    assert (ok[nout:] == SENTINEL).all() and (ov[nout:] == SENTINEL).all()
    return ok[:nout], ov[:nout], stats


def assert_matches_ref(k, v, op, out_k, out_v):
    rk, rv = sl.reduce_ref(op, k, v)
    o = np.argsort(out_k, kind="stable")
    assert len(out_k) == len(rk) and (out_k[o] == rk).all()
    bad = np.flatnonzero(out_v[o] != rv)
    assert len(bad) == 0, (len(bad), rk[bad][:8], out_v[o][bad][:8], rv[bad][:8])


@pytest.mark.parametrize("op", INT_OPS)
@pytest.mark.parametrize("strategy", ["narrow", "hash"])
@pytest.mark.parametrize("name", sorted(RUNS))
def test_leads(name, strategy, op):
    opn = sl.OPS[op]
    lay = layout(name, strategy)
    v = values(name, strategy, opn)
    out_k, out_v, stats = sort_reduce_sentinel(lay.k, v, opn)
    for scope in ("head_count", "seg_emit", "seg_fold"):
        assert stats[scope]["n"] == 1, stats
    assert ("hist8" in stats) == (strategy == "narrow"), stats
    assert_matches_ref(lay.k, v, opn, out_k, out_v)
    # grouped order: narrow rows come out in key order, hash rows in h32 order
    assert (out_k == lay.keys).all()


def test_extremes_sit_in_leads():
    """what values_with_extremes promises, on the layout itself"""
    lay = layout("one_long", "narrow")
    v = values("one_long", "narrow", sl.OP_MIN_I64)
    gv = np.empty(lay.n, dtype=np.int64)
    gv[lay.gpos] = v
    s = int(lay.gstart[lay.run_lens == LONG][0])
    for pos, want in ((s + sl.CHUNK, sl.I64_MIN), (s + sl.TILE + 100, sl.I64_MAX)):
        assert gv[pos] == want and pos // sl.CHUNK > s // sl.CHUNK and pos < s + LONG


@pytest.mark.parametrize("op", INT_OPS)
@pytest.mark.parametrize("kind", ["equal", "distinct_narrow", "distinct_wide"])
@pytest.mark.parametrize("n", [1, 7, 8, 9, 4095, 4096, 4097])
def test_sizes(n, kind, op):
    opn = sl.OPS[op]
    rng = np.random.RandomState(n)
    if kind == "equal":
        k = np.full(n, 0x0123456789ABCDEF, dtype=np.int64)
    elif kind == "distinct_narrow":
        k = rng.permutation(n).astype(np.int64)
    else:
        k = sl.draw_wide_keys(n, rng)
    v = rng.randint(-(1 << 40), 1 << 40, size=n, dtype=np.int64)
    v[rng.randint(0, n)] = sl.I64_MIN
    v[rng.randint(0, n)] = sl.I64_MAX
    out_k, out_v, stats = sort_reduce_sentinel(k, v, opn)
    assert stats["seg_emit"]["n"] == 1 and stats["seg_fold"]["n"] == 1, stats
    assert len(out_k) == (1 if kind == "equal" else n)
    assert_matches_ref(k, v, opn, out_k, out_v)
