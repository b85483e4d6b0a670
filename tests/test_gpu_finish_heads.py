"""The segmented reduce takes its per-tile head counts from k_bucket_finish
when the finish route grouped the rows, and initialises no accumulator.

Inputs come from tests/finish_heads_keys.py: the final order is chosen row by
row, with equal-key runs on the finish-tile, seg-tile and chunk edges. The
oracle is the four-pass route's grouped rows (vega_dev_group_rows_i64, route
1) reduced on the host in that order. Output tensors are pre-filled with
0x5A5A...: a slot the kernels fail to store, or one they only add into, shows.
"""
import functools

import numpy as np
import pytest

import bucket_keys as bk
import finish_heads_keys as fh
import seg_layout as sl

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A5A5A5A5A
OPS = ["SUM_I64", "COUNT", "MIN_I64", "MAX_I64", "SUM_F64"]


@functools.lru_cache(maxsize=None)
def crafted(n, runs=True):
    lay = fh.build(n, seed=n, runs=runs)
    lay.k.setflags(write=False)
    return lay


@functools.lru_cache(maxsize=None)
def values(op, n):
    v = fh.values_for(op, n, seed=17 + op)
    v.setflags(write=False)
    return v


def group_rows_route1(k):
    """grouped keys and the input row of every grouped row, four-pass route"""
    import torch
    from vega_amd import gpu
    kt = torch.from_numpy(np.array(k)).cuda()
    vt = torch.arange(len(k), dtype=torch.int64, device="cuda")
    ok, ov = torch.empty_like(kt), torch.empty_like(vt)
    taken = gpu.dev_group_rows(kt, vt, 1, ok, ov, gpu.alloc_ws(len(k)))
    assert taken == 1
    return ok.cpu().numpy(), ov.cpu().numpy()


@functools.lru_cache(maxsize=None)
def crafted_grouped(n, runs=True):
    return group_rows_route1(crafted(n, runs).k)


def sort_reduce_sentinel(k, v, op):
    """dev_sort_reduce into sentinel-filled outputs; (keys, value bits, tail
    bits of out_v beyond the result, profile)"""
    import torch
    from vega_amd import gpu
    kt = torch.from_numpy(np.array(k)).cuda()
    vt = torch.from_numpy(np.array(v).view(np.int64)).cuda()
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
    ov = out_v.cpu().numpy()
    return out_k[:nout].cpu().numpy(), ov[:nout], ov[nout:], stats


def check_against(gk, gv, v, op, got):
    out_k, out_v, tail, _ = got
    ek, ev = fh.reduce_in_order(op, gk, v[gv])
    assert len(out_k) == len(ek)
    assert (out_k == ek).all(), "keys are not in the four-pass route's order"
    bad = np.flatnonzero(out_v != ev.view(np.int64))
    assert len(bad) == 0, (len(bad), bad[:8], out_v[bad][:8], ev.view(np.int64)[bad][:8])
    assert (tail == SENTINEL).all(), "stores beyond the last segment"


def assert_finish_route(stats):
    assert stats["bucket_finish"]["n"] == 1, stats
    assert stats["radix_scatter"]["n"] == 3, stats
    assert stats["head_count"]["n"] == 1, stats
    assert stats["seg_emit"]["n"] == 1, stats


@pytest.mark.parametrize("n", fh.SIZES)
def test_oracle_order_is_the_crafted_order(n):
    gk, _ = crafted_grouped(n)
    assert (gk == crafted(n).final_k).all()


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("n", fh.SIZES)
def test_crafted_runs_on_finish_route(n, op):
    opn = sl.OPS[op]
    runs = op != "SUM_F64"       # f64: distinct keys, so the sum is the row itself
    lay = crafted(n, runs)
    v = values(opn, n)
    got = sort_reduce_sentinel(lay.k, v, opn)
    assert_finish_route(got[3])
    assert ("f64_combine" if op == "SUM_F64" else "seg_fold") in got[3], got[3]
    gk, gv = crafted_grouped(n, runs)
    check_against(gk, gv, v, opn, got)
    assert len(got[0]) == len(lay.run_lens)


@pytest.mark.parametrize("op", OPS[:4])
@pytest.mark.parametrize("name", ["oversized", "dirty_run"])
def test_finish_abort_uses_its_own_head_count(name, op):
    """the finish raises its flag after some tiles stored their counts: the
    four-pass route's rows must be counted again, not with those"""
    opn = sl.OPS[op]
    lay = getattr(bk, name)()
    v = values(opn, lay.n)
    got = sort_reduce_sentinel(lay.k, v, opn)
    stats = got[3]
    assert stats["bucket_finish"]["n"] == 1 and stats["radix_scatter"]["n"] >= 7, stats
    assert stats["head_count"]["n"] == 1 and stats["seg_emit"]["n"] == 1, stats
    gk, gv = group_rows_route1(lay.k)
    check_against(gk, gv, v, opn, got)


@pytest.mark.parametrize("op", OPS[:4])
def test_sampled_repeat_takes_four_pass_route(op):
    opn = sl.OPS[op]
    lay = bk.with_sampled_repeat(bk.poisson())
    v = values(opn, lay.n)
    got = sort_reduce_sentinel(lay.k, v, opn)
    stats = got[3]
    assert "bucket_finish" not in stats and stats["radix_scatter"]["n"] == 4, stats
    assert stats["head_count"]["n"] == 1 and stats["seg_fold"]["n"] == 1, stats
    gk, gv = group_rows_route1(lay.k)
    check_against(gk, gv, v, opn, got)


@pytest.mark.parametrize("n", fh.SIZES)
def test_stats_by_key_on_finish_route(n):
    import torch
    from vega_amd import gpu
    lay = crafted(n)
    v = values(sl.OP_MIN_I64, n)
    kt = torch.from_numpy(np.array(lay.k)).cuda()
    vt = torch.from_numpy(np.array(v)).cuda()
    outs = [torch.full_like(kt, SENTINEL) for _ in range(5)]
    ws = gpu.alloc_ws(n)
    gpu.prof_stats()
    gpu.prof_enable(True)
    try:
        nout = gpu.dev_sort_stats(kt, vt, *outs, ws)
        torch.cuda.synchronize()
        stats = gpu.prof_stats()
    finally:
        gpu.prof_enable(False)
    assert stats["bucket_finish"]["n"] == 1 and stats["radix_scatter"]["n"] == 3, stats
    assert stats["head_count"]["n"] == 1 and stats["seg_stats"]["n"] == 1, stats
    got = [o[:nout].cpu().numpy() for o in outs]
    o = np.argsort(got[0], kind="stable")
    ops = (sl.OP_COUNT, sl.OP_SUM_I64, sl.OP_MIN_I64, sl.OP_MAX_I64)
    ref = [sl.reduce_ref(op, lay.k, v) for op in ops]
    assert nout == len(ref[0][0]) and (got[0][o] == ref[0][0]).all()
    for name, g, (_, r) in zip(("count", "sum", "min", "max"), got[1:], ref):
        assert (g[o] == r).all(), name
    # and in the grouped order, like the single-op reduce
    assert (got[0] == fh.reduce_in_order(sl.OP_COUNT, *crafted_grouped(n))[0]).all()
