"""MSB radix select on device buffers (vega_dev_select_k_i64) with
cand_cap = 64, so small inputs walk the deep-digit paths. The expected
output is np.lexsort exactly, ascending and descending."""
import ctypes
import os
import sys

import numpy as np
import pytest

import actions_ref as ar
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vega_amd import datagen

pytestmark = pytest.mark.gpu

CAP = 64
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1


@pytest.fixture(scope="module")
def ctx():
    from vega_amd import gpu
    with gpu.VegaContext() as c:
        yield c


def select(k, v, num, descending, cand_cap=CAP):
    import torch
    from vega_amd import gpu
    kt = torch.from_numpy(np.ascontiguousarray(k)).cuda()
    vt = torch.from_numpy(np.ascontiguousarray(v)).cuda()
    ok, ov, passes = gpu.dev_select_k(kt, vt, num, descending=descending, cand_cap=cand_cap)
    torch.cuda.synchronize()
    # the input buffers are read-only to the select
    assert (kt.cpu().numpy() == k).all() and (vt.cpu().numpy() == v).all()
    return ok.cpu().numpy(), ov.cpu().numpy(), passes


def check_both(k, v, num):
    """exact lexsort parity in both directions; returns the two pass counts"""
    out = []
    for desc, ref in ((False, ar.take_ordered), (True, ar.top)):
        gk, gv, passes = select(k, v, num, desc)
        ek, ev = ref(k, v, num)
        assert gk.tolist() == ek.tolist() and gv.tolist() == ev.tolist(), (len(k), num, desc)
        out.append(passes)
    return out


@pytest.mark.parametrize("n", [65, 4097, 200_000])
def test_uniform_keys(ctx, n):
    k, v = datagen.uniform_pairs(300 + n, n, key_bits=63)
    for num in (1, 10, 1000):
        passes = check_both(k, v, num)
        if num < n:
            assert all(1 <= p <= 16 for p in passes)
        else:
            assert passes == [0, 0]


def test_mixed_sign_both_columns(ctx):
    n = 4097
    k, v = datagen.uniform_pairs(41, n, key_bits=64)  # full-range signed keys, values
    k[5], v[5] = I64_MIN, I64_MAX
    k[6], v[6] = I64_MIN, I64_MIN
    k[7], v[7] = I64_MAX, I64_MIN
    k[8], v[8] = I64_MAX, I64_MAX
    k[9], v[9] = 0, -1
    k[10], v[10] = -1, 0
    for num in (1, 2, 3, 100):
        check_both(k, v, num)
    # a narrow mixed-sign key column: the value sign flip decides the order
    k2 = (k % 3) - 1
    for num in (1, 70):
        check_both(k2, v, num)


def test_narrow_keys_enter_value_digits(ctx):
    n = 100_000
    k, v = datagen.uniform_pairs(42, n, key_bits=3)
    # every key owns ~12.5k rows >> cand_cap: all eight key digits are
    # consumed and the select goes on into the value digits
    assert np.bincount(k, minlength=8).min() > 10 * CAP
    for passes in check_both(k, v, 50):
        assert passes >= 9


def test_all_rows_identical(ctx):
    n = 70_000
    k = np.full(n, 7, dtype=np.int64)
    v = np.full(n, -3, dtype=np.int64)
    for desc in (False, True):
        gk, gv, passes = select(k, v, 100, desc)
        # the threshold bucket never shrinks below cand_cap: all 16 digits
        # are consumed and the result is padded with the threshold row
        assert passes == 16
        assert gk.tolist() == [7] * 100 and gv.tolist() == [-3] * 100


def test_rows_below_plus_identical_bucket(ctx):
    # 40 distinct smaller rows, then a 70k-row bucket of one repeated row:
    # candidates (sorted) followed by padding copies
    n = 70_000
    k = np.full(n, 7, dtype=np.int64)
    v = np.full(n, -3, dtype=np.int64)
    k[1000:1040] = np.arange(40) - 20
    v[1000:1040] = np.arange(40)[::-1]
    k[2000:2040] = 7
    v[2000:2040] = np.arange(40) + 10       # larger rows, for descending
    for passes in check_both(k, v, 100):
        assert passes == 16


def test_bucket_edge_cumulative_equals_num(ctx):
    k = np.arange(256, dtype=np.int64) << 48
    v = np.zeros(256, dtype=np.int64)
    gk, gv, passes = select(k, v, 16, False)
    assert gk.tolist() == [i << 48 for i in range(16)] and not gv.any()
    assert passes == 2  # byte 0 is constant, byte 1 isolates bucket 15
    gk, gv, _ = select(k, v, 16, True)
    assert gk.tolist() == [i << 48 for i in range(255, 239, -1)]


def test_num_at_least_n_and_zero(ctx):
    k, v = datagen.uniform_pairs(43, 4097, key_bits=5)
    for num in (4097, 4098, 1 << 33):
        assert check_both(k, v, num) == [0, 0]
    for desc in (False, True):
        gk, gv, passes = select(k, v, 0, desc)
        assert len(gk) == 0 and len(gv) == 0 and passes == 0
    e = np.zeros(0, dtype=np.int64)
    gk, gv, passes = select(e, e, 5, False)
    assert len(gk) == 0 and passes == 0


def test_default_cand_cap(ctx):
    k, v = datagen.uniform_pairs(44, 200_000, key_bits=63)
    for desc, ref in ((False, ar.take_ordered), (True, ar.top)):
        gk, gv, passes = select(k, v, 10, desc, cand_cap=0)
        ek, ev = ref(k, v, 10)
        assert gk.tolist() == ek.tolist() and gv.tolist() == ev.tolist()
        assert passes == 1  # 200k rows fit the default bucket bound at once


def test_short_workspace_is_refused(ctx):
    import torch
    from vega_amd import gpu
    n, num = 4097, 10
    k, v = datagen.uniform_pairs(45, n, key_bits=63)
    kt, vt = torch.from_numpy(k).cuda(), torch.from_numpy(v).cuda()
    need = gpu.select_ws_bytes(num, CAP)
    assert need < gpu.select_ws_bytes(num, 0)  # O(num + cand_cap)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    ok = torch.full((num,), -1, dtype=torch.int64, device="cuda")
    ov = torch.full((num,), -1, dtype=torch.int64, device="cuda")
    nout, passes = ctypes.c_uint64(99), ctypes.c_int(99)

    def call(nbytes):
        return gpu.lib().vega_dev_select_k_i64(
            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream),
            ctypes.c_void_p(kt.data_ptr()), ctypes.c_void_p(vt.data_ptr()),
            ctypes.c_uint64(n), ctypes.c_uint64(num), ctypes.c_int(0), ctypes.c_uint64(CAP),
            ctypes.c_void_p(ok.data_ptr()), ctypes.c_void_p(ov.data_ptr()),
            ctypes.byref(nout), ctypes.byref(passes),
            ctypes.c_void_p(ws.data_ptr()), ctypes.c_size_t(nbytes))

    gpu.prof_stats()        # drain events other tests may have left pending
    gpu.prof_enable(True)   # and start from an empty registry
    assert call(need - 1) == -5  # VEGA_ERR_CAP
    torch.cuda.synchronize()
    assert gpu.prof_stats() == {}  # nothing was launched
    assert nout.value == 0 and passes.value == 0
    assert (ok.cpu().numpy() == -1).all() and (ov.cpu().numpy() == -1).all()
    assert call(need) == 0
    torch.cuda.synchronize()
    stats = gpu.prof_stats()
    gpu.prof_enable(False)
    assert stats["select_hist"]["n"] == passes.value and stats["select_compact"]["n"] == 1
    ek, ev = ar.take_ordered(k, v, num)
    assert ok.cpu().numpy().tolist() == ek.tolist() and ov.cpu().numpy().tolist() == ev.tolist()
    assert nout.value == num and passes.value >= 1


def test_dev_reduce_pairs_matches_handle_reduce(ctx):
    import torch
    from vega_amd import gpu
    k, v = datagen.uniform_pairs(46, 4097, key_bits=64)
    kt, vt = torch.from_numpy(k).cuda(), torch.from_numpy(v).cuda()
    rdd = ctx.make_rdd(k, v)
    for op in (gpu.OP_SUM_I64, gpu.OP_MIN_I64, gpu.OP_MAX_I64):
        got = gpu.dev_reduce_pairs(kt, vt, op)
        assert got == rdd.reduce(op) == ar.reduce(k, v, op)
    # an 8-byte-aligned (not 16) view takes the scalar-load path
    got = gpu.dev_reduce_pairs(kt[1:], vt[1:], gpu.OP_SUM_I64)
    assert got == ar.reduce(k[1:], v[1:], ar.OP_SUM_I64)
    gk, gv, _ = gpu.dev_select_k(kt[1:], vt[1:], 10, cand_cap=CAP)
    ek, ev = ar.take_ordered(k[1:], v[1:], 10)
    assert gk.cpu().numpy().tolist() == ek.tolist() and gv.cpu().numpy().tolist() == ev.tolist()
    rdd.free()
