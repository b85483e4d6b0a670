"""CPU-side ABI checks for the samplers: the five entries are declared in
include/vega_gpu.h and exported by libvega_gpu.so, the Python surface exists,
the host-side Poisson table agrees with sample_ref, and the argument guards
that need no device return their codes. No kernel is launched."""
import ctypes
import os
import re

import numpy as np
import pytest

import sample_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "vega_gpu.h")
SO = os.path.join(ROOT, "vega_amd", "csrc", "libvega_gpu.so")

SAMPLE_SYMBOLS = ["vega_gpu_sample", "vega_gpu_random_split", "vega_gpu_take_sample",
                  "vega_dev_sample", "vega_sample_poisson_table"]
ERR_INVALID, ERR_NOMEM, ERR_UNSUPPORTED = -1, -2, -4


@pytest.fixture(scope="module")
def so():
    return ctypes.CDLL(SO)


def test_sample_symbols_declared():
    with open(HDR) as f:
        header = f.read()
    # the header's style: "int vega_xxx(" at a line start (what test_abi.py reads)
    declared = re.findall(r"^int\s+(vega_\w+)\s*\(", header, flags=re.M)
    assert [s for s in SAMPLE_SYMBOLS if s not in declared] == []


def test_sample_symbols_exported(so):
    assert [s for s in SAMPLE_SYMBOLS if not hasattr(so, s)] == []


def test_python_surface():
    from vega_amd import gpu
    for name in ("sample", "random_split", "take_sample"):
        assert callable(getattr(gpu.Rdd, name))
    assert callable(gpu.dev_sample)
    assert callable(gpu.sample_poisson_table)
    # seed=None draws 64 bits on the host
    a, b = gpu._seed(None), gpu._seed(None)
    assert 0 <= a < 1 << 64 and 0 <= b < 1 << 64 and a != b
    assert gpu._seed(-1) == (1 << 64) - 1 and gpu._seed(5) == 5


def table(so, lam):
    thr = np.zeros(256, dtype=np.uint64)
    n = ctypes.c_int(-7)
    rc = so.vega_sample_poisson_table(ctypes.c_double(lam),
                                      thr.ctypes.data_as(ctypes.c_void_p), ctypes.byref(n))
    return rc, thr, n.value


@pytest.mark.parametrize("lam", [0.0, 1e-6, 0.1, 0.27, 1.0, 1.3366, 3.5, 16.0])
def test_poisson_table_matches_sample_ref(so, lam):
    rc, thr, n = table(so, lam)
    assert rc == 0
    ref = sr.poisson_table(lam)
    assert n == len(ref)
    # the two sides share only exp() from libm: at most one unit apart
    diff = np.abs(thr[:n].astype(np.int64) - ref.astype(np.int64))
    assert int(diff.max()) <= 1, diff.max()
    assert not thr[n:].any()  # nothing written past the length


def test_poisson_table_guards(so):
    assert table(so, -0.5)[0] == ERR_INVALID
    assert table(so, float("nan"))[0] == ERR_INVALID
    rc, _, n = table(so, 16.5)
    assert rc == ERR_UNSUPPORTED and n == 0
    n = ctypes.c_int(0)
    assert so.vega_sample_poisson_table(ctypes.c_double(1.0), None, ctypes.byref(n)) == ERR_INVALID
    thr = np.zeros(256, dtype=np.uint64)
    assert so.vega_sample_poisson_table(ctypes.c_double(1.0),
                                        thr.ctypes.data_as(ctypes.c_void_p), None) == ERR_INVALID


def test_handle_entries_reject_a_null_context(so):
    out = ctypes.c_uint64(99)
    assert so.vega_gpu_sample(None, ctypes.c_uint64(1), 0, ctypes.c_double(0.5),
                              ctypes.c_uint64(1), ctypes.byref(out)) == ERR_INVALID
    w = (ctypes.c_double * 2)(1.0, 1.0)
    outs = (ctypes.c_uint64 * 2)()
    assert so.vega_gpu_random_split(None, ctypes.c_uint64(1), w, ctypes.c_uint32(2),
                                    ctypes.c_uint64(1), outs) == ERR_INVALID
    n = ctypes.c_uint64(0)
    assert so.vega_gpu_take_sample(None, ctypes.c_uint64(1), 0, ctypes.c_uint64(3),
                                   ctypes.c_uint64(1), None, None, ctypes.byref(n)) == ERR_INVALID


def dev_sample(so, n, repl, fraction, nout, ws=None, ws_bytes=0, keys=None, vals=None):
    return so.vega_dev_sample(None, keys, vals, ctypes.c_uint64(n), ctypes.c_int(repl),
                              ctypes.c_double(fraction), ctypes.c_uint64(1), ctypes.c_uint64(0),
                              None, None, ctypes.c_uint64(0), nout, ws, ctypes.c_size_t(ws_bytes))


def test_dev_sample_guards_without_a_device(so):
    nout = ctypes.c_uint64(123)
    ref = ctypes.byref(nout)
    assert dev_sample(so, 10, 0, 0.5, None) == ERR_INVALID            # no h_nout
    assert dev_sample(so, 10, 0, 1.5, ref) == ERR_INVALID             # fraction > 1 + 1e-6
    assert nout.value == 0
    assert dev_sample(so, 10, 0, -0.1, ref) == ERR_INVALID
    assert dev_sample(so, 10, 0, float("nan"), ref) == ERR_INVALID
    assert dev_sample(so, 10, 1, -0.1, ref) == ERR_INVALID            # Poisson mean < 0
    assert dev_sample(so, 10, 1, float("nan"), ref) == ERR_INVALID
    assert dev_sample(so, 10, 1, 16.5, ref) == ERR_UNSUPPORTED        # mean > 16
    assert dev_sample(so, 1 << 32, 0, 0.5, ref) == ERR_UNSUPPORTED    # per-call row limit
    assert dev_sample(so, 0, 0, 0.5, ref) == 0 and nout.value == 0    # empty input
    assert dev_sample(so, 0, 1, 2.0, ref) == 0 and nout.value == 0
    assert dev_sample(so, 10, 0, 0.5, ref) == ERR_INVALID             # null rows
    buf = (ctypes.c_int64 * 10)()
    assert dev_sample(so, 10, 0, 0.5, ref, keys=buf, vals=buf) == ERR_NOMEM  # no workspace
    assert dev_sample(so, 10, 0, 0.5, ref, ws=buf, ws_bytes=80, keys=buf, vals=buf) == ERR_NOMEM
