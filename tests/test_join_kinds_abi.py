"""CPU-side ABI checks for the join family: the three entries are declared in
include/vega_gpu.h and exported by libvega_gpu.so, the header's enum values
equal the Python constants, the Python surface exists, and the argument guards
of vega_dev_join_grouped_kind that precede any device call return their codes.
No kernel is launched."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "vega_gpu.h")
SO = os.path.join(ROOT, "vega_amd", "csrc", "libvega_gpu.so")

SYMBOLS = ["vega_gpu_join_kind", "vega_gpu_collect_join_outer", "vega_dev_join_grouped_kind"]
OK, ERR_INVALID = 0, -1


@pytest.fixture(scope="module")
def so():
    return ctypes.CDLL(SO)


@pytest.fixture(scope="module")
def header():
    with open(HDR) as f:
        return f.read()


def test_symbols_declared(header):
    declared = re.findall(r"^int\s+(vega_\w+)\s*\(", header, flags=re.M)
    assert [s for s in SYMBOLS if s not in declared] == []


def test_symbols_exported(so):
    assert [s for s in SYMBOLS if not hasattr(so, s)] == []


def test_header_values_equal_python_constants(header):
    from vega_amd import gpu
    body = re.search(r"typedef enum \{([^}]*)\}\s*vega_join_kind_t;", header).group(1)
    enum = {n: int(v) for n, v in re.findall(r"VEGA_JOIN_(\w+)\s*=\s*(\d+)", body)}
    assert enum == {"INNER": gpu.JOIN_INNER, "LEFT_OUTER": gpu.JOIN_LEFT_OUTER,
                    "RIGHT_OUTER": gpu.JOIN_RIGHT_OUTER, "FULL_OUTER": gpu.JOIN_FULL_OUTER,
                    "LEFT_SEMI": gpu.JOIN_LEFT_SEMI, "LEFT_ANTI": gpu.JOIN_LEFT_ANTI}
    assert sorted(enum.values()) == [0, 1, 2, 3, 4, 5]
    defs = {n: int(v) for n, v in re.findall(r"^#define VEGA_JOIN_(HAS_\w+)\s+(\d+)", header,
                                             flags=re.M)}
    assert defs == {"HAS_A": gpu.JOIN_HAS_A, "HAS_B": gpu.JOIN_HAS_B} == {"HAS_A": 1, "HAS_B": 2}


def test_python_surface():
    from vega_amd import gpu
    for name in ("join_kind", "left_outer_join", "right_outer_join", "full_outer_join",
                 "semi_join", "subtract_by_key", "collect_join_outer"):
        assert callable(getattr(gpu.Rdd, name))
    assert callable(gpu.dev_join_grouped_kind)


def dev_call(so, na, nb, order_mode, kind, nout):
    return so.vega_dev_join_grouped_kind(
        None, None, None, ctypes.c_uint64(na), None, None, ctypes.c_uint64(nb),
        ctypes.c_int(order_mode), ctypes.c_int(kind), None, None, None, None,
        ctypes.c_uint64(0), nout, None, ctypes.c_size_t(0))


def test_dev_entry_guards_without_a_device(so):
    nout = ctypes.c_uint64(123)
    ref = ctypes.byref(nout)
    assert dev_call(so, 10, 10, 3, 1, ref) == ERR_INVALID      # order_mode out of range
    assert nout.value == 0
    assert dev_call(so, 10, 10, -1, 1, ref) == ERR_INVALID
    assert dev_call(so, 10, 10, 2, 4, ref) == ERR_INVALID      # semi is not a device kind
    assert dev_call(so, 10, 10, 2, -1, ref) == ERR_INVALID
    for kind in range(4):                                      # two empty sides: no rows
        nout.value = 123
        assert dev_call(so, 0, 0, 2, kind, ref) == OK and nout.value == 0
    assert dev_call(so, 0, 0, 2, 1, None) == ERR_INVALID       # no h_nout


def test_handle_entries_reject_a_null_context(so):
    out = ctypes.c_uint64(99)
    assert so.vega_gpu_join_kind(None, ctypes.c_uint64(1), ctypes.c_uint64(2), 1,
                                 ctypes.c_uint32(4), ctypes.byref(out)) == ERR_INVALID
    n = ctypes.c_uint64(0)
    assert so.vega_gpu_collect_join_outer(None, ctypes.c_uint64(1), None, None, None, None,
                                          ctypes.byref(n)) == ERR_INVALID
