"""CPU-side ABI checks for the f64 combiner and the f64 order ops: the new
entries are declared in include/vega_gpu.h and exported by libvega_gpu.so,
VEGA_OP_MIN_F64 / MAX_F64 agree with the Python constants, and the Python
surface exists. No compute calls."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "vega_gpu.h")
SO = os.path.join(ROOT, "vega_amd", "csrc", "libvega_gpu.so")

INT_SYMBOLS = ["vega_gpu_stats_by_key_f64", "vega_gpu_collect_stats_f64",
               "vega_dev_sort_stats_f64"]
ORDER_KEY = "vega_f64_order_key"   # returns uint64_t, not an error code


@pytest.fixture(scope="module")
def header():
    with open(HDR) as f:
        return f.read()


def test_symbols_declared(header):
    # the header's style: "int vega_xxx(" at a line start (what test_abi.py reads)
    declared = re.findall(r"^int\s+(vega_\w+)\s*\(", header, flags=re.M)
    assert [s for s in INT_SYMBOLS if s not in declared] == []
    assert re.search(r"^uint64_t\s+%s\s*\(\s*uint64_t\s+\w+\s*\)\s*;" % ORDER_KEY, header, flags=re.M)


def test_symbols_exported():
    so = ctypes.CDLL(SO)
    assert [s for s in INT_SYMBOLS + [ORDER_KEY] if not hasattr(so, s)] == []


def test_op_enum_matches_python(header):
    from vega_amd import gpu
    m = re.search(r"typedef enum \{(.*?)\}\s*vega_op_t;", header, flags=re.S)
    assert m, "vega_op_t not found"
    vals = dict((name, int(v)) for name, v in re.findall(r"(VEGA_OP_\w+)\s*=\s*(\d+)", m.group(1)))
    assert vals["VEGA_OP_MIN_F64"] == 5 and vals["VEGA_OP_MAX_F64"] == 6
    assert (gpu.OP_MIN_F64, gpu.OP_MAX_F64) == (5, 6)
    # the ops that were there keep their values
    assert vals == {"VEGA_OP_SUM_I64": gpu.OP_SUM_I64, "VEGA_OP_COUNT": gpu.OP_COUNT,
                    "VEGA_OP_SUM_F64": gpu.OP_SUM_F64, "VEGA_OP_MIN_I64": gpu.OP_MIN_I64,
                    "VEGA_OP_MAX_I64": gpu.OP_MAX_I64, "VEGA_OP_MIN_F64": gpu.OP_MIN_F64,
                    "VEGA_OP_MAX_F64": gpu.OP_MAX_F64}
    assert (gpu.OP_SUM_I64, gpu.OP_COUNT, gpu.OP_SUM_F64, gpu.OP_MIN_I64, gpu.OP_MAX_I64) \
        == (0, 1, 2, 3, 4)


def test_old_entry_still_documents_its_refusal(header):
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int vega_gpu_stats_by_key\(", header, flags=re.S)
    assert m
    text = " ".join(m.group(1).split())
    assert "values: VEGA_ERR_UNSUPPORTED" in text and "vega_gpu_stats_by_key_f64" in text


def test_python_surface():
    from vega_amd import gpu
    assert callable(gpu.Rdd.stats_by_key_f64)
    assert callable(gpu.dev_sort_stats_f64)
    assert callable(gpu.f64_order_key)
    for name in ("collect", "column", "count", "free"):
        assert callable(getattr(gpu.StatsF64Rdd, name))
