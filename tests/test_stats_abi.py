"""CPU-side ABI checks for stats_by_key: the four entries are declared in
include/vega_gpu.h and exported by libvega_gpu.so, vega_stat_t agrees with the
Python constants, and the Python surface exists. No compute calls."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "vega_gpu.h")
SO = os.path.join(ROOT, "vega_amd", "csrc", "libvega_gpu.so")

STATS_SYMBOLS = ["vega_gpu_stats_by_key", "vega_gpu_collect_stats",
                 "vega_gpu_stats_column", "vega_dev_sort_stats_i64"]


@pytest.fixture(scope="module")
def header():
    with open(HDR) as f:
        return f.read()


def test_stats_symbols_declared(header):
    # the header's style: "int vega_xxx(" at a line start (what test_abi.py reads)
    declared = re.findall(r"^int\s+(vega_\w+)\s*\(", header, flags=re.M)
    assert [s for s in STATS_SYMBOLS if s not in declared] == []


def test_stats_symbols_exported():
    so = ctypes.CDLL(SO)
    assert [s for s in STATS_SYMBOLS if not hasattr(so, s)] == []


def test_stat_enum_matches_python(header):
    from vega_amd import gpu
    m = re.search(r"typedef enum \{([^}]*)\}\s*vega_stat_t;", header)
    assert m, "vega_stat_t not found"
    vals = dict((name, int(v)) for name, v in re.findall(r"(VEGA_STAT_\w+)\s*=\s*(\d+)", m.group(1)))
    assert vals == {"VEGA_STAT_COUNT": gpu.STAT_COUNT, "VEGA_STAT_SUM": gpu.STAT_SUM,
                    "VEGA_STAT_MIN": gpu.STAT_MIN, "VEGA_STAT_MAX": gpu.STAT_MAX}
    assert (gpu.STAT_COUNT, gpu.STAT_SUM, gpu.STAT_MIN, gpu.STAT_MAX) == (0, 1, 2, 3)


def test_python_surface():
    from vega_amd import gpu
    assert callable(gpu.Rdd.stats_by_key)
    assert callable(gpu.dev_sort_stats)
    for name in ("collect", "column", "count", "free"):
        assert callable(getattr(gpu.StatsRdd, name))
