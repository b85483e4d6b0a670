"""bench.py command line: the plain run's result line, --dump-outputs
(exact, repeatable, sampled above DUMP_SAMPLE_ROWS) and --full's extra legs.
Small shapes; the dumps are checked against the CPU oracle."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_ctypes as oc
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from vega_amd import datagen

BENCH = os.path.join(ROOT, "bench.py")
SEED = 0xC0FFEE + 1          # bench.py's default --seed
SAMPLE_ROWS = 1 << 20        # bench.DUMP_SAMPLE_ROWS


def run_bench(*extra, timeout=300):
    p = subprocess.run([sys.executable, BENCH, "--gpus", "1", *map(str, extra)],
                       capture_output=True, text=True, timeout=timeout, cwd=ROOT)
    assert p.returncode == 0, p.stdout + p.stderr
    lines = [l for l in p.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


def load_dump(d):
    out = {}
    for f in sorted(os.listdir(d)):
        assert f.endswith(".npy"), f
        a = np.load(os.path.join(d, f))
        assert a.dtype == np.float64
        out[f[:-4]] = a
    return out


def i64(d, name):
    hi = d[name + "_hi"].astype(np.int64)
    lo = d[name + "_lo"].astype(np.int64)
    assert (lo >= 0).all() and (lo < 2 ** 32).all()
    return (hi << 32) | lo


def oracle_reduce(rows, key_bits):
    hk, hv = datagen.uniform_pairs(SEED, rows, key_bits=key_bits)
    ok, ov = oc.reduce_by_key_i64(hk, hv, 256, 256)
    return dict(zip(ok.tolist(), ov.tolist()))


def test_cli_options():
    p = subprocess.run([sys.executable, BENCH, "--help"], capture_output=True,
                       text=True, timeout=60)
    assert p.returncode == 0
    assert "--dump-outputs" in p.stdout and "--full" in p.stdout
    p = subprocess.run([sys.executable, BENCH, "--steps", "0"],
                       capture_output=True, text=True, timeout=60)
    assert p.returncode == 2


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    d = tmp_path_factory.mktemp("dump_small")
    rows, key_bits = 300_007, 14
    line = run_bench("--steps", 3, "--warmup", 1, "--rows", rows,
                     "--key-bits", key_bits, "--dump-outputs", d)
    return rows, key_bits, line, load_dump(d)


@pytest.mark.gpu
def test_plain_result_line(plain):
    rows, _, line, _ = plain
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in line
    assert line["steps"] == 3 and line["warmup"] == 1
    assert line["unit"] == "rows/s" and line["higher_is_better"] is True
    assert line["dtype"] == "int64"
    assert line["ms_per_step"] > 0
    # value and ms_per_step describe the same timed steps
    assert line["value"] == pytest.approx(rows / (line["ms_per_step"] / 1e3), rel=1e-2)
    # a plain run measures nothing beyond the headline figure
    assert line["roofline"] is None and line["cpu_baseline"] is None


@pytest.mark.gpu
def test_dump_matches_oracle(plain):
    rows, key_bits, line, d = plain
    assert set(d) == {"keys_hi", "keys_lo", "values_hi", "values_lo", "nout"}
    exp = oracle_reduce(rows, key_bits)
    nout = int(d["nout"][0])
    assert nout == len(exp) == line["config"]["distinct_keys_out"]
    gk, gv = i64(d, "keys"), i64(d, "values")
    assert gk.shape == gv.shape == (nout,)
    assert dict(zip(gk.tolist(), gv.tolist())) == exp


@pytest.mark.gpu
def test_dump_sampled_and_repeatable(tmp_path):
    rows = 1_500_000            # 63-bit keys: ~all distinct, nout > SAMPLE_ROWS
    dumps = []
    for name in ("a", "b"):
        d = tmp_path / name
        run_bench("--steps", 1, "--warmup", 0, "--rows", rows, "--dump-outputs", d)
        dumps.append(load_dump(d))
    a, b = dumps
    assert set(a) == set(b)
    for name in a:
        assert np.array_equal(a[name], b[name]), name
    assert sum(x.nbytes for x in a.values()) <= 64 << 20
    exp = oracle_reduce(rows, 63)
    assert int(a["nout"][0]) == len(exp) > SAMPLE_ROWS
    gk, gv = i64(a, "keys"), i64(a, "values")
    assert gk.shape == gv.shape == (SAMPLE_ROWS,)
    assert all(exp.get(k) == v for k, v in zip(gk.tolist(), gv.tolist()))


@pytest.mark.gpu
def test_full_adds_roofline_and_cpu_baseline():
    line = run_bench("--steps", 2, "--warmup", 1, "--rows", 300_007,
                     "--key-bits", 14, "--full")
    assert line["steps"] == 2 and line["ms_per_step"] > 0
    assert line["roofline"]["kernel"] == "radix_scatter"
    assert line["roofline"]["launches"] > 0
    assert line["cpu_baseline"]["value"] > 0
    assert line["cpu_baseline"]["unit"] == "rows/s"
