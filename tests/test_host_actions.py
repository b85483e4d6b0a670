"""C++ host mirror of the device-side actions: `vega_cli actions` runs the
reference's action goldens (tests/golden/actions.json, literals repeated in
the binary) through vega_core.hpp. On CPU boxes it must fail LOUDLY."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "vega_amd", "host")
CSRC = os.path.join(ROOT, "vega_amd", "csrc")
BIN = os.path.join(HOST, "vega_cli")


def build_cli():
    if not os.path.exists(os.path.join(CSRC, "libvega_gpu.so")):
        subprocess.check_call(
            ["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC",
             "-shared", "vega_kernels.hip", "vega_api.hip", "-o", "libvega_gpu.so"],
            cwd=CSRC)
    subprocess.check_call(
        ["g++", "-O2", "-std=c++17", "-Wall", "vega_cli.cpp", "-o", "vega_cli",
         "-L" + CSRC, "-lvega_gpu", "-Wl,-rpath,$ORIGIN/../csrc",
         "-Wl,-rpath,/opt/rocm/lib"], cwd=HOST)


def test_actions_subcommand_fails_loudly_without_gpu():
    build_cli()
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present; loud-failure leg is for CPU boxes")
    p = subprocess.run([BIN, "actions"], capture_output=True, text=True, timeout=120)
    assert p.returncode != 0
    assert "FATAL" in p.stderr or "failed" in p.stderr.lower()
    assert "actions green" not in p.stdout


def test_unknown_subcommand_is_a_usage_error():
    build_cli()
    p = subprocess.run([BIN, "no-such-subcommand"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 2
    assert "actions" in p.stderr and "selftest" in p.stderr


@pytest.mark.gpu
def test_host_actions_gpu():
    build_cli()
    p = subprocess.run([BIN, "actions"], capture_output=True, text=True, timeout=120)
    print(p.stdout, p.stderr)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "actions green" in p.stdout
