#!/usr/bin/env python3
"""Per-phase breakdown of k_bucket_finish (VEGA_PHASE_PROF=1).

Runs dev_group_rows(route=2) on uniform keys at --rows and prints the
s_memtime sums every wave accumulated per phase of the finish kernel, as
shares of the waves' time and as ticks per tile and wave. The instrumented
instance of the kernel is a diagnostic build: read its shares, not its length.

Usage (GPU box): VEGA_PHASE_PROF=1 python tools/finish_phase_prof.py --rows 1000000000
A run of its own: not under rocprofv3 counters or tracing.
"""
import argparse
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PHASES = ["wait+stage+hash", "bucket ordinals", "count", "scan",
          "gather+store+heads", "tail barrier+count", "place", "run fix"]
FT, WAVES = 2048, 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--names", default=",".join(PHASES),
                    help="phase names, in slot order (an older kernel's phases differ)")
    args = ap.parse_args()
    if os.environ.get("VEGA_PHASE_PROF") not in ("1", "2"):
        print("set VEGA_PHASE_PROF=1", file=sys.stderr)
        sys.exit(2)
    import torch
    from vega_amd import gpu
    n = args.rows
    dev = torch.device("cuda")
    k = torch.empty(n, dtype=torch.int64, device=dev)
    v = torch.empty(n, dtype=torch.int64, device=dev)
    gpu.dev_gen_uniform(k, v, seed=1, key_bits=63)
    ws = gpu.alloc_ws(n)
    ok = torch.empty(n, dtype=torch.int64, device=dev)
    ov = torch.empty(n, dtype=torch.int64, device=dev)
    lib = gpu.lib()
    buf = (ctypes.c_ulonglong * 8)()
    taken = gpu.dev_group_rows(k, v, 2, ok, ov, ws)  # warm-up
    torch.cuda.synchronize()
    lib.vega_fin_phase_prof_read(buf, 1)
    for _ in range(args.reps):
        taken = gpu.dev_group_rows(k, v, 2, ok, ov, ws)
    torch.cuda.synchronize()
    rc = lib.vega_fin_phase_prof_read(buf, 1)
    if rc != 0:
        print(f"vega_fin_phase_prof_read rc={rc}", file=sys.stderr)
        sys.exit(1)
    names = args.names.split(",")
    total = sum(buf[:len(names)])
    per = args.reps * ((n + FT - 1) // FT) * WAVES
    print(f"rows={n} reps={args.reps} route taken={taken} rows/bucket={n / 2**24:.1f} "
          f"total wave-ticks={total}")
    for i, name in enumerate(names):
        print(f"  {i} {name:<20} {buf[i]:>16}  {100.0 * buf[i] / max(total, 1):6.2f}%"
              f"  {buf[i] / per:8.1f} ticks/tile/wave")


if __name__ == "__main__":
    main()
