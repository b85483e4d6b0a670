#!/usr/bin/env python3
"""Time the device-side actions against the only device route the ordered
answers had before them: a full sort_by_key at the same size.

Not part of the bench.py contract. One GPU, uniform (i64, i64) rows
generated on the device. For each of reduce(SUM_I64), max(),
take_ordered(10), top(1000) and sort_by_key it reports the wall time per
call (the actions synchronize internally; the sort is followed by a
context synchronize) and the per-kernel milliseconds from set_profiling /
kernel_stats of one extra profiled call.

Every GPU step runs under a time limit of its own. The tool sets none itself:
wrap each invocation in `timeout`, sized to what it runs. One invocation
with all ops keeps the sort and the actions in the same run (the committed
profiles); `--ops` runs any subset as a step of its own.

Usage (GPU box):
  timeout -k 10 400 python tools/bench_actions.py --rows 1000000000 \\
      --out profiles/actions_1e9.json
  timeout -k 10 120 python tools/bench_actions.py --ops take_ordered_10,sort_by_key
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ACHIEVABLE_TBPS = 6.3  # achievable HBM bandwidth on one MI355X
OP_NAMES = ["reduce_sum_i64", "max", "take_ordered_10", "top_1000", "sort_by_key"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=0xC0FFEE)
    ap.add_argument("--out", default="")
    ap.add_argument("--ops", default="all",
                    help="comma-separated subset of: " + ",".join(OP_NAMES))
    args = ap.parse_args()
    wanted = OP_NAMES if args.ops == "all" else args.ops.split(",")
    unknown = [o for o in wanted if o not in OP_NAMES]
    if unknown:
        ap.error(f"unknown op(s) {unknown}; choose from {OP_NAMES}")
    from vega_amd import gpu

    n = args.rows
    result = {"rows": n, "steps": args.steps, "warmup": args.warmup, "key_bits": 63,
              "ops": {}}
    with gpu.VegaContext() as ctx:
        rdd = ctx.gen_rdd_uniform(n, args.seed, key_bits=63)
        ctx.synchronize()

        def sort_step():
            s = rdd.sort_by_key()
            ctx.synchronize()
            s.free()

        ops = [
            ("reduce_sum_i64", lambda: rdd.reduce(gpu.OP_SUM_I64)),
            ("max", rdd.max),
            ("take_ordered_10", lambda: rdd.take_ordered(10)),
            ("top_1000", lambda: rdd.top(1000)),
            ("sort_by_key", sort_step),
        ]
        assert [name for name, _ in ops] == OP_NAMES
        for name, fn in ops:
            if name not in wanted:
                continue
            for _ in range(args.warmup):
                fn()
            times = []
            for _ in range(args.steps):
                t0 = time.perf_counter()
                fn()
                times.append((time.perf_counter() - t0) * 1e3)
            ctx.set_profiling(True)
            fn()
            kernels = ctx.kernel_stats()
            ctx.set_profiling(False)
            times.sort()
            result["ops"][name] = {
                "ms_median": times[len(times) // 2],
                "ms_min": times[0],
                "ms_all": times,
                "kernels": kernels,
            }
            print(f"{name:<16} median {times[len(times) // 2]:9.3f} ms  "
                  f"min {times[0]:9.3f} ms  kernels {json.dumps(kernels)}", flush=True)
        rdd.free()

    o = result["ops"]
    red_ms = o.get("reduce_sum_i64", {}).get("kernels", {}).get("col_reduce", {}).get("ms", 0.0)
    if red_ms:
        tbps = 16.0 * n / (red_ms * 1e-3) / 1e12
        result["reduce_kernel_tbps"] = tbps
        result["reduce_fraction_of_achievable"] = tbps / ACHIEVABLE_TBPS
    for name in ("take_ordered_10", "top_1000"):
        if name in o and "sort_by_key" in o:  # only a same-run sort is a fair yardstick
            result[name + "_vs_sort_speedup"] = (
                o["sort_by_key"]["ms_median"] / o[name]["ms_median"])
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
