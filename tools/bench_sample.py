#!/usr/bin/env python3
"""Time the device-side samplers against the only device route to a thinned
rdd that existed before them: filter(KEY_MOD_EQ) at the same selectivity
(not random, and it reads every row twice).

Not part of the bench.py contract. One GPU, uniform (i64, i64) rows generated
on the device. Measured, each as the median of --steps calls after --warmup,
timed to a context synchronize:
  sample(False, f) for f in 1e-4, 0.01, 0.5      sample(True, 1.0)
  random_split([1, 2, 3])                        take_sample(False, 1000)
  filter(KEY_MOD_EQ, p0, 0) for p0 in 10000, 100, 2   (the same selectivities)
Per-kernel milliseconds come from set_profiling / kernel_stats of one extra
profiled call. The byte model of DESIGN.md "Sampling" is evaluated next to
each kernel time.

Every GPU step runs under a time limit of its own. The tool sets none itself:
wrap each invocation in `timeout`, sized to what it runs.

Usage (GPU box):
  timeout -k 10 400 python tools/bench_sample.py --rows 1000000000 \\
      --out profiles/sample_1e9.json
  timeout -k 10 120 python tools/bench_sample.py --rows 100000000 --ops sample_0.01,filter_mod_100
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ACHIEVABLE_TBPS = 6.3  # achievable HBM bandwidth on one MI355X
OP_NAMES = ["sample_0.0001", "sample_0.01", "sample_0.5", "sample_repl_1.0",
            "random_split_1_2_3", "take_sample_1000",
            "filter_mod_10000", "filter_mod_100", "filter_mod_2"]
SAME_SELECTIVITY = {"sample_0.0001": "filter_mod_10000", "sample_0.01": "filter_mod_100",
                    "sample_0.5": "filter_mod_2"}


def sectors_read_model(n, f, sector=64):
    """expected bytes the emit pass reads: memory requests of `sector` bytes
    that hold >= 1 kept row (sector/8 rows each), for the key and the value
    column. 64 B is the unit the fetch counter tallies; a wide stream is
    served in 128-B requests, so the 128-B figure is the upper model."""
    rows = sector / 8.0
    return 2 * sector * (n / rows) * (1.0 - (1.0 - f) ** rows)


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
        out_rows = {}

        def sample_step(name, repl, f):
            def step():
                s = rdd.sample(repl, f, 12345)
                ctx.synchronize()
                out_rows[name] = s.count()
                s.free()
            return step

        def filter_step(name, p0):
            def step():
                s = rdd.filter(gpu.PRED_KEY_MOD_EQ, p0, 0)
                ctx.synchronize()
                out_rows[name] = s.count()
                s.free()
            return step

        def split_step():
            parts = rdd.random_split([1, 2, 3], 12345)
            ctx.synchronize()
            out_rows["random_split_1_2_3"] = sum(p.count() for p in parts)
            for p in parts:
                p.free()

        def take_step():
            k, _ = rdd.take_sample(False, 1000, 12345)
            out_rows["take_sample_1000"] = len(k)

        ops = [
            ("sample_0.0001", sample_step("sample_0.0001", False, 1e-4)),
            ("sample_0.01", sample_step("sample_0.01", False, 0.01)),
            ("sample_0.5", sample_step("sample_0.5", False, 0.5)),
            ("sample_repl_1.0", sample_step("sample_repl_1.0", True, 1.0)),
            ("random_split_1_2_3", split_step),
            ("take_sample_1000", take_step),
            ("filter_mod_10000", filter_step("filter_mod_10000", 10000)),
            ("filter_mod_100", filter_step("filter_mod_100", 100)),
            ("filter_mod_2", filter_step("filter_mod_2", 2)),
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
                "ms_max": times[-1],
                "ms_all": times,
                "out_rows": out_rows.get(name),
                "kernels": kernels,
            }
            print(f"{name:<20} median {times[len(times) // 2]:9.3f} ms  "
                  f"min {times[0]:9.3f}  max {times[-1]:9.3f}  rows {out_rows.get(name)}  "
                  f"kernels {json.dumps(kernels)}", flush=True)
        rdd.free()

    o = result["ops"]
    model = {}
    for name, f in (("sample_0.0001", 1e-4), ("sample_0.01", 0.01), ("sample_0.5", 0.5)):
        if name not in o:
            continue
        rows_out = o[name]["out_rows"] or 0
        emit_bytes = sectors_read_model(n, f) + 16.0 * rows_out
        k = o[name]["kernels"]
        m = {"count_bytes": 0.0, "emit_bytes_model": emit_bytes,
             "emit_bytes_model_128B": sectors_read_model(n, f, 128) + 16.0 * rows_out,
             "filter_bytes_model": 32.0 * n + 16.0 * rows_out}
        if "sample_emit" in k and k["sample_emit"]["ms"] > 0:
            m["emit_tbps_model"] = emit_bytes / (k["sample_emit"]["ms"] * 1e-3) / 1e12
        if "sample_count" in k:
            # one 8 B/row pass at the achievable bandwidth, the yardstick for the count
            m["one_8B_pass_ms_at_achievable"] = 8.0 * n / (ACHIEVABLE_TBPS * 1e12) * 1e3
            m["count_ms"] = k["sample_count"]["ms"]
        other = SAME_SELECTIVITY[name]
        if other in o:  # only a same-run filter is a fair yardstick
            m["filter_ms_median"] = o[other]["ms_median"]
            m["speedup_vs_filter"] = o[other]["ms_median"] / o[name]["ms_median"]
        model[name] = m
    if "random_split_1_2_3" in o:
        k = o["random_split_1_2_3"]["kernels"]
        nb = (n + 4095) // 4096
        b = 32.0 * n + 2 * 3 * nb * 4.0  # 16 read + 16 written + count matrix written and read
        m = {"scatter_bytes_model": b}
        if "split_scatter" in k and k["split_scatter"]["ms"] > 0:
            m["scatter_tbps_model"] = b / (k["split_scatter"]["ms"] * 1e-3) / 1e12
        model["random_split_1_2_3"] = m
    result["byte_model"] = model
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
