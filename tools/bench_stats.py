#!/usr/bin/env python3
"""Time stats_by_key against the four reduce_by_key calls it replaces.

Not part of the bench.py contract. One GPU, uniform (i64, i64) rows generated
on the device. For each key width it times, in the same run, stats_by_key and
reduce_by_key with SUM_I64, COUNT, MIN_I64 and MAX_I64 (wall time per call up
to a context synchronize; freeing the result is the caller's and is timed
apart as free_ms), and records the per-kernel
milliseconds from set_profiling / kernel_stats of `steps` further profiled
calls: seg_stats for the fused op, seg_emit for SUM_I64. r = keys / rows.

Two ratios per key width, both against this run's own baselines:
  whole_op_ratio    stats_by_key median / sum of the four reduce medians
  seg_kernel_ratio  seg_stats kernel ms / seg_emit (SUM_I64) kernel ms (medians)
with two spreads of the times next to them: spread_rel = (max - min) / median
and mad_rel = median absolute deviation / median, which one slow call does not
move; calls slower than 1.5 medians are listed as outliers_ms.

The handle API allocates its n-row result columns inside every call, which at
10^9 rows can cost more than the kernels. So the same five ops are also timed
through the device-pointer entries (dev_sort_stats, dev_sort_reduce) on
buffers allocated once, under "dev", with the same whole-op ratio.

The tool sets no time limits itself: wrap each invocation in `timeout`, sized
to what it runs.

Usage (GPU box):
  timeout -k 10 600 python tools/bench_stats.py --rows 1000000000 \\
      --out profiles/stats_1e9.json
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REDUCE_OPS = ["SUM_I64", "COUNT", "MIN_I64", "MAX_I64"]
OUTLIER_FACTOR = 1.5  # a call slower than this many medians is listed apart


def summarize(times):
    """median, min and two spreads of a list of ms: the range over the median
    (one slow call blows it up) and the median absolute deviation over the
    median (it does not); calls above OUTLIER_FACTOR medians are listed"""
    times = sorted(times)
    med = times[len(times) // 2]
    dev = sorted(abs(t - med) for t in times)
    return {"ms_median": med, "ms_min": times[0], "ms_all": times,
            "spread_rel": (times[-1] - times[0]) / med if med else 0.0,
            "mad_rel": dev[len(dev) // 2] / med if med else 0.0,
            "outliers_ms": [t for t in times if t > OUTLIER_FACTOR * med]}


def dev_pointer_times(gpu, n, args, bits):
    """The same five ops through the device-pointer entries, on buffers
    allocated once: the handle API allocates n-row result columns inside every
    call, and at large n that allocation can outweigh the kernels. Here a call
    is grouping sort + accumulator init + segmented pass and nothing else."""
    import torch
    k = torch.empty(n, dtype=torch.int64, device="cuda")
    v = torch.empty(n, dtype=torch.int64, device="cuda")
    gpu.dev_gen_uniform(k, v, args.seed, key_bits=bits)
    outs = [torch.empty(n, dtype=torch.int64, device="cuda") for _ in range(5)]
    ws = gpu.alloc_ws(n)
    torch.cuda.synchronize()
    ops = [("dev_sort_stats", lambda: gpu.dev_sort_stats(k, v, *outs, ws))]
    ops += [("dev_sort_reduce_" + name,
             (lambda op: lambda: gpu.dev_sort_reduce(k, v, op, outs[0], outs[1], ws))(
                 getattr(gpu, "OP_" + name)))
            for name in REDUCE_OPS]
    out = {"ops": {}}
    for name, fn in ops:
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        times = []
        for _ in range(args.steps):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
        out["ops"][name] = summarize(times)
        print(f"key_bits={bits:<3} {name:<22} median {out['ops'][name]['ms_median']:9.3f} ms  "
              f"min {min(times):9.3f} ms", flush=True)
    del ops, fn, k, v, outs, ws   # hand the buffers back before the next key width
    torch.cuda.empty_cache()
    o = out["ops"]
    four = sum(o["dev_sort_reduce_" + name]["ms_median"] for name in REDUCE_OPS)
    out["four_reduces_ms"] = four
    out["whole_op_ratio"] = o["dev_sort_stats"]["ms_median"] / four
    out["stats_over_one_reduce"] = (o["dev_sort_stats"]["ms_median"]
                                    / o["dev_sort_reduce_SUM_I64"]["ms_median"])
    out["whole_op_mad_rel"] = max(x["mad_rel"] for x in o.values())
    out["whole_op_outliers"] = sum(len(x["outliers_ms"]) for x in o.values())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=0xC0FFEE)
    ap.add_argument("--key-bits", default="63,20",
                    help="comma-separated key widths, one measurement each")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    widths = [int(b) for b in args.key_bits.split(",") if b]
    from vega_amd import gpu

    n = args.rows
    result = {"rows": n, "steps": args.steps, "warmup": args.warmup, "key_bits": {}}
    with gpu.VegaContext() as ctx:
        for bits in widths:
            rdd = ctx.gen_rdd_uniform(n, args.seed, key_bits=bits)
            ctx.synchronize()
            nkeys = [0]

            # a step returns (ms of the op up to a synchronize, ms of freeing
            # its result): the op allocates its result columns, the free is
            # the caller's and is timed apart
            def timed(make):
                t0 = time.perf_counter()
                res = make()
                ctx.synchronize()
                t1 = time.perf_counter()
                if isinstance(res, gpu.StatsRdd):
                    nkeys[0] = res.count()
                t2 = time.perf_counter()
                res.free()
                return (t1 - t0) * 1e3, (time.perf_counter() - t2) * 1e3

            def stats_step():
                return timed(rdd.stats_by_key)

            def reduce_step(op):
                return lambda: timed(lambda: rdd.reduce_by_key(op))

            ops = [("stats_by_key", stats_step)]
            ops += [("reduce_by_key_" + name, reduce_step(getattr(gpu, "OP_" + name)))
                    for name in REDUCE_OPS]
            entry = {"ops": {}}
            for name, fn in ops:
                for _ in range(args.warmup):
                    fn()
                times, frees = [], []
                for _ in range(args.steps):
                    call_ms, free_ms = fn()
                    times.append(call_ms)
                    frees.append(free_ms)
                # profiled calls, apart from the timed ones: the segmented
                # kernel's own ms per call (its spread), all kernels of the first
                seg_name = "seg_stats" if name == "stats_by_key" else "seg_emit"
                kernels, seg_ms = None, []
                for _ in range(args.steps):
                    ctx.set_profiling(True)
                    fn()
                    ks = ctx.kernel_stats()
                    ctx.set_profiling(False)
                    kernels = kernels or ks
                    seg_ms.append(ks.get(seg_name, {}).get("ms", 0.0))
                seg_ms.sort()
                seg_med = seg_ms[len(seg_ms) // 2]
                entry["ops"][name] = summarize(times)
                med = entry["ops"][name]["ms_median"]
                entry["ops"][name].update({
                    "free_ms_median": sorted(frees)[len(frees) // 2],
                    "free_ms_all": sorted(frees),
                    "seg_kernel": seg_name,
                    "seg_kernel_ms_median": seg_med,
                    "seg_kernel_ms_all": seg_ms,
                    "seg_kernel_spread_rel": (seg_ms[-1] - seg_ms[0]) / seg_med if seg_med else 0.0,
                    "kernels": kernels,
                })
                print(f"key_bits={bits:<3} {name:<22} median {med:9.3f} ms  "
                      f"min {min(times):9.3f} ms  free {entry['ops'][name]['free_ms_median']:9.3f} ms  "
                      f"kernels {json.dumps(kernels)}", flush=True)
            rdd.free()

            o = entry["ops"]
            entry["keys"] = nkeys[0]
            entry["r"] = nkeys[0] / n if n else 0.0
            four = sum(o["reduce_by_key_" + name]["ms_median"] for name in REDUCE_OPS)
            entry["four_reduces_ms"] = four
            entry["whole_op_ratio"] = o["stats_by_key"]["ms_median"] / four
            entry["stats_over_one_reduce"] = (o["stats_by_key"]["ms_median"]
                                              / o["reduce_by_key_SUM_I64"]["ms_median"])
            seg_stats = o["stats_by_key"]["seg_kernel_ms_median"]
            seg_emit = o["reduce_by_key_SUM_I64"]["seg_kernel_ms_median"]
            entry["seg_stats_ms"] = seg_stats
            entry["seg_emit_sum_i64_ms"] = seg_emit
            entry["seg_kernel_ratio"] = seg_stats / seg_emit if seg_emit else None
            entry["seg_kernel_spread_rel"] = max(
                o[name]["seg_kernel_spread_rel"]
                for name in ("stats_by_key", "reduce_by_key_SUM_I64"))
            entry["whole_op_mad_rel"] = max(v["mad_rel"] for v in o.values())
            entry["whole_op_outliers"] = sum(len(v["outliers_ms"]) for v in o.values())
            entry["dev"] = dev_pointer_times(gpu, n, args, bits)
            result["key_bits"][str(bits)] = entry

    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
