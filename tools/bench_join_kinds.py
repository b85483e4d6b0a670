#!/usr/bin/env python3
"""Time the six join kinds next to vega_gpu_join on the same inputs.

Not part of the bench.py contract. One GPU; both sides are
datagen.uniform_range_pairs rows with keys in [0, rows) — the C4 shape — so
about 1 - 1/e of each side's rows find a partner. In one run, after warm-up,
it times join and join_kind for INNER, LEFT_OUTER, RIGHT_OUTER, FULL_OUTER,
LEFT_SEMI and LEFT_ANTI: wall time per call up to a context synchronize, the
ops taken in turn within every step so that drift hits them alike; freeing the
result is the caller's and is timed apart as free_ms. Then one further call
per op runs under set_profiling for the per-kernel milliseconds of
kernel_stats. ratio_to_join = the op's median over join's median of this run;
spread_rel = (max - min) / median and mad_rel = median absolute deviation /
median say how far to trust it.

--kinds picks the kinds and their order within a step (an op's wall time
includes allocating its result, which can depend on what was freed before it).
--inner-only times vega_gpu_join alone and needs nothing of the join-kind
surface: the same tool then measures a checkout that predates it, for the
comparison of the untouched inner path.

The tool sets no time limits itself: wrap each invocation in `timeout`, sized
to what it runs.

Usage (GPU box):
  timeout -k 10 600 python tools/bench_join_kinds.py --rows 100000000 \\
      --out profiles/join_kinds_1e8.json
  timeout -k 10 900 python tools/bench_join_kinds.py --rows 500000000 \\
      --out profiles/join_kinds_1e9.json      # 5e8 x 5e8 = 1e9 input rows
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KINDS = ["INNER", "LEFT_OUTER", "RIGHT_OUTER", "FULL_OUTER", "LEFT_SEMI", "LEFT_ANTI"]


def summarize(times):
    """median, min and two spreads of a list of ms (as tools/bench_stats.py)"""
    times = sorted(times)
    med = times[len(times) // 2]
    dev = sorted(abs(t - med) for t in times)
    return {"ms_median": med, "ms_min": times[0], "ms_all": times,
            "spread_rel": (times[-1] - times[0]) / med if med else 0.0,
            "mad_rel": dev[len(dev) // 2] / med if med else 0.0}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000, help="rows per side")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=0xC0FFEE)
    ap.add_argument("--inner-only", action="store_true",
                    help="time vega_gpu_join alone (works on a build without join_kind)")
    ap.add_argument("--kinds", default=",".join(KINDS),
                    help="comma-separated kinds, timed in this order after join")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    from vega_amd import datagen, gpu

    n = args.rows
    result = {"rows_per_side": n, "key_range": n, "steps": args.steps, "warmup": args.warmup,
              "inner_only": bool(args.inner_only), "kinds": args.kinds, "ops": {}}
    with gpu.VegaContext() as ctx:
        ak, av = datagen.uniform_range_pairs(args.seed + 3, n, n)
        a = ctx.make_rdd(ak, av, nparts=256)
        del ak, av
        bk, bv = datagen.uniform_range_pairs(args.seed + 30, n, n)
        b = ctx.make_rdd(bk, bv, nparts=256)
        del bk, bv
        ctx.synchronize()

        ops = [("join", lambda: a.join(b))]
        if not args.inner_only:
            ops += [("join_kind_" + name,
                     (lambda kind: lambda: a.join_kind(b, kind))(getattr(gpu, "JOIN_" + name)))
                    for name in args.kinds.split(",") if name]
        rows_out = {}

        def timed(name, make):
            t0 = time.perf_counter()
            res = make()
            ctx.synchronize()
            t1 = time.perf_counter()
            rows_out[name] = res.count()
            t2 = time.perf_counter()
            res.free()
            return (t1 - t0) * 1e3, (time.perf_counter() - t2) * 1e3

        for _ in range(args.warmup):
            for name, make in ops:
                timed(name, make)
        times = {name: [] for name, _ in ops}
        frees = {name: [] for name, _ in ops}
        for _ in range(args.steps):
            for name, make in ops:   # in turn within a step: drift hits all alike
                call_ms, free_ms = timed(name, make)
                times[name].append(call_ms)
                frees[name].append(free_ms)
        for name, make in ops:       # profiled apart from the timed calls
            ctx.set_profiling(True)
            timed(name, make)
            kernels = ctx.kernel_stats()
            ctx.set_profiling(False)
            entry = summarize(times[name])
            entry.update({"rows_out": rows_out[name],
                          "free_ms_median": sorted(frees[name])[len(frees[name]) // 2],
                          "kernels": kernels})
            result["ops"][name] = entry
        a.free()
        b.free()

    base = result["ops"]["join"]["ms_median"]
    for name, entry in result["ops"].items():
        entry["ratio_to_join"] = entry["ms_median"] / base if base else None
        print(f"{name:<24} median {entry['ms_median']:10.3f} ms  min {entry['ms_min']:10.3f} ms  "
              f"x{entry['ratio_to_join']:.3f} of join  rows {entry['rows_out']:>12}  "
              f"mad {entry['mad_rel']:.3f}  kernels {json.dumps(entry['kernels'])}", flush=True)
    print(json.dumps(result))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
