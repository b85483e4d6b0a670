#!/usr/bin/env python3
"""Time stats_by_key_f64 against what a per-key mean of a float column cost
before it: reduce_by_key(SUM_F64) plus reduce_by_key(COUNT), two grouping sorts.

Not part of the bench.py contract. One GPU, uniform keys, f64 values from
dev_gen_uniform_f64. Per key width, through the device-pointer entries on
buffers allocated once (a call is grouping sort + segmented pass and nothing
else), the median of `steps` calls after `warmup`:
  dev_sort_stats_f64, dev_sort_reduce with SUM_F64, COUNT, MIN_F64 and MAX_F64,
  and dev_sort_stats (i64 values, same keys) as the byte-model yardstick;
then `steps` further profiled calls of the three fused / sum ops for the
per-kernel milliseconds (seg_stats_f64, stats_f64_fold, stats_f64_combine;
seg_emit, f64_combine; seg_stats). Spreads as tools/bench_stats.py reports
them: spread_rel = (max - min) / median, mad_rel = median absolute deviation /
median.

--root TREE imports vega_amd from another checkout (the parent commit's
export, built there): entries that tree lacks are skipped, so the same script
times the baseline. --handle also times the handle API (stats_by_key_f64,
reduce_by_key SUM_F64 / COUNT; result columns allocated inside every call) on
host-generated rows, for rows <= 2 * 10^8.

--compare --new NEW.json [...] --parent PARENT.json [...] pools the calls of
the files of each side and prints the ratios the f64 section of DESIGN.md
reports:
  mean_ratio     dev_sort_stats_f64 (new) / (SUM_F64 + COUNT) (parent)
  vs_stats_i64   dev_sort_stats_f64 (new) / dev_sort_stats (parent)

The tool sets no time limits itself: wrap each invocation in `timeout`.

Usage (GPU box):
  timeout -k 10 300 python tools/bench_stats_f64.py --rows 1000000000 \\
      --out profiles/stats_f64_1e9.json
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUTLIER_FACTOR = 1.5


def summarize(times):
    times = sorted(times)
    m = len(times)
    med = times[m // 2] if m % 2 else 0.5 * (times[m // 2 - 1] + times[m // 2])
    dev = sorted(abs(t - med) for t in times)
    return {"ms_median": med, "ms_min": times[0], "ms_all": times,
            "spread_rel": (times[-1] - times[0]) / med if med else 0.0,
            "mad_rel": dev[len(dev) // 2] / med if med else 0.0,
            "outliers_ms": [t for t in times if t > OUTLIER_FACTOR * med]}


def time_calls(fn, sync, warmup, steps):
    for _ in range(warmup):
        fn()
    sync()
    times = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        sync()
        times.append((time.perf_counter() - t0) * 1e3)
    return summarize(times)


def profiled_calls(gpu, fn, sync, steps):
    """per-kernel ms of `steps` calls: {scope: sorted list of ms}"""
    per = {}
    for _ in range(steps):
        gpu.prof_stats()
        gpu.prof_enable(True)
        try:
            fn()
            sync()
            ks = gpu.prof_stats()
        finally:
            gpu.prof_enable(False)
        for name, rec in ks.items():
            per.setdefault(name, []).append(rec["ms"])
    return {name: {"ms_median": sorted(ms)[len(ms) // 2], "ms_all": sorted(ms)}
            for name, ms in per.items()}


def dev_times(gpu, n, bits, args):
    import torch
    sync = torch.cuda.synchronize
    k = torch.empty(n, dtype=torch.int64, device="cuda")
    v = torch.empty(n, dtype=torch.float64, device="cuda")
    gpu.dev_gen_uniform_f64(k, v, args.seed, key_bits=bits)
    oi = [torch.empty(n, dtype=torch.int64, device="cuda") for _ in range(2)]
    of = [torch.empty(n, dtype=torch.float64, device="cuda") for _ in range(3)]
    ws = gpu.alloc_ws(n)
    sync()
    ops = []
    if hasattr(gpu, "dev_sort_stats_f64"):
        ops.append(("dev_sort_stats_f64", lambda: gpu.dev_sort_stats_f64(k, v, *oi, *of, ws), True))
    for name in ("SUM_F64", "COUNT", "MIN_F64", "MAX_F64"):
        if not hasattr(gpu, "OP_" + name):
            continue
        op = getattr(gpu, "OP_" + name)
        out_v = oi[1] if name == "COUNT" else of[0]
        ops.append(("dev_sort_reduce_" + name,
                    (lambda op, out_v: lambda: gpu.dev_sort_reduce(k, v, op, oi[0], out_v, ws))(op, out_v),
                    name == "SUM_F64"))
    # i64 values of the same key stream: the fused i64 pass moves the same bytes
    vi = v.view(torch.int64)
    oj = [x.view(torch.int64) for x in of]
    ops.append(("dev_sort_stats_i64", lambda: gpu.dev_sort_stats(k, vi, *oi, *oj, ws), True))
    out = {"ops": {}, "kernels": {}}
    for name, fn, prof in ops:
        out["ops"][name] = time_calls(fn, sync, args.warmup, args.steps)
        if prof:
            out["kernels"][name] = profiled_calls(gpu, fn, sync, args.steps)
        o = out["ops"][name]
        print(f"key_bits={bits:<3} {name:<26} median {o['ms_median']:9.3f} ms  "
              f"min {o['ms_min']:9.3f} ms  spread {o['spread_rel']:.3f}", flush=True)
    if "dev_sort_stats_f64" in out["ops"]:
        out["keys"] = int(gpu.dev_sort_stats_f64(k, v, *oi, *of, ws))
    else:
        out["keys"] = int(gpu.dev_sort_reduce(k, v, gpu.OP_COUNT, oi[0], oi[1], ws))
    out["r"] = out["keys"] / n if n else 0.0
    o = out["ops"]
    two = o["dev_sort_reduce_SUM_F64"]["ms_median"] + o["dev_sort_reduce_COUNT"]["ms_median"]
    out["sum_plus_count_ms"] = two
    if "dev_sort_stats_f64" in o:
        out["mean_ratio_same_build"] = o["dev_sort_stats_f64"]["ms_median"] / two
        out["vs_stats_i64_same_build"] = (o["dev_sort_stats_f64"]["ms_median"]
                                          / o["dev_sort_stats_i64"]["ms_median"])
    del ops, fn, k, v, vi, oi, of, oj, ws
    torch.cuda.empty_cache()
    return out


def handle_times(gpu, n, bits, args):
    from vega_amd import datagen
    hk, hv = datagen.uniform_pairs_f64(args.seed, n, key_bits=bits)
    out = {"ops": {}}
    with gpu.VegaContext() as ctx:
        rdd = ctx.make_rdd(hk, hv)
        del hk, hv

        def run(make):
            def fn():
                make().free()
            return fn

        ops = []
        if hasattr(rdd, "stats_by_key_f64"):
            ops.append(("stats_by_key_f64", run(rdd.stats_by_key_f64)))
        ops.append(("reduce_by_key_SUM_F64", run(lambda: rdd.reduce_by_key(gpu.OP_SUM_F64))))
        ops.append(("reduce_by_key_COUNT", run(rdd.group_count)))
        for name, fn in ops:
            out["ops"][name] = time_calls(fn, ctx.synchronize, args.warmup, args.steps)
            o = out["ops"][name]
            print(f"key_bits={bits:<3} {name:<26} median {o['ms_median']:9.3f} ms  "
                  f"min {o['ms_min']:9.3f} ms  (handle API, result freed inside)", flush=True)
        rdd.free()
    o = out["ops"]
    two = o["reduce_by_key_SUM_F64"]["ms_median"] + o["reduce_by_key_COUNT"]["ms_median"]
    out["sum_plus_count_ms"] = two
    if "stats_by_key_f64" in o:
        out["mean_ratio_same_build"] = o["stats_by_key_f64"]["ms_median"] / two
    return out


def pooled(files, bits, op):
    times = []
    for path in files:
        with open(path) as f:
            d = json.load(f)
        rec = d["key_bits"].get(bits, {}).get("dev", {}).get("ops", {}).get(op)
        if rec:
            times += rec["ms_all"]
    return summarize(times) if times else None


def compare(new_files, parent_files):
    with open(new_files[0]) as f:
        first = json.load(f)
    res = {"rows": first["rows"], "new": new_files, "parent": parent_files, "key_bits": {}}
    for bits in first["key_bits"]:
        st = pooled(new_files, bits, "dev_sort_stats_f64")
        ps = pooled(parent_files, bits, "dev_sort_reduce_SUM_F64")
        pc = pooled(parent_files, bits, "dev_sort_reduce_COUNT")
        pi = pooled(parent_files, bits, "dev_sort_stats_i64")
        two = ps["ms_median"] + pc["ms_median"]
        spread = max(x["spread_rel"] for x in (st, ps, pc))
        e = {"dev_sort_stats_f64_ms": st["ms_median"], "parent_sum_f64_ms": ps["ms_median"],
             "parent_count_ms": pc["ms_median"], "parent_sum_plus_count_ms": two,
             "mean_ratio": st["ms_median"] / two, "spread_rel_max": spread,
             "mad_rel_max": max(x["mad_rel"] for x in (st, ps, pc)),
             "bar_met": st["ms_median"] < two * (1.0 - spread),
             "parent_stats_i64_ms": pi["ms_median"],
             "vs_stats_i64": st["ms_median"] / pi["ms_median"],
             "vs_stats_i64_spread_rel_max": max(st["spread_rel"], pi["spread_rel"])}
        # did the ops both builds have move?
        for op in ("dev_sort_reduce_SUM_F64", "dev_sort_reduce_COUNT", "dev_sort_stats_i64"):
            a, b = pooled(new_files, bits, op), pooled(parent_files, bits, op)
            e[op + "_new_over_parent"] = a["ms_median"] / b["ms_median"]
        res["key_bits"][bits] = e
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=0xC0FFEE)
    ap.add_argument("--key-bits", default="63,20",
                    help="comma-separated key widths, one measurement each")
    ap.add_argument("--root", default=ROOT, help="checkout whose vega_amd is timed")
    ap.add_argument("--label", default="this tree", help="name of that build in the result")
    ap.add_argument("--handle", action="store_true", help="also time the handle API")
    ap.add_argument("--compare", action="store_true",
                    help="no GPU work: compare result files given with --new and --parent")
    ap.add_argument("--new", nargs="+", metavar="JSON", default=[])
    ap.add_argument("--parent", nargs="+", metavar="JSON", default=[])
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.compare:
        if not args.new or not args.parent:
            ap.error("--compare needs --new NEW.json [...] --parent PARENT.json [...]")
        result = compare(args.new, args.parent)
    else:
        if args.steps < 1:
            ap.error("--steps must be at least 1")
        sys.path.insert(0, os.path.abspath(args.root))
        from vega_amd import gpu
        n = args.rows
        result = {"rows": n, "steps": args.steps, "warmup": args.warmup,
                  "build": args.label, "key_bits": {}}
        for bits in [int(b) for b in args.key_bits.split(",") if b]:
            entry = {"dev": dev_times(gpu, n, bits, args)}
            if args.handle and n <= 200_000_000:
                entry["handle"] = handle_times(gpu, n, bits, args)
            result["key_bits"][str(bits)] = entry
    print(json.dumps(result))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
