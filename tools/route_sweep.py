#!/usr/bin/env python3
"""Route sweep of the hash grouping sort: wall ms per vega_dev_group_rows_i64
call on uniform 63-bit keys, incl. the unpack to SoA, routes called in the
order 1, 2, 0 three times per size (1 four passes + cleanup, 2 three passes +
bucket finish, 0 automatic). The break-even between routes 1 and 2 is what
FIN_MIN_BUCKET_ROWS gates on.

Usage (GPU box): python tools/route_sweep.py --out sweep.json
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = (100_000_000, 250_000_000, 350_000_000, 400_000_000, 410_000_000,
         450_000_000, 550_000_000, 700_000_000, 1_000_000_000)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default=",".join(map(str, SIZES)))
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from vega_amd import gpu
    dev = torch.device("cuda")
    res = {"what": "vega_dev_group_rows_i64 on uniform 63-bit keys, wall ms per call incl. "
                   "the unpack to SoA; routes called in the order 1,2,0 three times per "
                   "size; taken = route_taken", "rows": {}}
    for n in map(int, args.sizes.split(",")):
        k = torch.empty(n, dtype=torch.int64, device=dev)
        v = torch.empty(n, dtype=torch.int64, device=dev)
        gpu.dev_gen_uniform(k, v, seed=1, key_bits=63)
        ok, ov = torch.empty_like(k), torch.empty_like(v)
        ws = gpu.alloc_ws(n)
        for route in (1, 2, 0):     # warm-up
            gpu.dev_group_rows(k, v, route, ok, ov, ws)
        torch.cuda.synchronize()
        row = {f"route{r}": [] for r in (1, 2, 0)}
        for _ in range(args.calls):
            for route in (1, 2, 0):
                torch.cuda.synchronize()
                t = time.perf_counter()
                taken = gpu.dev_group_rows(k, v, route, ok, ov, ws)
                torch.cuda.synchronize()
                row[f"route{route}"].append(round((time.perf_counter() - t) * 1e3, 2))
                row[f"taken{route}"] = taken
        res["rows"][str(n)] = row
        print(n, json.dumps(row), flush=True)
        del k, v, ok, ov, ws
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
