#!/usr/bin/env python3
"""Constructing a Brownian motion from Sobol' points (fmhip_bm_generate_sobol_device, fm_sobol_bm_kernel), bridge and incremental, against
BrownianMotionFromMersenneRandomNumbers on the device (fm_mt_bm_kernel) in the same process.  Wall time from the constructor to the last
increment being stored on the device (a device synchronise ends the window), median of --repeat constructions after one warm-up each.

    python benchmarks/sobol.py [--paths 1000000] [--repeat 5] [--json out.json]
    rocprofv3 --kernel-trace --stats -d <dir> -- python benchmarks/sobol.py --repeat 1      # the kernels alone, in a run of its own
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--paths", type=int, default=1_000_000)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--shapes", default="40x5,200x5")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    fm = importlib.import_module("finmath-lib-cuda-extensions_amd")
    fm.init(0)
    name, cus, hbm = fm.device_info()
    rows = []
    for shape in args.shapes.split(","):
        steps, factors = (int(x) for x in shape.split("x"))
        paths = args.paths
        while 4 * steps * factors * paths > hbm // 8: paths //= 2          # the slab beside the pool
        td = fm.TimeDiscretization(0.0, steps, 0.25)
        makers = {"sobol bridge": lambda: fm.BrownianMotionFromSobolSequence(td, factors, paths, 1, "bridge"),
                  "sobol incremental": lambda: fm.BrownianMotionFromSobolSequence(td, factors, paths, 1, "incremental"),
                  "mersenne": lambda: fm.BrownianMotionFromMersenneRandomNumbers(td, factors, paths, 1)}
        for what, make in makers.items():
            times = []
            for k in range(args.repeat + 1):
                fm.synchronize()
                t0 = time.perf_counter()
                bm = make()
                bm.getBrownianIncrement(0, 0)
                fm.synchronize()
                times.append((time.perf_counter() - t0) * 1e3)
                del bm
                fm.purge()
            ms = statistics.median(times[1:])
            rows.append({"shape": f"{steps}x{factors}x{paths}", "generator": what, "median_ms": round(ms, 3), "all_ms": [round(t, 3) for t in times[1:]],
                         "stored_GB_per_second": round(4e-6 * steps * factors * paths / ms, 1)})
            print(rows[-1], flush=True)
    result = {"device": name, "compute_units": cus, "repeat": args.repeat, "rows": rows}
    if args.json:
        with open(args.json, "w") as fh: json.dump(result, fh, indent=1)
    fm.shutdown()


if __name__ == "__main__":
    main()
