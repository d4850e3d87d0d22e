"""Block order statistics on the device: µs per call at n elements and blocks of 16, 64, 256, 1024 and 4096 elements for
    rank99         block_quantiles(v, block, [0.99])                        reads 4n, writes 4n/block
    tail_mean      block_quantile_expectations(v, block, [(0.0, 0.05)])     reads 4n, writes 4n/block
    block_sort     block_sort(v, block)                                     reads 4n, writes 4n
  each beside block_moments([v], block, ("mean",)) of the SAME vector and block in the same process — the pass of equal bytes read, which
  adds where these sort — and beside the same call with FMHIP_DEVICE_NESTED=0 (download, the host definition on one core, upload);
    sort_by_key    sort_by_key(v) of the whole vector, for scale (a stable radix sort of (key, path) pairs);
    margin         montecarlo.nested_initial_margin_mc (4096 outer paths, 256 inner paths): wall time per run with the knob on and off.
Method: every figure is the median of `--repeats` calls after `--warmup` calls (the host path: `--host-repeats` after one), wall clock around
a call that ends in fm.synchronize() (the side passes themselves wait for their flag); no tracing beside the timings.  Writes one JSON
document (default: stdout).

    python benchmarks/block_order.py --out profiles/block_order.json
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def median_us(f, warmup, repeats):
    for _ in range(warmup): f()
    t = []
    for _ in range(repeats):
        t0 = time.perf_counter(); f(); t.append((time.perf_counter() - t0) * 1e6)
    return statistics.median(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 26)
    ap.add_argument("--blocks", default="16,64,256,1024,4096")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--host-repeats", type=int, default=3)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--no-driver", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    fm = importlib.import_module("finmath-lib-cuda-extensions_amd")
    mc = importlib.import_module("finmath-lib-cuda-extensions_amd.montecarlo")
    fm.init(0)
    name, cus, hbm = fm.device_info()
    rng = np.random.default_rng(1)
    os.environ["FMHIP_DEVICE_NESTED"] = "1"
    doc = {"device": name, "compute_units": cus,
           "method": f"median of {args.repeats} calls after {args.warmup} (host path: {args.host_repeats} after 1), wall clock per call through the Python mirror, every call ended by fm.synchronize(), no tracing",
           "yardstick": "block_moments([v], block, ('mean',)) of the same vector and block: reads the same 4 n bytes, adds where these sort",
           "host": "the same call with FMHIP_DEVICE_NESTED=0: download, the host definition on one core, upload",
           "ratio_to_yardstick": "device_us / yardstick_us", "speedup_over_host": "host_us / device_us", "cells": [], "sort_by_key": [], "driver": []}
    n = args.n
    v = fm.DeviceVector.from_host(rng.normal(0.0, 1.0, n).astype(np.float32))
    calls = (("rank99", lambda block: fm.block_quantiles(v, block, [0.99]), lambda block: 4.0 * n + 4.0 * (n // block)),
             ("tail_mean", lambda block: fm.block_quantile_expectations(v, block, [(0.0, 0.05)]), lambda block: 4.0 * n + 4.0 * (n // block)),
             ("block_sort", lambda block: fm.block_sort(v, block), lambda block: 8.0 * n))
    for block in [int(b) for b in args.blocks.split(",")]:
        if n % block: raise SystemExit(f"{n} is no multiple of {block}")
        yardstick = lambda: (fm.block_moments([v], block, ("mean",)), fm.synchronize())
        yard = median_us(yardstick, args.warmup, args.repeats)
        for what, call, traffic in calls:
            us = median_us(lambda: (call(block), fm.synchronize()), args.warmup, args.repeats)
            cell = {"n": n, "block": block, "call": what, "device_us": us, "yardstick_us": yard,
                    "yardstick_us_after": median_us(yardstick, 1, 5),                                # the same yardstick again, behind the cell: the drift of the box
                    "ratio_to_yardstick": us / yard, "tb_per_s": traffic(block) / (us * 1e-6) / 1e12}
            if not args.no_host:
                os.environ["FMHIP_DEVICE_NESTED"] = "0"
                cell["host_us"] = median_us(lambda: (call(block), fm.synchronize()), 1, args.host_repeats)
                os.environ["FMHIP_DEVICE_NESTED"] = "1"
                cell["speedup_over_host"] = cell["host_us"] / us
            doc["cells"].append(cell)
            print(json.dumps(cell), flush=True)
    row = {"n": n, "call": "sort_by_key", "device_us": median_us(lambda: (fm.sort_by_key(v), fm.synchronize()), 1, 5)}
    doc["sort_by_key"].append(row)
    print(json.dumps(row), flush=True)
    del v
    if not args.no_driver:
        m, k = 4096, 256
        prev = fm.set_fusion(True)
        outer = fm.BrownianMotionHip(fm.TimeDiscretization(0.0, 1, 1.0), 1, m, 27182)
        inner = fm.BrownianMotionHip(fm.TimeDiscretization(1.0, 1, 0.04), 1, m * k, 1000)
        run = lambda: mc.nested_initial_margin_mc(outer, inner, 100.0, 0.05, 0.2, 1.0, 0.04, 2.0, 100.0, k, 0.99)
        for knob in ("1", "0"):
            os.environ["FMHIP_DEVICE_NESTED"] = knob
            estimate, se = run()
            row = {"driver": "nested_initial_margin_mc", "FMHIP_DEVICE_NESTED": knob, "outer_paths": m, "inner_paths": k, "run_us": median_us(lambda: (run(), fm.synchronize()), 1, 5),
                   "initial_margin": estimate, "standard_error": se}
            doc["driver"].append(row)
            print(json.dumps(row), flush=True)
        os.environ["FMHIP_DEVICE_NESTED"] = "1"
        fm.set_fusion(prev)
    text = json.dumps(doc, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text + "\n")
    else:
        print(text)


if __name__ == "__main__":
    main()
