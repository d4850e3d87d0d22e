"""Nested simulation on the device: block moments against the streaming reduction of the same vector, the repeat against a
materialised elementwise operation of equal bytes written, and the primal–dual Bermudan driver with the device path and with the host path:
µs per call at n elements for
    block_mean     block_moments([v], block, ("mean",))                     reads 4n, writes 4n/block
    block_all      block_moments([v], block, ("sum", "mean", "variance"))   reads 4n, writes 12n/block
  at block = 16 (several blocks per wave), 256 (one wave per block), 4096 (two segments: the second stage) and 2^20 (512 segments) — the
  largest blocks that divide n are taken (n is rounded down to a multiple of the block) —, beside DeviceVector.moments() (fmhip_reduce_moments)
  of the SAME vector in the same process: the streaming reduction, which reads the same 4n bytes;
    repeat_each    repeat_each(v, 16) to n elements                         reads n/4, writes 4n
  beside ONE materialised fmhip_call_v1s1(FMHIP_OP_ADD_S) over n elements (reads 4n, writes 4n: equal bytes written);
    bounds         montecarlo.bermudan_option_bounds_mc (10 dates, 2^16 fit paths, 4096 outer paths, 64 inner paths): wall time per run with
                   FMHIP_DEVICE_NESTED=1 and =0.
Method: every figure is the median of `--repeats` calls after `--warmup` calls, wall clock around a call that ends in fm.synchronize() (the
side passes themselves wait for their flag); no tracing beside the timings; the small sizes measure the call, not the kernel.  Writes one
JSON document (default: stdout).

    python benchmarks/nested.py --out profiles/nested.json
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
    ap.add_argument("--sizes", default="100000,10000000,67108864")
    ap.add_argument("--blocks", default="16,256,4096,1048576")
    ap.add_argument("--repeat-sizes", default="10000000,67108864")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=15)
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
           "method": f"median of {args.repeats} calls after {args.warmup}, wall clock per call through the Python mirror, every call ended by fm.synchronize(), no tracing",
           "yardstick_block_moments": "DeviceVector.moments() (fmhip_reduce_moments) of the same vector: the streaming reduction, reads 4 n bytes",
           "yardstick_repeat": "one materialised fmhip_call_v1s1(FMHIP_OP_ADD_S) over the OUTPUT's n elements: reads 4 n bytes, writes 4 n",
           "ratio": "device_us / yardstick_us", "cells": [], "repeat": [], "driver": []}
    for n0 in [int(s) for s in args.sizes.split(",")]:
        for block in [int(b) for b in args.blocks.split(",")]:
            if block > n0: continue
            n = n0 - n0 % block
            v = fm.DeviceVector.from_host(rng.normal(0.0, 1.0, n).astype(np.float32))
            yard = median_us(lambda: (v.moments(), fm.synchronize()), args.warmup, args.repeats)
            for what, outputs in (("block_mean", ("mean",)), ("block_all", ("sum", "mean", "variance"))):
                us = median_us(lambda: (fm.block_moments([v], block, outputs), fm.synchronize()), args.warmup, args.repeats)
                cell = {"n": n, "block": block, "call": what, "device_us": us, "yardstick_us": yard,
                        "yardstick_us_after": median_us(lambda: (v.moments(), fm.synchronize()), 1, 5),      # the same yardstick again, behind the cell: the drift of the box
                        "ratio_to_yardstick": us / yard, "tb_per_s": (4.0 * n + 4.0 * len(outputs) * (n // block)) / (us * 1e-6) / 1e12}
                doc["cells"].append(cell)
                print(json.dumps(cell), flush=True)
            del v
    for n in [int(s) for s in args.repeat_sizes.split(",")]:
        each = 16
        src = fm.DeviceVector.from_host(rng.normal(0.0, 1.0, n // each).astype(np.float32))
        full = fm.DeviceVector.from_host(rng.normal(0.0, 1.0, (n // each) * each).astype(np.float32))

        def yardstick():
            y = full.v1s1("ADD_S", 1.0); fm.flush(); fm.synchronize(); return y
        yard = median_us(yardstick, args.warmup, args.repeats)
        us = median_us(lambda: (fm.repeat_each(src, each), fm.synchronize()), args.warmup, args.repeats)
        row = {"n_out": (n // each) * each, "each": each, "call": "repeat_each", "device_us": us, "yardstick_us": yard, "yardstick_us_after": median_us(yardstick, 1, 5),
               "ratio_to_yardstick": us / yard, "tb_per_s_written": 4.0 * (n // each) * each / (us * 1e-6) / 1e12}
        doc["repeat"].append(row)
        print(json.dumps(row), flush=True)
        del src, full
    if not args.no_driver:
        S0, R, SIGMA, K = 1.0, 0.05, 0.30, 1.05
        dates = [0.2 * k for k in range(1, 11)]
        td = fm.TimeDiscretization(0.0, 10, 0.2)
        prev = fm.set_fusion(True)
        fit, outer = fm.BrownianMotionHip(td, 1, 1 << 16, 31415), fm.BrownianMotionHip(td, 1, 4096, 27182)
        run = lambda: mc.bermudan_option_bounds_mc(fit, outer, 64, 1000, S0, R, SIGMA, dates, K)
        for knob in ("1", "0"):
            os.environ["FMHIP_DEVICE_NESTED"] = knob
            result = run()
            row = {"driver": "bermudan_option_bounds_mc", "FMHIP_DEVICE_NESTED": knob, "fit_paths": 1 << 16, "outer_paths": 4096, "inner_paths": 64, "dates": 10,
                   "run_us": median_us(lambda: (run(), fm.synchronize()), 1, 5), **result}
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
