"""Tabulated functions on the device against a yardstick of equal bytes and against the host path: µs per table_apply for
n paths x m knots x {uniform, geometric (clustered)} knots x {random, sorted} x and T = 1, 2, 4 functions per call.  Beside every figure stands
the yardstick of the same process and the same x: ONE materialised fmhip_call_v1s1(FMHIP_OP_ADD_S) — it reads 4n bytes and writes 4n, what
table_apply with T = 1 moves — and the ratio to it scaled by the bytes, (1 + T)/2 yardsticks being the traffic floor of T functions.  The host
path (FMHIP_DEVICE_TABLE=0: download, the definition on one core, upload) is timed for T = 1 on random x.
Method: every figure is the median of `--repeats` calls after `--warmup` calls, wall clock around a call that ends in fm.synchronize() (the call
itself returns once the launch is enqueued); no tracing beside the timings; a call includes what the engine does per call — the tables' copy
to the device and its wait, the launch — so the small sizes measure that, not the kernel.  The host path above `--host-max` paths is timed once.
Writes one JSON document (default: stdout).

    python benchmarks/table.py --sizes 100000,1000000,10000000,67108864 --out profiles/table.json
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


def knots_of(m, family):
    i = np.arange(m, dtype=np.float64)
    return 0.5 + 1.5 * i / max(m - 1, 1) if family == "uniform" else 1e-6 * 1e12 ** (i / max(m - 1, 1))


def sample(n, K, rng):
    """uniform knots: x uniform over the range and a twentieth beyond; geometric knots: x log-uniform over the range, so that every segment is as
    likely as every other (an x uniform over [1e-6, 1e6] would sit in the last few segments)."""
    if K[-1] / K[0] > 1e3:
        return (10.0 ** rng.uniform(np.log10(K[0]) - 0.3, np.log10(K[-1]) + 0.3, n)).astype(np.float32)
    span = K[-1] - K[0]
    return rng.uniform(K[0] - 0.05 * span, K[-1] + 0.05 * span, n).astype(np.float32)


def median_us(f, warmup, repeats):
    for _ in range(warmup): f()
    t = []
    for _ in range(repeats):
        t0 = time.perf_counter(); f(); t.append((time.perf_counter() - t0) * 1e6)
    return statistics.median(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="100000,1000000,10000000,67108864")
    ap.add_argument("--knots", default="2,16,128,1024")
    ap.add_argument("--tables", default="1,2,4")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--host-max", type=int, default=1_000_000)
    ap.add_argument("--no-host-path", action="store_true", help="leave the FMHIP_DEVICE_TABLE=0 timings out (a run under a kernel trace)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    fm = importlib.import_module("finmath-lib-cuda-extensions_amd")
    fm.init(0)
    name, cus, hbm = fm.device_info()
    rng = np.random.default_rng(1)
    doc = {"device": name, "compute_units": cus,
           "method": f"median of {args.repeats} calls after {args.warmup}, wall clock per call through the Python mirror, every call ended by fm.synchronize(), no tracing; "
                     f"host path (FMHIP_DEVICE_TABLE=0), T = 1, random x, above {args.host_max} paths: one call",
           "yardstick": "one materialised fmhip_call_v1s1(FMHIP_OP_ADD_S): reads 4 n bytes, writes 4 n; table_apply reads 4 n and writes 4 n T",
           "ratio": "device_us / (yardstick_us * (1 + T) / 2): 1.0 = the time the yardstick needs for the same bytes",
           "cells": []}
    interpolation = ["linear", "cubic_spline", "monotone_cubic", "linear"]
    for n in [int(s) for s in args.sizes.split(",")]:
        for family in ("uniform", "geometric"):
            base = sample(n, knots_of(1024, family), rng)
            for order in ("random", "sorted"):
                x = fm.DeviceVector.from_host(np.sort(base) if order == "sorted" else base)
                os.environ["FMHIP_DEVICE_TABLE"] = "1"

                def yardstick():
                    y = x.v1s1("ADD_S", 1.0); fm.flush(); fm.synchronize(); return y
                yard = median_us(yardstick, args.warmup, args.repeats)
                for m in [int(s) for s in args.knots.split(",")]:
                    K = knots_of(m, family)
                    V = np.sin(3.0 * np.arange(m) / m) + 1.5
                    for T in [int(s) for s in args.tables.split(",")]:
                        if m * T > 1024: continue
                        fs = [fm.TabulatedFunction(K, V + f, interpolation[f], "constant") for f in range(T)]
                        call = lambda: (fm.table_apply(x, fs), fm.synchronize())
                        cell = {"n": n, "knots": m, "family": family, "x": order, "tables": T, "yardstick_us": yard}
                        os.environ["FMHIP_DEVICE_TABLE"] = "1"
                        cell["device_us"] = median_us(call, args.warmup, args.repeats)
                        cell["yardstick_us_after"] = median_us(yardstick, 1, 5)          # the same yardstick again, behind the cell: the drift of the box
                        cell["ratio_to_yardstick_of_equal_bytes"] = cell["device_us"] / (yard * (1 + T) / 2.0)
                        cell["tb_per_s"] = 4.0 * n * (1 + T) / (cell["device_us"] * 1e-6) / 1e12
                        if T == 1 and order == "random" and not args.no_host_path:
                            os.environ["FMHIP_DEVICE_TABLE"] = "0"
                            cell["host_path_us"] = median_us(call, 0, 1) if n > args.host_max else median_us(call, 1, 5)
                            os.environ["FMHIP_DEVICE_TABLE"] = "1"
                        doc["cells"].append(cell)
                        print(json.dumps(cell), flush=True)
                del x
    text = json.dumps(doc, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text + "\n")
    else:
        print(text)


if __name__ == "__main__":
    main()
