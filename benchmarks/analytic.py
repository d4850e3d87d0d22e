"""Named functions and option formulas on the device against a yardstick of equal bytes, against the host path and — for Φ —
against a 1024-knot monotone-cubic table: µs per call at n paths for
    cdf            function_apply(x, [Φ])                                   reads 4n, writes 4n
    cdf_density    function_apply(x, [Φ, φ])                                reads 4n, writes 8n
    quantile       function_apply(u, [Φ⁻¹]), u uniform over (0, 1)          reads 4n, writes 4n
    bs_value       Black–Scholes value, forward a vector, σ and N scalars   reads 4n, writes 4n
    bs_all         value + delta + vega, forward, σ and N vectors           reads 12n, writes 12n
Beside every figure stands the yardstick of the same process and the same x: ONE materialised fmhip_call_v1s1(FMHIP_OP_ADD_S) — it reads 4n
bytes and writes 4n — and the ratio to it scaled by the bytes (a call that moves B bytes has the traffic floor of B / 8n yardsticks).  The
host path (FMHIP_DEVICE_ANALYTIC=0: download, the definition on one core, upload) is timed for every call.  The conditional Heston driver
stands beside heston_call_mc per run and per unit of variance.
Method: every figure is the median of `--repeats` calls after `--warmup` calls, wall clock around a call that ends in fm.synchronize() (the
call itself returns once the launch is enqueued); no tracing beside the timings; the small sizes measure the call, not the kernel.  The host
path above `--host-max` paths is timed once.  Writes one JSON document (default: stdout).

    python benchmarks/analytic.py --sizes 100000,1000000,10000000,67108864 --out profiles/analytic.json
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
    ap.add_argument("--sizes", default="100000,1000000,10000000,67108864")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--host-max", type=int, default=1_000_000)
    ap.add_argument("--no-host-path", action="store_true", help="leave the FMHIP_DEVICE_ANALYTIC=0 timings out (a run under a kernel trace)")
    ap.add_argument("--no-drivers", action="store_true", help="leave the Heston drivers out")
    ap.add_argument("--driver-paths", type=int, default=1 << 20)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    fm = importlib.import_module("finmath-lib-cuda-extensions_amd")
    mc = importlib.import_module("finmath-lib-cuda-extensions_amd.montecarlo")
    fm.init(0)
    name, cus, hbm = fm.device_info()
    rng = np.random.default_rng(1)
    doc = {"device": name, "compute_units": cus,
           "method": f"median of {args.repeats} calls after {args.warmup}, wall clock per call through the Python mirror, every call ended by fm.synchronize(), no tracing; "
                     f"host path (FMHIP_DEVICE_ANALYTIC=0) above {args.host_max} paths: one call",
           "yardstick": "one materialised fmhip_call_v1s1(FMHIP_OP_ADD_S): reads 4 n bytes, writes 4 n",
           "ratio": "device_us / (yardstick_us * bytes / 8n): 1.0 = the time the yardstick needs for the same bytes",
           "cells": [], "drivers": []}
    knots = np.linspace(-8.0, 8.0, 1024)
    table = fm.TabulatedFunction(knots, [fm.NORMAL_CDF(k) for k in knots], "monotone_cubic", "constant")
    for n in [int(s) for s in args.sizes.split(",")]:
        x = fm.DeviceVector.from_host(rng.normal(0.0, 2.0, n).astype(np.float32))
        u = fm.DeviceVector.from_host(rng.uniform(0.0, 1.0, n).astype(np.float32).clip(1e-7, 1.0 - 1e-7))
        F = fm.RandomVariableHip(0.0, fm.DeviceVector.from_host(rng.uniform(50.0, 150.0, n).astype(np.float32)))
        S = fm.RandomVariableHip(0.0, fm.DeviceVector.from_host(rng.uniform(0.05, 0.6, n).astype(np.float32)))
        U = fm.RandomVariableHip(0.0, fm.DeviceVector.from_host(rng.uniform(0.5, 1.5, n).astype(np.float32)))
        os.environ["FMHIP_DEVICE_ANALYTIC"] = "1"

        def yardstick():
            y = x.v1s1("ADD_S", 1.0); fm.flush(); fm.synchronize(); return y
        calls = {
            "cdf": (8, lambda: (fm.function_apply(x, [fm.NORMAL_CDF]), fm.synchronize())),
            "cdf_density": (12, lambda: (fm.function_apply(x, [fm.NORMAL_CDF, fm.NORMAL_DENSITY]), fm.synchronize())),
            "quantile": (8, lambda: (fm.function_apply(u, [fm.NORMAL_QUANTILE]), fm.synchronize())),
            "bs_value": (8, lambda: (fm.option_formula("black_scholes", F, 0.3, 1.5, 100.0, 0.9), fm.synchronize())),
            "bs_all": (24, lambda: (fm.option_formula("black_scholes", F, S, 1.5, 100.0, U, ("value", "delta", "vega")), fm.synchronize())),
            "cdf_table_1024_monotone_cubic": (8, lambda: (fm.table_apply(x, [table]), fm.synchronize())),
        }
        yard = median_us(yardstick, args.warmup, args.repeats)
        for what, (bytes_per_path, call) in calls.items():
            cell = {"n": n, "call": what, "bytes_per_path": bytes_per_path, "yardstick_us": yard}
            os.environ["FMHIP_DEVICE_ANALYTIC"] = "1"
            cell["device_us"] = median_us(call, args.warmup, args.repeats)
            cell["yardstick_us_after"] = median_us(yardstick, 1, 5)          # the same yardstick again, behind the cell: the drift of the box
            cell["ratio_to_yardstick_of_equal_bytes"] = cell["device_us"] / (yard * bytes_per_path / 8.0)
            cell["fraction_of_streaming_rate"] = 1.0 / cell["ratio_to_yardstick_of_equal_bytes"]
            cell["tb_per_s"] = float(bytes_per_path) * n / (cell["device_us"] * 1e-6) / 1e12
            cell["elements_per_ns"] = n / (cell["device_us"] * 1e3)
            if not args.no_host_path and not what.startswith("cdf_table"):
                os.environ["FMHIP_DEVICE_ANALYTIC"] = "0"
                cell["host_path_us"] = median_us(call, 0, 1) if n > args.host_max else median_us(call, 1, 5)
                os.environ["FMHIP_DEVICE_ANALYTIC"] = "1"
            doc["cells"].append(cell)
            print(json.dumps(cell), flush=True)
        del x, u, F, S, U
    if not args.no_drivers:
        parameters = (100.0, 0.05, 0.04, 1.5, 0.04, 0.5, -0.7, 1.0, 100.0)
        paths, steps = args.driver_paths, 50
        td = fm.TimeDiscretization(0.0, steps, 1.0 / steps)

        def conditional(seed=271828):
            value, vector = mc.heston_call_conditional_mc(fm.BrownianMotionHip(td, 1, paths, seed), *parameters)
            return value, vector.getStandardError()

        def plain(seed=31415):
            value, vector = mc.heston_call_mc(fm.BrownianMotionHip(td, 2, paths, seed), *parameters)
            return value, vector.getStandardError()
        for what, run in (("heston_call_conditional_mc", conditional), ("heston_call_mc", plain)):
            value, err = run()
            us = median_us(lambda: (run(), fm.synchronize()), 1, 5)
            row = {"driver": what, "paths": paths, "steps": steps, "value": value, "standard_error": err, "run_us": us, "us_times_variance": us * err * err}
            doc["drivers"].append(row)
            print(json.dumps(row), flush=True)
        # ξ = 0 with ρ = −0.7: the law is Black–Scholes at σ² = θ whatever ρ — the estimator against the closed form at this many paths
        value, vector = mc.heston_call_conditional_mc(fm.BrownianMotionHip(td, 1, paths, 99), 100.0, 0.05, 0.04, 1.5, 0.04, 0.0, -0.7, 1.0, 100.0)
        row = {"driver": "heston_call_conditional_mc, xi = 0, rho = -0.7", "paths": paths, "value": value, "standard_error": vector.getStandardError(),
               "black_scholes": mc.black_scholes_call_analytic(100.0, 0.05, 0.2, 1.0, 100.0)}
        doc["drivers"].append(row)
        print(json.dumps(row), flush=True)
    text = json.dumps(doc, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text + "\n")
    else:
        print(text)


if __name__ == "__main__":
    main()
