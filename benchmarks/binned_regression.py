"""The binned cross moments of a localized regression (fmhip_binned_cross_moments) against the yardstick of equal bytes — fmhip_cross_moments
over the same number of loaded vectors — and against the knob-off path of the same estimator (FMHIP_DEVICE_BINNED_MOMENTS=0: indicators by
choose, averages pair by pair): µs per call through the Python mirror for 16 and 64 bins, n_x = 1, 2, 3 (the constant among them from
n_x = 2 on) and one dependent at several path counts; the piecewise evaluation; the cost of the quantile bounds; and the Bermudan driver
with 10 exercise dates at 10^6 paths, bins=16 / basis_order=1 against the global basis_order=5, values beside the tree's.
Method: every figure is the median of `--repeats` calls after `--warmup` calls, wall clock around the call (a call returns when its sums
are on the host); launches from pool_stats().n_kernel_launches around one call.  Kernel times come from a run of their own:
    rocprofv3 --kernel-trace --stats -- python benchmarks/binned_regression.py --sizes 10000000 --skip-generic --skip-bermudan
Writes one JSON document (default: stdout).

    python benchmarks/binned_regression.py --out profiles/binned_regression.json
"""
import argparse
import importlib
import json
import math
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

S0, R, SIGMA, T, K = 1.0, 0.05, 0.30, 2.0, 1.05


def median_us(f, warmup, repeats):
    for _ in range(warmup): f()
    t = []
    for _ in range(repeats):
        t0 = time.perf_counter(); f(); t.append((time.perf_counter() - t0) * 1e6)
    return statistics.median(t)


def crr_bermudan_put(dates, steps_per_date=200):
    n_steps = steps_per_date * len(dates)
    dt = T / n_steps
    u = math.exp(SIGMA * math.sqrt(dt)); d = 1.0 / u
    p = (math.exp(R * dt) - d) / (u - d); disc = math.exp(-R * dt)
    j = np.arange(n_steps + 1)
    v = np.maximum(K - S0 * u ** (2.0 * j - n_steps), 0.0)
    for step in range(n_steps - 1, -1, -1):
        j = np.arange(step + 1)
        v = disc * (p * v[1:] + (1.0 - p) * v[:-1])
        if step > 0 and step % steps_per_date == 0:
            v = np.maximum(v, K - S0 * u ** (2.0 * j - step))
    return float(v[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="100000,1000000,10000000")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--skip-generic", action="store_true")
    ap.add_argument("--skip-bermudan", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    fm = importlib.import_module("finmath-lib-cuda-extensions_amd")
    mc = importlib.import_module("finmath-lib-cuda-extensions_amd.montecarlo")
    fm.init(0)
    fm.set_fusion(True)
    name, cus, hbm = fm.device_info()
    rng = np.random.default_rng(1)
    f = fm.RandomVariableHipFactory()
    doc = {"device": name, "compute_units": cus, "method": f"median of {args.repeats} calls after {args.warmup}, wall clock per call, fusion on", "sizes": {}}
    for n in [int(s) for s in args.sizes.split(",")]:
        per = {}
        key = f.createRandomVariable(0.0, rng.standard_normal(n, dtype=np.float32))
        dep = f.createRandomVariable(0.0, rng.standard_normal(n, dtype=np.float32))
        for bins in (16, 64):
            t_bounds = median_us(lambda: fm.quantile_bounds(key, bins), 1, 5)
            before = fm.pool_stats().n_kernel_launches
            bounds = fm.quantile_bounds(key, bins)
            bounds_launches = fm.pool_stats().n_kernel_launches - before
            for n_x in (1, 2, 3):
                vectors = [f.createRandomVariable(0.0, rng.standard_normal(n, dtype=np.float32)) for _ in range(max(n_x - 1, 1))]
                xs = vectors if n_x == 1 else [None] + vectors
                loaded = len(vectors) + 2                               # the x vectors, the key and the dependent
                row = {"loaded_vectors": loaded, "bytes_read_once": 4 * n * loaded}
                row["binned_us"] = median_us(lambda: fm.binned_cross_moments(key, bounds, xs, [dep]), args.warmup, args.repeats)
                before = fm.pool_stats().n_kernel_launches
                fm.binned_cross_moments(key, bounds, xs, [dep])
                row["binned_launches"] = fm.pool_stats().n_kernel_launches - before
                # the yardstick: the global cross moments over as many loaded vectors (the key stands in as one more x)
                row["cross_moments_equal_bytes_us"] = median_us(lambda: fm.cross_moments(xs + [key], [dep]), args.warmup, args.repeats)
                row["ratio_to_cross_moments"] = row["binned_us"] / row["cross_moments_equal_bytes_us"]
                coefficients = np.ones((bins, n_x))
                row["evaluate_us"] = median_us(lambda: (fm.binned_evaluate(key, bounds, xs, coefficients), fm.synchronize()), args.warmup, args.repeats)
                basis = [f.createRandomVariable(1.0)] + vectors if n_x > 1 else vectors
                est = fm.MonteCarloConditionalExpectationLocalizedRegression(key, bins, basis, bounds=bounds)
                row["estimator_parameters_us"] = median_us(lambda: est.getLinearRegressionParameters(dep), args.warmup, args.repeats)
                if not args.skip_generic and n <= 1_000_000:
                    os.environ["FMHIP_DEVICE_BINNED_MOMENTS"] = "0"
                    generic = fm.MonteCarloConditionalExpectationLocalizedRegression(key, bins, basis, bounds=bounds)
                    row["knob_off_parameters_us"] = median_us(lambda: generic.getLinearRegressionParameters(dep), 1, 3)
                    before = fm.pool_stats().n_kernel_launches
                    generic.getLinearRegressionParameters(dep)
                    row["knob_off_launches"] = fm.pool_stats().n_kernel_launches - before
                    os.environ["FMHIP_DEVICE_BINNED_MOMENTS"] = "1"
                    del generic
                per[f"bins={bins},n_x={n_x}"] = row
                del vectors, xs, basis, est
            per[f"bins={bins},quantile_bounds"] = {"us": t_bounds, "launches": bounds_launches}
        doc["sizes"][str(n)] = per
        del key, dep
    if not args.skip_bermudan:
        dates = [0.2 * k for k in range(1, 11)]
        bm = fm.BrownianMotionHip(fm.TimeDiscretization(0.0, 10, 0.2), 1, 1_000_000, 31415)
        berm = {"tree": crr_bermudan_put(dates)}
        for label, kw in (("global_basis_order_5", dict(basis_order=5)), ("bins_16_basis_order_1", dict(basis_order=1, bins=16)), ("bins_32_basis_order_1", dict(basis_order=1, bins=32))):
            us = median_us(lambda: mc.bermudan_option_mc(bm, S0, R, SIGMA, dates, K, **kw), 2, 7)
            before = fm.pool_stats().n_kernel_launches
            value, _ = mc.bermudan_option_mc(bm, S0, R, SIGMA, dates, K, **kw)
            berm[label] = {"us": us, "launches": fm.pool_stats().n_kernel_launches - before, "value": value, "distance_to_tree": abs(value - berm["tree"])}
        doc["bermudan_10_dates_1M_paths"] = berm
    text = json.dumps(doc, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
