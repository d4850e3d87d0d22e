"""The normal equations of a regression in one pass (fmhip_cross_moments) against the product-by-product path of the same estimator
(FMHIP_DEVICE_CROSS_MOMENTS=0): µs per getLinearRegressionParameters call for K = 3, 6, 12 basis functions (the constant among them) plus
one dependent at several path counts, the kernel launches per call, the bytes the one-pass call must read at least over its wall time, and
the Bermudan driver with 10 exercise dates at 10^6 paths both ways.
Method: every figure is the median of `--repeats` calls after `--warmup` calls, wall clock around the call (the call returns when the
coefficients are on the host); launches from pool_stats().n_kernel_launches around one call.  Writes one JSON document (default: stdout).

    python benchmarks/regression.py --sizes 100000,1000000,10000000 --out profiles/regression.json
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
    ap.add_argument("--sizes", default="100000,1000000,10000000")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=15)
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
        for K in (3, 6, 12):
            basis = [f.createRandomVariable(1.0)] + [f.createRandomVariable(0.0, rng.standard_normal(n, dtype=np.float32)) for _ in range(K - 1)]
            dep = f.createRandomVariable(0.0, rng.standard_normal(n, dtype=np.float32))
            est = fm.MonteCarloConditionalExpectationRegression(basis)
            row = {}
            for knob, label in (("1", "one_pass"), ("0", "product_by_product")):
                os.environ["FMHIP_DEVICE_CROSS_MOMENTS"] = knob
                us = median_us(lambda: est.getLinearRegressionParameters(dep), args.warmup, args.repeats)
                before = fm.pool_stats().n_kernel_launches
                est.getLinearRegressionParameters(dep)
                row[label] = {"us": us, "launches": fm.pool_stats().n_kernel_launches - before}
            os.environ["FMHIP_DEVICE_CROSS_MOMENTS"] = "1"
            row["bytes_read_once"] = 4 * n * K                  # K - 1 basis vectors and the dependent; the constant is not loaded
            row["one_pass_gb_per_s_lower_bound"] = 4.0 * n * K / (row["one_pass"]["us"] * 1e-6) / 1e9        # launch, round trip and solve are in the time
            per[f"K={K}"] = row
            del basis, dep, est
        doc["sizes"][str(n)] = per
    dates = [0.2 * k for k in range(1, 11)]
    bm = fm.BrownianMotionHip(fm.TimeDiscretization(0.0, 10, 0.2), 1, 1_000_000, 31415)
    berm = {}
    for knob, label in (("1", "one_pass"), ("0", "product_by_product")):
        os.environ["FMHIP_DEVICE_CROSS_MOMENTS"] = knob
        us = median_us(lambda: mc.bermudan_option_mc(bm, 1.0, 0.05, 0.30, dates, 1.05), 2, 7)
        before = fm.pool_stats().n_kernel_launches
        value, _ = mc.bermudan_option_mc(bm, 1.0, 0.05, 0.30, dates, 1.05)
        berm[label] = {"us": us, "launches": fm.pool_stats().n_kernel_launches - before, "value": value}
    os.environ["FMHIP_DEVICE_CROSS_MOMENTS"] = "1"
    doc["bermudan_10_dates_1M_paths"] = berm
    text = json.dumps(doc, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
