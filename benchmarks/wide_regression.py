"""The normal equations of a regression on more than 12 basis functions in one pass on the matrix cores (fmhip_cross_moments_wide, DESIGN.md
§4.14) against the product-by-product path of the same estimator (FMHIP_DEVICE_WIDE_MOMENTS=0, what the estimator did before the wide pass
existed): µs per getLinearRegressionParameters call for K = 13, 20, 40, 56 basis functions (the constant among them) plus one dependent at
several path counts, and the kernel launches per call.
Beside the wall clock, a time of the pass alone from HIP events recorded on the engine's stream around one raw fmhip_cross_moments_wide call on
stored vectors: the launch sits between the two events, together with the few µs the host needs between recording the first and launching
(argument checks, the pinned block), so at small sizes it is an upper bound of the kernel time.  From it: the bytes the call must read at
least over that time, and the MFMA FLOP (16 v_mfma_f64_16x16x4_f64 of 2048 FLOP per 64-path chunk and tile, padding included) over it.
Then the Bermudan max-call (Andersen–Broadie's contract: S0 = K = 100, r = 5 %, δ = 10 %, σ = 20 %, T = 3, 9 exercise dates) for 2, 3 and 5
assets, all monomials up to degree 3 (10, 20, 56 basis functions), both ways on the same paths.
Method: medians of `--repeats` calls after `--warmup` (knob off: `--generic-repeats`), wall clock around the call; event times: median and
minimum.  Writes one JSON document (default: stdout).

    python benchmarks/wide_regression.py --sizes 100000,1000000,10000000 --out profiles/wide_regression.json
"""
import argparse
import ctypes as C
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


class Events:
    """hipEventRecord on the engine's stream before and after a call that launches on it and waits for its results."""
    def __init__(self, fm):
        self.hip = C.CDLL("libamdhip64.so")
        self.stream = C.c_void_p()
        fm._native.check(fm._native.lib().fmhip_get_stream(C.byref(self.stream)))
        self.a, self.b = C.c_void_p(), C.c_void_p()
        assert self.hip.hipEventCreate(C.byref(self.a)) == 0 and self.hip.hipEventCreate(C.byref(self.b)) == 0

    def us(self, f):
        assert self.hip.hipEventRecord(self.a, self.stream) == 0
        f()
        assert self.hip.hipEventRecord(self.b, self.stream) == 0
        assert self.hip.hipEventSynchronize(self.b) == 0
        ms = C.c_float()
        assert self.hip.hipEventElapsedTime(C.byref(ms), self.a, self.b) == 0
        return ms.value * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="100000,1000000,10000000")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--generic-repeats", type=int, default=5)
    ap.add_argument("--max-call-paths", type=int, default=1 << 18)
    ap.add_argument("--skip-max-call", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    fm = importlib.import_module("finmath-lib-cuda-extensions_amd")
    mc = importlib.import_module("finmath-lib-cuda-extensions_amd.montecarlo")
    fm.init(0)
    fm.set_fusion(True)
    name, cus, hbm = fm.device_info()
    ev = Events(fm)
    lib = fm._native.lib()
    rng = np.random.default_rng(1)
    f = fm.RandomVariableHipFactory()
    doc = {"device": name, "compute_units": cus,
           "method": f"wall: median of {args.repeats} calls after {args.warmup} (knob off: {args.generic_repeats} after 1), fusion on; pass: HIP events on the engine's stream around one raw call, median and minimum of {args.repeats}",
           "sizes": {}}
    Ks = (13, 20, 40, 56)
    for n in [int(s) for s in args.sizes.split(",")]:
        vectors = [f.createRandomVariable(0.0, rng.standard_normal(n, dtype=np.float32)) for _ in range(max(Ks) - 1)]
        dep = f.createRandomVariable(0.0, rng.standard_normal(n, dtype=np.float32))
        per = {}
        for K in Ks:
            basis = [f.createRandomVariable(1.0)] + vectors[:K - 1]
            est = fm.MonteCarloConditionalExpectationRegression(basis)
            row = {}
            for knob, label, warm, rep in (("1", "one_pass", args.warmup, args.repeats), ("0", "product_by_product", 1, args.generic_repeats)):
                os.environ["FMHIP_DEVICE_WIDE_MOMENTS"] = knob
                us = median_us(lambda: est.getLinearRegressionParameters(dep), warm, rep)
                before = fm.pool_stats().n_kernel_launches
                est.getLinearRegressionParameters(dep)
                row[label] = {"us": us, "launches": fm.pool_stats().n_kernel_launches - before}
            os.environ["FMHIP_DEVICE_WIDE_MOMENTS"] = "1"
            row["one_pass_over_product_by_product"] = row["one_pass"]["us"] / row["product_by_product"]["us"]
            hx = (C.c_int64 * K)(0, *[v.realizations.handle for v in vectors[:K - 1]])
            hy = (C.c_int64 * 1)(dep.realizations.handle)
            out = (C.c_double * (K * (K + 1) // 2 + K))()
            call = lambda: fm._native.check(lib.fmhip_cross_moments_wide(hx, K, hy, 1, out))
            for _ in range(args.warmup): call()
            t = [ev.us(call) for _ in range(args.repeats)]
            groups = (K + 1 + 15) // 16
            flop = groups * (groups + 1) // 2 * 16 * 2048 * ((n + 63) // 64)
            row["pass_us_median"], row["pass_us_min"] = statistics.median(t), min(t)
            row["bytes_read_once"] = 4 * n * K                  # K - 1 basis vectors and the dependent; the constant is not loaded
            row["gb_per_s"] = row["bytes_read_once"] / (row["pass_us_min"] * 1e-6) / 1e9
            row["mfma_tflop_per_s"] = flop / (row["pass_us_min"] * 1e-6) / 1e12
            row["mfma_tiles"] = groups * (groups + 1) // 2
            per[f"K={K}"] = row
            del basis, est
        doc["sizes"][str(n)] = per
        del vectors, dep
        fm.purge()
    if not args.skip_max_call:
        dates = [3.0 * k / 9 for k in range(1, 10)]
        rows = {}
        for assets in (2, 3, 5):
            bm = fm.BrownianMotionHip(fm.TimeDiscretization(0.0, 9, 3.0 / 9), assets, args.max_call_paths, 31415)
            run = lambda: mc.bermudan_max_call_mc(bm, [100.0] * assets, 0.05, 0.10, 0.20, dates, 100.0, basis_order=3)
            row = {"basis_functions": len(mc.monomial_exponents(assets, 3)), "paths": args.max_call_paths}
            for knob, label in (("1", "one_pass"), ("0", "product_by_product")):
                os.environ["FMHIP_DEVICE_WIDE_MOMENTS"] = knob
                us = median_us(run, 1, 3)
                before = fm.pool_stats().n_kernel_launches
                value, error = run()
                row[label] = {"ms": us / 1e3, "launches": fm.pool_stats().n_kernel_launches - before, "value": value, "standard_error": error}
            os.environ["FMHIP_DEVICE_WIDE_MOMENTS"] = "1"
            rows[f"assets={assets}"] = row
            del bm
            fm.purge()
        doc["bermudan_max_call_9_dates"] = rows
    text = json.dumps(doc, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
