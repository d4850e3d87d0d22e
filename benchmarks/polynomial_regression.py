"""Polynomial regression in one pass (fmhip_polynomial_cross_moments / fmhip_polynomial_evaluate, DESIGN.md §4.15: the monomials are formed
in registers) against the materialised basis (FMHIP_DEVICE_POLYNOMIAL_MOMENTS=0: mult chains, the wide pass of §4.14, a mult / addProduct
chain — the code path there was before), for (assets, degree) = (2, 3), (3, 3), (5, 3), (8, 2) — 10, 20, 56, 45 basis functions — at
several path counts:
  - the raw pass alone from HIP events recorded on the engine's stream around one call on stored vectors (the fused call on the states; the
    wide call on the materialised monomials — which leaves their construction out, to the materialised path's advantage);
  - a whole getConditionalExpectation — basis, moments, solve, estimate, read through getAverage — on the wall clock, with launches and
    algorithmic bytes per call from the engine's counters;
  - the 9-date Bermudan max-call at 262 144 paths, one_pass_basis on and off.
Method: medians of `--repeats` calls after `--warmup`; event times: median and minimum.  Writes one JSON document (default: stdout).

    python benchmarks/polynomial_regression.py --sizes 100000,1000000,10000000 --out profiles/polynomial_regression.json
"""
import argparse
import ctypes as C
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
KNOB = "FMHIP_DEVICE_POLYNOMIAL_MOMENTS"


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
    ap.add_argument("--shapes", default="2:3,3:3,5:3,8:2")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--max-call-paths", type=int, default=1 << 18)
    ap.add_argument("--skip-max-call", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    fm = importlib.import_module("finmath-lib-cuda-extensions_amd")
    mc = importlib.import_module("finmath-lib-cuda-extensions_amd.montecarlo")
    reg = importlib.import_module("finmath-lib-cuda-extensions_amd.regression")
    fm.init(0)
    fm.set_fusion(True)
    name, cus, hbm = fm.device_info()
    ev = Events(fm)
    lib = fm._native.lib()
    rng = np.random.default_rng(1)
    f = fm.RandomVariableHipFactory()
    shapes = [tuple(int(x) for x in s.split(":")) for s in args.shapes.split(",")]
    doc = {"device": name, "compute_units": cus,
           "method": f"wall: median of {args.repeats} calls after {args.warmup}, fusion on; pass: HIP events on the engine's stream around one raw call on stored vectors, median and minimum of {args.repeats}",
           "sizes": {}}
    stats = lambda: fm.engine_stats()
    for n in [int(s) for s in args.sizes.split(",")]:
        per = {}
        for assets, degree in shapes:
            states = [f.createRandomVariable(0.0, np.exp(0.2 * rng.standard_normal(n, dtype=np.float32))) for _ in range(assets)]
            dep = f.createRandomVariable(0.0, rng.standard_normal(n, dtype=np.float32))
            table = mc.monomial_exponents(assets, degree)
            K = len(table)
            row = {"basis_functions": K}
            # the raw pass: the fused call on the states, the wide call on the stored monomials
            e = np.ascontiguousarray(table, dtype=np.uint8)
            hs = (C.c_int64 * assets)(*[v.realizations.handle for v in states])
            hy = (C.c_int64 * 1)(dep.realizations.handle)
            out = (C.c_double * (K * (K + 1) // 2 + K))()
            fused = lambda: fm._native.check(lib.fmhip_polynomial_cross_moments(hs, assets, e.ctypes.data_as(C.POINTER(C.c_uint8)), K, None, 0, hy, 1, out))
            one = f.createRandomVariable(1.0)
            basis = reg.monomial_basis(states, table, one)
            for b in basis[1:]: b.getAverage()                   # stored
            hx = (C.c_int64 * K)(*[0 if b is one else b.realizations.handle for b in basis])
            wide = lambda: fm._native.check(lib.fmhip_cross_moments_wide(hx, K, hy, 1, out))
            groups = (K + 1 + 15) // 16
            for label, call, vectors in (("fused", fused, assets + 1), ("materialised", wide, K)):
                for _ in range(args.warmup): call()
                t = [ev.us(call) for _ in range(args.repeats)]
                row[f"pass_{label}"] = {"us_median": statistics.median(t), "us_min": min(t), "bytes_read_once": 4 * n * vectors,
                                        "gb_per_s": 4 * n * vectors / (min(t) * 1e-6) / 1e9}
            row["mfma_tiles"] = groups * (groups + 1) // 2
            row["mfma_tflop_per_s_fused"] = row["mfma_tiles"] * 16 * 2048 * ((n + 63) // 64) / (row["pass_fused"]["us_min"] * 1e-6) / 1e12
            row["pass_fused_over_materialised"] = row["pass_fused"]["us_median"] / row["pass_materialised"]["us_median"]
            del basis, hx
            # a whole conditional expectation: basis + moments + solve + estimate
            est = reg.MonteCarloConditionalExpectationPolynomialRegression(states, exponents=table, one=one)
            whole = lambda: est.getConditionalExpectation(dep).getAverage()
            for knob, label in (("1", "fused"), ("0", "materialised")):
                os.environ[KNOB] = knob
                est._materialised = None                        # (the materialised basis is part of what is timed)
                def call():
                    est._materialised = None
                    return whole()
                us = median_us(call, args.warmup, args.repeats)
                before = stats()
                call()
                after = stats()
                row[f"conditional_expectation_{label}"] = {"us": us, "launches": after["kernel_launches"] - before["kernel_launches"],
                                                           "algorithmic_bytes": after["algorithmic_bytes"] - before["algorithmic_bytes"]}
            os.environ[KNOB] = "1"
            row["conditional_expectation_fused_over_materialised"] = row["conditional_expectation_fused"]["us"] / row["conditional_expectation_materialised"]["us"]
            per[f"assets={assets},degree={degree}"] = row
            del states, dep, est
            fm.purge()
        doc["sizes"][str(n)] = per
    if not args.skip_max_call:
        dates = [3.0 * k / 9 for k in range(1, 10)]
        rows = {}
        for assets, degree in shapes:
            bm = fm.BrownianMotionHip(fm.TimeDiscretization(0.0, 9, 3.0 / 9), assets, args.max_call_paths, 31415)
            row = {"basis_functions": len(mc.monomial_exponents(assets, degree)), "paths": args.max_call_paths}
            for flag, label in ((True, "fused"), (False, "materialised")):
                run = lambda: mc.bermudan_max_call_mc(bm, [100.0] * assets, 0.05, 0.10, 0.20, dates, 100.0, basis_order=degree, one_pass_basis=flag)
                us = median_us(run, 1, 5)
                before = stats()
                value, error = run()
                after = stats()
                row[label] = {"ms": us / 1e3, "launches": after["kernel_launches"] - before["kernel_launches"],
                              "algorithmic_bytes": after["algorithmic_bytes"] - before["algorithmic_bytes"], "value": value, "standard_error": error}
            row["fused_over_materialised"] = row["fused"]["ms"] / row["materialised"]["ms"]
            rows[f"assets={assets},degree={degree}"] = row
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
