"""The kernel-weighted local moments (fmhip_kernel_moments) against their closest relative as the yardstick —
fmhip_binned_cross_moments on the same vectors with the same number of slices, in the same process: µs per call through the Python mirror
at 10^5, 10^6 and 10^7 paths, 16 / 64 / 256 points, order 0 and 1 with one dependent, bandwidths of 1.5 and 6 times the spacing of the
points (3 and 12 members per element), Epanechnikov weights; and the local-stochastic-volatility driver per time step with the device
pass and with FMHIP_DEVICE_KERNEL_MOMENTS=0.
The binned pass has at most 64 bins and 18 entries per bin, that is at most 16 slices: where the kernel pass has more (256 points at order
1: 19), the yardstick runs 16 and the ratio per slice is the figure to read.
Method: every figure is the median of `--repeats` calls after `--warmup` calls, wall clock around the call (a call returns when its sums
are on the host); launches from pool_stats().n_kernel_launches around one call.  Writes one JSON document.

    python benchmarks/kernel_regression.py --out profiles/kernel_regression.json
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

ENTRIES = 72


def median_us(f, warmup, repeats):
    for _ in range(warmup): f()
    t = []
    for _ in range(repeats):
        t0 = time.perf_counter(); f(); t.append((time.perf_counter() - t0) * 1e6)
    return statistics.median(t)


def kernel_slices(Q, order, n_y):
    qe = 1 + n_y if order == 0 else 3 + 2 * n_y
    return -(-Q // min(Q, ENTRIES // qe)), qe


def binned_shape(slices):
    """(n_bins, n_x, n_y, entries per bin, slices) of a binned call over the key and ONE other vector (named several times) with `slices`
    slices, or with the most it can have (16) if that is fewer."""
    best = None
    for n_x in (2, 3):
        for n_y in range(0, 5):
            qe = n_x * (n_x + 1) // 2 - 1 + n_x * n_y                  # the constant first: (1, 1) is the count and takes no entry
            per = ENTRIES // qe
            for n_bins in range(64, 0, -1):                            # as many bins as the slice count allows
                s = -(-n_bins // min(n_bins, per))
                if s == slices: return n_bins, n_x, n_y, qe, s
                if s < slices and (best is None or s > best[4]): best = (n_bins, n_x, n_y, qe, s)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="100000,1000000,10000000")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--skip-lsv", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kernel_regression.json"))
    args = ap.parse_args()
    fm = importlib.import_module("finmath-lib-cuda-extensions_amd")
    mc = importlib.import_module("finmath-lib-cuda-extensions_amd.montecarlo")
    fm.init(0)
    fm.set_fusion(True)
    name, cus, hbm = fm.device_info()
    rng = np.random.default_rng(1)
    f = fm.RandomVariableHipFactory()
    doc = {"device": name, "compute_units": cus, "method": f"median of {args.repeats} calls after {args.warmup}, wall clock per call, fusion on; Epanechnikov, one dependent",
           "sizes": {}}
    launches = lambda: fm.pool_stats().n_kernel_launches
    for n in [int(s) for s in args.sizes.split(",")]:
        per = {}
        key = f.createRandomVariable(0.0, rng.standard_normal(n, dtype=np.float32))
        dep = f.createRandomVariable(0.0, rng.standard_normal(n, dtype=np.float32))
        for Q in (16, 64, 256):
            points = np.linspace(-3.0, 3.0, Q)
            spacing = points[1] - points[0]
            for order in (0, 1):
                s, qe = kernel_slices(Q, order, 1)
                n_bins, n_x, n_y, bqe, bs = binned_shape(s)
                bounds = np.linspace(-3.0, 3.0, n_bins + 1)[1:-1]
                xs, ys = [None] + [dep] * (n_x - 1), [dep] * n_y
                binned_us = median_us(lambda: fm.binned_cross_moments(key, bounds, xs, ys), args.warmup, args.repeats)
                for factor in (1.5, 6.0):
                    h = factor * spacing
                    row = {"slices": s, "entries_per_point": qe, "members_per_element_inside_the_grid": 2 * factor,
                           "bytes_read": 4 * n * 2 * s}
                    row["kernel_moments_us"] = median_us(lambda: fm.kernel_moments(key, points, h, [dep], "epanechnikov", order), args.warmup, args.repeats)
                    t0 = launches(); fm.kernel_moments(key, points, h, [dep], "epanechnikov", order); row["launches"] = launches() - t0
                    row["binned"] = {"us": binned_us, "bins": n_bins, "n_x": n_x, "n_y": n_y, "entries_per_bin": bqe, "slices": bs}
                    row["ratio_to_binned"] = row["kernel_moments_us"] / binned_us
                    row["ratio_to_binned_per_slice"] = (row["kernel_moments_us"] / s) / (binned_us / bs)
                    per[f"Q={Q},order={order},h={factor}xspacing"] = row
        doc["sizes"][str(n)] = per
        del key, dep
    if not args.skip_lsv:
        lsv = {}
        surface = dict(times=[0.0], spots=[50.0, 100.0, 200.0], dupire_vols=[[0.2, 0.2, 0.2]])
        for paths in (2 ** 16, 10 ** 6):
            steps = 50
            bm = fm.BrownianMotionHip(fm.TimeDiscretization(0.0, steps, 1.0 / steps), 2, paths, 31415)
            run = lambda: mc.stochastic_local_volatility_call_mc(bm, 100.0, 0.05, **surface, v0=0.09, kappa=1.5, theta=0.04, xi=0.5, rho=-0.5, maturity=1.0, strike=100.0)
            row = {}
            for label, knob in (("device", "1"), ("knob_off", "0")):
                os.environ["FMHIP_DEVICE_KERNEL_MOMENTS"] = knob
                us = median_us(run, 1, 3 if knob == "0" else 5)
                t0 = launches(); value, se = run()
                row[label] = {"us_per_time_step": us / steps, "launches_per_time_step": (launches() - t0) / steps, "value": value, "standard_error": se}
            os.environ["FMHIP_DEVICE_KERNEL_MOMENTS"] = "1"
            row["black_scholes"] = mc.black_scholes_call_analytic(100.0, 0.05, 0.2, 1.0, 100.0)
            lsv[str(paths)] = row
            del bm
        doc["lsv_50_steps_per_time_step"] = lsv
    text = json.dumps(doc, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
