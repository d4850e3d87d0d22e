#!/usr/bin/env python3
"""Constructing increments with a law per (time step, factor): device path (fmhip_increments_generate_device) against host path
(FMHIP_DEVICE_INCREMENTS=0: fmhip_increments_host on one core, then one upload per vector).  Wall time from the constructor to the last
increment being stored on the device, median of `--repeat` constructions after one warm-up construction per path, at
    40 x 3 x 10^6   the Merton shape: Brownian increment, normal jump size, Poisson jump count (mean 0.0125 per step)
    40 x 1 x 10^6   Poisson only, for means 0.0125, 1 and 30 (the table is walked from 0 / bisected: FMHIP_ICDF_LINEAR_MAX, --search)
    40 x 5 x 10^6   all normal — beside the same shape through BrownianMotionFromMersenneRandomNumbers (fm_mt_bm_kernel) in the same run
--levy: instead, the shapes of the gamma and exponential laws (fm_mt_levy_kernel) —
    40 x 2 x 10^6   variance-gamma: gamma clock (shape dt/nu = 1.25) and standard normal
    40 x 1 x 10^6   gamma only, shapes 0.06, 1 and 30; exponential only
  and, in the same run, the Merton and all-normal shapes, which run the untouched fm_mt_icdf_kernel.  The host definition of a gamma draw
  takes about a microsecond on one core, so the host path is timed at --host-paths paths (default 10^5) and reported per draw.
Writes one JSON document (--out) with the command that made it.  Kernel time: run this under
`rocprofv3 --kernel-trace --stats -- python benchmarks/increments.py --device-only`."""
import argparse
import importlib
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def construct(fm, make, steps, factors):
    t0 = time.perf_counter()
    inc = make()
    inc.getIncrement(steps - 1, factors - 1)
    fm.synchronize()
    return time.perf_counter() - t0


def median(fm, make, steps, factors, repeat, env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        construct(fm, make, steps, factors)                          # warm-up: code objects, pool, pinned stage
        times = [construct(fm, make, steps, factors) for _ in range(repeat)]
        return 1e3 * statistics.median(times), [round(1e3 * t, 3) for t in times]
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
        fm.purge()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--paths", type=int, default=1_000_000)
    ap.add_argument("--device-only", action="store_true")
    ap.add_argument("--search", action="store_true", help="Poisson shapes also with every table bisected and every table walked from 0")
    ap.add_argument("--levy", action="store_true", help="the gamma / exponential shapes (and Merton, all-normal beside them)")
    ap.add_argument("--host-paths", type=int, default=100_000, help="--levy: paths of the host-path timing")
    ap.add_argument("--out")
    a = ap.parse_args()
    fm = importlib.import_module("finmath-lib-cuda-extensions_amd")
    fm.init(0)
    n, steps = a.paths, 40
    td = fm.TimeDiscretization(0.0, steps, 0.25)
    seeds = iter(range(1, 1 << 20))
    shapes = [("merton 40 x 3", 3, lambda: fm.merton_increments(td, n, next(seeds), 0.05))]
    for mean in (0.0125, 1.0, 30.0):
        shapes.append((f"poisson 40 x 1, mean {mean}", 1, lambda mean=mean: fm.JumpProcessIncrements(td, [mean / 0.25], n, next(seeds))))
    shapes.append(("normal 40 x 5", 5, lambda: fm.IndependentIncrementsFromICDF(td, 5, n, next(seeds), lambda i, f: fm.NormalLaw(math.sqrt(td.getTimeStep(i))))))
    if a.levy:
        gamma_only = lambda shape, paths: fm.IndependentIncrementsFromICDF(td, 1, paths, next(seeds), lambda i, f: fm.GammaLaw(shape, 0.2))
        levy = [("variance-gamma 40 x 2", 2, lambda paths=n: fm.VarianceGammaProcess(td, paths, next(seeds), 0.2, -0.14, 0.2).increments)]
        for shape in (0.06, 1.0, 30.0):
            levy.append((f"gamma 40 x 1, shape {shape}", 1, lambda paths=n, shape=shape: gamma_only(shape, paths)))
        levy.append(("exponential 40 x 1", 1, lambda paths=n: fm.IndependentIncrementsFromICDF(td, 1, paths, next(seeds), lambda i, f: fm.ExponentialLaw(2.0))))
        shapes = levy + [shapes[0], shapes[-1]]
    out = {"command": "python " + " ".join(sys.argv), "device": fm.device_info()[0], "paths": n, "repeat": a.repeat, "rows": []}
    for name, factors, make in shapes:
        row = {"shape": name, "draws": steps * factors * n}
        row["device_ms"], row["device_ms_all"] = median(fm, make, steps, factors, a.repeat, {"FMHIP_DEVICE_INCREMENTS": "1"})
        if a.levy and not a.device_only and name in [x[0] for x in shapes[:5]]:
            row["host_paths"] = a.host_paths
            ms, row["host_ms_all"] = median(fm, lambda: make(a.host_paths), steps, factors, a.repeat, {"FMHIP_DEVICE_INCREMENTS": "0"})
            row["host_ns_per_draw"] = 1e6 * ms / (steps * factors * a.host_paths)
            row["device_ns_per_draw"] = 1e6 * row["device_ms"] / row["draws"]
        elif not a.device_only:
            row["host_ms"], row["host_ms_all"] = median(fm, make, steps, factors, a.repeat, {"FMHIP_DEVICE_INCREMENTS": "0"})
            row["host_ns_per_draw"] = 1e6 * row["host_ms"] / row["draws"]
        if a.search and name.startswith("poisson"):
            row["device_bisect_ms"], _ = median(fm, make, steps, factors, a.repeat, {"FMHIP_DEVICE_INCREMENTS": "1", "FMHIP_ICDF_LINEAR_MAX": "0"})
            row["device_walk_ms"], _ = median(fm, make, steps, factors, a.repeat, {"FMHIP_DEVICE_INCREMENTS": "1", "FMHIP_ICDF_LINEAR_MAX": "512"})
        if name.startswith("normal"):                                # the Brownian kernel at the same shape, same run
            make_bm = lambda: fm.BrownianMotionFromMersenneRandomNumbers(td, 5, n, next(seeds))
            row["brownian_kernel_ms"], row["brownian_kernel_ms_all"] = median(fm, make_bm, steps, factors, a.repeat, {"FMHIP_DEVICE_MERSENNE": "1"})
        out["rows"].append(row)
        print(json.dumps(row), flush=True)
    text = json.dumps(out, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    fm.shutdown()


if __name__ == "__main__":
    main()
