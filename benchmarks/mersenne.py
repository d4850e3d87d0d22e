#!/usr/bin/env python3
"""Constructing finmath's Mersenne-Twister Brownian motion: host path (one core draws, the vectors are uploaded) against device path
(fmhip_bm_generate_mersenne_device).  Wall time from the constructor to the last increment being stored on the device, median of
`--repeat` constructions, at 40 x 5 x {10^5, 10^6} and 2 x 1 x 10^7; with --stores also the device path with element-wise stores
(FMHIP_MT_TILE=0) and, with --segments, at forced segment lengths (FMHIP_MT_SEGMENT_LOG2; one workgroup = no prologue).
Prints one JSON line.  Kernel time: run this under `rocprofv3 --kernel-trace --stats -- python benchmarks/mersenne.py --device-only`."""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def construct(fm, shape, seed):
    steps, factors, paths = shape
    td = fm.TimeDiscretization(0.0, steps, 0.25)
    t0 = time.perf_counter()
    bm = fm.BrownianMotionFromMersenneRandomNumbers(td, factors, paths, seed)
    last = bm.getBrownianIncrement(steps - 1, factors - 1)
    fm.synchronize() if hasattr(fm, "synchronize") else last.realizations.to_float32()[:1]
    return time.perf_counter() - t0


def median(fm, shape, repeat, env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        construct(fm, shape, 1)                                      # warm-up: code objects, pool
        return statistics.median(construct(fm, shape, 2 + i) for i in range(repeat))
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--device-only", action="store_true")
    ap.add_argument("--stores", action="store_true")
    ap.add_argument("--segments", action="store_true")
    a = ap.parse_args()
    fm = importlib.import_module("finmath-lib-cuda-extensions_amd")
    fm.init(0)
    out = {"device": fm.device_info()[0], "rows": []}
    for shape in ((40, 5, 100_000), (40, 5, 1_000_000), (2, 1, 10_000_000)):
        row = {"steps": shape[0], "factors": shape[1], "paths": shape[2]}
        row["device_ms"] = 1e3 * median(fm, shape, a.repeat, {"FMHIP_DEVICE_MERSENNE": "1"})
        if not a.device_only:
            row["host_ms"] = 1e3 * median(fm, shape, max(1, a.repeat // 3), {"FMHIP_DEVICE_MERSENNE": "0"})
        if a.stores:
            row["device_elementwise_stores_ms"] = 1e3 * median(fm, shape, a.repeat, {"FMHIP_DEVICE_MERSENNE": "1", "FMHIP_MT_TILE": "0"})
        if a.segments:
            row["by_segment_log2"] = {str(j): 1e3 * median(fm, shape, a.repeat, {"FMHIP_DEVICE_MERSENNE": "1", "FMHIP_MT_SEGMENT_LOG2": str(j)}) for j in (17, 19, 21, 43)}
        out["rows"].append(row)
        fm.purge()
    print(json.dumps(out))
    fm.shutdown()


if __name__ == "__main__":
    main()
