"""Order statistics on the device against the host sort (FMHIP_DEVICE_ORDER_STATS=0): µs per getQuantile, getQuantileExpectation and a
20-point getHistogram for four input shapes (uniform, clustered in [0.5, 2), a payoff that is half exact zeros, a constant) and several
path counts; the 200-vector exposure profile as one batched call; the bandwidth of one radix-select pass at the largest size.
Method: every figure is the median of `--repeats` calls after `--warmup` calls, wall clock around the call (the call returns when the
answer is on the host).  Writes one JSON document (default: stdout).

    python benchmarks/order_statistics.py --sizes 100000,1000000,10000000,67108864 --out profiles/order_statistics.json
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


def shapes(n, rng):
    yield "uniform", rng.random(n, dtype=np.float32)
    yield "clustered", np.clip(np.exp(0.3 * rng.standard_normal(n, dtype=np.float32)), 0.5, 1.999).astype(np.float32)
    yield "half_zeros", np.maximum(rng.standard_normal(n, dtype=np.float32), 0.0)
    yield "constant", np.full(n, 1.25, dtype=np.float32)


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
    ap.add_argument("--host-repeats", type=int, default=3)
    ap.add_argument("--host-max", type=int, default=10_000_000)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    fm = importlib.import_module("finmath-lib-cuda-extensions_amd")
    fm.init(0)
    name, cus, hbm = fm.device_info()
    rng = np.random.default_rng(1)
    doc = {"device": name, "compute_units": cus, "method": f"median of {args.repeats} calls after {args.warmup} (host sort: {args.host_repeats} after 1), wall clock per call", "sizes": {}}
    points = np.linspace(-2.0, 2.5, 20)
    for n in [int(s) for s in args.sizes.split(",")]:
        per = {}
        for shape, a in shapes(n, rng):
            x = fm.RandomVariableHipFactory().createRandomVariable(0.0, a)
            row = {}
            for knob, label, w, r in (("1", "device_us", args.warmup, args.repeats), ("0", "host_sort_us", 1, args.host_repeats)):
                if knob == "0" and n > args.host_max: continue        # (a host sort of 2^26 floats takes seconds: not repeated for every shape)
                os.environ["FMHIP_DEVICE_ORDER_STATS"] = knob
                row[label] = {"getQuantile": median_us(lambda: x.getQuantile(0.05), w, r),
                              "getQuantileExpectation": median_us(lambda: x.getQuantileExpectation(0.0, 0.05), w, r),
                              "getHistogram20": median_us(lambda: x.getHistogram(points), w, r)}
            os.environ["FMHIP_DEVICE_ORDER_STATS"] = "1"
            # one pass: the first pass of a select reads the vector once (4 bytes per element)
            t4 = median_us(lambda: x.realizations.select_ranks([n // 2]), args.warmup, args.repeats)
            row["select_us"] = t4
            row["pass_gb_per_s_lower_bound"] = 4.0 * n / (t4 / 4.0 * 1e-6) / 1e9      # four passes and their round trips in t4: a lower bound per pass
            per[shape] = row
            del x
        doc["sizes"][str(n)] = per
    n, count = 1_000_000, 200
    vs = [fm.DeviceVector.from_host(np.maximum(rng.standard_normal(n, dtype=np.float32) + 0.01 * k, 0.0)) for k in range(count)]
    doc["profile_200_vectors_1M_paths_us"] = {"batched": median_us(lambda: fm.quantiles(vs, 0.95), 2, 7),
                                               "one_by_one": median_us(lambda: [v.select_ranks([n // 20]) for v in vs], 1, 3)}
    text = json.dumps(doc, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
