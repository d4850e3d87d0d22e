"""The device reduce-by-key against what it is made of and what it replaces: µs per group_moments call at n paths and m
groups (m capped at 2^24 and at n), with one and four value vectors, sums only and all three outputs, and from the same process:
  (a) sort_by_key(index, [v]) followed by cumulative_sums of the same n — the parts it is built from (four radix passes and a gather,
      then the plain prefix passes): a one-pass m should come in under it, a three-pass m near it;
  (b) binned_cross_moments with 16 bins and one dependent, at m = 16 only — the LDS path that already covers small m;
  (c) the host path (FMHIP_DEVICE_GROUP=0: download, the definition on one core, upload).
Method: every figure is the median of `--repeats` calls after `--warmup` calls, wall clock around the call through the Python mirror; a
group call returns when the flag behind its chain has arrived (one wait), the comparisons end in a device synchronise; device and host
path alternate inside one process; no tracing beside the timings and no counters (what binds a kernel is therefore SUPPOSED, not
measured).  The host path above `--host-max` paths is timed once.  Writes one JSON document (default: stdout).

    python benchmarks/group.py --sizes 100000,10000000,67108864 --out profiles/group.json
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
    ap.add_argument("--sizes", default="100000,10000000,67108864")
    ap.add_argument("--groups", default="16,4096,1048576,16777216")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=11)
    ap.add_argument("--host-max", type=int, default=10_000_000)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    fm = importlib.import_module("finmath-lib-cuda-extensions_amd")
    fm.init(0)
    name, cus, hbm = fm.device_info()
    rng = np.random.default_rng(1)
    doc = {"device": name, "compute_units": cus,
           "method": f"median of {args.repeats} calls after {args.warmup}, wall clock per call through the Python mirror (a group call returns when the flag behind its chain has arrived: one wait; "
                     f"the comparisons end in a synchronise), everything in one process, no tracing, no counters; host path (FMHIP_DEVICE_GROUP=0) above {args.host_max} paths: one call",
           "yardsticks": "a: sort_by_key(index, [v]) then cumulative_sums(v); b: binned_cross_moments, 16 bins, x = 1, one y (m = 16 only); c: the host path",
           "sizes": {}}
    variants = {"sum_1": (1, ("sum",)), "all_1": (1, ("sum", "mean", "variance")), "sum_4": (4, ("sum",)), "all_4": (4, ("sum", "mean", "variance"))}
    for n in [int(s) for s in args.sizes.split(",")]:
        per = {}
        xs = [fm.DeviceVector.from_host(rng.standard_normal(n, dtype=np.float32)) for _ in range(4)]
        for m in sorted({min(int(s), n, 1 << 24) for s in args.groups.split(",")}):
            index = fm.DeviceVector.from_host(rng.integers(0, m, n).astype(np.float32))
            calls = {k: (lambda k=k: fm.group_moments(index, xs[:variants[k][0]], m, what=variants[k][1], counts=True)) for k in variants}
            calls["counts"] = lambda: fm.group_counts(index, m)
            row = {"radix_passes": 1 if m <= 255 else 2 if m <= 65535 else 3 if m < (1 << 24) else 4}
            for knob, label in (("1", "device_us"), ("0", "host_path_us")):
                os.environ["FMHIP_DEVICE_GROUP"] = knob
                if knob == "0" and n > args.host_max: row[label] = {k: median_us(f, 0, 1) for k, f in calls.items() if k in ("sum_1", "all_4")}
                else: row[label] = {k: median_us(f, args.warmup, args.repeats) for k, f in calls.items()}
            os.environ["FMHIP_DEVICE_GROUP"] = "1"
            row["a_sort_by_key_then_cumulative_sums_us"] = median_us(lambda: (fm.sort_by_key(index, xs[:1]), fm.cumulative_sums(xs[0]), fm.synchronize()), args.warmup, args.repeats)
            row["sum_1_over_a"] = row["device_us"]["sum_1"] / row["a_sort_by_key_then_cumulative_sums_us"]
            if m == 16:
                bounds = np.arange(15, dtype=np.float64) + 0.5
                row["b_binned_cross_moments_us"] = median_us(lambda: (fm.binned_cross_moments(index, bounds, [None], [xs[0]]), fm.synchronize()), args.warmup, args.repeats)
                row["sum_1_over_b"] = row["device_us"]["sum_1"] / row["b_binned_cross_moments_us"]
            row["sum_1_over_c"] = row["device_us"]["sum_1"] / row["host_path_us"]["sum_1"]
            row["all_4_over_c"] = row["device_us"]["all_4"] / row["host_path_us"]["all_4"]
            per[str(m)] = row
            del index
        doc["sizes"][str(n)] = per
        del xs
    text = json.dumps(doc, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
