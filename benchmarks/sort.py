"""The device sort against the host path (FMHIP_DEVICE_SORT=0: download, numpy's stable argsort of the keys, upload) and
against the radix select it stands beside: µs per argsort, sort_by_key with 0 and 4 companions, rank_scores and sorted_quantiles at 100
levels, for three input shapes (uniform, clustered in [0.5, 2), a payoff that is half exact zeros) and several path counts; the same 100
levels through select_ranks_batch; quantile_bounds(key, 64) beside one sort and one read of the same 63 ranks; the fraction of a pass's
algorithmic traffic (20·n bytes: the count reads 4n, the scatter reads 8n and writes 8n) that argsort achieves at the largest size.
Method: every figure is the median of `--repeats` calls after `--warmup` calls, wall clock around the call through the Python mirror (the
call returns when the answer is on the host or the flag of the chain has arrived).  The host path above `--host-max` paths is timed once,
on the uniform shape only: a stable host sort of 2^26 keys takes seconds.  Writes one JSON document (default: stdout).

    python benchmarks/sort.py --sizes 100000,1000000,10000000,67108864 --out profiles/sort.json
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
    ap.add_argument("--host-max", type=int, default=10_000_000)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    fm = importlib.import_module("finmath-lib-cuda-extensions_amd")
    from importlib import import_module
    quantile_rank = import_module(fm.__name__ + ".regression").quantile_rank
    quantile_index = import_module(fm.__name__ + ".random_variable").quantile_index
    fm.init(0)
    name, cus, hbm = fm.device_info()
    rng = np.random.default_rng(1)
    doc = {"device": name, "compute_units": cus,
           "method": f"median of {args.repeats} calls after {args.warmup}, wall clock per call through the Python mirror; host path (FMHIP_DEVICE_SORT=0) above {args.host_max} paths: one call, uniform only",
           "pass_algorithmic_bytes": "20 n per pass (count reads 4n, scatter reads 8n and writes 8n), four passes", "sizes": {}}
    levels = np.linspace(0.005, 0.995, 100)
    for n in [int(s) for s in args.sizes.split(",")]:
        per = {}
        ranks63 = [quantile_rank(j, n, 64) for j in range(1, 64)]
        for shape, a in shapes(n, rng):
            key = fm.DeviceVector.from_host(a)
            comps = [fm.DeviceVector.from_host(rng.random(n, dtype=np.float32)) for _ in range(4)]
            calls = {"argsort": lambda: fm.argsort(key),
                     "sort_by_key_0": lambda: (fm.sort_by_key(key), fm.synchronize()),
                     "sort_by_key_4": lambda: (fm.sort_by_key(key, comps), fm.synchronize()),
                     "rank_scores": lambda: (fm.rank_scores(key), fm.synchronize()),
                     "sorted_quantiles_100": lambda: fm.sorted_quantiles(key, levels)}
            row = {}
            for knob, label in (("1", "device_us"), ("0", "host_path_us")):
                os.environ["FMHIP_DEVICE_SORT"] = knob
                if knob == "0" and n > args.host_max:
                    if shape != "uniform": continue
                    row[label] = {k: median_us(f, 0, 1) for k, f in calls.items()}
                else:
                    row[label] = {k: median_us(f, args.warmup, args.repeats) for k, f in calls.items()}
            os.environ["FMHIP_DEVICE_SORT"] = "1"
            # the radix select on the same commit: 100 levels (13 rounds of four launches), and the 63 bounds of 64 bins beside one sort + one read
            r100 = [quantile_index(n, float(q)) for q in levels]
            row["select_ranks_batch_100_us"] = median_us(lambda: fm.select_ranks_batch([key], r100), args.warmup, args.repeats)
            row["quantile_bounds_64_us"] = median_us(lambda: fm.quantile_bounds(key, 64), args.warmup, args.repeats)
            row["sort_and_read_63_ranks_us"] = median_us(lambda: fm.read_elements(fm.sort_by_key(key)[0], ranks63), args.warmup, args.repeats)
            # argsort = four passes + the permutation's way down (4n bytes over the host link, 8n written on the host); sort_by_key_0 = four
            # passes + a gather (12n): the passes' share of either is below the whole, so these fractions are lower bounds
            for call in ("sort_by_key_0", "rank_scores"):
                row[f"{call}_gb_per_s_of_80n"] = 80.0 * n / (row["device_us"][call] * 1e-6) / 1e9
            per[shape] = row
            del key, comps
        worst = max(per, key=lambda s: per[s]["device_us"]["sort_by_key_0"])
        per["worst_shape_over_uniform_sort_by_key_0"] = {"shape": worst, "ratio": per[worst]["device_us"]["sort_by_key_0"] / per["uniform"]["device_us"]["sort_by_key_0"]}
        doc["sizes"][str(n)] = per
    text = json.dumps(doc, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
