"""The device prefix sums against the host path (FMHIP_DEVICE_PREFIX=0: download, the definition on one core, upload), the
streaming yardstick and the sort of the same n: µs per cumulative_sums (both modes), prefix_sums_at (9 positions), prefix_search (9 relative
levels) and weighted_quantiles at 9 levels (one sort_by_key with a companion, one search, one read), for three input shapes (uniform,
magnitudes over sixteen decades, a payoff that is half exact zeros) and several path counts; sort_by_key(x, [w]) from the same run; and the
fraction of the streaming rate that the algorithmic traffic — 12·n bytes for cumulative_sums, 4·n for the two query calls — achieves.
Method: every figure is the median of `--repeats` calls after `--warmup` calls, wall clock around the call through the Python mirror (the
call returns when the answer is on the host or the flag of the chain has arrived); no tracing beside the timings.  The host path above
`--host-max` paths is timed once, on the uniform shape only.  Writes one JSON document (default: stdout).

    python benchmarks/prefix.py --sizes 100000,1000000,10000000,67108864 --out profiles/prefix.json
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

STREAM_TB_PER_S = 6.35          # what this project measures for a streaming triad on an MI355X


def shapes(n, rng):
    yield "uniform", rng.random(n, dtype=np.float32)
    yield "wide_range", (10.0 ** rng.uniform(-8.0, 8.0, n)).astype(np.float32)
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
    ap.add_argument("--host-max", type=int, default=1_000_000)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    fm = importlib.import_module("finmath-lib-cuda-extensions_amd")
    fm.init(0)
    name, cus, hbm = fm.device_info()
    rng = np.random.default_rng(1)
    doc = {"device": name, "compute_units": cus,
           "method": f"median of {args.repeats} calls after {args.warmup}, wall clock per call through the Python mirror, no tracing; host path (FMHIP_DEVICE_PREFIX=0) above {args.host_max} paths: one call, uniform only",
           "algorithmic_bytes": "cumulative_sums 12 n (totals read 4n, apply reads 4n and writes 4n); prefix_sums_at and prefix_search 4 n (and one chunk per query)",
           "stream_tb_per_s": STREAM_TB_PER_S, "sizes": {}}
    levels = np.linspace(0.1, 0.9, 9)
    for n in [int(s) for s in args.sizes.split(",")]:
        per = {}
        positions = [int(q * (n - 1)) for q in levels]
        for shape, a in shapes(n, rng):
            w = fm.DeviceVector.from_host(a)
            x = fm.DeviceVector.from_host(rng.standard_normal(n, dtype=np.float32))
            calls = {"cumulative_sums": lambda: (fm.cumulative_sums(w), fm.synchronize()),
                     "running_average": lambda: (fm.running_average(w), fm.synchronize()),
                     "prefix_sums_at_9": lambda: fm.prefix_sums_at(w, positions),
                     "prefix_search_9": lambda: fm.prefix_search(w, levels, relative=True),
                     "weighted_quantiles_9": lambda: fm.weighted_quantiles(x, w, levels)}
            row = {}
            for knob, label in (("1", "device_us"), ("0", "host_path_us")):
                os.environ["FMHIP_DEVICE_PREFIX"] = knob
                if knob == "0" and n > args.host_max:
                    if shape != "uniform": continue
                    row[label] = {k: median_us(f, 0, 1) for k, f in calls.items()}
                else:
                    row[label] = {k: median_us(f, args.warmup, args.repeats) for k, f in calls.items()}
            os.environ["FMHIP_DEVICE_PREFIX"] = "1"
            row["sort_by_key_1_us"] = median_us(lambda: (fm.sort_by_key(x, [w]), fm.synchronize()), args.warmup, args.repeats)
            for call, nbytes in (("cumulative_sums", 12.0), ("running_average", 12.0), ("prefix_sums_at_9", 4.0), ("prefix_search_9", 4.0)):
                tb = nbytes * n / (row["device_us"][call] * 1e-6) / 1e12
                row[f"{call}_tb_per_s"] = tb
                row[f"{call}_fraction_of_stream"] = tb / STREAM_TB_PER_S
            per[shape] = row
            del w, x
        doc["sizes"][str(n)] = per
    text = json.dumps(doc, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
