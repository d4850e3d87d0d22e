"""The device selection against what it is made of and what it replaces: µs per compress (1 and 8 value vectors, with
the positions beside one), per count_selected (phase 1 alone), per expand of what the compress made and per gather by its positions, at
selection shares 0.5 and 0.01, and from the same process: cumulative_sums (fmhip_prefix_sums) of the same n — the pass whose chunk
geometry this one shares —, a materialised ADD_S per value vector (equal bytes read, the streaming yardstick) and the host path
(FMHIP_DEVICE_SELECT=0: download, the definition on one core, upload).  Beside every compress its floor, the algorithmic traffic 8n (the
two reads of the mask) + 4n per value vector + 4·count per output, as TB/s reached.  Then the Bermudan driver
(montecarlo.bermudan_option_mc, 10 dates, cubic basis) with and without in_the_money_only, as time and as value.
Method: every figure is the median of `--repeats` calls after `--warmup` calls, wall clock around the call through the Python mirror; a
compress returns when the flag behind its second phase has arrived (it waits twice), the comparisons end in a device synchronise; device
and host path alternate inside one process; no tracing beside the timings and no counters (what binds a kernel is therefore SUPPOSED,
not measured).  The host path above `--host-max` paths is timed once.  Writes one JSON document (default: stdout).

    python benchmarks/selection.py --sizes 100000,10000000,67108864 --out profiles/selection.json
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
    ap.add_argument("--shares", default="0.5,0.01")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=11)
    ap.add_argument("--host-max", type=int, default=10_000_000)
    ap.add_argument("--bermudan-paths", type=int, default=1_000_000)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    fm = importlib.import_module("finmath-lib-cuda-extensions_amd")
    mc = importlib.import_module("finmath-lib-cuda-extensions_amd.montecarlo")
    fm.init(0)
    name, cus, hbm = fm.device_info()
    rng = np.random.default_rng(1)
    doc = {"device": name, "compute_units": cus,
           "method": f"median of {args.repeats} calls after {args.warmup}, wall clock per call through the Python mirror (a compress or an expand returns when the flag behind its second phase has arrived: two waits; "
                     f"the comparisons end in a synchronise), everything in one process, no tracing, no counters; host path (FMHIP_DEVICE_SELECT=0) above {args.host_max} paths: one call",
           "algorithmic_bytes": "compress: 8 n (the mask, read in both phases) + 4 n per value vector + 4 count per output; expand: 8 n + (4 count + 4 n) per vector; gather: 4 m + 8 m per vector",
           "sizes": {}}
    for n in [int(s) for s in args.sizes.split(",")]:
        per = {}
        xs = [fm.DeviceVector.from_host(rng.standard_normal(n, dtype=np.float32)) for _ in range(8)]
        base = rng.random(n, dtype=np.float32)
        for share in [float(s) for s in args.shares.split(",")]:
            mask = fm.DeviceVector.from_host((np.float32(share) - base).astype(np.float32))
            with_positions = n <= fm.selection.MAX_POSITION_N
            made, count = fm.compress(mask, xs[:1], positions=with_positions)
            short, positions = made[0], (made[1] if with_positions else None)
            calls = {"count_selected": lambda: fm.count_selected(mask),
                     "compress_1": lambda: fm.compress(mask, xs[:1]),
                     "compress_1_positions": lambda: fm.compress(mask, xs[:1], positions=True),
                     "compress_8": lambda: fm.compress(mask, xs),
                     "expand_1": lambda: fm.expand(mask, [short], fill=0.0),
                     "gather_1": lambda: fm.gather(positions, xs[:1]),
                     "gather_8": lambda: fm.gather(positions, xs)}
            if not with_positions:
                for k in ("compress_1_positions", "gather_1", "gather_8"): del calls[k]
            row = {"count": count}
            for knob, label in (("1", "device_us"), ("0", "host_path_us")):
                os.environ["FMHIP_DEVICE_SELECT"] = knob
                if knob == "0" and n > args.host_max: row[label] = {k: median_us(f, 0, 1) for k, f in calls.items()}
                else: row[label] = {k: median_us(f, args.warmup, args.repeats) for k, f in calls.items()}
            os.environ["FMHIP_DEVICE_SELECT"] = "1"
            row["cumulative_sums_us"] = median_us(lambda: (fm.cumulative_sums(mask), fm.synchronize()), args.warmup, args.repeats)
            row["add_s_1_us"] = median_us(lambda: (xs[0].v1s1("ADD_S", 1.0), fm.flush(), fm.synchronize()), args.warmup, args.repeats)
            row["add_s_8_us"] = median_us(lambda: ([x.v1s1("ADD_S", 1.0) for x in xs], fm.flush(), fm.synchronize()), args.warmup, args.repeats)
            row["add_s_tb_per_s"] = 8.0 * n / (row["add_s_1_us"] * 1e-6) / 1e12
            for call, k, outs in (("compress_1", 1, 1), ("compress_8", 8, 8)):
                floor_bytes = 8.0 * n + 4.0 * n * k + 4.0 * count * outs
                row[f"{call}_floor_bytes"] = floor_bytes
                row[f"{call}_tb_per_s"] = floor_bytes / (row["device_us"][call] * 1e-6) / 1e12
                row[f"{call}_share_of_add_s_rate"] = row[f"{call}_tb_per_s"] / row["add_s_tb_per_s"]
            per[str(share)] = row
            del mask, short, positions
        doc["sizes"][str(n)] = per
        del xs
    # the Bermudan driver of tests/test_gpu_regression.py, all paths against the in-the-money paths, alternating
    paths = args.bermudan_paths
    dates = [0.2 * k for k in range(1, 11)]
    bm = fm.BrownianMotionHip(fm.TimeDiscretization(0.0, 10, 0.2), 1, paths, 31415)
    [bm.getBrownianIncrement(t, 0) for t in range(10)]                                          # the increments exist before anything is timed
    prev = fm.set_fusion(True)
    timings, values = {False: [], True: []}, {}
    for r in range(2 + 5):
        for itm in (False, True):
            t0 = time.perf_counter(); values[itm] = mc.bermudan_option_mc(bm, 1.0, 0.05, 0.30, dates, 1.05, basis_order=3, in_the_money_only=itm)[0]; dt = (time.perf_counter() - t0) * 1e3
            if r >= 2: timings[itm].append(dt)
    os.environ["FMHIP_DEVICE_SELECT"] = "0"
    t0 = time.perf_counter(); host_value = mc.bermudan_option_mc(bm, 1.0, 0.05, 0.30, dates, 1.05, basis_order=3, in_the_money_only=True)[0]; host_ms = (time.perf_counter() - t0) * 1e3
    os.environ["FMHIP_DEVICE_SELECT"] = "1"
    fm.set_fusion(prev)
    doc["bermudan_put"] = {"paths": paths, "dates": 10, "basis_order": 3, "tree": 0.153540, "method": "median of 5 runs after 2, alternating; host path: one run",
                           "all_paths_ms": statistics.median(timings[False]), "all_paths_value": values[False],
                           "in_the_money_only_ms": statistics.median(timings[True]), "in_the_money_only_value": values[True],
                           "in_the_money_only_host_path_ms": host_ms, "same_bits_with_the_knob_off": host_value == values[True]}
    text = json.dumps(doc, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
