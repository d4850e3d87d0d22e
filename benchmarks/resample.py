"""The device resampling against what it is made of and what it replaces: µs per resample call with n = m — systematic with
1 and with 8 companions, multinomial with 1, the bootstrap (no weights) with 1 — for two weight shapes (uniform-random; 99 % of the mass on
1 % of the paths), and from the same process: cumulative_sums (fmhip_prefix_sums) of the same n, a materialised ADD_S per output vector
(equal bytes written: the streaming yardstick), sort_by_key with the same companions (the only other gather the project has), and the
host path (FMHIP_DEVICE_RESAMPLE=0: download, the definition on one core, upload).  Then the filter driver
(montecarlo.particle_filter_log_likelihood) at 2^16 particles × 100 steps with the knob on and off.
Method: every figure is the median of `--repeats` calls after `--warmup` calls, wall clock around the call through the Python mirror; a
resample call returns when the flag behind its launches has arrived, the others end in a device synchronise; device and host path and the
comparisons alternate inside one process; no tracing beside the timings and no counters (what binds a kernel is therefore SUPPOSED, not
measured).  The host path above `--host-max` paths is timed once.  Writes one JSON document (default: stdout).

    python benchmarks/resample.py --sizes 100000,1000000,10000000,67108864 --out profiles/resample.json
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
    w = rng.random(n, dtype=np.float32)
    heavy = rng.random(n) < 0.01
    w[heavy] *= np.float32(99.0 * w[~heavy].sum(dtype=np.float64) / max(w[heavy].sum(dtype=np.float64), 1e-30))
    yield "concentrated", w


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
    ap.add_argument("--repeats", type=int, default=11)
    ap.add_argument("--host-max", type=int, default=1_000_000)
    ap.add_argument("--filter-particles", type=int, default=1 << 16)
    ap.add_argument("--filter-steps", type=int, default=100)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    fm = importlib.import_module("finmath-lib-cuda-extensions_amd")
    mc = importlib.import_module("finmath-lib-cuda-extensions_amd.montecarlo")
    fm.init(0)
    name, cus, hbm = fm.device_info()
    rng = np.random.default_rng(1)
    doc = {"device": name, "compute_units": cus,
           "method": f"median of {args.repeats} calls after {args.warmup}, wall clock per call through the Python mirror (a resample returns when its flag has arrived, the comparisons end in a synchronise), "
                     f"n = m, everything in one process, no tracing, no counters; host path (FMHIP_DEVICE_RESAMPLE=0) above {args.host_max} paths: one call",
           "algorithmic_bytes": "weighted: 16 n (totals read 4n, prefixes read 4n and write 8n) + per output 8 (prefix reads, counted once) + 4 (uniform, not systematic) + 8 per companion (read, write); bootstrap: 12 m",
           "sizes": {}}
    for n in [int(s) for s in args.sizes.split(",")]:
        per = {}
        xs = [fm.DeviceVector.from_host(rng.standard_normal(n, dtype=np.float32)) for _ in range(8)]
        u = fm.DeviceVector.from_host(rng.random(n, dtype=np.float32))
        for shape, a in shapes(n, rng):
            w = fm.DeviceVector.from_host(a)
            calls = {"systematic_1": lambda: fm.resample(w, xs[:1], offset=0.5),
                     "systematic_8": lambda: fm.resample(w, xs, offset=0.5),
                     "multinomial_1": lambda: fm.resample(w, xs[:1], scheme="multinomial", uniforms=u),
                     "bootstrap_1": lambda: fm.bootstrap_resample(xs[:1], u)}
            row = {}
            for knob, label in (("1", "device_us"), ("0", "host_path_us")):
                os.environ["FMHIP_DEVICE_RESAMPLE"] = knob
                if knob == "0" and n > args.host_max: row[label] = {k: median_us(f, 0, 1) for k, f in calls.items()}
                else: row[label] = {k: median_us(f, args.warmup, args.repeats) for k, f in calls.items()}
            os.environ["FMHIP_DEVICE_RESAMPLE"] = "1"
            row["cumulative_sums_us"] = median_us(lambda: (fm.cumulative_sums(w), fm.synchronize()), args.warmup, args.repeats)
            row["add_s_1_us"] = median_us(lambda: (xs[0].v1s1("ADD_S", 1.0), fm.flush(), fm.synchronize()), args.warmup, args.repeats)
            row["add_s_8_us"] = median_us(lambda: ([x.v1s1("ADD_S", 1.0) for x in xs], fm.flush(), fm.synchronize()), args.warmup, args.repeats)
            row["sort_by_key_1_us"] = median_us(lambda: (fm.sort_by_key(w, xs[:1]), fm.synchronize()), args.warmup, args.repeats)
            row["sort_by_key_8_us"] = median_us(lambda: (fm.sort_by_key(w, xs), fm.synchronize()), args.warmup, args.repeats)
            for call, nbytes in (("systematic_1", 16.0 + 8 + 8), ("systematic_8", 16.0 + 8 + 64), ("multinomial_1", 16.0 + 8 + 4 + 8), ("bootstrap_1", 12.0)):
                row[f"{call}_tb_per_s"] = nbytes * n / (row["device_us"][call] * 1e-6) / 1e12
            per[shape] = row
            del w
        doc["sizes"][str(n)] = per
        del xs, u
    # the filter driver, knob on against knob off, alternating
    steps, particles = args.filter_steps, args.filter_particles
    obs = np.random.default_rng(4).standard_normal(steps) * 0.8
    bm = fm.BrownianMotionHip(fm.TimeDiscretization(0.0, steps + 1, 1.0), 1, particles, 3141)
    [bm.getBrownianIncrement(t, 0) for t in range(steps + 1)]                                   # the increments exist before anything is timed
    run = lambda: mc.particle_filter_log_likelihood(obs, 0.9, 0.25, 0.25, 1.0, bm, 7)
    timings = {"1": [], "0": []}
    values = {}
    for r in range(2 + 5):
        for knob in ("1", "0"):
            os.environ["FMHIP_DEVICE_RESAMPLE"] = knob
            t0 = time.perf_counter(); values[knob] = run(); dt = (time.perf_counter() - t0) * 1e3
            if r >= 2: timings[knob].append(dt)
    os.environ["FMHIP_DEVICE_RESAMPLE"] = "1"
    doc["particle_filter"] = {"particles": particles, "steps": steps, "method": "median of 5 runs after 2, knob on and off alternating",
                              "device_ms": statistics.median(timings["1"]), "host_path_ms": statistics.median(timings["0"]),
                              "log_likelihood": values["1"], "same_bits": values["1"] == values["0"]}
    text = json.dumps(doc, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
