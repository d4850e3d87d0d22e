"""Implied volatility per path on the device beside the forward formula on the same shapes, a yardstick of equal bytes and
the host path: µs per call at n paths, for both models, for
    price          implied_volatility(price, F, …), the price the only vector, mask 1 (volatility)          reads 4n, writes 4n
    price_all      the same with mask 7 (volatility, ∂/∂price, ∂/∂forward)                                   reads 4n, writes 12n
    three          price, forward and payoff unit vectors, mask 1                                            reads 12n, writes 4n
    three_all      the same with mask 7                                                                      reads 12n, writes 12n
The inputs are prices made by option_formula from volatilities uniform in [0.05, 0.8] (times the strike under Bachelier) at moneyness 0.5
to 2.  Beside every figure stand, from the same process: option_formula's VALUE on the same operand shapes (forward_us), its ratio
(inverse_over_forward — one forward value is two Φ evaluations and one log under Black–Scholes, one Φ and one φ under Bachelier), ONE
materialised fmhip_call_v1s1(FMHIP_OP_ADD_S) of n elements (the yardstick: reads 4n, writes 4n) and the host path (FMHIP_DEVICE_ANALYTIC=0:
download, the definition on one core, upload).  A device time worse than the host path's is flagged in the row ("slower_than_host_path").
The driver montecarlo.forward_implied_volatility_mc (4096 outer x 256 inner paths, 10 + 10 steps, three moneynesses) is timed per run with
FMHIP_DEVICE_ANALYTIC and FMHIP_DEVICE_NESTED on and with both off, its numbers beside the times.
Method (benchmarks/analytic.py's): every figure is the median of `--repeats` calls after `--warmup` calls, wall clock around a call that ends
in fm.synchronize(); no tracing; the small sizes measure the call, not the kernel.  The host path above `--host-max` paths is timed once,
and not at all above `--host-path-max-n` paths where that is given.

    python benchmarks/implied_volatility.py --sizes 100000,1000000,10000000,67108864 --out profiles/implied_volatility.json
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
    ap.add_argument("--sizes", default="100000,1000000,10000000,67108864")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--host-max", type=int, default=1_000_000)
    ap.add_argument("--no-host-path", action="store_true", help="leave the FMHIP_DEVICE_ANALYTIC=0 timings out")
    ap.add_argument("--host-path-max-n", type=int, default=0, help="time the host path only up to this many paths (0: at every size; one core needs about a microsecond per element)")
    ap.add_argument("--no-driver", action="store_true", help="leave montecarlo.forward_implied_volatility_mc out")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    fm = importlib.import_module("finmath-lib-cuda-extensions_amd")
    fm.init(0)
    name, cus, hbm = fm.device_info()
    rng = np.random.default_rng(1)
    doc = {"device": name, "compute_units": cus,
           "method": f"median of {args.repeats} calls after {args.warmup}, wall clock per call through the Python mirror, every call ended by fm.synchronize(), no tracing; "
                     f"host path (FMHIP_DEVICE_ANALYTIC=0) above {args.host_max} paths: one call",
           "yardstick": "one materialised fmhip_call_v1s1(FMHIP_OP_ADD_S): reads 4 n bytes, writes 4 n",
           "inputs": "prices made by option_formula from volatilities uniform in [0.05, 0.8] at moneyness 0.5 to 2, T = 1.5, K = 100",
           "cells": [], "driver": []}
    T, K = 1.5, 100.0
    everything = ("volatility", "d_price", "d_forward")
    for n in [int(s) for s in args.sizes.split(",")]:
        os.environ["FMHIP_DEVICE_ANALYTIC"] = "1"
        x = fm.DeviceVector.from_host(rng.normal(0.0, 2.0, n).astype(np.float32))
        F = fm.RandomVariableHip(0.0, fm.DeviceVector.from_host((K * rng.uniform(0.5, 2.0, n)).astype(np.float32)))
        U = fm.RandomVariableHip(0.0, fm.DeviceVector.from_host(rng.uniform(0.5, 1.5, n).astype(np.float32)))
        base = rng.uniform(0.05, 0.8, n).astype(np.float32)

        def yardstick():
            y = x.v1s1("ADD_S", 1.0); fm.flush(); fm.synchronize(); return y
        yard = median_us(yardstick, args.warmup, args.repeats)
        for model in ("black_scholes", "bachelier"):
            S = fm.RandomVariableHip(0.0, fm.DeviceVector.from_host(base * np.float32(K if model == "bachelier" else 1.0)))
            P1f = fm.option_formula(model, 120.0, S, T, K, 0.9)[0]           # the price the only vector of the inverse: the forward is 120, moneyness 1.2
            P3 = fm.option_formula(model, F, S, T, K, U)[0]
            fm.synchronize()
            calls = {
                "price": (8, lambda: (fm.implied_volatility(model, P1f, 120.0, T, K, 0.9), fm.synchronize()), lambda: (fm.option_formula(model, 120.0, S, T, K, 0.9), fm.synchronize())),
                "price_all": (16, lambda: (fm.implied_volatility(model, P1f, 120.0, T, K, 0.9, everything), fm.synchronize()), lambda: (fm.option_formula(model, 120.0, S, T, K, 0.9), fm.synchronize())),
                "three": (16, lambda: (fm.implied_volatility(model, P3, F, T, K, U), fm.synchronize()), lambda: (fm.option_formula(model, F, S, T, K, U), fm.synchronize())),
                "three_all": (24, lambda: (fm.implied_volatility(model, P3, F, T, K, U, everything), fm.synchronize()), lambda: (fm.option_formula(model, F, S, T, K, U), fm.synchronize())),
            }
            for what, (bytes_per_path, call, forward) in calls.items():
                cell = {"n": n, "model": model, "call": what, "bytes_per_path": bytes_per_path, "yardstick_us": yard}
                os.environ["FMHIP_DEVICE_ANALYTIC"] = "1"
                cell["device_us"] = median_us(call, args.warmup, args.repeats)
                cell["forward_us"] = median_us(forward, args.warmup, args.repeats)
                cell["inverse_over_forward"] = cell["device_us"] / cell["forward_us"]
                cell["yardstick_us_after"] = median_us(yardstick, 1, 5)      # the same yardstick again, behind the cell: the drift of the box
                cell["ratio_to_yardstick_of_equal_bytes"] = cell["device_us"] / (yard * bytes_per_path / 8.0)
                cell["elements_per_ns"] = n / (cell["device_us"] * 1e3)
                if not args.no_host_path and (args.host_path_max_n == 0 or n <= args.host_path_max_n):
                    os.environ["FMHIP_DEVICE_ANALYTIC"] = "0"
                    cell["host_path_us"] = median_us(call, 0, 1) if n > args.host_max else median_us(call, 1, 5)
                    os.environ["FMHIP_DEVICE_ANALYTIC"] = "1"
                    cell["slower_than_host_path"] = bool(cell["device_us"] > cell["host_path_us"])
                doc["cells"].append(cell)
                print(json.dumps(cell), flush=True)
            del S, P1f, P3
        del x, F, U
    if not args.no_driver:
        mc = importlib.import_module("finmath-lib-cuda-extensions_amd.montecarlo")
        m, k = 4096, 256
        prev = fm.set_fusion(True)
        outer = fm.BrownianMotionHip(fm.TimeDiscretization(0.0, 10, 0.1), 2, m, 27182)
        inner = fm.BrownianMotionHip(fm.TimeDiscretization(1.0, 10, 0.1), 2, m * k, 1000)
        run = lambda: mc.forward_implied_volatility_mc(outer, inner, k, 100.0, 0.05, 0.04, 1.5, 0.04, 0.5, -0.7, 1.0, 2.0, moneyness=(0.9, 1.0, 1.1))
        for knob in ("1", "0"):
            os.environ["FMHIP_DEVICE_ANALYTIC"] = os.environ["FMHIP_DEVICE_NESTED"] = knob
            rows = run()
            row = {"driver": "forward_implied_volatility_mc", "FMHIP_DEVICE_ANALYTIC": knob, "FMHIP_DEVICE_NESTED": knob, "outer_paths": m, "inner_paths": k, "steps": "10 + 10",
                   "moneyness": [0.9, 1.0, 1.1], "run_us": median_us(lambda: (run(), fm.synchronize()), 1, 5), "rows": rows}
            doc["driver"].append(row)
            print(json.dumps(row), flush=True)
        os.environ["FMHIP_DEVICE_ANALYTIC"] = os.environ["FMHIP_DEVICE_NESTED"] = "1"
        if doc["driver"][0]["run_us"] > doc["driver"][1]["run_us"]: doc["driver"][0]["slower_than_knobs_off"] = True
        fm.set_fusion(prev)
    text = json.dumps(doc, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text + "\n")
    else:
        print(text)


if __name__ == "__main__":
    main()
