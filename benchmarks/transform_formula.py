"""Transform option values per path on the device: µs per call of fmhip_transform_option at n paths, one state (Heston's
variance), for J = 32, 64, 128 and 256 nodes, with
    value          forward and variance vectors, mask 1                       reads 8n, writes 4n
    all            the same with mask 7 (value, ∂/∂forward, ∂/∂variance)      reads 8n, writes 12n
as node evaluations per ns (n·J / time), and beside them the fp64 VALU instructions per node and element counted in the loop body of the
compiled kernel (`--valu-per-node`, from the disassembly; DESIGN.md §4.28 says how) set against the fp64 vector rate of the device that
`--fp64-vector-tflops` states (an FMA counted as two): the fraction of it that the pass reaches.  The tables are heston_transform_nodes(1.5,
0.04, 0.5, −0.7, 1.0, n_nodes=J): the time does not depend on what the nodes hold.  Beside every figure the host path (FMHIP_DEVICE_ANALYTIC=0:
download, the definition on one core, upload) up to `--host-path-max-evaluations` node evaluations, with a flag where the device is slower.
The drivers: montecarlo.forward_implied_volatility_transform_mc beside forward_implied_volatility_mc at 4096 outer paths (256 inner paths for
the latter) and three moneynesses — time per run, the "not_invertible" shares and the two means with their standard errors, reported, not
asserted (they differ by the inner Euler bias and noise) — and heston_call_analytic beside heston_call_conditional_mc at 2¹⁸ paths.
Method (benchmarks/analytic.py's): every figure is the median of `--repeats` calls after `--warmup` calls, wall clock around a call that ends
in fm.synchronize(); no tracing; the small sizes measure the call, not the kernel.

    python benchmarks/transform_formula.py --out profiles/transform_formula.json
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
    ap.add_argument("--nodes", default="32,64,128,256")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--host-path-max-evaluations", type=float, default=4e8, help="time the host path only up to this many node evaluations (one core needs some 50 ns each)")
    ap.add_argument("--valu-per-node", type=float, default=98.0, help="fp64 VALU instructions per node and element in the kernel's loop body (S = 1)")
    ap.add_argument("--fp64-vector-tflops", type=float, default=78.6, help="the device's fp64 vector rate, an FMA counted as two")
    ap.add_argument("--no-drivers", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    fm = importlib.import_module("finmath-lib-cuda-extensions_amd")
    fm.init(0)
    name, cus, hbm = fm.device_info()
    rng = np.random.default_rng(1)
    doc = {"device": name, "compute_units": cus,
           "method": f"median of {args.repeats} calls after {args.warmup}, wall clock per call through the Python mirror, every call ended by fm.synchronize(), no tracing; "
                     "host path (FMHIP_DEVICE_ANALYTIC=0): one call",
           "fp64_valu_instructions_per_node": args.valu_per_node, "fp64_vector_tflops_assumed": args.fp64_vector_tflops, "cells": [], "drivers": []}
    every = ("value", "delta", "state_delta")
    tables = {J: fm.heston_transform_nodes(1.5, 0.04, 0.5, -0.7, 1.0, n_nodes=J) for J in [int(s) for s in args.nodes.split(",")]}
    for n in [int(s) for s in args.sizes.split(",")]:
        F = fm.RandomVariableHip(0.0, fm.DeviceVector.from_host(rng.uniform(60.0, 160.0, n).astype(np.float32)))
        V = fm.RandomVariableHip(0.0, fm.DeviceVector.from_host(rng.uniform(0.0, 0.3, n).astype(np.float32)))
        for J, nodes in tables.items():
            for what, names in (("value", ("value",)), ("all", every)):
                call = lambda: (fm.transform_option_value(nodes, F, (V,), 100.0, 1.0, names), fm.synchronize())
                os.environ["FMHIP_DEVICE_ANALYTIC"] = "1"
                cell = {"n": n, "nodes": J, "call": what, "device_us": median_us(call, args.warmup, args.repeats)}
                cell["node_evaluations_per_ns"] = n * J / (cell["device_us"] * 1e3)
                # instructions per second over the lanes, against the rate at one instruction per lane and cycle (half the FMA-counted rate)
                cell["fraction_of_fp64_vector_rate"] = cell["node_evaluations_per_ns"] * 1e9 * args.valu_per_node / (args.fp64_vector_tflops * 1e12 / 2.0)
                if n * J <= args.host_path_max_evaluations:
                    os.environ["FMHIP_DEVICE_ANALYTIC"] = "0"
                    cell["host_path_us"] = median_us(call, 0, 1)
                    os.environ["FMHIP_DEVICE_ANALYTIC"] = "1"
                    cell["slower_than_host_path"] = bool(cell["device_us"] > cell["host_path_us"])
                doc["cells"].append(cell)
                print(json.dumps(cell), flush=True)
        del F, V
    if not args.no_drivers:
        mc = importlib.import_module("finmath-lib-cuda-extensions_amd.montecarlo")
        m, k = 4096, 256
        prev = fm.set_fusion(True)
        outer = fm.BrownianMotionHip(fm.TimeDiscretization(0.0, 10, 0.1), 2, m, 27182)
        inner = fm.BrownianMotionHip(fm.TimeDiscretization(1.0, 10, 0.1), 2, m * k, 1000)
        model = (100.0, 0.05, 0.04, 1.5, 0.04, 0.5, -0.7)
        runs = {"forward_implied_volatility_transform_mc": lambda: mc.forward_implied_volatility_transform_mc(outer, *model, 1.0, 2.0, moneyness=(0.9, 1.0, 1.1)),
                "forward_implied_volatility_mc": lambda: mc.forward_implied_volatility_mc(outer, inner, k, *model, 1.0, 2.0, moneyness=(0.9, 1.0, 1.1))}
        for driver, run in runs.items():
            rows = run()
            row = {"driver": driver, "outer_paths": m, "inner_paths": k if driver.endswith("volatility_mc") else 0, "moneyness": [0.9, 1.0, 1.1],
                   "run_us": median_us(lambda: (run(), fm.synchronize()), 1, 5), "rows": rows}
            doc["drivers"].append(row)
            print(json.dumps(row), flush=True)
        paths = 1 << 18
        bm = fm.BrownianMotionHip(fm.TimeDiscretization(0.0, 20, 0.05), 2, paths, 31415)
        t0 = time.perf_counter(); analytic = mc.heston_call_analytic(*model, 1.0, 100.0); analytic_us = (time.perf_counter() - t0) * 1e6
        average, vector = mc.heston_call_conditional_mc(bm, *model, 1.0, 100.0)
        row = {"driver": "heston_call_analytic beside heston_call_conditional_mc", "paths": paths, "steps": 20, "analytic": analytic, "analytic_us": analytic_us,
               "conditional_mc": average, "conditional_mc_standard_error": float(np.sqrt(vector.getVariance() / paths)),
               "conditional_mc_us": median_us(lambda: (mc.heston_call_conditional_mc(bm, *model, 1.0, 100.0), fm.synchronize()), 1, 3)}
        doc["drivers"].append(row)
        print(json.dumps(row), flush=True)
        fm.set_fusion(prev)
    text = json.dumps(doc, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text + "\n")
    else:
        print(text)


if __name__ == "__main__":
    main()
