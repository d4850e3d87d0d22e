"""Order statistics across vectors on the device: µs per call for K = 2, 3, 5, 8, 16, 32 vectors at 10⁵, 10⁷ and 2²⁶ / K
paths for
    max            max_across(vs)                                  reads 4nK, writes 4n   (the network on keys alone)
    sort           sort_across(vs)                                 reads 4nK, writes 4nK
    argmax         argmax_across(vs)                               reads 4nK, writes 4n   (the network on (key, slot) pairs)
    select         select_across(index, vs)                        reads 8n, writes 4n
  each beside
    (a) yardstick  a materialised ADD_S over a vector of as many bytes as the call reads and writes, in the same process;
    (b) chain      the composed floor chain for the maximum alone (K − 1 recorded ops, fused, one flush);
    (c) host       the same call with FMHIP_DEVICE_CROSS_ORDER=0 (download, the host definition on one core, upload);
    driver         montecarlo.bermudan_max_call_mc with and without ordered_states for 2, 3 and 5 assets (9 dates, degree 3, 2¹⁸ paths):
                   values and wall time per run.
Method: every figure is the median of `--repeats` calls after `--warmup` calls (the host path: `--host-repeats` after one), wall clock around
a call that ends in fm.synchronize(); no tracing beside the timings.  Writes one JSON document (default: stdout); --merge keeps the other
keys of an existing file (benchmarks/cross_order_restatement.py stores its own there).

    python benchmarks/cross_order.py --merge profiles/cross_order.json
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
    ap.add_argument("--ks", default="2,3,5,8,16,32")
    ap.add_argument("--paths", default="100000,10000000,0")          # 0: 2^26 / K
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=11)
    ap.add_argument("--host-repeats", type=int, default=1)
    ap.add_argument("--host-max-elements", type=int, default=20000000)
    ap.add_argument("--no-driver", action="store_true")
    ap.add_argument("--merge", default="")
    args = ap.parse_args()
    fm = importlib.import_module("finmath-lib-cuda-extensions_amd")
    mc = importlib.import_module("finmath-lib-cuda-extensions_amd.montecarlo")
    fm.init(0)
    name, cus, hbm = fm.device_info()
    os.environ["FMHIP_DEVICE_CROSS_ORDER"] = "1"
    doc = {"device": name, "compute_units": cus,
           "method": f"median of {args.repeats} calls after {args.warmup} (host path: {args.host_repeats} after 1, shapes of at most {args.host_max_elements} input elements), wall clock per call through the Python mirror, every call ended by fm.synchronize(), no tracing",
           "yardstick": "a materialised ADD_S over a vector of (bytes read + bytes written) / 8 elements: the same bytes through the stream kernel",
           "chain": "max alone as K - 1 floor ops on the fused op stream, one flush", "host": "the same call with FMHIP_DEVICE_CROSS_ORDER=0",
           "ratio_to_yardstick": "device_us / yardstick_us", "ratio_to_chain": "device_us / chain_us (max only)", "cells": [], "driver": []}
    rng = np.random.default_rng(1)
    for k in [int(x) for x in args.ks.split(",")]:
        for paths in [int(x) for x in args.paths.split(",")]:
            n = paths if paths else (1 << 26) // k
            vs = [fm.RandomVariableHip(0.0, fm.DeviceVector.from_host(rng.standard_normal(n).astype(np.float32))) for _ in range(k)]
            index = fm.argmax_across(vs)
            calls = (("max", lambda: fm.max_across(vs), k + 1), ("sort", lambda: fm.sort_across(vs), 2 * k), ("argmax", lambda: fm.argmax_across(vs), k + 1),
                     ("select", lambda: fm.select_across(index, vs), 3))
            prev = fm.set_fusion(True)
            def chain():
                best = vs[0]
                for v in vs[1:]: best = best.floor(v)
                fm.flush(); fm.synchronize()
                return best
            chain_us = median_us(chain, args.warmup, args.repeats)
            fm.set_fusion(False)
            for what, call, vectors_moved in calls:
                m = n * vectors_moved // 2
                big = fm.DeviceVector.from_host(np.zeros(m, dtype=np.float32))
                yard = median_us(lambda: (big.v1s1("ADD_S", 1.0), fm.synchronize()), args.warmup, args.repeats)
                del big
                us = median_us(lambda: (call(), fm.synchronize()), args.warmup, args.repeats)
                cell = {"K": k, "n": n, "call": what, "device_us": us, "yardstick_us": yard, "ratio_to_yardstick": us / yard, "tb_per_s": 4.0 * n * vectors_moved / (us * 1e-6) / 1e12}
                if what == "max": cell.update({"chain_us": chain_us, "ratio_to_chain": us / chain_us})
                if n * k <= args.host_max_elements:
                    os.environ["FMHIP_DEVICE_CROSS_ORDER"] = "0"
                    cell["host_us"] = median_us(lambda: (call(), fm.synchronize()), 1, args.host_repeats)
                    os.environ["FMHIP_DEVICE_CROSS_ORDER"] = "1"
                    cell["speedup_over_host"] = cell["host_us"] / us
                doc["cells"].append(cell)
                print(json.dumps(cell), flush=True)
            fm.set_fusion(prev)
            del vs, index
    if not args.no_driver:
        prev = fm.set_fusion(True)
        dates = [j / 3 for j in range(1, 10)]
        for assets in (2, 3, 5):
            bm = fm.BrownianMotionHip(fm.TimeDiscretization(0.0, 9, 1.0 / 3), assets, 1 << 18, 3141)
            for ordered in (False, True):
                run = lambda: mc.bermudan_max_call_mc(bm, [100.0] * assets, 0.05, 0.10, 0.20, dates, 100.0, basis_order=3, ordered_states=ordered)
                value, se = run()
                row = {"driver": "bermudan_max_call_mc", "assets": assets, "ordered_states": ordered, "paths": 1 << 18, "dates": 9, "degree": 3, "value": value, "standard_error": se,
                       "run_us": median_us(lambda: (run(), fm.synchronize()), 1, 3)}
                doc["driver"].append(row)
                print(json.dumps(row), flush=True)
        fm.set_fusion(prev)
    if args.merge:
        stored = json.load(open(args.merge)) if os.path.exists(args.merge) else {}
        stored.update(doc)
        os.makedirs(os.path.dirname(os.path.abspath(args.merge)), exist_ok=True)
        open(args.merge, "w").write(json.dumps(stored, indent=1) + "\n")
    else:
        print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main()
