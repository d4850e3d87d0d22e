"""A float64 numpy restatement of montecarlo.bermudan_max_call_mc with and without ordered_states, run on the CPU: no
device, no library.  It derives the margin that tests/test_gpu_cross_order.py asserts for `ordered − unordered` — half the smallest gap
over 8 seeds — BEFORE the device's values are looked at.

The driver, restated: independent Black–Scholes assets (log-Euler, exact for ln S), states at the exercise dates, the value started as the
last date's discounted payoff; at each earlier date a least-squares regression over ALL paths on all monomials of total degree <= order in
the strike-scaled states — sorted descending across the assets per path when ordered — and the discounted exercise value taken on the paths
where exercise − continuation >= 0.  Both runs of a seed use the same paths.

    python benchmarks/cross_order_restatement.py [--merge profiles/cross_order.json]

prints one JSON object; with --merge it is stored under "restatement" in that file (the other keys are kept).
"""
import argparse
import itertools
import json
import math
import os

import numpy as np

S0, R, DELTA, SIGMA, STRIKE, DATES, ORDER = 100.0, 0.05, 0.10, 0.20, 100.0, [k / 3 for k in range(1, 10)], 3


def exponents(assets, order):
    return [e for e in itertools.product(range(order + 1), repeat=assets) if sum(e) <= order]


def max_call(states, ordered, order=ORDER):
    """states[k]: (assets, n) prices at DATES[k].  (value, standard error)."""
    def exercise_value(s, date): return np.maximum(s.max(axis=0) - STRIKE, 0.0) / math.exp(R * date)
    value = exercise_value(states[-1], DATES[-1])
    es = exponents(states[0].shape[0], order)
    for k in range(len(DATES) - 2, -1, -1):
        scaled = states[k] / STRIKE
        if ordered: scaled = -np.sort(-scaled, axis=0)
        basis = np.stack([np.prod([scaled[a] ** ea for a, ea in enumerate(e)], axis=0) for e in es], axis=1)
        coefficients = np.linalg.lstsq(basis, value, rcond=None)[0]
        exercise = exercise_value(states[k], DATES[k])
        value = np.where(exercise - basis @ coefficients >= 0.0, exercise, value)
    return float(value.mean()), float(value.std() / math.sqrt(value.size))


def simulate(assets, n, seed):
    rng = np.random.default_rng(seed)
    x = np.full((assets, n), math.log(S0))
    states, t = [], 0.0
    for date in DATES:
        dt = date - t
        x = x + (R - DELTA - 0.5 * SIGMA * SIGMA) * dt + SIGMA * math.sqrt(dt) * rng.standard_normal((assets, n))
        states.append(np.exp(x))
        t = date
    return states


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--paths", type=int, default=1 << 18)
    ap.add_argument("--seeds", type=int, default=8)
    ap.add_argument("--assets", type=int, nargs="*", default=[2, 3, 5])
    ap.add_argument("--merge", default=None)
    args = ap.parse_args()
    out = {"configuration": {"S0": S0, "r": R, "dividend": DELTA, "sigma": SIGMA, "strike": STRIKE, "dates": len(DATES), "degree": ORDER, "paths": args.paths, "seeds": args.seeds},
           "by_assets": {}}
    for assets in args.assets:
        rows = []
        for seed in range(args.seeds):
            states = simulate(assets, args.paths, 1000 + seed)
            unordered, se_u = max_call(states, False)
            ordered, se_o = max_call(states, True)
            rows.append({"seed": 1000 + seed, "unordered": unordered, "ordered": ordered, "gap": ordered - unordered, "standard_error": max(se_u, se_o)})
        gaps = [r["gap"] for r in rows]
        out["by_assets"][str(assets)] = {"runs": rows, "smallest_gap": min(gaps), "largest_gap": max(gaps), "mean_unordered": float(np.mean([r["unordered"] for r in rows])),
                                         "mean_ordered": float(np.mean([r["ordered"] for r in rows])), "half_smallest_gap": 0.5 * min(gaps),
                                         "largest_standard_error": max(r["standard_error"] for r in rows)}
    print(json.dumps(out, indent=1))
    if args.merge:
        stored = json.load(open(args.merge)) if os.path.exists(args.merge) else {}
        stored["restatement"] = out
        json.dump(stored, open(args.merge, "w"), indent=1)
        open(args.merge, "a").write("\n")


if __name__ == "__main__":
    main()
