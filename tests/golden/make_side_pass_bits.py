#!/usr/bin/env python3
"""Records tests/golden/side_pass_bits.json: the BITS of the fp64 sums of the reducing side passes — rank sums, cross moments, binned cross
moments, kernel moments, wide and polynomial cross moments — at the sizes where the end of a pass (csrc/side_pass_device.hpp) takes another
path.  The derived error bounds of the passes' own GPU tests hold for any order of the additions; this fixture pins THE order, so that a change
to the tree shows even where it stays inside the bound.  tests/test_gpu_side_pass_bits.py recomputes every case and compares.

    python tests/golden/make_side_pass_bits.py --commit <the commit the package at --package-root was built from> [--package-root DIR]

Only public functions of the package are used, so the recorder runs unchanged against a build of an older commit (--package-root).  Needs
the GPU.  Per case the file holds the SHA-256 of the result's little-endian fp64 bytes and its first eight values as hex.

Inputs come from integer arithmetic, not from a random generator whose stream may change: element i of vector c is
f(i)·2^e(i) with f(i) = float32(((i·2654435761 + c) mod 2³²)/2³² − ½): full mantissas and mixed exponents, so that the order of the additions
shows.  The keys of the binned and the kernel pass have e(i) = ((i + c) mod 7) − 3, which spreads them over the bins and the points.  A
vector that is summed needs more: fp32 values within a factor 2⁶ of each other add without ANY rounding in fp64 (a rank sum of them is
exact in every order), and a tree of additions is accurate — without cancellation it returns the correctly rounded sum more often than not,
whatever its order.  So e(i) = 12·(((3i + c) mod 7) − 3), neighbours 36 bits apart, and the elements of the first half of the vector that are
1 or larger in scale return at the same place of the second half, negated in the vectors of even c: the large terms of a sum (of the vector, or
of its products with a vector of odd c) cancel exactly, and what is left is the small terms and the roundings on the way.  A case whose sums
ALL equal the exact sum rounded once (math.fsum of the exact terms) would pin nothing: it is refused.

Sizes, per pass with tile T and grid cap C (read from the headers the kernels are compiled with): 7 (one ragged workgroup), T (one full),
T + 1 (two), 65·T − 3 (65 workgroups: the lane-strided loop over the partials takes a second turn, the tail is ragged), C·T + 1 (a
workgroup takes two tiles)."""
import argparse
import ctypes as C
import functools
import hashlib
import importlib
import json
import math
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
FIXTURE = os.path.join(HERE, "side_pass_bits.json")
PKG = "finmath-lib-cuda-extensions_amd"
KEEP = 8


def constants(root=ROOT):
    """(tile, grid cap) per pass, from the headers."""
    csrc = os.path.join(root, PKG, "csrc")
    text = "".join(open(os.path.join(csrc, h)).read() for h in ("kernels.h", "binned_kernel.h", "xmom_wide_kernel.h"))
    const = lambda name: int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1))
    cap = lambda fn: int(re.search(r"inline uint32_t %s\(int64_t n\)\s*\{.*?> (\d+)" % fn, text, re.S).group(1))
    wide_tile = 2 * (const("FM_XMOMW_BLOCK") // 64) * const("FM_XMOMW_CHUNK")       # xmom_wide_blocks: two chunks per wave before the grid grows
    out = {"rank_sums": (const("FM_OS_TILE"), cap("os_sum_blocks")), "cross_moments": (const("FM_XMOM_TILE"), cap("xmom_blocks")),
           "binned": (const("FM_BINNED_TILE"), cap("binned_blocks")), "kernel": (const("FM_BINNED_TILE"), cap("binned_blocks")),
           "wide": (wide_tile, const("FM_XMOMW_MAX_GRID"))}
    out["polynomial"] = out["wide"]
    return out


def sizes(tile, cap):
    return [7, tile, tile + 1, 65 * tile - 3, cap * tile + 1]


@functools.lru_cache(maxsize=80)
def vector(c, n, summed=True):
    """Element i of vector c: see the module's docstring."""
    i = np.arange(n, dtype=np.uint64)
    frac = ((i * np.uint64(2654435761) + np.uint64(c)) & np.uint64(0xffffffff)).astype(np.float64) / 4294967296.0 - 0.5
    if not summed:
        v = frac.astype(np.float32) * np.exp2(((i + np.uint64(c)) % np.uint64(7)).astype(np.float32) - 3.0).astype(np.float32)
    else:
        size = (np.uint64(3) * i + np.uint64(c)) % np.uint64(7)
        v = frac.astype(np.float32) * np.exp2(12.0 * (size.astype(np.float32) - 3.0)).astype(np.float32)
        h = n // 2
        mirrored = size[:h] >= 3                                    # the large elements of the first half return in the second, negated in every other vector
        v[h:2 * h][mirrored] = v[:h][mirrored] * np.float32(-1.0 if c % 2 == 0 else 1.0)
    v.setflags(write=False)
    return v


def vectors(first, count, n):
    return [vector(1000003 * (first + k), n) for k in range(count)]


BINNED_BOUNDS = np.array(sorted([-0.3 - 0.12 * k for k in range(31)] + [0.3 + 0.12 * k for k in range(32)]))       # 64 bins, a wide one in the middle
KERNEL_POINTS = {16: (np.linspace(-1.5, 1.5, 16), 0.75), 256: (np.linspace(-2.0, 2.0, 256), 0.5)}              # points, bandwidth
POLY_EXPONENTS = [e for e in np.ndindex(4, 4, 4) if sum(e) <= 3]                                               # 3 states, degree 3: 20 monomials

# (pass, shape name, parameters): along gridDim.y the shapes of the issue that introduced this fixture
SHAPES = [
    ("rank_sums", "batch1", {"batch": 1}), ("rank_sums", "batch3", {"batch": 3}),
    ("cross_moments", "x3_y1", {"nx": 3, "ny": 1, "one": False}), ("cross_moments", "one_x5_y4", {"nx": 5, "ny": 4, "one": True}),
    ("cross_moments", "x12_y4", {"nx": 12, "ny": 4, "one": False}),
    ("binned", "bins4_x2_y1", {"bins": 4, "nx": 2, "ny": 1, "one": False, "nan": False}),
    ("binned", "bins64_one_x2_y4_nan", {"bins": 64, "nx": 2, "ny": 4, "one": True, "nan": True}),
    ("kernel", "points16_order0_y1", {"points": 16, "order": 0, "ny": 1}), ("kernel", "points256_order1_y4", {"points": 256, "order": 1, "ny": 4}),
    ("wide", "vectors20", {"nx": 20, "ny": 0}), ("wide", "vectors64", {"nx": 60, "ny": 4}),
    ("polynomial", "states3_degree3_y2", {"ny": 2}),
]


def cases(root=ROOT):
    k = constants(root)
    return [{"id": f"{p}-{shape}-n{n}", "pass": p, "n": n, **par} for p, shape, par in SHAPES for n in sizes(*k[p])]


def inputs(case):
    """The host arrays of a case, by role."""
    p, n = case["pass"], case["n"]
    if p == "rank_sums": return {"x": vectors(0, case["batch"], n)}
    if p in ("cross_moments", "wide"): return {"x": vectors(0, case["nx"], n), "y": vectors(case["nx"], case["ny"], n)}
    if p == "binned":
        key = vector(99991, n, False)
        if case["nan"]:
            key = key.copy(); key[n // 2] = np.nan
        return {"key": key, "x": vectors(0, case["nx"], n), "y": vectors(case["nx"], case["ny"], n)}
    if p == "kernel": return {"key": vector(99991, n, False), "y": vectors(0, case["ny"], n)}
    return {"x": vectors(0, 3, n), "y": vectors(3, case["ny"], n)}


def rank_range(n):
    return n // 16, n - 1 - n // 16                                # inside: part of the largest elements of either sign


def binned_bounds(case):
    return BINNED_BOUNDS if case["bins"] == 64 else BINNED_BOUNDS[[15, 31, 47]]


def packed(S, T):
    """[..., products]: the upper triangle of S, then T."""
    iu = np.triu_indices(S.shape[-1])
    return np.concatenate([S[..., iu[0], iu[1]], T.reshape(T.shape[:-2] + (-1,))], axis=-1)


def run(fm, case):
    """The case on the device: its sums (and counts), flat, fp64."""
    a = inputs(case)
    up = fm.DeviceVector.from_host
    p = case["pass"]
    if p == "rank_sums":
        X = [up(v) for v in a["x"]]
        i0, i1 = rank_range(case["n"])
        if case["batch"] == 1: return np.array([X[0].rank_sum(i0, i1)])
        out = (C.c_double * len(X))()
        fm._native.check(fm.lib().fmhip_rank_sums_batch((C.c_int64 * len(X))(*[v.handle for v in X]), len(X), i0, i1, out))
        return np.array(list(out))
    if p in ("cross_moments", "wide"):
        S, T = fm.cross_moments(([None] if case.get("one") else []) + [up(v) for v in a["x"]], [up(v) for v in a["y"]])
        return packed(S, T).ravel()
    if p == "binned":
        counts, S, T = fm.binned_cross_moments(up(a["key"]), binned_bounds(case), ([None] if case["one"] else []) + [up(v) for v in a["x"]], [up(v) for v in a["y"]])
        return np.concatenate([counts.astype(np.float64), packed(S, T).ravel()])
    if p == "kernel":
        pts, h = KERNEL_POINTS[case["points"]]
        return fm.kernel_moments(up(a["key"]), pts, h, [up(v) for v in a["y"]], "epanechnikov", case["order"]).ravel()
    S, T = fm.polynomial_cross_moments([up(v) for v in a["x"]], POLY_EXPONENTS, (), [up(v) for v in a["y"]])
    return packed(S, T).ravel()


def exact_terms(case):
    """Yields (index into run()'s result, the exact terms of that sum as fp64) — every sum of the case whose terms are known exactly on the
    host.  A product of two fp32 values is exact in fp64; a kernel term is rounded where host/kernel_regression.hpp forms it."""
    a = inputs(case)
    p, n = case["pass"], case["n"]
    if p == "rank_sums":
        i0, i1 = rank_range(n)
        for k, v in enumerate(a["x"]): yield k, np.sort(v)[i0:i1 + 1].astype(np.float64)
        return
    if p == "kernel":
        pts, h = KERNEL_POINTS[case["points"]]
        xd = a["key"].astype(np.float64)
        ys = [v.astype(np.float64) for v in a["y"]]
        qe = (1 + len(ys)) if case["order"] == 0 else 3 + 2 * len(ys)
        rh = 1.0 / h
        for q, pt in enumerate(pts):
            m = (pt - h < xd) & (xd < pt + h)
            d = xd[m] - pt
            u = d * rh
            w = np.maximum(1.0 - u * u, 0.0)
            e1 = w * d
            terms = [w] + [w * y[m] for y in ys] if case["order"] == 0 else [w, e1, e1 * d] + [w * y[m] for y in ys] + [e1 * y[m] for y in ys]
            for e, t in enumerate(terms): yield q * qe + e, t
        return
    if p == "polynomial":                                             # the monomials of degree <= 1 are the states themselves: their products are exact
        cols = {i: (np.ones(n) if sum(e) == 0 else a["x"][e.index(1)].astype(np.float64)) for i, e in enumerate(POLY_EXPONENTS) if sum(e) <= 1}
        nx = len(POLY_EXPONENTS)
    else:
        xs = ([np.ones(n)] if case.get("one") else []) + [v.astype(np.float64) for v in a["x"]]
        cols, nx = dict(enumerate(xs)), len(xs)
    ys = [v.astype(np.float64) for v in a["y"]]
    iu = np.triu_indices(nx)
    products = [(s, cols[i], cols[j]) for s, (i, j) in enumerate(zip(*iu)) if i in cols and j in cols]
    products += [(iu[0].size + i * len(ys) + m, cols[i], y) for i in sorted(cols) for m, y in enumerate(ys)]
    if p != "binned":
        for s, u, v in products: yield s, u * v
        return
    bounds = binned_bounds(case)
    key = a["key"].astype(np.float64)
    bins = np.where(np.isnan(key), -1, np.searchsorted(bounds, key, side="left"))     # bin(k) = #{ j : bounds[j] < k }
    q = iu[0].size + nx * len(ys)
    for b in np.argsort(-np.bincount(bins[bins >= 0], minlength=case["bins"]), kind="stable"):    # the fullest bins first
        m = bins == b
        for s, u, v in products: yield case["bins"] + int(b) * q + s, u[m] * v[m]


def pins_the_order(case, got):
    """True as soon as one sum differs from the exact sum of its terms rounded once."""
    return any(got[i] != math.fsum(t) for i, t in exact_terms(case))


def digest(values):
    v = np.ascontiguousarray(values, dtype="<f8")
    return {"sha256": hashlib.sha256(v.tobytes()).hexdigest(), "first": [float(x).hex() for x in v[:KEEP]]}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--commit", required=True, help="the commit the package was built from: the fixture names it")
    ap.add_argument("--package-root", default=ROOT, help="the tree whose built package computes the sums (default: this one)")
    ap.add_argument("--out", default=FIXTURE)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.package_root))
    fm = importlib.import_module(PKG)
    fm.init(0)
    recorded = {}
    for case in cases(args.package_root):
        got = run(fm, case)
        if not pins_the_order(case, got):
            raise SystemExit(f"{case['id']}: every sum equals the exact sum rounded once — the case pins nothing; choose other inputs")
        recorded[case["id"]] = digest(got)
        print(case["id"], got.size, "values", recorded[case["id"]]["sha256"][:16], flush=True)
    fixture = {"_comment": "recorded on an MI355X by tests/golden/make_side_pass_bits.py; the bits of the fp64 sums of the reducing side passes",
               "commit": args.commit, "cases": recorded}
    json.dump(fixture, open(args.out, "w"), indent=0)
    print("written", len(recorded), "cases to", args.out)
    fm.shutdown()


if __name__ == "__main__":
    main()
