"""Implied volatility per path without a GPU (include/fmhip.h: fmhip_implied_volatility_host; host/implied_volatility.hpp; analytic.py;
DESIGN.md §4.25): the host DEFINITION against the 60-digit mpmath root of the exact formula on the grid of §4.21 — the bound of check A with
its measured constant, the relative error where the price is below 2^-30 of the scale (check B), the fp32 result within one ulp of the
correctly rounded root where A allows it (check C), the residual of repricing, the iteration counts —; monotonicity over 100 000 sorted
prices; the partials against central differences of mpmath's root and against the forward formula at the root; every line of the
semantics as an equality, in the first, a middle and the last, incomplete group, and every combination of vector and scalar operands; the
Python mirrors (put, vector strike, convert_volatility, AAD on the oracle's float class); a numpy restatement of
montecarlo.forward_implied_volatility_mc on the driver's own draws; the host half under the sanitizers
(tests/cpp/test_implied_volatility_host.cpp); the engine's side on the null device under ASan/UBSan and TSan (tests/nulldev/implied_volatility.mk); the kernel's resource usage for gfx950."""
import ctypes as C
import itertools
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "finmath-lib-cuda-extensions_amd")
CSRC = os.path.join(PKG, "csrc")
NULLDEV = os.path.join(ROOT, "tests", "nulldev")
PD = C.POINTER(C.c_double)
PI32 = C.POINTER(C.c_int32)

MODELS = {"black_scholes": 0, "bachelier": 1}
CANONICAL_NAN = 0x7fc00000
POSITIVE_INFINITY = 0x7f800000
# check A: |sigma − sigma*| <= IMPLIED_C[model]·2^-50·(|F| + |K|)/vega1(sigma*): four times the c measured on the grid below, of the fp64 roots,
# rounded up (printed by the test: 0.177 for Black–Scholes, 0.771 for Bachelier); the issue's ceilings are 8e4 and 5
IMPLIED_C = {0: 1.0, 1: 4.0}
IMPLIED_C_CEILING = {0: 8.0e4, 1: 5.0}
# check B: the relative error of sigma where the exact price is below 2^-30·N·(|F| + |K|), in units of 2^-52: four times the measured one
# (1.33e5 for Black–Scholes — the 2^-53 of F/K against log(F/K) = 5e-6 —, 2.6 for Bachelier)
IMPLIED_TAIL = {0: 6.0e5, 1: 12.0}
FORMULA_C = {0: 4.0e4, 1: 2.5}                                              # tests/test_analytic_cpu.py: the forward formula's asserted constants
GRID_POINTS = {0: 915, 1: 900}                                              # what stays live of the grid


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def mp60():
    mpmath = pytest.importorskip("mpmath")
    mpmath.mp.dps = 60
    return mpmath


def correctly_rounded(mpmath, exact):
    c = np.float32(float(exact))
    best = c
    for cand in (np.nextafter(c, np.float32(np.inf)), np.nextafter(c, np.float32(-np.inf))):
        if np.isfinite(cand) and abs(mpmath.mpf(float(cand)) - exact) < abs(mpmath.mpf(float(best)) - exact): best = cand
    return best


def implied_host(fm, model, P, F, unit, T, K, mask):
    """fmhip_implied_volatility_host through ctypes: P, F, unit are float32 arrays or floats; the columns in bit order."""
    ops = [P, F, unit]
    n = next(np.asarray(o).size for o in ops if not np.isscalar(o))
    arrays = [None if np.isscalar(o) else np.ascontiguousarray(o, dtype=np.float32) for o in ops]
    scalars = [float(o) if np.isscalar(o) else 0.0 for o in ops]
    out = [np.full(n, -7.0, dtype=np.float32) for _ in range(bin(mask).count("1"))]
    cols = (C.c_void_p * len(out))(*[o.ctypes.data for o in out])
    ptr = [a.ctypes.data_as(C.c_void_p) if a is not None else None for a in arrays]
    fm._native.check(fm.lib().fmhip_implied_volatility_host(model, ptr[0], scalars[0], ptr[1], scalars[1], ptr[2], scalars[2], n, float(T), float(K), mask, cols))
    return out


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    """tests/cpp/implied_volatility_double_shim.cpp: the definition's DOUBLES and iteration counts, built with the library's flags."""
    gxx = shutil.which("g++")
    if not gxx: pytest.skip("needs g++")
    so = tmp_path_factory.mktemp("implied_shim") / "libimplied_shim.so"
    r = subprocess.run([gxx, "-std=c++17", "-O2", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Werror",
                        os.path.join(ROOT, "tests", "cpp", "implied_volatility_double_shim.cpp"), "-o", str(so)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    lib = C.CDLL(str(so))
    lib.shim_implied64.argtypes = [C.c_int, PD, PD, PD, C.c_int64, C.c_double, C.c_double, PD, PI32, PI32]
    lib.shim_implied_formula64.argtypes = [C.c_int, PD, PD, PD, C.c_int64, C.c_double, C.c_double, PD]

    def three(a, b, c):
        return (np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=np.float64), np.broadcast(a, b, c).shape)).ravel() for v in (a, b, c))

    class Shim:
        max_iterations = lib.shim_implied_max_iterations()

        @staticmethod
        def implied(model, P, F, unit, T, K):
            P, F, unit = three(P, F, unit)
            out = np.empty((P.size, 3)); iterations = np.empty(P.size, dtype=np.int32); converged = np.empty(P.size, dtype=np.int32)
            lib.shim_implied64(model, P.ctypes.data_as(PD), F.ctypes.data_as(PD), unit.ctypes.data_as(PD), P.size, float(T), float(K), out.ctypes.data_as(PD),
                               iterations.ctypes.data_as(PI32), converged.ctypes.data_as(PI32))
            return out, iterations, converged

        @staticmethod
        def formula(model, F, sigma, unit, T, K):
            F, sigma, unit = three(F, sigma, unit)
            out = np.empty((F.size, 3))
            lib.shim_implied_formula64(model, F.ctypes.data_as(PD), sigma.ctypes.data_as(PD), unit.ctypes.data_as(PD), F.size, float(T), float(K), out.ctypes.data_as(PD))
            return out
    return Shim


# ---------------------------------------------------------------- the exact formula, its root, the grid
def exact_value(mpmath, model, F, sigma, T, K):
    """Value, delta and vega of the call with payoff unit 1, as mpf."""
    s = sigma * mpmath.sqrt(T)
    if model == 0:
        d1 = (mpmath.log(F / K) + s * s / 2) / s
        return F * mpmath.ncdf(d1) - K * mpmath.ncdf(d1 - s), mpmath.ncdf(d1), F * mpmath.npdf(d1) * mpmath.sqrt(T)
    d = (F - K) / s
    return (F - K) * mpmath.ncdf(d) + s * mpmath.npdf(d), mpmath.ncdf(d), mpmath.sqrt(T) * mpmath.npdf(d)


def exact_time_value(mpmath, model, F, sigma, T, K):
    """The time value from the out-of-the-money side: no cancellation against the intrinsic value."""
    s = sigma * mpmath.sqrt(T)
    if model == 0:
        A, B = min(F, K), max(F, K)
        d1 = (mpmath.log(A / B) + s * s / 2) / s
        return A * mpmath.ncdf(d1) - B * mpmath.ncdf(d1 - s)
    m = abs(F - K)
    return s * mpmath.npdf(m / s) - m * mpmath.ncdf(-m / s) if m else s * mpmath.npdf(0)


def exact_root(mpmath, model, P, F, N, T, K, start):
    """The sigma with N·value(sigma) = P for the doubles P, F, N, T, K: a bracketed Newton iteration on ln(time value) in ln sigma, then Newton
    steps on the value itself, at 60 digits."""
    P, F, N, T, K = (mpmath.mpf(float(v)) for v in (P, F, N, T, K))
    target = P / N - max(F - K, 0)
    assert target > 0
    log_target = mpmath.log(target)
    f = lambda y: mpmath.log(exact_time_value(mpmath, model, F, mpmath.exp(y), T, K)) - log_target
    y = mpmath.log(mpmath.mpf(float(start)))
    lo = hi = y
    while f(lo) > 0: lo -= 1
    while f(hi) < 0: hi += 1
    h = mpmath.mpf(10) ** -30
    for _ in range(400):
        fy = f(y)
        if fy > 0: hi = y
        else: lo = y
        nxt = y - fy * h / (f(y + h) - fy)
        if not lo < nxt < hi: nxt = (lo + hi) / 2
        done = abs(nxt - y) < mpmath.mpf(10) ** -25
        y = nxt
        if done: break
    else:
        raise AssertionError("the reference root was not found")
    sigma = mpmath.exp(y)
    for _ in range(2):
        sigma -= (exact_time_value(mpmath, model, F, sigma, T, K) - target) / exact_value(mpmath, model, F, sigma, T, K)[2]
    return sigma


def grid_rows(model):
    """§4.21's grid: (F, sigma, unit, T, K) with σ√T from 1e-6 to 10 and the forward from deep out of to deep in the money."""
    K = 100.0
    rows = []
    for T in (0.25, 1.0, 4.0):
        for s in (1e-6, 1e-4, 1e-2, 0.1, 0.3, 1.0, 3.0, 10.0):
            sigma = s / math.sqrt(T) * (K if model == 1 else 1.0)
            for moneyness in (0.01, 0.5, 0.9, 0.999, 1.0, 1.001, 1.1, 2.0, 100.0, 1.0 + s, 1.0 - 2.0 * s, math.exp(3.0 * s), math.exp(-5.0 * s)):
                if model == 0 and not moneyness > 0.0: continue
                for unit in (1.0, 0.37):
                    rows.append((float(np.float32(K * moneyness)), float(np.float32(sigma)), float(np.float32(unit)), T, K))
    return rows


def is_live(model, P, F, N, K):
    c = P / N
    return c > max(F - K, 0.0) and (c < F if model == 0 else math.isfinite(c))


_REFERENCE = {}


def reference(model):
    """[(P, F, N, T, K, sigma* (mpf), the exact price of the grid point (mpf), "fp32" | "fp64")]: the price rounded to fp32 (a vector's
    element) and to double (a scalar operand) of every grid point, where it is strictly inside the live range.  Computed once."""
    if model not in _REFERENCE:
        mpmath = mp60()
        out = []
        for F, sigma, N, T, K in grid_rows(model):
            value = exact_value(mpmath, model, *(mpmath.mpf(v) for v in (F, sigma, T, K)))[0] * mpmath.mpf(N)
            for precision, P in (("fp32", float(np.float32(float(value)))), ("fp64", float(value))):
                if not (P > 0 and math.isfinite(P) and is_live(model, P, F, N, K)): continue
                out.append((P, F, N, T, K, exact_root(mpmath, model, P, F, N, T, K, sigma), value, precision))
        _REFERENCE[model] = out
    return _REFERENCE[model]


# ---------------------------------------------------------------- checks A, B, C, the residual, the iterations
@pytest.mark.parametrize("model", [0, 1])
def test_the_root_against_mpmath(fm, shim, model):
    mpmath = mp60()
    points = reference(model)
    assert len(points) == GRID_POINTS[model]                                 # the grid cannot empty itself
    two50 = mpmath.mpf(2) ** -50
    c_measured, worst, tail_measured, worst_tail, most, rounded = 0.0, None, 0.0, None, 0, 0
    for P, F, N, T, K, star, value, precision in points:
        out, iterations, converged = shim.implied(model, P, F, N, T, K)
        sigma64 = float(out[0, 0])
        assert converged[0] == 1 and iterations[0] <= shim.max_iterations, (model, P, F, N, T, K)
        most = max(most, int(iterations[0]))
        vega1 = exact_value(mpmath, model, mpmath.mpf(F), star, mpmath.mpf(T), mpmath.mpf(K))[2]
        error = abs(mpmath.mpf(sigma64) - star)
        # A
        c = float(error * vega1 / (two50 * (abs(F) + abs(K))))
        if c > c_measured: c_measured, worst = c, (P, F, N, T, K, precision)
        assert error <= IMPLIED_C[model] * two50 * (abs(F) + abs(K)) / vega1, (model, P, F, N, T, K, sigma64, float(star), c)
        # B
        if value < mpmath.mpf(2) ** -30 * N * (abs(F) + abs(K)):
            relative = float(error / star) / 2.0 ** -52
            if relative > tail_measured: tail_measured, worst_tail = relative, (P, F, N, T, K, precision)
            assert relative <= IMPLIED_TAIL[model], (model, P, F, N, T, K, sigma64, float(star), relative)
        # C: the entry point narrows the definition's double once, and that is within one ulp of the correctly rounded root
        got32 = implied_host(fm, model, np.array([P], dtype=np.float32), F, N, T, K, 1)[0][0] if precision == "fp32" else implied_host(fm, model, P, np.array([F], dtype=np.float32), N, T, K, 1)[0][0]
        assert got32 == np.float32(sigma64)
        if IMPLIED_C[model] * two50 * (abs(F) + abs(K)) / vega1 < mpmath.mpf(2) ** -26 * star:
            rounded += 1
            want32 = correctly_rounded(mpmath, star)
            assert got32 in (want32, np.nextafter(want32, np.float32(np.inf)), np.nextafter(want32, np.float32(-np.inf))), (model, P, F, N, T, K, got32, want32)
        # the residual: repricing at the fp64 root
        again = shim.formula(model, F, sigma64, N, T, K)[0]
        assert abs(again[0] - P) <= 2 * FORMULA_C[model] * 2.0 ** -50 * N * (abs(F) + abs(K)) + again[2] * sigma64 * 2.0 ** -52, (model, P, F, N, T, K, sigma64, again[0])
    print(f"model {model}: {len(points)} points; measured c = {c_measured:.3g} at {worst} (asserted {IMPLIED_C[model]}); tail relative error {tail_measured:.3g}·2^-52 at {worst_tail} "
          f"(asserted {IMPLIED_TAIL[model]:.3g}); at most {most} iterations of {shim.max_iterations}; {rounded} points under check C")
    assert 4 * c_measured <= IMPLIED_C[model] <= IMPLIED_C_CEILING[model]
    assert 4 * tail_measured <= IMPLIED_TAIL[model]
    assert rounded > len(points) // 3 and most < shim.max_iterations


@pytest.mark.parametrize("model", [0, 1])
def test_the_volatility_does_not_decrease_with_the_price(fm, model):
    """100 000 sorted fp32 prices between those of sigma = 0.05 and sigma = 5 (times K under Bachelier) at F/K = e^0.1 resp. F − K = 0.1·K, T = 1."""
    K, T = 100.0, 1.0
    F = float(np.float32(K * math.exp(0.1))) if model == 0 else 110.0
    scale = K if model == 1 else 1.0
    lo, hi = (fm.option_formula_double("black_scholes" if model == 0 else "bachelier", F, s * scale, T, K)["value"] for s in (0.05, 5.0))
    P = np.unique(np.linspace(lo, hi, 100000).astype(np.float32))
    assert P.size > 99000
    sigma = implied_host(fm, model, P, F, 1.0, T, K, 1)[0]
    assert np.isfinite(sigma).all() and (np.diff(sigma) >= 0).all()
    assert abs(sigma[0] - 0.05 * scale) < 1e-3 * scale and abs(sigma[-1] - 5.0 * scale) < 1e-3 * scale


@pytest.mark.parametrize("model", [0, 1])
def test_the_partials(shim, model):
    """∂σ/∂price and ∂σ/∂forward against central differences of mpmath's root (relative steps of 1e-8 at 60 digits: the truncation is below
    1e-12 of the partial), and EQUAL to 1/(N·vega1) and −delta1/vega1 of the forward formula at the returned fp64 root."""
    mpmath = mp60()
    K, T, N = 100.0, 1.5, 0.8
    scale = K if model == 1 else 1.0
    for F in (70.0, 98.0, 100.0, 125.0):
        for s in (0.1, 0.3, 0.9):
            P = float(exact_value(mpmath, model, mpmath.mpf(F), mpmath.mpf(s * scale), mpmath.mpf(T), mpmath.mpf(K))[0]) * N
            out, _, _ = shim.implied(model, P, F, N, T, K)
            sigma, d_price, d_forward = out[0]
            hP, hF = mpmath.mpf(P) * mpmath.mpf(10) ** -8, mpmath.mpf(F) * mpmath.mpf(10) ** -8
            root = lambda p, f: exact_root_mpf(mpmath, model, p, f, N, T, K, s * scale)
            by_price = (root(mpmath.mpf(P) + hP, mpmath.mpf(F)) - root(mpmath.mpf(P) - hP, mpmath.mpf(F))) / (2 * hP)
            by_forward = (root(mpmath.mpf(P), mpmath.mpf(F) + hF) - root(mpmath.mpf(P), mpmath.mpf(F) - hF)) / (2 * hF)
            assert abs(d_price - float(by_price)) <= 1e-9 * abs(float(by_price)), (model, F, s)
            assert abs(d_forward - float(by_forward)) <= 1e-9 * abs(float(by_forward)) + 1e-12 * scale, (model, F, s)
            at = shim.formula(model, F, sigma, 1.0, T, K)[0]
            assert d_price == 1.0 / (N * at[2]) and d_forward == (0.0 - at[1]) / at[2]


def exact_root_mpf(mpmath, model, P, F, N, T, K, start):
    """exact_root for mpf prices and forwards (the central differences' arguments are no doubles): Newton on the value from a close start."""
    N, T, K = (mpmath.mpf(float(v)) for v in (N, T, K))
    sigma = mpmath.mpf(float(start))
    for _ in range(12):
        value, _, vega = exact_value(mpmath, model, F, sigma, T, K)
        sigma -= (value - P / N) / vega
    return sigma


# ---------------------------------------------------------------- the semantics, line by line
def edge_rows(model):
    """(price, forward, payoff unit, what sigma is: "nan" | "zero" | "inf" | "live") at T = 1, K = 100."""
    nan, inf = math.nan, math.inf
    rows = [(nan, 100.0, 1.0, "nan"), (8.0, nan, 1.0, "nan"), (8.0, 100.0, nan, "nan"), (8.0, 100.0, 0.0, "nan"), (8.0, 100.0, -1.0, "nan"), (8.0, 100.0, -inf, "nan"),
            (0.0, 80.0, 1.0, "zero"), (-0.0, 80.0, 1.0, "zero"), (10.0, 120.0, 0.5, "zero"), (0.0, 100.0, 2.0, "zero"), (0.0, 80.0, inf, "zero"),
            (19.0, 120.0, 1.0, "nan"), (-1.0, 80.0, 1.0, "nan"), (-inf, 80.0, 1.0, "nan"), (5.0, inf, 1.0, "nan"), (5.0, -inf, 1.0, "nan"),
            (8.0, 100.0, 1.0, "live"), (25.0, 120.0, 1.0, "live"), (1e-30, 80.0, 1.0, "live"), (4.0, 100.0, 0.5, "live")]
    if model == 0:
        rows += [(100.0, 100.0, 1.0, "inf"), (60.0, 120.0, 0.5, "inf"), (150.0, 100.0, 1.0, "nan"), (inf, 100.0, 1.0, "nan"), (1.0, 0.0, 1.0, "nan"), (1.0, -3.0, 1.0, "nan"),
                 (0.0, -3.0, 1.0, "zero"), (0.0, 0.0, 1.0, "zero")]
    else:
        rows += [(inf, 100.0, 1.0, "inf"), (inf, 80.0, 0.5, "inf"), (150.0, 100.0, 1.0, "live"), (1.0, -3.0, 1.0, "live"), (1.0, 0.0, 1.0, "live"), (1.0e30, 100.0, 1.0, "live")]
    return rows


def check_edges(columns, at, rows):
    sigma, d_price, d_forward = columns
    for p, (_, _, _, what) in zip(at, rows):
        if what == "live":
            assert np.isfinite(sigma[p]) and sigma[p] > 0 and np.isfinite(d_price[p]) and d_price[p] > 0 and np.isfinite(d_forward[p]) and d_forward[p] < 0, (p, what)
            continue
        assert bits(sigma[p:p + 1])[0] == {"nan": CANONICAL_NAN, "zero": 0, "inf": POSITIVE_INFINITY}[what], (p, what, sigma[p])
        assert bits(d_price[p:p + 1])[0] == CANONICAL_NAN and bits(d_forward[p:p + 1])[0] == CANONICAL_NAN, (p, what)


@pytest.mark.parametrize("model", [0, 1])
def test_every_line_of_the_semantics_in_the_first_a_middle_and_the_last_group(fm, model):
    rng = np.random.default_rng(5)
    n = 1003                                                                 # the last group is incomplete
    scale = 100.0 if model == 1 else 1.0
    F = rng.uniform(60, 150, n).astype(np.float32); unit = rng.uniform(0.5, 1.5, n).astype(np.float32)
    sigma = (rng.uniform(0.05, 0.8, n) * scale).astype(np.float32)
    P = fm.option_formula_host("black_scholes" if model == 0 else "bachelier", F, sigma, 1.0, 100.0, unit)[0]
    rows = edge_rows(model)
    for start in (0, 480, n - len(rows)):
        p, f, u = P.copy(), F.copy(), unit.copy()
        at = list(range(start, start + len(rows)))
        for i, (price, forward, payoff_unit, _) in zip(at, rows): p[i], f[i], u[i] = price, forward, payoff_unit
        columns = implied_host(fm, model, p, f, u, 1.0, 100.0, 7)
        check_edges(columns, at, rows)
        untouched = np.ones(n, dtype=bool); untouched[at] = False
        untouched &= np.abs(F - 100.0) < 15.0                                # near the money, where an fp32 price still carries the volatility
        assert np.allclose(columns[0][untouched], sigma[untouched], rtol=2e-3, atol=0)      # the live elements around them: the volatility the price was made from
        # a mask's columns are the columns of the full mask
        for mask in range(1, 8):
            for g, w in zip(implied_host(fm, model, p, f, u, 1.0, 100.0, mask), [columns[b] for b in range(3) if mask >> b & 1]): assert (bits(g) == bits(w)).all()
    # T = 0: +0 without a time value, NaN with one; a non-positive strike under Black–Scholes likewise
    p = np.array([0.0, 20.0, 5.0, 25.0, np.nan], dtype=np.float32); f = np.array([80.0, 120.0, 80.0, 120.0, 100.0], dtype=np.float32)
    s, dp, df = implied_host(fm, model, p, f, 1.0, 0.0, 100.0, 7)
    assert list(bits(s)) == [0, 0, CANONICAL_NAN, CANONICAL_NAN, CANONICAL_NAN] and (bits(dp) == CANONICAL_NAN).all() and (bits(df) == CANONICAL_NAN).all()
    p = np.array([105.0, 106.0, 100.0], dtype=np.float32); f = np.array([100.0, 100.0, 100.0], dtype=np.float32)
    s = implied_host(fm, model, p, f, 1.0, 1.0, -5.0, 1)[0]
    assert bits(s)[0] == 0 and (bits(s)[1] == CANONICAL_NAN if model == 0 else s[1] > 0) and bits(s)[2] == CANONICAL_NAN


@pytest.mark.parametrize("model", [0, 1])
def test_every_combination_of_vector_and_scalar_operands_gives_the_bits_of_the_broadcast_call(fm, model):
    rng = np.random.default_rng(12)
    n = 1003
    scale = 100.0 if model == 1 else 1.0
    name = "black_scholes" if model == 0 else "bachelier"
    F = rng.uniform(60, 150, n).astype(np.float32); unit = rng.uniform(0.5, 1.5, n).astype(np.float32)
    P = fm.option_formula_host(name, F, (rng.uniform(0.05, 0.8, n) * scale).astype(np.float32), 1.5, 100.0, unit)[0]
    P[::97] = -1.0; P[3::89] = 0.0; F[5::101] = -2.0; unit[7::103] = np.nan; unit[9::107] = 0.0; P[11::109] = np.inf
    scalars = (9.25, 101.25, 0.75)                                           # doubles that are fp32 numbers: the broadcast array holds them exactly
    for use_vector in itertools.product([True, False], repeat=3):
        if not any(use_vector): continue
        ops = [v if use else s for use, v, s in zip(use_vector, (P, F, unit), scalars)]
        full = [v if use else np.full(n, s, dtype=np.float32) for use, v, s in zip(use_vector, (P, F, unit), scalars)]
        for mask in range(1, 8):
            got, want = implied_host(fm, model, *ops, 1.5, 100.0, mask), implied_host(fm, model, *full, 1.5, 100.0, mask)
            assert len(got) == bin(mask).count("1")
            for g, w in zip(got, want): assert (bits(g) == bits(w)).all(), (model, use_vector, mask)


def test_refusals(fm):
    lib, E = fm.lib(), fm._native
    x = np.full(8, 8.0, dtype=np.float32)
    out = [np.zeros(8, dtype=np.float32) for _ in range(3)]
    cols = (C.c_void_p * 3)(*[o.ctypes.data for o in out])
    px = x.ctypes.data_as(C.c_void_p)
    ok = (0, px, 0.0, None, 100.0, None, 1.0, 8, 1.0, 100.0, 7, cols)
    assert lib.fmhip_implied_volatility_host(*ok) == E.OK
    for at, value in ((0, 2), (0, -1), (7, 0), (8, -1.0), (8, math.nan), (8, math.inf), (9, math.nan), (9, math.inf), (10, 0), (10, 8), (11, None)):
        args = list(ok); args[at] = value
        assert lib.fmhip_implied_volatility_host(*args) == E.ERR_INVALID_ARGUMENT, (at, value)
    # the device entry point: refused before the engine is asked for anything (no device here)
    h = (C.c_int64 * 3)()
    assert lib.fmhip_implied_volatility(0, 0, 8.0, 0, 100.0, 0, 1.0, 1.0, 100.0, 1, h) in (E.ERR_INVALID_ARGUMENT, E.ERR_NOT_INITIALIZED)
    assert list(h) == [0, 0, 0]


# ---------------------------------------------------------------- the Python mirrors
def test_deterministic_operands_give_a_deterministic_volatility_in_double(fm):
    for model, sigma in (("black_scholes", 0.2), ("bachelier", 20.0)):
        for F in (80.0, 100.0, 130.0):
            value = fm.option_formula_double(model, F, sigma, 1.5, 100.0, 0.9)
            got = fm.implied_volatility_double(model, value["value"], F, 1.5, 100.0, 0.9)
            unit = fm.option_formula_double(model, F, sigma, 1.5, 100.0, 1.0)
            assert got["volatility"] == pytest.approx(sigma, rel=1e-12) and got["d_price"] == pytest.approx(1.0 / (0.9 * unit["vega"]), rel=1e-9)
            assert got["d_forward"] == pytest.approx(-unit["delta"] / unit["vega"], rel=1e-9)
    r = fm.implied_volatility("black_scholes", fm.RandomVariableHip(1.0, 7.965567455405804), 100.0, 1.0, 100.0, fm.RandomVariableHip(2.0, 1.0), ("volatility", "d_price"))
    assert r[0].isDeterministic() and r[0].getFiltrationTime() == 2.0 and r[0].value == pytest.approx(0.2, rel=1e-12)
    assert fm.bachelier_implied_volatility(20.0 / math.sqrt(2 * math.pi), 100.0, 1.0, 100.0).value == pytest.approx(20.0, rel=1e-14)
    assert fm.implied_volatility_double("black_scholes", 20.0, 120.0, 1.0, 100.0)["volatility"] == 0.0
    assert fm.implied_volatility_double("black_scholes", 120.0, 120.0, 1.0, 100.0)["volatility"] == math.inf
    assert math.isnan(fm.implied_volatility_double("black_scholes", 19.0, 120.0, 1.0, 100.0)["volatility"])
    assert math.isnan(fm.implied_volatility_double("bachelier", 8.0, 100.0, 1.0, 100.0, 0.0)["volatility"])
    host = fm.implied_volatility_host("black_scholes", np.array([7.9655676], dtype=np.float32), 100.0, 1.0, 100.0, 1.0, ("d_price", "volatility"))
    assert host[1][0] == pytest.approx(0.2, rel=1e-6) and host[0][0] == pytest.approx(1.0 / 39.695254747701185, rel=1e-6)      # in the order asked
    with pytest.raises(ValueError): fm.implied_volatility("heston", 1.0, 1.0, 1.0, 1.0)
    with pytest.raises(ValueError): fm.implied_volatility("bachelier", 1.0, 1.0, -1.0, 1.0)
    with pytest.raises(ValueError): fm.implied_volatility("bachelier", 1.0, 1.0, 1.0, 1.0, outputs=("vega",))
    with pytest.raises(ValueError): fm.implied_volatility("bachelier", 1.0, 1.0, 1.0, 1.0, outputs=())


@pytest.mark.parametrize("model", ["black_scholes", "bachelier"])
def test_put_vector_strike_conversion_and_aad_on_the_oracle_backed_factory(fm, oracle, shim, model):
    factory = fm.RandomVariableDifferentiableAADFactory(oracle.RandomVariableFloatFactory())
    rng = np.random.default_rng(21)
    n, T, K = 501, 1.5, 100.0
    scale = 100.0 if model == "bachelier" else 1.0
    F = rng.uniform(70, 140, n).astype(np.float32); sigma = (rng.uniform(0.1, 0.5, n) * scale).astype(np.float32); unit = rng.uniform(0.5, 1.5, n).astype(np.float32)
    call = fm.option_formula_host(model, F, sigma, T, K, unit)[0]
    p, f, u = (factory.createRandomVariable(0.0, a) for a in (call, F, unit))
    # the value and the three partials from one call of the host definition with mask 7 on c = price/unit
    vol, = fm.implied_volatility(model, p, f, T, K, u)
    c32 = np.asarray(p.div(u).getRealizations(), dtype=np.float32)
    want = fm.implied_volatility_host(model, c32, F, T, K, 1.0, ("volatility", "d_price", "d_forward"))
    assert (bits(vol.getRealizations()) == bits(want[0])).all() and np.allclose(want[0], sigma, rtol=1e-4)
    gradient = vol.average().getGradient()
    assert np.allclose(gradient[p.getID()].getRealizations(), want[1] / unit, rtol=1e-6)
    assert np.allclose(gradient[f.getID()].getRealizations(), want[2], rtol=1e-6)
    assert np.allclose(gradient[u.getID()].getRealizations(), -(call / unit) * (want[1] / unit), rtol=1e-5)      # ∂σ/∂N = −(price/N)·∂σ/∂price
    # … against central differences of the definition's doubles
    root = lambda P_, F_, N_: shim.implied(MODELS[model], P_, F_, N_, T, K)[0][:, 0]
    P64, F64, N64 = call.astype(np.float64), F.astype(np.float64), unit.astype(np.float64)
    # (steps of 2^-22 relative: the truncation is below 1e-9 of the partial near the money, the rounding of two fp64 roots below 1e-8 of it)
    near = np.abs(F - K) < 20.0
    for k, (operand, partial) in enumerate(((P64, want[1] / unit), (F64, want[2]), (N64, -(call / unit) * (want[1] / unit)))):
        h = operand * 2.0 ** -22
        up, down = ([P64, F64, N64] for _ in range(2))
        up[k] = operand + h; down[k] = operand - h
        difference = (root(*up) - root(*down)) / (up[k] - down[k])
        assert np.allclose(partial[near], difference[near], rtol=1e-5, atol=0), (model, k)
    # a put by parity
    put = (call.astype(np.float64) - unit.astype(np.float64) * (F.astype(np.float64) - K)).astype(np.float32)
    from_put, = fm.implied_volatility(model, factory.createRandomVariable(0.0, put), f, T, K, u, put=True)
    assert np.allclose(from_put.getRealizations(), sigma, rtol=2e-3)
    # a strike per path: normalised away in the mirror
    Ks = rng.uniform(80, 120, n).astype(np.float32)
    prices = np.array([fm.option_formula_host(model, F[i:i + 1], sigma[i:i + 1], T, float(Ks[i]), 1.0)[0][0] for i in range(n)], dtype=np.float32)
    per_path, = fm.implied_volatility(model, factory.createRandomVariable(0.0, prices), f, T, factory.createRandomVariable(0.0, Ks))
    ok = prices > 1e-3 * Ks                                                  # where the fp32 price still carries the volatility
    assert ok.sum() > n // 2 and np.allclose(np.asarray(per_path.getRealizations())[ok], sigma[ok], rtol=5e-3)
    # the partials asked for by NAME with AAD operands are those in the operands given — a put's, a strike per path, a payoff unit —: what the
    # recorded operations give as the gradient of the volatility
    puts = (unit.astype(np.float64) * (prices.astype(np.float64) - (F.astype(np.float64) - Ks.astype(np.float64)))).astype(np.float32)
    q, k = factory.createRandomVariable(0.0, puts), factory.createRandomVariable(0.0, Ks)
    vol, by_price, by_forward = fm.implied_volatility(model, q, f, T, k, u, ("volatility", "d_price", "d_forward"), put=True)
    gradient = vol.average().getGradient()
    live = np.isfinite(np.asarray(by_price.getRealizations())) & ok
    assert live.sum() > n // 2
    for named, operand in ((by_price, q), (by_forward, f)):
        assert np.allclose(np.asarray(named.getRealizations())[live], np.asarray(gradient[operand.getID()].getRealizations())[live], rtol=2e-5, atol=0), model
    plain = fm.implied_volatility_host(model, (puts / unit + (F - Ks)).astype(np.float32) / (Ks if model == "black_scholes" else np.float32(1.0)),
                                       F / Ks if model == "black_scholes" else F - Ks, T, 1.0 if model == "black_scholes" else 0.0, 1.0, ("d_price",))[0]
    assert np.allclose(np.asarray(by_price.getRealizations())[live], (plain / unit / (Ks if model == "black_scholes" else 1.0))[live], rtol=1e-3)
    # Black → Bachelier → Black (resp. the other way round) closes within the two bounds of check A, plus the fp32 roundings in between
    other = "bachelier" if model == "black_scholes" else "black_scholes"
    s = factory.createRandomVariable(0.0, sigma)
    there = fm.convert_volatility(model, other, f, s, T, K)
    back = fm.convert_volatility(other, model, f, there, T, K)
    near = np.abs(F - K) < 25.0                                              # away from the wings, where an fp32 price has lost the volatility
    assert np.allclose(np.asarray(back.getRealizations())[near], sigma[near], rtol=1e-3)


# ---------------------------------------------------------------- the driver, restated on the device's own draws
DRIVER_CASE = dict(outer=256, inner=64, initial_value=100.0, risk_free_rate=0.05, theta=0.04, kappa=1.5, rho=-0.7, time=1.0, maturity=2.0, steps=10, dt=0.1,
                   moneyness=(0.9, 1.0, 1.1), quantiles=(0.05, 0.5, 0.95), seeds=((4711, 1147), (31415, 27182)))      # (outer, inner) seeds of BrownianMotionHip


def restated_forward_smile(fm, oracle, seed_outer, seed_inner, case=DRIVER_CASE):
    """montecarlo.forward_implied_volatility_mc with xi = 0 and v0 = theta, restated in numpy on THE DRIVER'S draws (oracle.bm_generate gives
    the bits of BrownianMotionHip for a seed): the scheme step by step in fp32, the inner means and the inversion by the host DEFINITIONS
    (fmhip_block_moments_host, fmhip_implied_volatility_host with the per-path strike normalised away), the statistics as the driver's
    docstring states them.  Not the device's bits (numpy's exp and sqrt are not the kernels'), but the same numbers to about 1e-5."""
    from importlib import import_module
    quantile_index = import_module("finmath-lib-cuda-extensions_amd.random_variable").quantile_index
    f32 = np.float32
    outer, inner, r, theta, dt = case["outer"], case["inner"], case["risk_free_rate"], case["theta"], case["dt"]
    span = case["maturity"] - case["time"]
    assert abs(case["steps"] * dt - case["time"]) < 1e-12 and abs(case["steps"] * dt - span) < 1e-12
    step = lambda x, dw: (x + f32(r * dt) + f32(theta) * f32(-0.5 * dt) + np.sqrt(f32(theta)) * dw).astype(f32)      # v stays theta: kappa·(theta − v⁺) = 0
    x = np.full(outer, f32(math.log(case["initial_value"])), dtype=f32)
    for increments in oracle.bm_generate(seed_outer, [dt] * case["steps"], 2, outer): x = step(x, increments[0])
    x_T = np.repeat(x, inner)
    for increments in oracle.bm_generate(seed_inner, [dt] * case["steps"], 2, outer * inner): x_T = step(x_T, increments[0])
    forward = (np.exp(x) * f32(math.exp(r * span))).astype(f32)
    rows = []
    for m in case["moneyness"]:
        strike = (forward * f32(m)).astype(f32)
        payoff = np.maximum(np.exp(x_T).astype(f32) - np.repeat(strike, inner), 0).astype(f32)
        price = fm.block_moments_host(payoff, inner, ("mean",))[0]
        sigma = fm.implied_volatility_host("black_scholes", (price / strike).astype(f32), (forward / strike).astype(f32), span, 1.0)[0]
        valid = np.isfinite(sigma) & (sigma > 0)
        share = float(valid.mean())
        clean = np.where(valid, sigma, f32(0)).astype(np.float64)
        mean = float(clean.mean() / share)
        error = math.sqrt(max(float((clean * clean).mean()) / share - mean * mean, 0.0) / (outer * share))
        ascending = np.sort(clean)
        rows.append({"moneyness": m, "mean": mean, "standard_error": error, "not_invertible": 1.0 - share,
                     "quantiles": [float(ascending[quantile_index(outer, q * share)]) for q in case["quantiles"]]})
    return rows


def test_the_restatement_of_the_forward_implied_volatility_on_the_drivers_draws(fm, oracle):
    """The check that comes BEFORE tests/test_gpu_implied_volatility.py runs the driver itself at 256 outer × 64 inner paths with xi = 0 and
    v0 = theta (Black–Scholes with sigma = √theta, for which the log-Euler scheme is exact): on the same draws the host definitions alone give
    a mean future implied volatility at moneyness 1 within 5 of its standard errors of √theta, and every outer price is invertible (at the
    forward at-the-money strike a zero price needs all 64 payoffs to be zero), for both pairs of seeds that the GPU test uses."""
    for seed_outer, seed_inner in DRIVER_CASE["seeds"]:
        rows = restated_forward_smile(fm, oracle, seed_outer, seed_inner)
        at_the_money = rows[1]
        print(f"seeds {seed_outer}, {seed_inner}: " + "; ".join(f"m = {row['moneyness']}: {row['mean']:.5f} +- {row['standard_error']:.5f}, {row['not_invertible']:.4f} not invertible" for row in rows))
        assert at_the_money["moneyness"] == 1.0 and at_the_money["not_invertible"] == 0.0
        assert abs(at_the_money["mean"] - math.sqrt(DRIVER_CASE["theta"])) <= 5 * at_the_money["standard_error"]
        for row in rows: assert row["quantiles"] == sorted(row["quantiles"], reverse=True) and 0.0 < row["standard_error"] < 0.01


# ---------------------------------------------------------------- the host half under the sanitizers
def test_host_half_under_the_sanitizers(tmp_path):
    """tests/cpp/test_implied_volatility_host.cpp, a stand-alone program: the argument check, every line of the semantics, a sweep of bit patterns."""
    gxx = shutil.which("g++")
    if not gxx: pytest.skip("needs g++")
    exe = tmp_path / "implied_volatility_host"
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-ffp-contract=off",
                        os.path.join(ROOT, "tests", "cpp", "test_implied_volatility_host.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "implied volatility host ok" in r.stdout and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stdout[-1500:] + r.stderr[-3000:]


def test_the_kernel_is_in_the_library(fm):
    """A missing kernel is an error, never a fallback: the launcher is a weak reference, so the library must be shown to hold it."""
    out = subprocess.check_output(["nm", "-D", "--defined-only", fm._native.LIB_PATH], text=True) + subprocess.check_output(["nm", "--defined-only", fm._native.LIB_PATH], text=True, stderr=subprocess.DEVNULL)
    assert "launch_implied_volatility" in out
    assert b"fm_implied_volatility_kernel" in open(fm._native.LIB_PATH, "rb").read()


def test_the_kernel_compiles_for_gfx950_without_scratch():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc): pytest.skip("needs hipcc")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                        "-c", os.path.join(CSRC, "implied_volatility_kernel.hip"), "-o", os.devnull], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    seen = {}
    for blk in re.split(r"remark: Function Name: ", r.stderr)[1:]:
        seen[blk.split()[0]] = tuple(int(re.search(pattern, blk).group(1)) for pattern in (r"ScratchSize \[bytes/lane\]: (\d+)", r"LDS Size \[bytes/block\]: (\d+)", r" VGPRs: (\d+)", r"Occupancy \[waves/SIMD\]: (\d+)"))
    kernels = {k: v for k, v in seen.items() if "fm_implied_volatility_kernel" in k}
    assert len(kernels) == 2, seen                                           # two models
    for name, (scratch, lds, vgprs, waves) in sorted(kernels.items()):
        print(f"{name}: {vgprs} VGPRs, {waves} waves per SIMD, {scratch} bytes of scratch, {lds} bytes of LDS")
        assert scratch == 0 and lds == 0 and vgprs <= 256, (name, scratch, lds, vgprs)


# ---------------------------------------------------------------- the engine's side on the null device
@pytest.fixture(scope="module")
def built():
    if not shutil.which("g++") or not os.path.exists("/opt/rocm/include/hip/hip_runtime_api.h"):
        pytest.skip("needs g++ and the HIP headers")
    r = subprocess.run(["make", "-C", NULLDEV, "-f", "implied_volatility.mk", "-j8", "implied_volatility_asan", "implied_volatility_tsan", "implied_volatility_absent_asan", "implied_volatility_absent_tsan"],
                       capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return os.path.join(NULLDEV, "build")


def _env(tmp_path, env):
    return dict(os.environ, FMHIP_JIT_CACHE_DIR=str(tmp_path / "code_objects"), FMHIP_JIT_PACK_DIR="off", FMHIP_RING_BYTES="16384", FMHIP_ARENA_BYTES="4096",
                ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1", TSAN_OPTIONS="halt_on_error=1", **env)


@pytest.mark.parametrize("env", [{}, {"FMNULL_DEVICES": "2"}, {"FMNULL_THREAD_ENGINES": "1"}])
def test_engine_pass_is_clean_under_the_sanitizers(built, tmp_path, env):
    """drive_implied_volatility: fmhip_implied_volatility on vectors of real data at n = 1 … 100 003, checked against the host entry point;
    pending operands, a given-up operand, every argument refusal with nothing flushed or allocated — on one engine, behind a device list of
    two (every shard its block), with thread engines (a caller that does not own the vectors)."""
    full = _env(tmp_path, env)
    a = subprocess.run([os.path.join(built, "drive_implied_volatility_asan")], capture_output=True, text=True, timeout=600, env=full)
    assert a.returncode == 0 and "Sanitizer" not in a.stderr and "runtime error" not in a.stderr, a.stdout[-500:] + a.stderr[-6000:]
    assert "implied volatility done" in a.stdout and a.stderr == ""
    t = subprocess.run([os.path.join(built, "drive_implied_volatility_tsan")], capture_output=True, text=True, timeout=600, env=full)
    assert t.returncode == 0 and "ThreadSanitizer" not in t.stderr, t.stdout[-500:] + t.stderr[-6000:]
    assert "implied volatility done" in t.stdout and t.stderr == ""


def test_a_failing_allocation_leaves_nothing_behind(built, tmp_path):
    """One fmhip_implied_volatility of three outputs: THREE buffers from the pool, the outputs.  FMHIP_TEST_FAIL_ALLOC_AT is set on each of them
    (their positions from a counting run), and once where nothing reaches it: the call answers FMHIP_OK or FMHIP_ERR_OUT_OF_MEMORY, a failed
    call writes no handle, live vectors and bytes in use are what they were, the same call succeeds afterwards (the driver checks all of
    it), and the process ends without a leak."""
    exe = os.path.join(built, "drive_implied_volatility_asan")
    counting = subprocess.run([exe, "failure"], capture_output=True, text=True, timeout=600, env=_env(tmp_path, {}))
    assert counting.returncode == 0 and "Sanitizer" not in counting.stderr, counting.stdout[-500:] + counting.stderr[-6000:]
    before, inside, status = map(int, re.search(r"failure: (\d+) allocations before the call, (\d+) in it, status (-?\d+)", counting.stdout).groups())
    assert inside == 3 and status == 0
    for at in list(range(before + 1, before + inside + 1)) + [10**9]:
        r = subprocess.run([exe, "failure"], capture_output=True, text=True, timeout=600, env=_env(tmp_path, {"FMHIP_TEST_FAIL_ALLOC_AT": str(at)}))
        assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr and r.stderr == "", (at, r.stdout[-500:] + r.stderr[-6000:])
        assert "failure done" in r.stdout
        failed = int(re.search(r"status (-?\d+)", r.stdout).group(1)) != 0
        assert failed == (at <= before + inside), (at, r.stdout)


@pytest.mark.parametrize("env", [{}, {"FMNULL_DEVICES": "2"}, {"FMNULL_THREAD_ENGINES": "1"}])
def test_a_build_without_the_kernel_answers_unsupported(built, tmp_path, env):
    a = subprocess.run([os.path.join(built, "drive_implied_volatility_absent_asan")], capture_output=True, text=True, timeout=600, env=_env(tmp_path, env))
    assert a.returncode == 0 and "Sanitizer" not in a.stderr and "runtime error" not in a.stderr, a.stdout[-500:] + a.stderr[-6000:]
    assert "implied volatility absent done" in a.stdout
    t = subprocess.run([os.path.join(built, "drive_implied_volatility_absent_tsan")], capture_output=True, text=True, timeout=600, env=_env(tmp_path, env))
    assert t.returncode == 0 and "ThreadSanitizer" not in t.stderr, t.stdout[-500:] + t.stderr[-6000:]
    assert "implied volatility absent done" in t.stdout
