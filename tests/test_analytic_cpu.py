"""Named functions and option formulas without a GPU (include/fmhip.h: fmhip_function_apply_host, fmhip_option_formula_host;
host/normal_functions.hpp; analytic.py): the generated coefficient header against its generator; the host DEFINITION against
mpmath at 50 digits — the fp64 distribution function and density within 2^-40 relative over fp32 arguments, every fp32 result within one ulp
of the correctly rounded one, the quantile's error measured —; the edge list; monotonicity; Φ⁻¹(Φ(x)) within the conditioning bound; the
formulas against mpmath within the bound of DESIGN.md §4.21, their degenerate elements, delta and vega against central differences, every
combination of vector and scalar operands; the Python mirrors and AAD on the oracle's float class against finite differences; the host half
under the sanitizers (tests/cpp/test_analytic_host.cpp); the engine's side on the null device under ASan/UBSan and TSan
(tests/nulldev/analytic.mk); the kernels' resource usage for gfx950 (0 bytes of scratch, the VGPR counts printed)."""
import ctypes as C
import itertools
import math
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "finmath-lib-cuda-extensions_amd")
CSRC = os.path.join(PKG, "csrc")
NULLDEV = os.path.join(ROOT, "tests", "nulldev")
GENERATOR = os.path.join(ROOT, "tools", "normal_cdf_coefficients.py")
HEADER = os.path.join(PKG, "host", "normal_cdf_coefficients.hpp")
PD = C.POINTER(C.c_double)

CDF, DENSITY, QUANTILE = 0, 1, 2
MODELS = {"black_scholes": 0, "bachelier": 1}
CANONICAL_NAN = 0x7fc00000
BOUND = 2.0 ** -40                    # the accuracy condition of the fp64 Φ and φ over fp32 arguments
CDF_RANGE = (-14.3, 8.3)
DENSITY_RANGE = (-14.3, 14.3)
# |host − exact| <= 2^-24·|exact| + FORMULA_C[model]·2^-50·|N|·(|F| + |K|): four times the c measured on the grid below, of the fp64 values
# (printed by the test: 9.68e3 for Black–Scholes — the 2^-53 of log(F/K) divided by s = 1e-6, next to the money — and 0.62 for Bachelier)
FORMULA_C = {0: 4.0e4, 1: 2.5}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def ordered(a):
    """fp32 bit patterns as integers in the order of the values (−0 and +0 adjacent)."""
    b = bits(a).astype(np.int64)
    return np.where(b & 0x80000000, -(b & 0x7fffffff) - 1, b)


def f32_between(lo, hi, count):
    """About `count` fp32 numbers of [lo, hi], strided evenly through the BIT PATTERNS (so denormals and every binade are met)."""
    lo_o, hi_o = (int(ordered(np.array([v], dtype=np.float32))[0]) for v in (lo, hi))
    o = np.unique(np.linspace(lo_o, hi_o, count).astype(np.int64))
    b = np.where(o < 0, (-(o + 1)) | 0x80000000, o).astype(np.uint32)
    x = b.view(np.float32)
    return x[(x >= np.float32(lo)) & (x <= np.float32(hi))]


def neighbours(values, k=3):
    out = []
    for v in values:
        up = down = np.float32(v)
        out.append(up)
        for _ in range(k):
            up = np.nextafter(up, np.float32(np.inf)); down = np.nextafter(down, np.float32(-np.inf))
            out += [up, down]
    return np.array(out, dtype=np.float32)


def mills_breaks():
    text = open(HEADER, encoding="utf-8").read()
    return [float.fromhex(h) for h in re.search(r"FM_MILLS_BREAKS\[[^\]]*\] = \{([^}]*)\}", text).group(1).replace(" ", "").split(",")]


def sweep(lo, hi):
    """The arguments the accuracy condition is checked on: bit patterns strided over [lo, hi], a uniform grid of values, a dense
    neighbourhood of 0 (the first 64 denormals of either sign among it), every branch boundary of Φ with its fp32 neighbours."""
    breaks = [b for b in mills_breaks() if b <= hi]
    dense = np.concatenate([np.arange(0, 64, dtype=np.uint32).view(np.float32), np.linspace(0, 2.0 ** -10, 97, dtype=np.float32), 2.0 ** -np.arange(1, 127, 5, dtype=np.float32)])
    x = np.concatenate([f32_between(lo, hi, 1500), np.linspace(lo, hi, 1200).astype(np.float32), dense, -dense, neighbours(breaks), -neighbours(breaks), neighbours([lo, hi])])
    x = np.unique(x[(x >= np.float32(lo)) & (x <= np.float32(hi))])
    return np.sort(x)


def mp50():
    mpmath = pytest.importorskip("mpmath")
    mpmath.mp.dps = 50
    return mpmath


def correctly_rounded(mpmath, exact):
    """The fp32 number nearest to the mpmath value (ties cannot be told apart at 50 digits and do not occur for these functions)."""
    c = np.float32(float(exact))
    best = c
    for cand in (np.nextafter(c, np.float32(np.inf)), np.nextafter(c, np.float32(-np.inf))):
        if np.isfinite(cand) and abs(mpmath.mpf(float(cand)) - exact) < abs(mpmath.mpf(float(best)) - exact): best = cand
    return best


# ---------------------------------------------------------------- the library's host entry points and the fp64 shim
def apply_host(fm, x, kinds):
    x = np.ascontiguousarray(x, dtype=np.float32)
    kinds = np.array(kinds, dtype=np.int32)
    out = [np.full(x.size, -7.0, dtype=np.float32) for _ in kinds]
    cols = (C.c_void_p * len(out))(*[o.ctypes.data for o in out])
    fm._native.check(fm.lib().fmhip_function_apply_host(x.ctypes.data_as(C.c_void_p), x.size, kinds.ctypes.data_as(C.POINTER(C.c_int32)), kinds.size, cols))
    return out


def formula_host(fm, model, F, sigma, unit, T, K, mask):
    """fmhip_option_formula_host through ctypes: F, sigma, unit are float32 arrays or floats; the columns in bit order."""
    ops = [F, sigma, unit]
    n = next(np.asarray(o).size for o in ops if not np.isscalar(o))
    arrays = [None if np.isscalar(o) else np.ascontiguousarray(o, dtype=np.float32) for o in ops]
    scalars = [float(o) if np.isscalar(o) else 0.0 for o in ops]
    out = [np.full(n, -7.0, dtype=np.float32) for _ in range(bin(mask).count("1"))]
    cols = (C.c_void_p * len(out))(*[o.ctypes.data for o in out])
    ptr = [a.ctypes.data_as(C.c_void_p) if a is not None else None for a in arrays]
    fm._native.check(fm.lib().fmhip_option_formula_host(model, ptr[0], scalars[0], ptr[1], scalars[1], ptr[2], scalars[2], n, float(T), float(K), mask, cols))
    return out


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    """tests/cpp/analytic_double_shim.cpp: the definition's DOUBLES (the library narrows to fp32), built with the library's flags."""
    gxx = shutil.which("g++")
    if not gxx: pytest.skip("needs g++")
    so = tmp_path_factory.mktemp("analytic_shim") / "libanalytic_shim.so"
    r = subprocess.run([gxx, "-std=c++17", "-O2", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Werror",
                        os.path.join(ROOT, "tests", "cpp", "analytic_double_shim.cpp"), "-o", str(so)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    lib = C.CDLL(str(so))
    lib.shim_function64.argtypes = [C.c_int, PD, C.c_int64, PD]
    lib.shim_formula64.argtypes = [C.c_int, PD, PD, PD, C.c_int64, C.c_double, C.c_double, PD]

    class Shim:
        @staticmethod
        def function(kind, x):
            x = np.ascontiguousarray(x, dtype=np.float64); out = np.empty_like(x)
            lib.shim_function64(kind, x.ctypes.data_as(PD), x.size, out.ctypes.data_as(PD))
            return out

        @staticmethod
        def formula(model, F, sigma, unit, T, K):
            F, sigma, unit = (np.ascontiguousarray(np.broadcast_to(np.asarray(a, dtype=np.float64), np.broadcast(F, sigma, unit).shape)).ravel() for a in (F, sigma, unit))
            out = np.empty((F.size, 3))
            lib.shim_formula64(model, F.ctypes.data_as(PD), sigma.ctypes.data_as(PD), unit.ctypes.data_as(PD), F.size, float(T), float(K), out.ctypes.data_as(PD))
            return out
    return Shim


# ---------------------------------------------------------------- the generated header
def test_the_generated_header_equals_the_committed_one():
    pytest.importorskip("mpmath")
    r = subprocess.run([sys.executable, GENERATOR, "--check"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr


def test_the_header_check_sees_drift(tmp_path):
    pytest.importorskip("mpmath")
    tools = tmp_path / "tools"; host = tmp_path / "finmath-lib-cuda-extensions_amd" / "host"
    tools.mkdir(); host.mkdir(parents=True)
    (tools / "normal_cdf_coefficients.py").write_text(open(GENERATOR, encoding="utf-8").read(), encoding="utf-8")
    text = open(HEADER, encoding="utf-8").read()
    assert text.count("FM_MILLS_DEGREE = ") == 1
    (host / "normal_cdf_coefficients.hpp").write_text(text.replace("p-1, ", "p-2, ", 1), encoding="utf-8")
    r = subprocess.run([sys.executable, str(tools / "normal_cdf_coefficients.py"), "--check"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 1 and "DRIFT" in r.stdout


# ---------------------------------------------------------------- accuracy against mpmath
@pytest.fixture(scope="module")
def cdf_reference():
    mpmath = mp50()
    x = sweep(*CDF_RANGE)
    return x, [mpmath.ncdf(mpmath.mpf(float(v))) for v in x]


@pytest.fixture(scope="module")
def density_reference():
    mpmath = mp50()
    x = sweep(*DENSITY_RANGE)
    return x, [mpmath.npdf(mpmath.mpf(float(v))) for v in x]


def relative_errors(mpmath, got64, exact):
    return np.array([float(abs(mpmath.mpf(float(g)) - e) / e) for g, e in zip(got64, exact)])


def one_ulp(mpmath, got32, exact, what):
    rounded = np.array([correctly_rounded(mpmath, e) for e in exact], dtype=np.float32)
    distance = np.abs(ordered(got32) - ordered(rounded))
    print(f"{what}: {int((distance != 0).sum())} of {distance.size} fp32 results are not the correctly rounded one, none further than {int(distance.max())} ulp")
    assert distance.max() <= 1, (what, np.flatnonzero(distance > 1)[:5])


def test_the_distribution_function_is_within_2_to_the_minus_40(fm, shim, cdf_reference):
    mpmath = mp50()
    x, exact = cdf_reference
    assert x.size > 2500 and x[0] == np.float32(-14.3) and x[-1] == np.float32(8.3) and (x == 0).any()
    err = relative_errors(mpmath, shim.function(CDF, x.astype(np.float64)), exact)
    worst = int(err.argmax())
    print(f"Phi: max relative error of the fp64 value 2^{math.log2(err.max()):.2f} at x = {x[worst]!r} over {x.size} fp32 arguments in [-14.3, 8.3]")
    assert err.max() <= BOUND
    one_ulp(mpmath, apply_host(fm, x, [CDF])[0], exact, "Phi")


def test_the_density_is_within_2_to_the_minus_40(fm, shim, density_reference):
    mpmath = mp50()
    x, exact = density_reference
    err = relative_errors(mpmath, shim.function(DENSITY, x.astype(np.float64)), exact)
    worst = int(err.argmax())
    print(f"phi: max relative error of the fp64 value 2^{math.log2(err.max()):.2f} at x = {x[worst]!r} over {x.size} fp32 arguments in [-14.3, 14.3]")
    assert err.max() <= BOUND
    one_ulp(mpmath, apply_host(fm, x, [DENSITY])[0], exact, "phi")


def test_the_distribution_function_of_a_double_keeps_its_accuracy(shim):
    """Inside the formulas Φ takes doubles that are no fp32 numbers: the same bound on random doubles of [-14.3, 8.3] (the square is rounded:
    |X|²·2^-54 more, 2^-46 at the far end)."""
    mpmath = mp50()
    x = np.random.default_rng(5).uniform(CDF_RANGE[0], CDF_RANGE[1], 600)
    err = relative_errors(mpmath, shim.function(CDF, x), [mpmath.ncdf(mpmath.mpf(float(v))) for v in x])
    print(f"Phi of doubles: max relative error 2^{math.log2(err.max()):.2f}")
    assert err.max() <= BOUND


def test_the_quantile_error_is_measured(fm, shim):
    """Measured, not asserted beyond sanity: |Φ⁻¹ − exact| relative, fp64, over fp32 u strided through the bit patterns of (0, 1)."""
    mpmath = mp50()
    u = np.concatenate([f32_between(1e-45, 1.0 - 2.0 ** -24, 500), np.linspace(0.001, 0.999, 200).astype(np.float32), neighbours([0.075, 0.925, 0.5], 2)])
    u = np.unique(u[(u > 0) & (u < 1)])
    got = shim.function(QUANTILE, u.astype(np.float64))
    exact = [mpmath.sqrt(2) * mpmath.erfinv(2 * mpmath.mpf(float(v)) - 1) if v >= 0.25 else -mpmath.sqrt(2) * mpmath.erfinv(1 - 2 * mpmath.mpf(float(v))) for v in u]
    exact = [mpmath.findroot(lambda q, v=v: mpmath.ncdf(q) - mpmath.mpf(float(v)), e) if abs(e) > 3 else e for v, e in zip(u, exact)]
    err = np.array([float(abs(mpmath.mpf(float(g)) - e) / abs(e)) if e != 0 else abs(float(g)) for g, e in zip(got, exact)])
    print(f"quantile: max relative error of the fp64 value 2^{math.log2(max(err.max(), 2.0 ** -60)):.2f} at u = {u[int(err.argmax())]!r} over {u.size} fp32 arguments in (0, 1)")
    assert err.max() < 1e-9                                                  # sanity only: the figure is recorded, not bounded
    got32 = apply_host(fm, u, [QUANTILE])[0]
    assert np.isfinite(got32).all() and (np.diff(got32[np.argsort(u)]) >= 0).all()


# ---------------------------------------------------------------- edges, monotonicity, the round trip
def edge_inputs():
    tiny = np.array([1, 2, 0x007fffff, 0x00800000], dtype=np.uint32).view(np.float32)
    return np.concatenate([np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, 1.0 - 2.0 ** -24, -1.0, 2.0, 0.5, -14.3, 14.3, -8.0, 8.0], dtype=np.float32), tiny, -tiny])


def test_the_edge_list(fm):
    x = edge_inputs()
    cdf, den, q, again = apply_host(fm, x, [CDF, DENSITY, QUANTILE, CDF])
    assert (bits(cdf) == bits(again)).all()
    where = {float(v) if v == v else "nan": i for i, v in enumerate(x) if not (v == 0 and np.signbit(v))}

    class at:                                                               # at[-14.3]: the position of the fp32 number nearest to −14.3
        def __class_getitem__(cls, k): return where[k if isinstance(k, str) else float(np.float32(k))]
    for zero in np.flatnonzero(x == 0): assert cdf[zero] == 0.5 and den[zero] == np.float32(0.3989422804014327) and q[zero] == -np.inf
    assert cdf[at[np.inf]] == 1.0 and den[at[np.inf]] == 0.0 and bits(q)[at[np.inf]] == CANONICAL_NAN
    assert cdf[at[-np.inf]] == 0.0 and den[at[-np.inf]] == 0.0 and bits(q)[at[-np.inf]] == CANONICAL_NAN
    assert bits(cdf)[at["nan"]] == CANONICAL_NAN and bits(den)[at["nan"]] == CANONICAL_NAN and bits(q)[at["nan"]] == CANONICAL_NAN
    assert q[at[1.0]] == np.inf and bits(q)[at[-1.0]] == CANONICAL_NAN and bits(q)[at[2.0]] == CANONICAL_NAN and q[at[0.5]] == 0.0
    last = q[at[float(np.float32(1.0 - 2.0 ** -24))]]
    from statistics import NormalDist
    assert np.isfinite(last) and abs(last - NormalDist().inv_cdf(1.0 - 2.0 ** -24)) < 1e-6 * last          # Φ⁻¹(1 − 2^-24) = 5.29…
    denormal = np.array([1], dtype=np.uint32).view(np.float32)[0]
    smallest = q[at[float(denormal)]]
    assert np.isfinite(smallest) and abs(smallest - NormalDist().inv_cdf(2.0 ** -149)) < 1e-6 * abs(smallest)   # Φ⁻¹(2^-149) = −14.1…
    for i, v in enumerate(x):
        if v == v and abs(v) < 1e-37:                                        # denormals and the smallest normal: Φ is ½, φ its maximum
            assert cdf[i] == 0.5 and den[i] == np.float32(0.3989422804014327)
        if v == v and v < 0: assert bits(q)[i] == CANONICAL_NAN or v == 0
    assert cdf[at[-14.3]] == 0.0 and cdf[at[14.3]] == 1.0 and 0 < cdf[at[-8.0]] < 1e-15 and cdf[at[8.0]] == 1.0


def test_the_distribution_function_does_not_decrease(fm):
    x = np.sort(np.concatenate([f32_between(-15.0, 9.0, 200_000), np.linspace(-15, 9, 100_001).astype(np.float32), neighbours(mills_breaks(), 8), -neighbours(mills_breaks(), 8)]))
    cdf = apply_host(fm, x, [CDF])[0]
    assert (np.diff(cdf) >= 0).all(), x[np.flatnonzero(np.diff(cdf) < 0)[:5]]
    assert cdf[0] == 0.0 and cdf[-1] == 1.0


def test_the_quantile_of_the_distribution_function_closes(fm):
    """q = Φ⁻¹(p), p = (float)Φ(x) within (½ + 2^-16) ulp of Φ(x): by the mean value theorem |q − x| <= |δp| / min(φ(x), φ(q)) (φ is unimodal:
    its minimum over an interval is at an end), plus the narrowing of q to fp32 and AS 241's own error (1e-15 relative, as measured)."""
    x = np.concatenate([np.linspace(-8.0, 5.0, 4001), np.random.default_rng(2).normal(size=4000)]).astype(np.float32)
    p = apply_host(fm, x, [CDF])[0]
    q = apply_host(fm, p, [QUANTILE])[0].astype(np.float64)
    ok = (p > 0) & (p < 1)
    assert ok.sum() > 7900
    X, Q = x.astype(np.float64)[ok], q[ok]
    density = lambda v: np.exp(-0.5 * v * v) / math.sqrt(2 * math.pi)
    dp = (0.5 + 2.0 ** -16) * np.spacing(p[ok]).astype(np.float64)
    bound = dp / np.minimum(density(X), density(Q)) + 2.0 ** -24 * np.abs(Q) + 1e-14 * (1 + np.abs(Q))
    assert (np.abs(Q - X) <= bound).all(), (X[np.abs(Q - X) > bound][:5], Q[np.abs(Q - X) > bound][:5])


# ---------------------------------------------------------------- the formulas
def exact_formula(mpmath, model, F, sigma, unit, T, K):
    F, sigma, unit, T, K = (mpmath.mpf(float(v)) for v in (F, sigma, unit, T, K))
    s = sigma * mpmath.sqrt(T)
    if not (s > 0 and (model != 0 or (F > 0 and K > 0))):
        return unit * max(F - K, 0), unit * (1 if F > K else 0), mpmath.mpf(0)
    if model == 0:
        d1 = (mpmath.log(F / K) + s * s / 2) / s
        return unit * (F * mpmath.ncdf(d1) - K * mpmath.ncdf(d1 - s)), unit * mpmath.ncdf(d1), unit * F * mpmath.npdf(d1) * mpmath.sqrt(T)
    d = (F - K) / s
    return unit * ((F - K) * mpmath.ncdf(d) + s * mpmath.npdf(d)), unit * mpmath.ncdf(d), unit * mpmath.sqrt(T) * mpmath.npdf(d)


def formula_grid(model):
    """(F, sigma, unit, T, K) with σ√T from 1e-6 to 10, the forward from deep out of to deep in the money, and the degenerate cases."""
    K = 100.0
    rows = []
    for T in (0.25, 1.0, 4.0):
        for s in (1e-6, 1e-4, 1e-2, 0.1, 0.3, 1.0, 3.0, 10.0):
            sigma = s / math.sqrt(T) * (K if model == 1 else 1.0)
            for moneyness in (0.01, 0.5, 0.9, 0.999, 1.0, 1.001, 1.1, 2.0, 100.0, 1.0 + s, 1.0 - 2.0 * s, math.exp(3.0 * s), math.exp(-5.0 * s)):
                if model == 0 and not moneyness > 0.0: continue
                for unit in (1.0, 0.37):
                    rows.append((K * moneyness, sigma, unit, T, K))
    rows += [(120.0, 0.0, 2.0, 1.0, K), (80.0, 0.0, 2.0, 1.0, K), (120.0, -0.2, 2.0, 1.0, K), (120.0, 0.2, 2.0, 0.0, K), (80.0, 0.2, 2.0, 0.0, K)]      # s <= 0
    rows += [(0.0, 0.2, 1.0, 1.0, K), (-3.0, 0.2, 1.0, 1.0, K), (100.0, 0.2, 1.0, 1.0, 0.0), (100.0, 0.2, 1.0, 1.0, -5.0), (-7.0, 0.2, 1.0, 1.0, -5.0)]   # F <= 0, K <= 0
    return [tuple(float(np.float32(v)) if i < 3 else v for i, v in enumerate(r)) for r in rows]


@pytest.mark.parametrize("model", [0, 1])
def test_the_formulas_against_mpmath(fm, shim, model):
    mpmath = mp50()
    c_measured = 0.0
    worst = None
    for (T, K), group in itertools.groupby(sorted(formula_grid(model), key=lambda r: (r[3], r[4])), key=lambda r: (r[3], r[4])):
        group = list(group)
        F, sigma, unit = (np.array([r[i] for r in group], dtype=np.float32) for i in range(3))
        host = formula_host(fm, model, F, sigma, unit, T, K, 7)
        host64 = shim.formula(model, F, sigma, unit, T, K)
        for p, r in enumerate(group):
            exact = exact_formula(mpmath, model, *r)
            degenerate = not (r[1] * math.sqrt(T) > 0 and (model != 0 or (r[0] > 0 and K > 0)))
            scale = abs(r[2]) * (abs(r[0]) + abs(K))
            for o in range(3):
                got = mpmath.mpf(float(host[o][p]))
                if degenerate:
                    assert host[o][p] == np.float32(float(exact[o])), (model, r, o)
                    continue
                assert host[o][p] == np.float32(host64[p, o])                # the entry point narrows the definition's double, once
                c = float(abs(mpmath.mpf(float(host64[p, o])) - exact[o]) / (mpmath.mpf(2) ** -50 * scale))      # of the fp64 value: what is left after the narrowing
                if c > c_measured: c_measured, worst = c, (r, o)
                assert abs(got - exact[o]) <= mpmath.mpf(2) ** -24 * abs(exact[o]) + FORMULA_C[model] * mpmath.mpf(2) ** -50 * scale, (model, r, o, float(got), float(exact[o]), c)
    print(f"model {model}: measured c = {c_measured:.3g} at {worst} (asserted: {FORMULA_C[model]}, four times it, rounded up)")
    assert 4 * c_measured <= FORMULA_C[model]


@pytest.mark.parametrize("model", [0, 1])
def test_delta_and_vega_are_the_derivatives_of_the_value(shim, model):
    """Central differences of the fp64 value with steps h = 2^-14·(F resp. σ): truncation h²/6·|∂³V| <= 2^-28·scale·(1/s² + 1) for s = σ√T in
    [0.1, 1] at these moneynesses, rounding 2^-50·scale/(h/scale): both far below the 1e-6·scale asserted."""
    K, T = 100.0, 1.0
    for F in (60.0, 95.0, 100.0, 130.0):
        for s in (0.1, 0.3, 1.0):
            sigma = s * (K if model == 1 else 1.0)
            hF, hS = F * 2.0 ** -14, sigma * 2.0 ** -14
            base = shim.formula(model, F, sigma, 1.0, T, K)[0]
            up, down = shim.formula(model, F + hF, sigma, 1.0, T, K)[0, 0], shim.formula(model, F - hF, sigma, 1.0, T, K)[0, 0]
            assert abs((up - down) / (2 * hF) - base[1]) <= 1e-6, (model, F, s)
            up, down = shim.formula(model, F, sigma + hS, 1.0, T, K)[0, 0], shim.formula(model, F, sigma - hS, 1.0, T, K)[0, 0]
            assert abs((up - down) / (2 * hS) - base[2]) <= 1e-6 * max(1.0, abs(base[2])), (model, F, s)


@pytest.mark.parametrize("model", [0, 1])
def test_every_combination_of_vector_and_scalar_operands_gives_the_bits_of_the_broadcast_call(fm, model):
    rng = np.random.default_rng(11)
    n = 1003
    F = rng.uniform(50, 150, n).astype(np.float32); sigma = (rng.uniform(0.05, 0.6, n) * (100.0 if model == 1 else 1.0)).astype(np.float32)
    unit = rng.uniform(0.5, 1.5, n).astype(np.float32)
    F[::97] = -1.0; sigma[5::101] = 0.0; unit[7::103] = np.nan
    scalars = (101.25, 0.3125 * (100.0 if model == 1 else 1.0), 0.75)          # doubles that are fp32 numbers: the broadcast array holds them exactly
    for use_vector in itertools.product([True, False], repeat=3):
        if not any(use_vector): continue
        ops = [v if use else s for use, v, s in zip(use_vector, (F, sigma, unit), scalars)]
        full = [v if use else np.full(n, s, dtype=np.float32) for use, v, s in zip(use_vector, (F, sigma, unit), scalars)]
        for mask in range(1, 8):
            got, want = formula_host(fm, model, *ops, 1.5, 100.0, mask), formula_host(fm, model, *full, 1.5, 100.0, mask)
            assert len(got) == bin(mask).count("1")
            for g, w in zip(got, want): assert (bits(g) == bits(w)).all(), (model, use_vector, mask)
    # a mask's columns are the columns of the full mask
    all_three = formula_host(fm, model, F, sigma, unit, 1.5, 100.0, 7)
    for mask in range(1, 8):
        want = [all_three[b] for b in range(3) if mask >> b & 1]
        for g, w in zip(formula_host(fm, model, F, sigma, unit, 1.5, 100.0, mask), want): assert (bits(g) == bits(w)).all()


def test_refusals(fm):
    lib, E = fm.lib(), fm._native
    x = np.zeros(8, dtype=np.float32); kinds = np.array([0, 1, 2, 0], dtype=np.int32)
    out = [np.zeros(8, dtype=np.float32) for _ in range(4)]
    cols = (C.c_void_p * 4)(*[o.ctypes.data for o in out])
    px, pk = x.ctypes.data_as(C.c_void_p), kinds.ctypes.data_as(C.POINTER(C.c_int32))
    assert lib.fmhip_function_apply_host(px, 8, pk, 4, cols) == E.OK
    for args in ((None, 8, pk, 1, cols), (px, 0, pk, 1, cols), (px, 8, None, 1, cols), (px, 8, pk, 0, cols), (px, 8, pk, 5, cols), (px, 8, pk, 1, None)):
        assert lib.fmhip_function_apply_host(*args) == E.ERR_INVALID_ARGUMENT, args
    bad = np.array([3], dtype=np.int32)
    assert lib.fmhip_function_apply_host(px, 8, bad.ctypes.data_as(C.POINTER(C.c_int32)), 1, cols) == E.ERR_INVALID_ARGUMENT
    ok = (0, px, 0.0, None, 0.2, None, 1.0, 8, 1.0, 100.0, 7, cols)
    assert lib.fmhip_option_formula_host(*ok) == E.OK
    for at, value in ((0, 2), (0, -1), (7, 0), (8, -1.0), (8, math.nan), (8, math.inf), (9, math.nan), (9, math.inf), (10, 0), (10, 8), (11, None)):
        args = list(ok); args[at] = value
        assert lib.fmhip_option_formula_host(*args) == E.ERR_INVALID_ARGUMENT, (at, value)
    # the device entry points: refused before the engine is asked for anything (no device here)
    h = (C.c_int64 * 4)()
    assert lib.fmhip_function_apply(0, pk, 1, h) in (E.ERR_INVALID_ARGUMENT, E.ERR_NOT_INITIALIZED)
    assert lib.fmhip_option_formula(0, 0, 100.0, 0, 0.2, 0, 1.0, 1.0, 100.0, 1, h) in (E.ERR_INVALID_ARGUMENT, E.ERR_NOT_INITIALIZED)
    assert list(h) == [0, 0, 0, 0]


# ---------------------------------------------------------------- the Python mirrors
def test_the_named_functions_at_a_double(fm):
    assert fm.NORMAL_CDF.derivative() is fm.NORMAL_DENSITY and fm.NORMAL_DENSITY.derivative() is None and fm.NORMAL_QUANTILE.derivative() is None
    x = np.array([-5.0, -1.0, 0.0, 0.3, 2.5], dtype=np.float32)
    cdf, den = fm.function_apply_host(x, [fm.NORMAL_CDF, fm.NORMAL_DENSITY])
    assert np.allclose([fm.NORMAL_CDF(v) for v in x], cdf, rtol=2e-7, atol=0) and np.allclose([fm.NORMAL_DENSITY(v) for v in x], den, rtol=2e-7, atol=0)
    u = np.array([1e-30, 0.01, 0.5, 0.975], dtype=np.float32)
    assert np.allclose([fm.NORMAL_QUANTILE(v) for v in u], fm.function_apply_host(u, fm.NORMAL_QUANTILE)[0], rtol=2e-7, atol=0)
    assert fm.NORMAL_QUANTILE(0.0) == -math.inf and fm.NORMAL_QUANTILE(1.0) == math.inf and math.isnan(fm.NORMAL_QUANTILE(-0.1)) and math.isnan(fm.NORMAL_QUANTILE(float("nan")))
    assert fm.NORMAL_CDF(-math.inf) == 0.0 and fm.NORMAL_CDF(math.inf) == 1.0 and fm.NORMAL_DENSITY(math.inf) == 0.0 and math.isnan(fm.NORMAL_CDF(float("nan")))
    with pytest.raises(ValueError): fm.function_apply_host(x, [fm.NORMAL_CDF] * 5)
    with pytest.raises(ValueError): fm.function_apply_host(x, [])
    with pytest.raises(TypeError): fm.function_apply_host(x, [abs])
    c = fm.RandomVariableHip(2.5, 0.3).apply(fm.NORMAL_CDF)                  # a constant: in double, the time kept, no device
    assert c.isDeterministic() and c.getFiltrationTime() == 2.5 and c.value == fm.NORMAL_CDF(0.3)


def test_deterministic_operands_give_a_deterministic_value_in_double(fm):
    value, delta, vega = fm.option_formula("black_scholes", fm.RandomVariableHip(1.0, 100.0), 0.2, 1.0, 100.0, fm.RandomVariableHip(2.0, 0.9), ("value", "delta", "vega"))
    assert value.isDeterministic() and value.getFiltrationTime() == 2.0
    want = fm.option_formula_double("black_scholes", 100.0, 0.2, 1.0, 100.0, 0.9)
    assert (value.value, delta.value, vega.value) == (want["value"], want["delta"], want["vega"])
    assert abs(want["value"] - 0.9 * 7.965567455405804) < 1e-13 and abs(want["delta"] - 0.9 * 0.539827837277029) < 1e-14
    assert fm.bachelier_option_value(100.0, 20.0, 1.0, 100.0).value == pytest.approx(20.0 / math.sqrt(2 * math.pi), rel=1e-15)
    host = fm.option_formula_host("black_scholes", np.array([100.0], dtype=np.float32), 0.2, 1.0, 100.0, 0.9, ("vega", "value"))
    assert host[0][0] == np.float32(want["vega"]) and host[1][0] == np.float32(want["value"])       # in the order asked
    assert fm.option_formula_double("black_scholes", 120.0, 0.0, 1.0, 100.0, 2.0) == {"value": 40.0, "delta": 2.0, "vega": 0.0}
    with pytest.raises(ValueError): fm.option_formula("heston", 1.0, 1.0, 1.0, 1.0)
    with pytest.raises(ValueError): fm.option_formula("bachelier", 1.0, 1.0, -1.0, 1.0)
    with pytest.raises(ValueError): fm.option_formula("bachelier", 1.0, 1.0, 1.0, 1.0, outputs=("gamma",))
    with pytest.raises(ValueError): fm.option_formula("bachelier", 1.0, 1.0, 1.0, 1.0, outputs=())


def test_aad_through_the_named_functions_on_the_oracle_backed_factory(fm, oracle):
    """d E[f(x)]/dx per path against the named derivative, and the chain rule against central differences of the host definition."""
    factory = fm.RandomVariableDifferentiableAADFactory(oracle.RandomVariableFloatFactory())
    xs = np.random.default_rng(3).normal(size=2001).astype(np.float32)
    X = factory.createRandomVariable(0.0, xs)
    cdf, den = fm.function_apply_host(xs, [fm.NORMAL_CDF, fm.NORMAL_DENSITY])
    Y = X.apply(fm.NORMAL_CDF)
    assert (bits(Y.getRealizations()) == bits(cdf)).all()
    g = Y.average().getGradient()[X.getID()]
    assert (bits(np.broadcast_to(g.getRealizations(), xs.shape)) == bits(den)).all()                 # Φ' = φ, from the same call
    g = X.apply(fm.NORMAL_DENSITY).average().getGradient()[X.getID()].getRealizations()
    assert np.allclose(g, -xs.astype(np.float64) * den, rtol=1e-6, atol=1e-9)                        # φ' = −x·φ
    us = np.random.default_rng(4).uniform(0.01, 0.99, 2001).astype(np.float32)
    U = factory.createRandomVariable(0.0, us)
    Q = U.apply(fm.NORMAL_QUANTILE)
    q = fm.function_apply_host(us, [fm.NORMAL_QUANTILE])[0]
    assert (bits(Q.getRealizations()) == bits(q)).all()
    g = Q.average().getGradient()[U.getID()].getRealizations()
    h = 1e-3
    up, down = (fm.function_apply_host((us + np.float32(s)).astype(np.float32), [fm.NORMAL_QUANTILE])[0].astype(np.float64) for s in (h, -h))
    step = (us + np.float32(h)).astype(np.float64) - (us - np.float32(h)).astype(np.float64)
    assert np.allclose(g, (up - down) / step, rtol=2e-2, atol=0) and np.allclose(g, 1.0 / fm.function_apply_host(q, [fm.NORMAL_DENSITY])[0], rtol=1e-6)
    with pytest.raises(NotImplementedError): X.apply(abs)


@pytest.mark.parametrize("model", ["black_scholes", "bachelier"])
def test_aad_through_the_option_formula_on_the_oracle_backed_factory(fm, oracle, shim, model):
    """The gradient of E[N·V(F, σ)] against central differences of the host definition in each operand: ∂/∂F = N·delta, ∂/∂σ = N·vega,
    ∂/∂N = the unit value; and through a chain, F = exp(x)."""
    factory = fm.RandomVariableDifferentiableAADFactory(oracle.RandomVariableFloatFactory())
    rng = np.random.default_rng(8)
    n, T, K = 501, 1.5, 100.0
    scale = 100.0 if model == "bachelier" else 1.0
    F = rng.uniform(70, 140, n).astype(np.float32); sigma = (rng.uniform(0.1, 0.5, n) * scale).astype(np.float32); unit = rng.uniform(0.5, 1.5, n).astype(np.float32)
    f, s, u = (factory.createRandomVariable(0.0, a) for a in (F, sigma, unit))
    value, = fm.option_formula(model, f, s, T, K, u)
    v1, d1, g1 = fm.option_formula_host(model, F, sigma, T, K, 1.0, ("value", "delta", "vega"))
    assert np.allclose(value.getRealizations(), v1 * unit, rtol=2e-7, atol=0)
    gradient = value.average().getGradient()
    assert np.allclose(gradient[f.getID()].getRealizations(), d1 * unit, rtol=3e-7) and np.allclose(gradient[s.getID()].getRealizations(), g1 * unit, rtol=3e-7)
    assert np.allclose(gradient[u.getID()].getRealizations(), v1, rtol=3e-7)
    # against central differences of the definition's fp64 value (steps of 2^-14 relative: truncation and rounding both below 1e-6 of the scale)
    def value_at(Fv, Sv): return shim.formula(MODELS[model], Fv, Sv, 1.0, T, K)[:, 0]
    F64, S64 = F.astype(np.float64), sigma.astype(np.float64)
    hF, hS = F64 * 2.0 ** -14, S64 * 2.0 ** -14
    cdF = (value_at(F64 + hF, S64) - value_at(F64 - hF, S64)) / (2 * hF)
    cdS = (value_at(F64, S64 + hS) - value_at(F64, S64 - hS)) / (2 * hS)
    assert np.allclose(d1, cdF, rtol=1e-6, atol=1e-6) and np.allclose(g1, cdS, rtol=1e-6, atol=1e-4 / scale)
    # a chain: F = exp(x), scalar volatility and unit; delta and vega asked for with AAD operands
    xs = np.log(F).astype(np.float32)
    x = factory.createRandomVariable(0.0, xs)
    value, delta = fm.option_formula(model, x.exp(), 0.3 * scale, T, K, 0.9, ("value", "delta"))
    Fx = np.asarray(x.exp().getRealizations(), dtype=np.float32)            # the inner implementation's exp
    vd = fm.option_formula_host(model, Fx, 0.3 * scale, T, K, 1.0, ("value", "delta"))
    assert np.allclose(value.getRealizations(), vd[0] * np.float32(0.9), rtol=3e-7) and np.allclose(delta.getRealizations(), vd[1] * np.float32(0.9), rtol=3e-7)
    g = value.average().getGradient()[x.getID()].getRealizations()
    assert np.allclose(g, vd[1] * np.float32(0.9) * Fx, rtol=1e-6)


# ---------------------------------------------------------------- the host half under the sanitizers
def test_host_half_under_the_sanitizers(tmp_path):
    """tests/cpp/test_analytic_host.cpp, a stand-alone program: the argument checks and the definitions over the edge list."""
    gxx = shutil.which("g++")
    if not gxx: pytest.skip("needs g++")
    exe = tmp_path / "analytic_host"
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-ffp-contract=off",
                        os.path.join(ROOT, "tests", "cpp", "test_analytic_host.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "analytic host ok" in r.stdout and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stdout[-1500:] + r.stderr[-3000:]


def test_the_kernels_are_in_the_library(fm):
    """A missing kernel is an error, never a fallback: the launchers are weak references, so the library must be shown to hold them."""
    out = subprocess.check_output(["nm", "-D", "--defined-only", fm._native.LIB_PATH], text=True) + subprocess.check_output(["nm", "--defined-only", fm._native.LIB_PATH], text=True, stderr=subprocess.DEVNULL)
    assert "launch_function_apply" in out and "launch_option_formula" in out
    blob = open(fm._native.LIB_PATH, "rb").read()
    assert b"fm_function_apply_kernel" in blob and b"fm_option_formula_kernel" in blob


def test_kernels_compile_for_gfx950_without_scratch():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc): pytest.skip("needs hipcc")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                        "-c", os.path.join(CSRC, "analytic_kernel.hip"), "-o", os.devnull], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    seen = {}
    for blk in re.split(r"remark: Function Name: ", r.stderr)[1:]:
        seen[blk.split()[0]] = tuple(int(re.search(pattern, blk).group(1)) for pattern in (r"ScratchSize \[bytes/lane\]: (\d+)", r"LDS Size \[bytes/block\]: (\d+)", r" VGPRs: (\d+)"))
    kernels = {k: v for k, v in seen.items() if "fm_function_apply_kernel" in k or "fm_option_formula_kernel" in k}
    assert len(kernels) == 6, seen                                           # 1 … 4 functions; two models
    for name, (scratch, lds, vgprs) in sorted(kernels.items()):
        print(f"{name}: {vgprs} VGPRs, {scratch} bytes of scratch, {lds} bytes of LDS")
        assert scratch == 0 and lds == 0 and vgprs <= 256, (name, scratch, lds, vgprs)


# ---------------------------------------------------------------- the engine's side on the null device
@pytest.fixture(scope="module")
def built():
    if not shutil.which("g++") or not os.path.exists("/opt/rocm/include/hip/hip_runtime_api.h"):
        pytest.skip("needs g++ and the HIP headers")
    r = subprocess.run(["make", "-C", NULLDEV, "-f", "analytic.mk", "-j8", "analytic_asan", "analytic_tsan", "analytic_absent_asan"], capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return os.path.join(NULLDEV, "build")


def _env(tmp_path, env):
    return dict(os.environ, FMHIP_JIT_CACHE_DIR=str(tmp_path / "code_objects"), FMHIP_JIT_PACK_DIR="off", FMHIP_RING_BYTES="16384", FMHIP_ARENA_BYTES="4096",
                ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1", TSAN_OPTIONS="halt_on_error=1", **env)


@pytest.mark.parametrize("env", [{}, {"FMNULL_DEVICES": "2"}, {"FMNULL_THREAD_ENGINES": "1"}])
def test_engine_pass_is_clean_under_the_sanitizers(built, tmp_path, env):
    """drive_analytic: fmhip_function_apply and fmhip_option_formula on vectors of real data at n = 1 … 100 003, checked against the host
    entry points; pending operands, a given-up operand, every argument refusal with nothing flushed or allocated — on one engine, behind a
    device list of two (every shard its block), with thread engines (a caller that does not own the vectors)."""
    full = _env(tmp_path, env)
    a = subprocess.run([os.path.join(built, "drive_analytic_asan")], capture_output=True, text=True, timeout=600, env=full)
    assert a.returncode == 0 and "Sanitizer" not in a.stderr and "runtime error" not in a.stderr, a.stdout[-500:] + a.stderr[-6000:]
    assert "analytic done" in a.stdout and a.stderr == ""
    t = subprocess.run([os.path.join(built, "drive_analytic_tsan")], capture_output=True, text=True, timeout=600, env=full)
    assert t.returncode == 0 and "ThreadSanitizer" not in t.stderr, t.stdout[-500:] + t.stderr[-6000:]
    assert "analytic done" in t.stdout and t.stderr == ""


@pytest.mark.parametrize("call", ["function", "formula"])
def test_a_failing_allocation_leaves_nothing_behind(built, tmp_path, call):
    """One fmhip_function_apply of three functions, one fmhip_option_formula of three outputs: THREE buffers from the pool each, the outputs.
    FMHIP_TEST_FAIL_ALLOC_AT is set on each of them (their positions from a counting run), and once where nothing reaches it: the call
    answers FMHIP_OK or FMHIP_ERR_OUT_OF_MEMORY, a failed call writes no handle, live vectors and bytes in use are what they were, the
    same call succeeds afterwards (the driver checks all of it), and the process ends without a leak."""
    exe = os.path.join(built, "drive_analytic_asan")
    counting = subprocess.run([exe, "failure", call], capture_output=True, text=True, timeout=600, env=_env(tmp_path, {}))
    assert counting.returncode == 0 and "Sanitizer" not in counting.stderr, counting.stdout[-500:] + counting.stderr[-6000:]
    before, inside, status = map(int, re.search(r"failure: (\d+) allocations before the call, (\d+) in it, status (-?\d+)", counting.stdout).groups())
    assert inside == 3 and status == 0
    for at in list(range(before + 1, before + inside + 1)) + [10**9]:
        r = subprocess.run([exe, "failure", call], capture_output=True, text=True, timeout=600, env=_env(tmp_path, {"FMHIP_TEST_FAIL_ALLOC_AT": str(at)}))
        assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr and r.stderr == "", (at, r.stdout[-500:] + r.stderr[-6000:])
        assert "failure done" in r.stdout
        failed = int(re.search(r"status (-?\d+)", r.stdout).group(1)) != 0
        assert failed == (at <= before + inside), (at, r.stdout)


@pytest.mark.parametrize("env", [{}, {"FMNULL_DEVICES": "2"}, {"FMNULL_THREAD_ENGINES": "1"}])
def test_a_build_without_the_kernels_answers_unsupported(built, tmp_path, env):
    a = subprocess.run([os.path.join(built, "drive_analytic_absent_asan")], capture_output=True, text=True, timeout=600, env=_env(tmp_path, env))
    assert a.returncode == 0 and "Sanitizer" not in a.stderr and "runtime error" not in a.stderr, a.stdout[-500:] + a.stderr[-6000:]
    assert "analytic absent done" in a.stdout
