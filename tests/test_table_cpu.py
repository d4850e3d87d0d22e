"""Tabulated functions without a GPU (include/fmhip.h: fmhip_table_build, fmhip_table_apply_host; host/tabulated_function.hpp):
the DEFINITION against a numpy fp64 restatement written here (searchsorted + Horner with separate operations) for EQUALITY of the output
bits; fmhip_table_build against its own contract, against scipy's CubicSpline / PchipInterpolator and against a second numpy restatement;
the coarse index, the kernel's loop and the tail in a stand-alone program under AddressSanitizer / UBSan (tests/cpp/test_table_host.cpp);
the engine's side of fmhip_table_apply (csrc/table_engine.hpp, the fronts of csrc/sharded.cpp and csrc/abi.cpp) on the test-only null
device under AddressSanitizer + UBSan and ThreadSanitizer (tests/nulldev/table.mk: drive_table.cpp with the stand-in launcher of
null_table.cpp, drive_table_absent.cpp without it); the Python mirror; AAD through apply on the oracle-backed factory.  Stand-alone
programs only: nothing sanitized is loaded into this process."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NULLDEV = os.path.join(ROOT, "tests", "nulldev")
PD = C.POINTER(C.c_double)
KNOT_COUNTS = [1, 2, 3, 4, 5, 64, 65, 1023, 1024]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_f32(a, b):
    """Bit for bit; of a NaN only that it is one."""
    with np.errstate(over="ignore"):                                   # a double beyond fp32 narrows to inf, as the definition's does
        a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    return a.shape == b.shape and bool(((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))).all())


def knots_of(m, kind):
    """uniform on fp32 numbers (multiples of 1/8), uniform on numbers that are no fp32 numbers (0.1·i), geometric over twelve decades, two clusters."""
    i = np.arange(m, dtype=np.float64)
    if kind == "dyadic": return -3.0 + 0.125 * i
    if kind == "tenths": return 0.1 * i - 1.7
    if kind == "geometric": return 1e-6 * 1e12 ** (i / max(m - 1, 1))
    if kind == "clusters": return np.where(i < m // 2, -100.0 + 1e-3 * i, 100.0 + 1e-3 * i)
    raise ValueError(kind)


def edge_inputs(K):
    """Every knot narrowed to fp32 and its fp32 neighbours on both sides, below the first knot and above the last, ±0, ±inf, NaN, denormals,
    the largest fp32 numbers."""
    k32 = K.astype(np.float32)
    tiny = np.float32(1e-45)
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, tiny, -tiny, np.float32(1.1754942e-38), -np.float32(1.1754942e-38), np.finfo(np.float32).max, -np.finfo(np.float32).max], dtype=np.float32)
    span = max(float(K[-1] - K[0]), 1.0)
    outside = np.array([K[0] - 1e-3 * span, K[0] - span, K[0] - 1e6 * span, K[-1] + 1e-3 * span, K[-1] + span, K[-1] + 1e6 * span]).astype(np.float32)
    mid = ((K[:-1] + K[1:]) / 2).astype(np.float32)
    return np.concatenate([k32, np.nextafter(k32, np.float32(np.inf)), np.nextafter(k32, np.float32(-np.inf)), special, outside, mid])


def build(fm, K, V, interpolation, extrapolation=0, derivative=0):
    K, V = np.ascontiguousarray(K, dtype=np.float64), np.ascontiguousarray(V, dtype=np.float64)
    out = np.full((K.size + 1, 4), np.nan)
    st = fm.lib().fmhip_table_build(K.ctypes.data_as(PD), V.ctypes.data_as(PD), K.size, interpolation, extrapolation, derivative, out.ctypes.data_as(PD))
    assert st == 0, fm.lib().fmhip_last_error()
    return out


def apply_host(fm, x, K, coefs):
    """fmhip_table_apply_host: coefs (T, m + 1, 4) -> (T, n) float32."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    K = np.ascontiguousarray(K, dtype=np.float64)
    coefs = np.ascontiguousarray(coefs, dtype=np.float64).reshape(-1, K.size + 1, 4)
    out = np.full((coefs.shape[0], x.size), -7.0, dtype=np.float32)
    cols = (C.c_void_p * coefs.shape[0])(*[out[f].ctypes.data for f in range(coefs.shape[0])])
    st = fm.lib().fmhip_table_apply_host(x.ctypes.data_as(C.c_void_p), x.size, K.ctypes.data_as(PD), K.size, coefs.ctypes.data_as(PD), coefs.shape[0], cols)
    assert st == 0, fm.lib().fmhip_last_error()
    return out


def restatement(x, K, coef):
    """The definition in numpy: s = searchsorted(K, X, "right"), t = X − K[max(s − 1, 0)], Horner with every operation on its own in fp64, one
    narrowing; a segment with C1 = C2 = C3 = 0 is (float)C0."""
    X = np.asarray(x, dtype=np.float32).astype(np.float64)
    s = np.searchsorted(K, X, side="right")
    s[np.isnan(X)] = 0
    c = coef[s]
    with np.errstate(invalid="ignore", over="ignore"):
        t = X - K[np.maximum(s - 1, 0)]
        r = c[:, 3] * t
        r = r + c[:, 2]
        r = r * t
        r = r + c[:, 1]
        r = r * t
        r = r + c[:, 0]
        flat = (c[:, 1] == 0) & (c[:, 2] == 0) & (c[:, 3] == 0)
        out = np.where(flat, c[:, 0], r).astype(np.float32)
    out[np.isnan(X)] = np.nan
    return out


def values_of(K, seed):
    rng = np.random.default_rng(seed)
    return np.sin(0.37 * np.arange(K.size) + seed) + 0.2 * rng.standard_normal(K.size)


# ---------------------------------------------------------------- the definition
@pytest.mark.parametrize("kind", ["dyadic", "tenths", "geometric", "clusters"])
@pytest.mark.parametrize("m", KNOT_COUNTS)
def test_the_definition_equals_the_numpy_restatement(fm, m, kind):
    K = knots_of(m, kind)
    x = np.concatenate([edge_inputs(K), np.random.default_rng(m).uniform(K[0] - 1.0, K[-1] + 1.0, 2000).astype(np.float32)])
    rng = np.random.default_rng(1000 + m)
    for interpolation in range(4):
        for extrapolation in range(2):
            for derivative in range(2):
                coef = build(fm, K, values_of(K, interpolation), interpolation, extrapolation, derivative)
                got = apply_host(fm, x, K, coef)[0]
                assert same_f32(got, restatement(x, K, coef)), (m, kind, interpolation, extrapolation, derivative)
                assert (bits(got[np.isnan(x)]) == 0x7fc00000).all()
    coef = rng.standard_normal((m + 1, 4)) * 10.0 ** rng.integers(-3, 4, (m + 1, 4))      # arbitrary coefficients, not a built table
    coef[rng.random(m + 1) < 0.2, 1:] = 0.0
    assert same_f32(apply_host(fm, x, K, coef)[0], restatement(x, K, coef))


def test_several_tables_in_one_call_are_the_tables_one_by_one(fm):
    K = knots_of(256, "tenths")
    x = edge_inputs(K)
    coefs = np.stack([build(fm, K, values_of(K, f), f, f % 2, f // 3) for f in range(4)])
    together = apply_host(fm, x, K, coefs)
    for f in range(4):
        assert (bits(together[f]) == bits(apply_host(fm, x, K, coefs[f])[0])).all()


def test_a_flat_segment_survives_infinite_arguments(fm):
    """No 0·∞: constant extrapolation (and a piecewise-constant segment) yields (float)C0 at ±inf and at the largest fp32 numbers."""
    K = knots_of(5, "tenths")
    V = values_of(K, 3)
    x = np.array([-np.inf, np.inf, -np.finfo(np.float32).max, np.finfo(np.float32).max], dtype=np.float32)
    for interpolation in range(4):
        got = apply_host(fm, x, K, build(fm, K, V, interpolation, 0))[0]
        assert (bits(got) == bits(np.array([V[0], V[-1], V[0], V[-1]], dtype=np.float32))).all(), interpolation
        slope = apply_host(fm, x, K, build(fm, K, V, interpolation, 0, 1))[0]
        assert (bits(slope) == 0).all(), interpolation


# ---------------------------------------------------------------- table_build
@pytest.mark.parametrize("m", KNOT_COUNTS)
def test_at_a_knot_that_is_an_fp32_number_the_result_is_its_value(fm, m):
    K = knots_of(m, "dyadic")
    V = values_of(K, 5)
    for interpolation in range(4):
        for extrapolation in range(2):
            got = apply_host(fm, K.astype(np.float32), K, build(fm, K, V, interpolation, extrapolation))[0]
            assert (bits(got) == bits(V.astype(np.float32))).all(), (m, interpolation, extrapolation)


@pytest.mark.parametrize("m", [2, 3, 4, 5, 64, 65, 1024])
def test_a_straight_line_is_reproduced_exactly(fm, m):
    """Dyadic knots and values on a line: every mode but piecewise-constant has the segments (V[i], slope, 0, 0) exactly, and with linear
    extrapolation the end segments as well; derivative=1 of the linear mode is the slopes."""
    K = np.cumsum(np.concatenate([[-3.0], np.where(np.arange(m - 1) % 3 == 0, 0.25, 0.125)]))
    slope = 0.75
    V = 2.0 + slope * (K - K[0])
    want = np.zeros((m + 1, 4)); want[1:, 0] = V; want[0, 0] = V[0]; want[:, 1] = slope
    for interpolation in (1, 2, 3):
        assert (build(fm, K, V, interpolation, 1) == want).all(), interpolation
        ends_flat = want.copy(); ends_flat[0, 1] = ends_flat[m, 1] = 0.0
        assert (build(fm, K, V, interpolation, 0) == ends_flat).all(), interpolation
    d = build(fm, K, V, 1, 1, 1)
    assert (d[:, 0] == slope).all() and (d[:, 1:] == 0).all()
    rng = np.random.default_rng(m)
    V = rng.integers(-8, 9, m).astype(np.float64)
    lin, dlin = build(fm, K, V, 1, 0), build(fm, K, V, 1, 0, 1)
    assert (dlin[1:m, 0] == np.diff(V) / np.diff(K)).all() and (dlin[[0, m], 0] == 0).all() and (dlin[:, 1:] == 0).all()
    assert (lin[1:m, 1] == np.diff(V) / np.diff(K)).all()
    pc = build(fm, K, V, 0, 1)
    assert (pc[1:, 0] == V).all() and pc[0, 0] == V[0] and (pc[:, 1:] == 0).all()


def test_one_knot_is_the_constant_and_two_knots_are_linear(fm):
    one = np.array([[2.5, 0, 0, 0], [2.5, 0, 0, 0]])
    for interpolation in range(4):
        for extrapolation in range(2):
            assert (build(fm, [1.0], [2.5], interpolation, extrapolation) == one).all()
            assert (build(fm, [1.0], [2.5], interpolation, extrapolation, 1) == 0).all()
    for interpolation in (2, 3):
        for extrapolation in range(2):
            assert (build(fm, [1.0, 3.0], [2.0, 5.0], interpolation, extrapolation) == build(fm, [1.0, 3.0], [2.0, 5.0], 1, extrapolation)).all()


def test_the_derivative_is_the_derivative_of_the_segments(fm):
    K = knots_of(65, "tenths"); V = values_of(K, 2)
    for interpolation in range(4):
        for extrapolation in range(2):
            c, d = build(fm, K, V, interpolation, extrapolation), build(fm, K, V, interpolation, extrapolation, 1)
            assert (d[:, 0] == c[:, 1]).all() and (d[:, 1] == 2.0 * c[:, 2]).all() and (d[:, 2] == 3.0 * c[:, 3]).all() and (d[:, 3] == 0).all()


def natural_spline_numpy(K, V):
    """Second restatement: the natural cubic spline by a dense solve for the second derivatives; coefficients per interval."""
    m = K.size
    h, delta = np.diff(K), np.diff(V) / np.diff(K)
    A = np.zeros((m, m)); b = np.zeros(m)
    A[0, 0] = A[-1, -1] = 1.0
    for i in range(1, m - 1):
        A[i, i - 1], A[i, i], A[i, i + 1] = h[i - 1], 2.0 * (h[i - 1] + h[i]), h[i]
        b[i] = 6.0 * (delta[i] - delta[i - 1])
    M = np.linalg.solve(A, b)
    return np.stack([V[:-1], delta - h * (2.0 * M[:-1] + M[1:]) / 6.0, M[:-1] / 2.0, (M[1:] - M[:-1]) / (6.0 * h)], axis=1)


def pchip_numpy(K, V):
    """Second restatement: Fritsch–Carlson slopes (weighted harmonic mean, three-point ends with the shape-preserving limits)."""
    h, delta = np.diff(K), np.diff(V) / np.diff(K)
    m = K.size
    d = np.zeros(m)
    for i in range(1, m - 1):
        if delta[i - 1] * delta[i] > 0:
            w1, w2 = 2.0 * h[i] + h[i - 1], h[i] + 2.0 * h[i - 1]
            d[i] = (w1 + w2) / (w1 / delta[i - 1] + w2 / delta[i])
    def end(h0, h1, d0, d1):
        e = ((2.0 * h0 + h1) * d0 - h0 * d1) / (h0 + h1)
        if np.sign(e) != np.sign(d0): return 0.0
        if np.sign(d0) != np.sign(d1) and abs(e) > 3.0 * abs(d0): return 3.0 * d0
        return e
    d[0], d[-1] = end(h[0], h[1], delta[0], delta[1]), end(h[-1], h[-2], delta[-1], delta[-2])
    return np.stack([V[:-1], d[:-1], (3.0 * delta - 2.0 * d[:-1] - d[1:]) / h, (d[:-1] + d[1:] - 2.0 * delta) / (h * h)], axis=1)


def interval_values(K, coef, per=7):
    """The interior segments' polynomials on a grid inside every interval, in plain fp64."""
    t = np.linspace(0.0, 1.0, per)[None, :] * np.diff(K)[:, None]
    return ((coef[:, 3:4] * t + coef[:, 2:3]) * t + coef[:, 1:2]) * t + coef[:, 0:1]


CUBIC_CASES = [(m, kind) for m in (3, 4, 5, 64, 65, 1024) for kind in ("tenths", "geometric", "clusters")]


def cubic_differences(fm, with_scipy):
    """(largest relative difference between scipy and the numpy restatements, the same for the code under test against scipy — or against
    the restatements where scipy is absent) over CUBIC_CASES, relative to the largest |value| of the case."""
    if with_scipy:
        from scipy.interpolate import CubicSpline, PchipInterpolator
    reference, under_test = 0.0, 0.0
    for m, kind in CUBIC_CASES:
        K = knots_of(m, kind); V = values_of(K, m)
        scale = np.abs(V).max()
        grid = K[:-1, None] + np.linspace(0.0, 1.0, 7)[None, :] * np.diff(K)[:, None]
        for interpolation, numpy_version in ((2, natural_spline_numpy), (3, pchip_numpy)):
            mine = interval_values(K, numpy_version(K, V))
            got = interval_values(K, build(fm, K, V, interpolation, 0)[1:m])
            if with_scipy:
                want = (CubicSpline(K, V, bc_type="natural") if interpolation == 2 else PchipInterpolator(K, V))(grid)
                reference = max(reference, np.abs(want - mine).max() / scale)
            else:
                want = mine
            under_test = max(under_test, np.abs(want - got).max() / scale)
    return reference, under_test


def test_the_cubic_modes_agree_with_scipy(fm):
    """Natural cubic spline against scipy.interpolate.CubicSpline(bc_type="natural"), monotone cubic against PchipInterpolator, on a grid of
    seven points inside every interval of CUBIC_CASES (3 … 1024 knots; uniform, geometric over twelve decades, two clusters).  Tolerance: 16
    times the largest relative difference between scipy and this file's own numpy restatements over the same inputs, which measures
    2.5e-9 here (the two-cluster knots: intervals of 1e-3 beside one of 200 make the tridiagonal system ill-conditioned, and the dense solve
    and scipy's banded one part ways there); the code under test measures 4.0e-9 against scipy."""
    pytest.importorskip("scipy")
    reference, under_test = cubic_differences(fm, True)
    print(f"scipy vs numpy restatement: {reference:.3e}; code under test vs scipy: {under_test:.3e}")
    assert reference > 0.0
    assert under_test <= 16.0 * reference


def test_the_cubic_modes_agree_with_the_numpy_restatement(fm):
    """The same where scipy is absent (and where it is not): against the second numpy restatement, within the 16-fold of the figure that
    test_the_cubic_modes_agree_with_scipy's docstring records."""
    _, under_test = cubic_differences(fm, False)
    print(f"code under test vs numpy restatement: {under_test:.3e}")
    assert under_test <= 16.0 * 2.5e-9


def test_monotone_data_gives_a_monotone_result(fm):
    rng = np.random.default_rng(11)
    for m in (3, 5, 64, 257):
        for kind in ("tenths", "geometric"):
            K = knots_of(m, kind)
            V = np.cumsum(rng.random(m) ** 4 * (rng.random(m) < 0.7))                # non-decreasing with flat stretches and jumps
            coef = build(fm, K, V, 3, 0)
            x = np.sort(np.concatenate([rng.uniform(K[0], K[-1], 20000), K])).astype(np.float32)
            y = apply_host(fm, x, K, coef)[0]
            assert (np.diff(y.astype(np.float64)) >= 0).all(), (m, kind)
            assert (apply_host(fm, x, K, build(fm, K, V, 3, 0, 1))[0] >= 0).all(), (m, kind)


def test_refusals(fm):
    lib = fm.lib()
    bad = fm._native.ERR_INVALID_ARGUMENT
    K = np.array([0.0, 1.0, 2.0]); V = np.array([1.0, 2.0, 0.5]); out = np.zeros(16)
    def b(k, v, m, i=1, e=0, d=0, o=out):
        k = None if k is None else np.ascontiguousarray(k, dtype=np.float64); v = None if v is None else np.ascontiguousarray(v, dtype=np.float64)
        return lib.fmhip_table_build(None if k is None else k.ctypes.data_as(PD), None if v is None else v.ctypes.data_as(PD), m, i, e, d, None if o is None else o.ctypes.data_as(PD))
    assert b(K, V, 3) == 0
    for args in ((None, V, 3), (K, None, 3), (K, V, 0), (K, V, -1), (K, V, 3, 4), (K, V, 3, -1), (K, V, 3, 1, 2), (K, V, 3, 1, -1), (K, V, 3, 1, 0, 2), (K, V, 3, 1, 0, -1), (K, V, 3, 1, 0, 0, None),
                 ([0.0, 0.0, 1.0], V, 3), ([0.0, 2.0, 1.0], V, 3), ([0.0, np.nan, 1.0], V, 3), ([0.0, 1.0, np.inf], V, 3), (K, [1.0, np.nan, 1.0], 3), (K, [1.0, np.inf, 1.0], 3)):
        assert b(*args) == bad, args
    big = np.arange(1025, dtype=np.float64); obig = np.zeros(1026 * 4)
    assert b(big, big, 1025, o=obig) == bad and b(big, big, 1024, o=obig) == 0
    x = np.zeros(4, dtype=np.float32); o = np.zeros(4, dtype=np.float32); coef = np.zeros(4 * 4 * 4)
    def a(xp, n, k, m, T, cols):
        k = np.ascontiguousarray(k, dtype=np.float64)
        return lib.fmhip_table_apply_host(xp, n, k.ctypes.data_as(PD), m, coef.ctypes.data_as(PD), T, cols)
    cols = (C.c_void_p * 4)(*[o.ctypes.data] * 4); holes = (C.c_void_p * 4)(o.ctypes.data, None, None, None)
    xp = x.ctypes.data_as(C.c_void_p)
    assert a(xp, 4, K, 3, 1, cols) == 0 and a(xp, 4, K, 3, 4, cols) == 0
    for args in ((None, 4, K, 3, 1, cols), (xp, 0, K, 3, 1, cols), (xp, -1, K, 3, 1, cols), (xp, 4, K, 0, 1, cols), (xp, 4, K, 3, 0, cols), (xp, 4, K, 3, 5, cols), (xp, 4, K, 3, 1, None),
                 (xp, 4, K, 3, 2, holes), (xp, 4, [0.0, 0.0, 1.0], 3, 1, cols), (xp, 4, [0.0, np.nan, 1.0], 3, 1, cols)):
        assert a(*args) == bad, args
    k513 = np.arange(513, dtype=np.float64); coef = np.zeros(2 * 514 * 4)
    assert a(xp, 4, k513, 513, 2, cols) == bad and a(xp, 4, k513[:512], 512, 2, cols) == 0
    # the device call needs an engine: without one it says so, it does not evaluate on the host
    if not lib.fmhip_is_initialized():
        h = (C.c_int64 * 4)()
        assert lib.fmhip_table_apply(1, K.ctypes.data_as(PD), 3, coef.ctypes.data_as(PD), 1, h) == fm._native.ERR_NOT_INITIALIZED


# ---------------------------------------------------------------- the Python mirror
def test_the_python_mirror(fm):
    K = knots_of(9, "tenths"); V = values_of(K, 1)
    f = fm.TabulatedFunction(K, V, "monotone_cubic", "linear")
    assert f.coefficients.shape == (10, 4) and (f.coefficients == build(fm, K, V, 3, 1)).all()
    df = f.derivative()
    assert (df.coefficients == build(fm, K, V, 3, 1, 1)).all() and (df.knots == f.knots).all()
    with pytest.raises(ValueError): df.derivative()
    x = edge_inputs(K); x = x[np.isfinite(x)]
    got = fm.table_apply_host(x, [f, df])
    assert same_f32(got[0], [f(v) for v in x]) and same_f32(got[1], [df(v) for v in x])          # __call__: the polynomial at the double
    assert np.isnan(f(float("nan")))
    with pytest.raises(ValueError): fm.TabulatedFunction(K, V, "quadratic")
    with pytest.raises(ValueError): fm.TabulatedFunction(K, V, "linear", "periodic")
    with pytest.raises(ValueError): fm.TabulatedFunction(K, V[:-1])
    with pytest.raises(fm.FmhipError): fm.TabulatedFunction(K[::-1], V)
    with pytest.raises(ValueError): fm.table_apply_host(x, [f, fm.TabulatedFunction(K + 1.0, V)])     # other knots
    with pytest.raises(ValueError): fm.table_apply_host(x, [f] * 5)
    with pytest.raises(ValueError): fm.table_apply_host(x, [])


def test_apply_of_anything_else_still_raises(fm, oracle):
    factory = fm.RandomVariableDifferentiableAADFactory(oracle.RandomVariableFloatFactory())
    x = factory.createRandomVariable(0.0, np.linspace(-1, 1, 16).astype(np.float32))
    with pytest.raises(NotImplementedError): x.apply(abs)
    with pytest.raises(NotImplementedError): x.apply(lambda v: v)
    with pytest.raises(NotImplementedError): fm.RandomVariableHip(0.0, 1.5).apply(abs)
    f = fm.TabulatedFunction([0.0, 1.0, 3.0], [1.0, 3.0, 2.0])
    c = fm.RandomVariableHip(2.5, 2.0).apply(f)                                      # a constant: f(value) in double, the time kept, no device
    assert c.isDeterministic() and c.getFiltrationTime() == 2.5 and c.value == f(2.0) == 2.5


@pytest.mark.parametrize("mode", ["linear", "cubic_spline", "monotone_cubic"])
def test_aad_through_apply_on_the_oracle_backed_factory(fm, oracle, mode):
    """d E[f(x)] / dx = f'(x) · 1: the gradient of x.apply(f).average() is x.apply(f.derivative()) bit for bit (the adjoint 1 times the slope)."""
    K = knots_of(17, "tenths"); V = values_of(K, 4)
    f = fm.TabulatedFunction(K, V, mode, "linear")
    xs = np.random.default_rng(3).uniform(K[0] - 0.3, K[-1] + 0.3, 4001).astype(np.float32)
    factory = fm.RandomVariableDifferentiableAADFactory(oracle.RandomVariableFloatFactory())
    X = factory.createRandomVariable(0.0, xs)
    Y = X.apply(f)
    value, slope = fm.table_apply_host(xs, [f, f.derivative()])
    assert (bits(Y.getRealizations()) == bits(value)).all()
    g = Y.average().getGradient()[X.getID()]
    assert (bits(np.broadcast_to(g.getRealizations(), xs.shape)) == bits(slope)).all()
    # the chain rule around it: d E[f(2x)²] / dx = 2 f(2x) f'(2x) · 2, in the inner implementation's fp32 arithmetic
    Z = X.mult(2.0).apply(f).squared()
    g = Z.average().getGradient()[X.getID()].getRealizations()
    v2, s2 = fm.table_apply_host((xs * np.float32(2.0)).astype(np.float32), [f, f.derivative()])
    want = (v2 * np.float32(2.0)) * s2 * np.float32(2.0)
    assert np.allclose(g, want, rtol=1e-6, atol=0)


# ---------------------------------------------------------------- the host half of the kernel under the sanitizers
def test_host_half_under_the_sanitizers(tmp_path):
    """tests/cpp/test_table_host.cpp: the coarse index against the plain search with X on and one ulp beside every cell boundary and every
    knot (uniform, geometric 1e-6 … 1e6, two clusters; 1 … 1024 knots), an index that is wrong on purpose (the correction still finds the
    definition's s), and a model of the kernel's loop — 16-byte groups, the grid-stride wrap, the tail into the padding — against the
    definition."""
    gxx = shutil.which("g++")
    if not gxx or not os.path.exists("/opt/rocm/include/hip/hip_runtime_api.h"):
        pytest.skip("needs g++ and the HIP headers (csrc/table_kernel.h declares the launcher)")
    exe = tmp_path / "table_host"
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-ffp-contract=off",
                        "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-Wno-deprecated-declarations",
                        os.path.join(ROOT, "tests", "cpp", "test_table_host.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "table host ok" in r.stdout and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stdout[-1500:] + r.stderr[-3000:]


def test_the_kernel_is_in_the_library(fm):
    """A missing kernel is an error, never a fallback: the launcher is a weak reference, so the library must be shown to hold it."""
    out = subprocess.check_output(["nm", "-D", "--defined-only", fm._native.LIB_PATH], text=True) + subprocess.check_output(["nm", "--defined-only", fm._native.LIB_PATH], text=True, stderr=subprocess.DEVNULL)
    assert "launch_table_apply" in out
    assert b"fm_table_apply_kernel" in open(fm._native.LIB_PATH, "rb").read()


# ---------------------------------------------------------------- the engine's side on the null device
@pytest.fixture(scope="module")
def built():
    if not shutil.which("g++") or not os.path.exists("/opt/rocm/include/hip/hip_runtime_api.h"):
        pytest.skip("needs g++ and the HIP headers")
    r = subprocess.run(["make", "-C", NULLDEV, "-f", "table.mk", "-j8", "table_asan", "table_tsan", "table_absent_asan"], capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return os.path.join(NULLDEV, "build")


def _env(tmp_path, env):
    return dict(os.environ, FMHIP_JIT_CACHE_DIR=str(tmp_path / "code_objects"), FMHIP_JIT_PACK_DIR="off", FMHIP_RING_BYTES="16384", FMHIP_ARENA_BYTES="4096",
                ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1", TSAN_OPTIONS="halt_on_error=1", **env)


@pytest.mark.parametrize("env", [{}, {"FMNULL_DEVICES": "2"}, {"FMNULL_DEVICES": "3"}, {"FMNULL_THREAD_ENGINES": "1"}])
def test_engine_pass_is_clean_under_the_sanitizers(built, tmp_path, env):
    """drive_table: fmhip_table_apply on vectors of real data at n = 1 … 100 003, three families of knots with 1 … 1024 of them, 1 … 4 tables
    per call, checked against fmhip_table_apply_host; a pending x, a given-up x, a second thread releasing the inputs of pending operands
    during the call, every argument refusal with nothing allocated — on one engine and behind a device list of one shard, behind 2 and 3
    shards (every shard its block), with thread engines (a caller that does not own the vector)."""
    full = _env(tmp_path, env)
    a = subprocess.run([os.path.join(built, "drive_table_asan")], capture_output=True, text=True, timeout=600, env=full)
    assert a.returncode == 0 and "Sanitizer" not in a.stderr and "runtime error" not in a.stderr, a.stdout[-500:] + a.stderr[-6000:]
    assert a.stdout.count("table done") == 2 and a.stderr == ""
    assert ("a device list of one shard: checked" in a.stdout) == (not env)
    t = subprocess.run([os.path.join(built, "drive_table_tsan")], capture_output=True, text=True, timeout=600, env=full)
    assert t.returncode == 0 and "ThreadSanitizer" not in t.stderr, t.stdout[-500:] + t.stderr[-6000:]
    assert t.stdout.count("table done") == 2 and t.stderr == ""


def test_a_failing_allocation_inside_table_apply_leaves_nothing_behind(built, tmp_path):
    """One fmhip_table_apply of three tables takes THREE buffers from the pool, its outputs.  The hook FMHIP_TEST_FAIL_ALLOC_AT is set on each
    of them (their positions from a counting run), and once where nothing reaches it: the call answers FMHIP_OK or FMHIP_ERR_OUT_OF_MEMORY,
    a result it gives is right, a failed call writes no handle, live vectors and bytes in use are what they were, the same call succeeds
    afterwards (the driver checks all of it), and the process ends without a leak."""
    exe = os.path.join(built, "drive_table_asan")
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
    a = subprocess.run([os.path.join(built, "drive_table_absent_asan")], capture_output=True, text=True, timeout=600, env=_env(tmp_path, env))
    assert a.returncode == 0 and "Sanitizer" not in a.stderr and "runtime error" not in a.stderr, a.stdout[-500:] + a.stderr[-6000:]
    assert a.stdout.count("table absent done") == 2
