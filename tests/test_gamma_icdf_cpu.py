"""CPU-only: the definition of the gamma and the exponential law (host/gamma_icdf.hpp) — fm_exp64 / fm_log64 against
libm, the inverse of the regularised incomplete gamma function against a 60-digit solution computed here with `decimal` (the series for
P, ln Γ by Stirling's series, bisection), identities that need no reference, the host entry point with mixed laws, every new argument
error, the Python mirrors, and the resource figures of the two untouched kernels from a cross-compile.  tests/cpp/test_gamma_icdf.cpp,
which this file builds, is the header compiled as host C++."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess
from decimal import Decimal, getcontext
from fractions import Fraction
from importlib import import_module

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NORMAL, UNIFORM, POISSON, GAMMA, EXPONENTIAL = 0, 1, 2, 4, 5
INVALID = -5
BOUND = 2.0 ** -40                    # relative, wherever the result is a normal fp32 number: 15 bits below fp32's half ulp
FP32_MIN_NORMAL, FP32_DENORMAL_STEP = 2.0 ** -126, 2.0 ** -149
GRID_SHAPES = [0.01, 0.0625, 0.5, 1.0, 2.5, 30.0, 1000.0]
GRID_U = [2.0 ** -53, 1e-12, 1e-6] + [k / 100 for k in range(1, 100)] + [1 - 1e-6, 1 - 2.0 ** -53]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("gamma_icdf") / "test_gamma_icdf")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-o", path, os.path.join(ROOT, "tests", "cpp", "test_gamma_icdf.cpp")])
    return path


def pipe(exe, mode, rows):
    text = "".join(" ".join(float(v).hex() for v in (row if isinstance(row, tuple) else (row,))) + "\n" for row in rows)
    r = subprocess.run([exe, mode], input=text, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return [line.split() for line in r.stdout.splitlines()]


def ulps(got, want):
    """|got − want| in units of want's last place (want: correctly rounded within libm's own half ulp or so)"""
    return np.abs(got - want) / np.spacing(np.abs(want))


def test_exp_and_log_against_libm(exe):
    """3 x 10^5 seeded arguments over what the ICDF feeds them: exp over [−745, 40] (the front factor of P, the guess), log over 1e-320 …
    1e6, log-uniform, and over (0, 1] (log u, log(1 − u)).  The requirement follows from the ICDF's bound, 2^-40 relative: its error is the
    relative error of P over shape (small shapes) and P's is that of exp, whose argument of size up to 7000 (shape 1000) carries a
    rounding of 2^-53 · 7000 = 2^-40.2 whatever exp itself does — so a few ulp in exp and log cost nothing: 4 ulp is asked for, against a
    libm that is itself within an ulp.  Measured here: exp 1.00 ulp, log 1.00 ulp."""
    rng = np.random.default_rng(20261016)
    x = np.concatenate([rng.uniform(-745.0, 40.0, 100_000), rng.uniform(-1.0, 1.0, 50_000), [0.0, -0.0, 709.7, -708.4, -745.1, 1e-300, -1e-300]])
    got = np.array([float.fromhex(r[0]) for r in pipe(exe, "exp", x)])
    want = np.exp(x)
    normal = want >= 2.3e-308
    worst_exp = ulps(got[normal], want[normal]).max()
    assert (np.abs(got[~normal] - want[~normal]) <= 2 * 5e-324).all()
    y = np.concatenate([10.0 ** rng.uniform(-320, 6, 100_000), rng.uniform(0.0, 1.0, 50_000), 1.0 - rng.uniform(0.0, 1.0, 50_000) * 2.0 ** -30,
                        [1.0, 2.0, 0.5, 5e-324, 2.0 ** 0.5, 1.7976931348623157e308]])
    y = y[y > 0]
    got = np.array([float.fromhex(r[0]) for r in pipe(exe, "log", y)])
    want = np.log(y)
    assert got[np.flatnonzero(y == 1.0)[0]] == 0.0
    nonzero = want != 0
    worst_log = ulps(got[nonzero], want[nonzero]).max()
    print(f"fm_exp64: {worst_exp:.2f} ulp, fm_log64: {worst_log:.2f} ulp at most, against libm")
    assert worst_exp <= 4 and worst_log <= 4
    special = [float.fromhex(r[0]) for r in pipe(exe, "exp", [float("inf"), -float("inf"), 800.0, -800.0])]
    assert special == [float("inf"), 0.0, float("inf"), 0.0]
    special = [float.fromhex(r[0]) for r in pipe(exe, "log", [0.0, float("inf")])]
    assert special == [-float("inf"), float("inf")]


# ---- the reference: 60 digits, standard library only

getcontext().prec = 60


def bernoulli(n_max):
    """B_0 … B_n_max as fractions (B_1 = −1/2)"""
    B = [Fraction(0)] * (n_max + 1)
    B[0] = Fraction(1)
    for m in range(1, n_max + 1):
        B[m] = -sum(Fraction(math.comb(m + 1, k)) * B[k] for k in range(m)) / (m + 1)
    return B


_B = bernoulli(40)


def ln_gamma(z):
    """ln Γ(z) for a Decimal z > 0: Γ(z) = Γ(z + 120) / (z (z + 1) … (z + 119)), Stirling's series with 20 Bernoulli terms at z + 120
    (its 20th term is about 1e-68 there, the first neglected one smaller)."""
    shift = Decimal(0)
    for k in range(120):
        shift += (z + k).ln()
    w = z + 120
    s = (w - Decimal("0.5")) * w.ln() - w + (Decimal(2) * Decimal("3.14159265358979323846264338327950288419716939937510582097494459")).ln() / 2
    for k in range(1, 21):
        b = _B[2 * k]
        s += Decimal(b.numerator) / Decimal(b.denominator) / (Decimal(2 * k * (2 * k - 1)) * w ** (2 * k - 1))
    return s - shift


def reference_p(shape, ln_gamma_shape1, x):
    """P(shape, x) = x^shape e^−x / Γ(shape + 1) · Σ x^n / ((shape + 1) … (shape + n)): all terms positive, summed to 1e-62 of the sum"""
    term = total = Decimal(1)
    n = 0
    while term > total * Decimal("1e-62"):
        n += 1
        term = term * x / (shape + n)
        total += term
    return (shape * x.ln() - x - ln_gamma_shape1).exp() * total


def reference_root(shape, u, near):
    """The x with P(shape, x) = u, by bisection from a bracket around `near` that is checked, not believed."""
    a, target, x0 = Decimal(shape), Decimal(u), Decimal(near)
    lg1 = ln_gamma(a + 1)
    width = Decimal(2) ** -34
    while True:
        lo, hi = x0 * (1 - width), x0 * (1 + width)
        if reference_p(a, lg1, lo) <= target <= reference_p(a, lg1, hi):
            break
        width *= 16
        assert width < 1, (shape, u, near)
    for _ in range(int(math.log2(float(width))) + 66):
        mid = (lo + hi) / 2
        if reference_p(a, lg1, mid) < target: lo = mid
        else: hi = mid
    return (lo + hi) / 2


def test_reference_knows_closed_forms():
    assert abs(ln_gamma(Decimal("0.5")) - (Decimal("3.14159265358979323846264338327950288419716939937510582097494459").ln() / 2)) < Decimal("1e-55")
    assert abs(ln_gamma(Decimal(11)) - Decimal(3628800).ln()) < Decimal("1e-55")
    # shape 1: P = 1 − e^−x
    assert abs(reference_p(Decimal(1), ln_gamma(Decimal(2)), Decimal("0.7")) - (1 - (-Decimal("0.7")).exp())) < Decimal("1e-55")
    assert abs(reference_root(1.0, 0.5, 0.6931471) - Decimal(2).ln()) < Decimal("1e-18")         # u = 0.5 exactly; the bracket was 1e-8 off


@pytest.mark.parametrize("shape", GRID_SHAPES)
def test_inverse_gamma_cdf_against_the_reference(exe, shape):
    """The issue's grid.  Relative error at most 2^-40 wherever the result is a normal fp32 number, absolute error at most one fp32 denormal
    step below.  Measured maxima per shape (relative, normal range): 0.01: 1.37e-13 = 2^-42.7; 0.0625: 1.41e-14;
    0.5: 2.75e-15; 1: 1.59e-15; 2.5: 1.1e-15; 30: 5.77e-15; 1000: 4.57e-14 = 2^-44.3; at most 7 Halley steps — DESIGN.md §4.11."""
    rows = pipe(exe, "icdf", [(shape, u) for u in GRID_U])
    worst, most_steps = 0.0, 0
    for u, (hexed, steps) in zip(GRID_U, rows):
        x = float.fromhex(hexed)
        most_steps = max(most_steps, int(steps))
        assert x >= 0 and math.isfinite(x)
        if x < 1e-290:                                                     # far below fp32's denormals: the root is (u Γ(shape + 1))^(1/shape) to all digits
            root = ((Decimal(u).ln() + ln_gamma(Decimal(shape) + 1)) / Decimal(shape)).exp()
            assert abs(Decimal(x) - root) <= Decimal(FP32_DENORMAL_STEP), (shape, u)
            continue
        root = reference_root(shape, u, x)
        error = abs(Decimal(x) - root)
        if root >= Decimal(FP32_MIN_NORMAL):
            relative = float(error / root)
            worst = max(worst, relative)
            assert relative <= BOUND, (shape, u, x, relative)
        else:
            assert error <= Decimal(FP32_DENORMAL_STEP), (shape, u, x)
    print(f"shape {shape}: largest relative error {worst:.3g} (2^{math.log2(worst) if worst else -math.inf:.1f}), at most {most_steps} Halley steps")


def test_inverse_gamma_cdf_against_scipy(exe):
    """In addition, where scipy happens to be installed: its gammaincinv is double precision itself, so this is a check of the reference as
    much as of the header — 1e-9 is asked for over the central grid."""
    special = pytest.importorskip("scipy.special")
    for shape in GRID_SHAPES:
        us = [u for u in GRID_U if 0.005 < u < 0.995]
        got = np.array([float.fromhex(r[0]) for r in pipe(exe, "icdf", [(shape, u) for u in us])])
        want = special.gammaincinv(shape, np.array(us))
        ok = want > 1e-290
        assert (np.abs(got[ok] - want[ok]) <= 1e-9 * want[ok]).all(), shape


def test_identities_without_a_reference(exe):
    """shape 1 is the exponential law to the last bit of the fp32 narrowing; shape 1/2 is inverseNormalCdf((1 + u)/2)²/2 within the bound;
    monotone in u over 10^5 sorted draws per shape; u = 0 → +0.0; the iteration stays below its cap (all inside the C++ program)."""
    r = subprocess.run([exe, "identities"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
    print(r.stdout)
    assert r.stdout.strip().splitlines()[-1] == "OK identities"


# ---- the host entry point

def call_host(fm, seed, laws, n_paths):
    flat = [law for row in laws for law in row]
    kinds = np.array([k for k, _, _ in flat], dtype=np.int32)
    a = np.array([v for _, v, _ in flat], dtype=np.float64)
    b = np.array([v for _, _, v in flat], dtype=np.float64)
    out = np.zeros((len(flat), max(n_paths, 0)), dtype=np.float64)
    rc = fm.lib().fmhip_increments_host(seed, len(laws), len(laws[0]), n_paths, kinds.ctypes.data_as(C.POINTER(C.c_int32)),
                                        a.ctypes.data_as(C.POINTER(C.c_double)), b.ctypes.data_as(C.POINTER(C.c_double)), out.ctypes.data_as(C.POINTER(C.c_double)))
    return rc, out


def test_header_and_bindings(fm):
    header = open(os.path.join(ROOT, "include", "fmhip.h"), encoding="utf-8").read()
    assert "enum { FMHIP_LAW_GAMMA = 4, FMHIP_LAW_EXPONENTIAL = 5 };" in header
    assert not [name for name in fm._native.SYMBOLS if "gamma" in name or "levy" in name]       # no new entry point: the two laws go through the two old ones
    assert fm.GammaLaw(2.0, 3.0).kind == GAMMA and fm.ExponentialLaw(2.0).kind == EXPONENTIAL
    assert (fm.GammaLaw(2.0, 3.0).a, fm.GammaLaw(2.0, 3.0).b) == (2.0, 3.0) and repr(fm.GammaLaw(2.0, 3.0)) == "GammaLaw(2.0, 3.0)"


def test_host_increments_with_mixed_laws(fm, exe):
    n = 4001
    u = fm.host_increments(31415, lambda i, f: fm.UniformLaw(0.0, 1.0), 2, 3, n)
    mixed = fm.host_increments(31415, lambda i, f: [fm.GammaLaw(0.06, 0.2), fm.NormalLaw(1.0), fm.ExponentialLaw(2.0)][f] if i == 0 else
                               [fm.GammaLaw(2.5, 1.0), fm.PoissonLaw(1.0), fm.GammaLaw(0.06, 3.0)][f], 2, 3, n)
    # layout [step][factor][path], every law fed the uniform of its place in the stream
    want = np.array([float.fromhex(r[0]) for r in pipe(exe, "icdf", [(0.06, v) for v in u[0, 0]])]) * 0.2
    assert (mixed[0, 0] == want).all()
    want = np.array([float.fromhex(r[0]) for r in pipe(exe, "icdf", [(2.5, v) for v in u[1, 0]])])
    assert (mixed[1, 0] == want).all()
    log1m = np.array([float.fromhex(r[0]) for r in pipe(exe, "log", list(1.0 - u[0, 2]))])
    assert (mixed[0, 2] == (0.0 - log1m) / 2.0).all()
    assert (mixed[0, 1] == np.vectorize(fm.lib().fmhip_inverse_normal_cdf)(u[0, 1])).all()
    # equal shapes, another scale: the same constants, the same root, times the scale
    base = np.array([float.fromhex(r[0]) for r in pipe(exe, "icdf", [(0.06, v) for v in u[1, 2]])])
    assert (mixed[1, 2] == base * 3.0).all()
    # a law's draws do not change when another factor's law changes
    other = fm.host_increments(31415, lambda i, f: [fm.GammaLaw(0.06, 0.2), fm.GammaLaw(700.0, 1.0), fm.UniformLaw(0.0, 1.0)][f] if i == 0 else
                               [fm.GammaLaw(2.5, 1.0), fm.ExponentialLaw(1.0), fm.NormalLaw(1.0)][f], 2, 3, n)
    assert (other[:, 0] == mixed[:, 0]).all() and (other[0, 2] == u[0, 2]).all()
    # the old laws alone: the definition as it was — normal by AS 241, uniform by a + (b − a) u, Poisson by its table
    old = fm.host_increments(31415, lambda i, f: [fm.NormalLaw(0.5), fm.UniformLaw(-1.0, 3.0), fm.PoissonLaw(1.0)][f], 2, 3, n)
    assert (old[:, 0] == np.vectorize(fm.lib().fmhip_inverse_normal_cdf)(u[:, 0]) * 0.5).all() and (old[:, 1] == -1.0 + 4.0 * u[:, 1]).all()
    F = np.cumsum([math.exp(-1.0), math.exp(-1.0), math.exp(-1.0) / 2])
    sure = (np.abs(u[:, 2, :, None] - F).min(axis=-1) > 1e-12) & (u[:, 2] < F[-1])
    assert (old[:, 2] == np.searchsorted(F, u[:, 2]))[sure].all()
    dt = np.array([0.25, 1.5])
    assert (fm.host_increments(7, lambda i, f: fm.NormalLaw(math.sqrt(dt[i])), 2, 2, 500).view(np.uint64) == fm.mersenne_increments(7, dt, 2, 500).view(np.uint64)).all()


@pytest.mark.parametrize("shape,scale", [(0.06, 0.2), (1.0, 1.0), (30.0, 0.5)])
def test_gamma_sample_moments_on_the_host(fm, shape, scale):
    n = 400_000
    x = fm.host_increments(7, lambda i, f: fm.GammaLaw(shape, scale), 1, 1, n)[0, 0]
    var = shape * scale * scale
    assert (x >= 0).all() and abs(x.mean() - shape * scale) <= 4 * math.sqrt(var / n)
    assert abs(x.var() - var) <= 4 * math.sqrt((3 * shape * (shape + 2) * scale ** 4 - var * var) / n)
    e = fm.host_increments(7, lambda i, f: fm.ExponentialLaw(4.0), 1, 1, n)[0, 0]
    assert (e >= 0).all() and abs(e.mean() - 0.25) <= 4 * 0.25 / math.sqrt(n)


def test_argument_errors(fm):
    nan, inf = float("nan"), float("inf")
    assert call_host(fm, 1, [[(GAMMA, 0.01, 1.0), (GAMMA, 1000.0, 1e-300), (EXPONENTIAL, 1e300, 0.0)]], 10)[0] == 0
    bad = [
        [[(3, 1.0, 0.0)]], [[(6, 1.0, 1.0)]],
        [[(GAMMA, 0.0, 1.0)]], [[(GAMMA, -1.0, 1.0)]], [[(GAMMA, nan, 1.0)]], [[(GAMMA, inf, 1.0)]], [[(GAMMA, 0.009999, 1.0)]], [[(GAMMA, 1000.0000001, 1.0)]],
        [[(GAMMA, 1.0, 0.0)]], [[(GAMMA, 1.0, -2.0)]], [[(GAMMA, 1.0, nan)]], [[(GAMMA, 1.0, inf)]],
        [[(EXPONENTIAL, 0.0, 0.0)]], [[(EXPONENTIAL, -1.0, 0.0)]], [[(EXPONENTIAL, nan, 0.0)]], [[(EXPONENTIAL, inf, 0.0)]],
    ]
    for laws in bad:
        rc, _ = call_host(fm, 1, laws + [[(NORMAL, 1.0, 0.0)]], 10)
        assert rc == INVALID, laws[0]
        assert b"(step 0, factor 0)" in fm.lib().fmhip_last_error(), fm.lib().fmhip_last_error()
    # 6 constants per distinct shape: 10 922 shapes fit the 2^16 table doubles, one more does not; equal shapes share an entry
    many = [[(GAMMA, 1.0 + 1e-4 * i, 1.0)] for i in range(10_922)]
    assert call_host(fm, 1, many, 1)[0] == 0
    assert call_host(fm, 1, many + [[(GAMMA, 1.0, 1.0)]] * 50, 1)[0] == 0
    assert call_host(fm, 1, many + [[(GAMMA, 5.0, 1.0)]], 1)[0] == INVALID and b"step 10922" in fm.lib().fmhip_last_error()
    # … and they share it with the Poisson tables
    assert call_host(fm, 1, many + [[(POISSON, 1.0, 0.0)]], 1)[0] == INVALID
    with pytest.raises(fm.FmhipError):
        fm.host_increments(1, lambda i, f: fm.GammaLaw(2000.0, 1.0), 1, 1, 10)


def test_processes_and_the_model_over_the_cpu_twin(fm, oracle):
    """A factory that is not the device's is handed host-drawn increments (no device is touched).  The seed is fixed and the host path
    deterministic: what is asserted on the device at 10^6 paths is checked here first."""
    mc = import_module("finmath-lib-cuda-extensions_amd.montecarlo")
    td = fm.TimeDiscretization(0.0, 10, 0.1)
    factory = oracle.RandomVariableFloatFactory()
    g = fm.GammaProcess(td, 1000, 5, 5.0, 0.2, factory)
    assert g.getNumberOfFactors() == 1 and g._law_table()[3][0] == fm.GammaLaw(5.0 * td.getTimeStep(3), 0.2)
    assert isinstance(g.getCloneWithModifiedSeed(6), fm.GammaProcess) and g.getCloneWithModifiedSeed(6).getSeed() == 6
    want = fm.host_increments(5, lambda i, f: fm.GammaLaw(5.0 * td.getTimeStep(i), 0.2), 10, 1, 1000)
    assert (g.getIncrement(4, 0).getRealizations() == want[4, 0].astype(np.float32)).all()
    exact = mc.variance_gamma_call_analytic(100.0, 0.05, 0.2, -0.14, 0.2, 1.0, 100.0)
    assert abs(exact - mc.variance_gamma_call_analytic(100.0, 0.05, 0.2, -0.14, 0.2, 1.0, 100.0, nodes=150)) <= 1e-9 and 10.5 < exact < 10.7
    # the quadrature against a plain trapezoid over the gamma time g ~ Gamma(5, 0.2)
    g = np.linspace(1e-9, 12.0, 200_001)
    density = g ** 4 * np.exp(-g / 0.2) / (24.0 * 0.2 ** 5)
    omega = mc.variance_gamma_martingale_correction(0.2, -0.14, 0.2)
    forward = 100.0 * np.exp(0.05 + omega + (-0.14 + 0.02) * g)
    s = 0.2 * np.sqrt(g)
    cdf = np.vectorize(lambda v: 0.5 * (1.0 + math.erf(v / math.sqrt(2.0))))
    d1 = (np.log(forward / 100.0) + 0.5 * s * s) / s
    integrand = math.exp(-0.05) * (forward * cdf(d1) - 100.0 * cdf(d1 - s)) * density
    assert abs(float(np.sum(0.5 * (integrand[1:] + integrand[:-1]) * np.diff(g))) - exact) <= 1e-8
    n = 200_000
    vg = fm.VarianceGammaProcess(td, n, 3141, 0.2, -0.14, 0.2, factory)
    value, rv = mc.variance_gamma_call_mc(vg, 100.0, 0.05, 1.0, 100.0)
    assert abs(value - exact) <= 3 * rv.getStandardError()
    assert vg.getIncrement(3, 0).getFiltrationTime() == td.getTime(4) and vg.getNumberOfFactors() == 1
    # θ = 0, σ²ν → 0: ω → −σ²/2; no gamma randomness left in the limit
    assert abs(mc.variance_gamma_martingale_correction(0.2, 0.0, 1e-9) + 0.02) < 1e-9
    assert abs(mc.variance_gamma_call_analytic(100.0, 0.05, 0.2, 0.0, 1e-4, 1.0, 100.0) - mc.black_scholes_call_analytic(100.0, 0.05, 0.2, 1.0, 100.0)) < 2e-3
    with pytest.raises(ValueError):
        mc.variance_gamma_martingale_correction(0.2, 3.0, 1.0)


def test_cpp_mirror_without_a_device(tmp_path):
    exe = str(tmp_path / "test_levy_mirror")
    libdir = os.path.join(ROOT, "finmath-lib-cuda-extensions_amd", "lib")
    orcdir = os.path.join(ROOT, "oracle")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_levy_increments.cpp"),
                           f"-L{libdir}", "-lfmhip", f"-L{orcdir}", "-lfm_oracle", f"-Wl,-rpath,{libdir}", f"-Wl,-rpath,{orcdir}", "-lm"])
    out = subprocess.run([exe, "cpu"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().splitlines()[-1] == "OK cpu"


def test_resource_figures_of_the_kernels():
    """fm_mt_bm_kernel and fm_mt_icdf_kernel keep DESIGN.md §4.10's figures — 128 VGPRs, no scratch, 33 792 B of LDS, 4 waves per SIMD — and
    fm_mt_levy_kernel uses no scratch either: the compiler's own remarks of a cross-compile with the build's flags."""
    hipcc = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else shutil.which("hipcc")
    if not hipcc:
        pytest.skip("needs hipcc")
    csrc = os.path.join(ROOT, "finmath-lib-cuda-extensions_amd", "csrc")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-mllvm", "-structurizecfg-skip-uniform-regions",
                        "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(csrc, "mt_bm_kernel.hip"), "-o", os.devnull],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    figures, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark:\s+(Function Name|VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\S+)", line)
        if not m: continue
        if m.group(1) == "Function Name": name = m.group(2); figures[name] = {}
        else: figures[name][m.group(1).split(" ")[0]] = int(m.group(2))
    kernel = lambda part: next(v for k, v in figures.items() if part in k)
    for part in ("fm_mt_bm_kernel", "fm_mt_icdf_kernel"):
        assert kernel(part) == {"VGPRs": 128, "ScratchSize": 0, "Occupancy": 4, "LDS": 33792}, (part, kernel(part))
    levy = kernel("fm_mt_levy_kernel")
    print("fm_mt_levy_kernel:", levy)
    assert levy["ScratchSize"] == 0 and levy["LDS"] == 33792 and levy["Occupancy"] >= 2
