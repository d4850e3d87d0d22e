"""Localized regression without a GPU (include/fmhip.h: fmhip_binned_cross_moments_host, fmhip_binned_evaluate_host; regression.py):
the host DEFINITION against math.fsum over the exact fp64 products per bin, the piecewise evaluation against a numpy fp32 restatement bit
for bit, every argument error, the estimator's generic path (the oracle's float class) against numpy's per-bin least squares, and the
kernels' resource usage for gfx950 (0 bytes of scratch)."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "finmath-lib-cuda-extensions_amd", "csrc")


def host_moments(fm, key, bounds, xs, ys, n_bins=None, counts=True, sums=True):
    """fmhip_binned_cross_moments_host through ctypes: (status, counts, sums[n_bins][q]); None in xs = the constant 1."""
    key = np.ascontiguousarray(key, dtype=np.float32)
    b = np.ascontiguousarray(bounds, dtype=np.float64)
    n_bins = b.size + 1 if n_bins is None else n_bins
    keep = [None if v is None else np.ascontiguousarray(v, dtype=np.float32) for v in list(xs) + list(ys)]
    ptr = lambda v: None if v is None else v.ctypes.data_as(C.c_void_p)
    px = (C.c_void_p * max(len(xs), 1))(*[ptr(v) for v in keep[:len(xs)]])
    py = (C.c_void_p * max(len(ys), 1))(*[ptr(v) for v in keep[len(xs):]])
    q = len(xs) * (len(xs) + 1) // 2 + len(xs) * len(ys)
    c = np.full(max(n_bins, 1), -1, dtype=np.int64)
    s = np.full(max(n_bins, 1) * max(q, 1), np.nan)
    st = fm.lib().fmhip_binned_cross_moments_host(key.ctypes.data_as(C.c_void_p), key.size, b.ctypes.data_as(C.POINTER(C.c_double)) if b.size else None, n_bins,
                                                   px, len(xs), py if ys else None, len(ys),
                                                   c.ctypes.data_as(C.POINTER(C.c_int64)) if counts else None, s.ctypes.data_as(C.POINTER(C.c_double)) if sums else None)
    return st, c[:max(n_bins, 0)], s[:max(n_bins, 0) * q].reshape(max(n_bins, 0), q) if q else s[:0]


def host_evaluate(fm, key, bounds, xs, coefficients, n_bins=None):
    key = np.ascontiguousarray(key, dtype=np.float32)
    b = np.ascontiguousarray(bounds, dtype=np.float64)
    n_bins = b.size + 1 if n_bins is None else n_bins
    keep = [None if v is None else np.ascontiguousarray(v, dtype=np.float32) for v in xs]
    px = (C.c_void_p * max(len(xs), 1))(*[None if v is None else v.ctypes.data_as(C.c_void_p) for v in keep])
    co = np.ascontiguousarray(coefficients, dtype=np.float64)
    out = np.empty(key.size, dtype=np.float32)
    st = fm.lib().fmhip_binned_evaluate_host(key.ctypes.data_as(C.c_void_p), key.size, b.ctypes.data_as(C.POINTER(C.c_double)) if b.size else None, n_bins,
                                              px, len(xs), co.ctypes.data_as(C.POINTER(C.c_double)), out.ctypes.data_as(C.c_void_p))
    return st, out


def bin_of(key, bounds):
    """#{ j : bounds[j] < (double) key }, -1 for NaN: the contract, restated with numpy."""
    k = np.asarray(key, dtype=np.float32).astype(np.float64)
    b = np.asarray(bounds, dtype=np.float64)
    pos = (b[None, :] < k[:, None]).sum(axis=1) if b.size else np.zeros(k.size, dtype=np.int64)
    return np.where(np.isnan(k), -1, pos)


def exact_and_bound(key, bounds, xs, ys):
    """Per bin: counts, math.fsum of the exact fp64 products in the packed layout, and m·2⁻⁵³·Σ|terms| — the worst case of ANY summation
    order of m terms (each of the m − 1 additions rounds a partial sum that is at most Σ|terms| in magnitude, relatively 2⁻⁵³)."""
    bins = bin_of(key, bounds)
    n_bins = len(bounds) + 1
    cols = lambda vs: [np.ones(len(key)) if v is None else np.asarray(v, dtype=np.float32).astype(np.float64) for v in vs]
    X, Y = cols(xs), cols(ys)
    pairs = [(X[i], X[j]) for i in range(len(X)) for j in range(i, len(X))] + [(X[i], Y[m]) for i in range(len(X)) for m in range(len(Y))]
    counts = np.array([(bins == b).sum() for b in range(n_bins)], dtype=np.int64)
    want = np.zeros((n_bins, len(pairs))); tol = np.zeros((n_bins, len(pairs)))
    for b in range(n_bins):
        sel = bins == b
        for q, (u, v) in enumerate(pairs):
            terms = u[sel] * v[sel]                                 # exact: 24 x 24 significant bits
            want[b, q] = math.fsum(terms)
            tol[b, q] = counts[b] * 2.0 ** -53 * math.fsum(np.abs(terms))
    return counts, want, tol


def edge_keys(n, seed):
    rng = np.random.default_rng(seed)
    key = rng.standard_normal(n).astype(np.float32)
    key[:8] = [np.nan, np.inf, -np.inf, -0.0, 0.0, 0.5, -0.5, np.nan][:min(n, 8)] if n >= 8 else key[:8]
    return key, rng


@pytest.mark.parametrize("n_bins", [1, 2, 16, 64])
@pytest.mark.parametrize("shape", [(1, 0), (2, 1), (3, 1), (3, 4)])
def test_definition_against_exact_sums(fm, n_bins, shape):
    n = 5003
    key, rng = edge_keys(n, 100 * n_bins + shape[0])
    bounds = np.sort(rng.standard_normal(n_bins - 1))
    if n_bins >= 2: bounds[0] = 0.0; bounds.sort()                  # ±0.0 against a bound of 0; 0.5 / −0.5 may equal no bound
    if n_bins >= 16: bounds[3] = bounds[4]                          # an empty bin
    if n_bins == 64: bounds[0], bounds[-1] = -np.inf, np.inf
    bounds = np.sort(bounds)
    key[8] = np.float32(bounds[n_bins // 2 - 1]) if n_bins > 1 else key[8]      # a key equal to a bound (where the bound is a float)
    xs = [None] + [rng.standard_normal(n).astype(np.float32) for _ in range(shape[0] - 1)] if shape[0] > 1 else [rng.standard_normal(n).astype(np.float32)]
    ys = [rng.standard_normal(n).astype(np.float32) for _ in range(shape[1])]
    st, counts, sums = host_moments(fm, key, bounds, xs, ys)
    assert st == 0, fm.lib().fmhip_last_error()
    want_counts, want, tol = exact_and_bound(key, bounds, xs, ys)
    assert (counts == want_counts).all() and counts.sum() == n - 2   # the two NaN keys belong to no bin
    assert (np.abs(sums - want) <= tol).all()
    if n_bins >= 16: assert counts[4] == 0 and (sums[4] == 0.0).all()


def test_edge_keys_fall_where_the_contract_says(fm):
    key = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 1.0, np.nextafter(np.float32(1.0), np.float32(2.0)), -1.0], dtype=np.float32)
    st, counts, sums = host_moments(fm, key, [-1.0, 0.0, 1.0], [None], [])
    assert st == 0
    # (-inf,-1]: -inf, -1 | (-1,0]: -0.0, +0.0 | (0,1]: 1 | (1,inf): inf, 1+ulp
    assert counts.tolist() == [2, 2, 1, 2] and sums[:, 0].tolist() == [2.0, 2.0, 1.0, 2.0]
    st, counts, _ = host_moments(fm, key, [-np.inf, np.inf], [None], [])
    assert st == 0 and counts.tolist() == [1, 6, 0]                 # -inf is not above a bound of -inf; +inf is not above +inf
    st, counts, _ = host_moments(fm, np.full(100, 2.5, dtype=np.float32), [1.0, 2.5, 3.0], [None], [])
    assert st == 0 and counts.tolist() == [0, 100, 0, 0]            # all keys equal, and equal to a bound


def evaluate_numpy(key, bounds, xs, coefficients):
    """The chain in numpy fp32: every product and every sum is one fp32 operation."""
    bins = bin_of(key, bounds)
    c = np.asarray(coefficients, dtype=np.float64).reshape(len(bounds) + 1, len(xs)).astype(np.float32)
    col = lambda v: np.ones(len(key), dtype=np.float32) if v is None else np.asarray(v, dtype=np.float32)
    safe = np.maximum(bins, 0)
    with np.errstate(all="ignore"):
        r = col(xs[0]) * c[safe, 0]
        for i in range(1, len(xs)): r = r + col(xs[i]) * c[safe, i]
    return np.where(bins < 0, np.float32(np.nan), r).astype(np.float32)


@pytest.mark.parametrize("n_bins", [1, 2, 16, 64])
@pytest.mark.parametrize("n_x", [1, 2, 3])
def test_evaluation_is_the_fp32_chain_bit_for_bit(fm, n_bins, n_x):
    from conftest import assert_bits_equal
    n = 4099
    key, rng = edge_keys(n, 7 * n_bins + n_x)
    bounds = np.sort(rng.standard_normal(n_bins - 1))
    xs = ([None] if n_x > 1 else []) + [(rng.standard_normal(n) * 3).astype(np.float32) for _ in range(n_x - (1 if n_x > 1 else 0))]
    coefficients = rng.standard_normal((n_bins, n_x)) * 1.7           # doubles that are not floats: the narrowing is part of the contract
    st, out = host_evaluate(fm, key, bounds, xs, coefficients)
    assert st == 0, fm.lib().fmhip_last_error()
    assert np.isnan(out[0]) and np.isnan(out[7])
    assert_bits_equal(out, evaluate_numpy(key, bounds, xs, coefficients), "binned evaluation")


def test_argument_errors(fm):
    N = fm._native
    key = np.arange(10, dtype=np.float32); x = key + 1
    bad = N.ERR_INVALID_ARGUMENT
    assert host_moments(fm, key, [0.0], [None, x], [x])[0] == 0
    assert host_moments(fm, key, [0.0], [], [])[0] == bad                                    # n_x out of range
    assert host_moments(fm, key, [0.0], [x] * 4, [])[0] == bad
    assert host_moments(fm, key, [0.0], [x], [x] * 5)[0] == bad
    assert host_moments(fm, key, [], [x], [], n_bins=0)[0] == bad                            # n_bins out of range
    assert host_moments(fm, key, np.zeros(64), [x], [], n_bins=65)[0] == bad
    assert host_moments(fm, key, [], [x], [], n_bins=3)[0] == bad                            # bounds NULL
    assert host_moments(fm, key, [1.0, 0.5], [x], [])[0] == bad                              # unsorted
    assert host_moments(fm, key, [0.0, np.nan], [x], [])[0] == bad                           # NaN bound
    assert host_moments(fm, key, [0.0], [x], [None])[0] == bad                               # the constant 1 among y
    assert host_moments(fm, key, [0.0], [x], [], counts=False)[0] == bad
    assert host_moments(fm, key, [0.0], [x], [], sums=False)[0] == bad
    assert host_moments(fm, key[:0], [0.0], [x[:0]], [])[0] == bad                           # n == 0
    lib = fm.lib()
    c = (C.c_int64 * 4)(); s = (C.c_double * 16)(); px = (C.c_void_p * 1)(x.ctypes.data_as(C.c_void_p)); b = (C.c_double * 1)(0.0)
    assert lib.fmhip_binned_cross_moments_host(None, 10, b, 2, px, 1, None, 0, c, s) == bad   # no key
    assert lib.fmhip_binned_cross_moments_host(key.ctypes.data_as(C.c_void_p), 10, b, 2, None, 1, None, 0, c, s) == bad
    assert lib.fmhip_binned_cross_moments_host(key.ctypes.data_as(C.c_void_p), 10, b, 2, px, 1, None, 1, c, s) == bad
    out = np.empty(10, dtype=np.float32); co = (C.c_double * 6)()
    assert host_evaluate(fm, key, [0.0], [x], [1.0, 2.0])[0] == 0
    assert host_evaluate(fm, key, [1.0, 0.0], [x], [1.0] * 3)[0] == bad
    assert host_evaluate(fm, key, [0.0], [x] * 4, [1.0] * 8)[0] == bad
    assert lib.fmhip_binned_evaluate_host(key.ctypes.data_as(C.c_void_p), 10, b, 2, px, 1, None, out.ctypes.data_as(C.c_void_p)) == bad
    assert lib.fmhip_binned_evaluate_host(key.ctypes.data_as(C.c_void_p), 10, b, 2, px, 1, co, None) == bad
    assert lib.fmhip_binned_evaluate_host(None, 10, b, 2, px, 1, co, out.ctypes.data_as(C.c_void_p)) == bad
    assert lib.fmhip_binned_evaluate_host(key.ctypes.data_as(C.c_void_p), 0, b, 2, px, 1, co, out.ctypes.data_as(C.c_void_p)) == bad
    for name in ("fmhip_binned_cross_moments", "fmhip_binned_cross_moments_host", "fmhip_binned_evaluate", "fmhip_binned_evaluate_host"):
        assert name in N.SYMBOLS and hasattr(lib, name)
    # the device entry points without a device: an error, never a fallback to the host definition
    if not lib.fmhip_is_initialized():
        h = (C.c_int64 * 1)(1)
        assert lib.fmhip_binned_cross_moments(1, b, 2, h, 1, None, 0, c, s) != 0
        assert lib.fmhip_binned_evaluate(1, b, 2, h, 1, co, h) != 0


def per_bin_lstsq(key, bounds, cols, y):
    bins = bin_of(key, bounds)
    beta = np.zeros((len(bounds) + 1, len(cols)))
    for b in range(len(bounds) + 1):
        sel = bins == b
        if sel.any(): beta[b] = np.linalg.lstsq(np.stack([c[sel] for c in cols], axis=1).astype(np.float64), y[sel].astype(np.float64), rcond=None)[0]
    return beta


def test_estimator_generic_path_against_per_bin_lstsq(fm, oracle):
    """The oracle's float class: indicators by choose, averages pair by pair.  Products round to fp32 (2⁻²⁴ relative per element) before the
    fp64 average; a bin's 2 x 2 block of {1, s} on a bin of width w has condition number ~ (|s|/w)²: with 8 quantile bins of a standard
    normal key that is below 1e3 in the inner bins and the data are O(1), so 1e-3 absolute on the coefficients leaves a decade of room."""
    n = 40_000
    rng = np.random.default_rng(5)
    s = rng.standard_normal(n).astype(np.float32)
    y = (np.maximum(0.3 - s, 0.0) + 0.1 * rng.standard_normal(n)).astype(np.float32)      # a kinked conditional expectation
    fo = oracle.RandomVariableFloatFactory()
    S, Y = fo.createRandomVariable(0.0, s), fo.createRandomVariable(0.0, y)
    est = fm.MonteCarloConditionalExpectationLocalizedRegression(S, 8, [fo.createRandomVariable(1.0), S])
    counts = est.getBinCounts()
    assert counts.sum() == n and counts.max() - counts.min() <= 1      # distinct keys (a continuous law): quantile bins differ by at most 1
    assert (counts == np.bincount(bin_of(s, est.bounds), minlength=8)).all()
    beta = est.getLinearRegressionParameters(Y)
    assert beta.shape == (8, 2)
    want = per_bin_lstsq(s, est.bounds, [np.ones(n, dtype=np.float32), s], y)
    assert np.abs(beta - want).max() <= 1e-3, np.abs(beta - want).max()
    ce = est.getConditionalExpectation(Y).getRealizations()
    bins = bin_of(s, est.bounds)
    fit = want[bins, 0] + want[bins, 1] * s.astype(np.float64)
    assert np.abs(ce - fit).max() <= 2e-3
    # the kink is resolved: a global line is far worse
    line = np.linalg.lstsq(np.stack([np.ones(n), s], axis=1).astype(np.float64), y.astype(np.float64), rcond=None)[0]
    truth = np.maximum(0.3 - s.astype(np.float64), 0.0)
    assert np.abs(ce - truth).mean() < 0.25 * np.abs(line[0] + line[1] * s - truth).mean()
    # several dependents; empty bins get coefficients 0
    est2 = fm.MonteCarloConditionalExpectationLocalizedRegression(S, 4, [fo.createRandomVariable(1.0), S], bounds=[-100.0, 0.0, 100.0])
    beta2 = est2.getLinearRegressionParameters([Y, S])
    assert beta2.shape == (4, 2, 2) and (beta2[0] == 0.0).all() and (beta2[3] == 0.0).all()
    assert np.abs(beta2[1:3, :, 1] - np.array([0.0, 1.0])).max() <= 1e-4      # S regressed on {1, S}
    with pytest.raises(ValueError): fm.MonteCarloConditionalExpectationLocalizedRegression(S, 65, [S])
    with pytest.raises(ValueError): fm.MonteCarloConditionalExpectationLocalizedRegression(S, 3, [S], bounds=[1.0, 0.0])


def test_generic_path_puts_edge_keys_where_the_definition_does(fm, oracle):
    """NaN, ±inf, ±0.0 and a key equal to a bound, bounds that are fp32 values, +inf among them: counts per bin and the estimate of the
    generic path against the host definition (the estimate bit for bit: both are the fp32 chain)."""
    from conftest import assert_bits_equal
    rng = np.random.default_rng(9)
    n = 2000
    key = rng.standard_normal(n).astype(np.float32)
    key[:7] = [np.nan, np.inf, -np.inf, -0.0, 0.0, 0.5, np.nan]
    x = rng.standard_normal(n).astype(np.float32)
    y = rng.standard_normal(n).astype(np.float32)
    bounds = [-0.5, 0.0, 0.5, np.inf]
    fo = oracle.RandomVariableFloatFactory()
    Kv, X, Y = fo.createRandomVariable(0.0, key), fo.createRandomVariable(0.0, x), fo.createRandomVariable(0.0, y)
    est = fm.MonteCarloConditionalExpectationLocalizedRegression(Kv, 5, [fo.createRandomVariable(1.0), X], bounds=bounds)
    st, counts, _ = host_moments(fm, key, bounds, [None], [])
    assert st == 0 and est.getBinCounts().tolist() == counts.tolist() and counts.sum() == n - 2 and counts[4] == 0
    beta = est.getLinearRegressionParameters(Y)
    assert np.isfinite(beta).all() and (beta[4] == 0.0).all()          # NaN keys enter no block; the bin above +inf is empty
    st, want = host_evaluate(fm, key, bounds, [None, x], beta)
    assert st == 0
    assert_bits_equal(est.getConditionalExpectation(Y).getRealizations().astype(np.float32), want, "generic estimate")


def test_cpp_mirror_compiles_against_the_library_and_shares_the_definition(fm, tmp_path):
    """host/localized_regression.hpp (the C++ estimator) builds with all warnings on against random_variable.hpp and links against the
    library; the definition it shares with the entry points (host/binned_regression.hpp) gives the bits of fmhip_binned_*_host."""
    gxx = shutil.which("g++")
    if not gxx: pytest.skip("needs g++")
    host = os.path.join(ROOT, "finmath-lib-cuda-extensions_amd", "host")
    src = tmp_path / "mirror.cpp"
    src.write_text(r'''
#include <cstdio>
#include <cstring>
#include "hip_backend.hpp"
#include "localized_regression.hpp"
int main() {
    const int n = 1000;
    std::vector<float> key(n), x(n), y(n), e1(n), e2(n);
    for (int p = 0; p < n; ++p) { key[p] = (float)((p * 37) % 101) * 0.01f; x[p] = (float)((p * 7) % 13) * 0.3f - 1.0f; y[p] = (float)((p * 11) % 17) * 0.1f; }
    const double bounds[3] = { 0.25, 0.5, 0.75 }, coef[8] = { 0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8 };
    const float* xs[2] = { nullptr, x.data() }; const float* ys[1] = { y.data() };
    int64_t c1[4] = { 0 }, c2[4] = { 0 }; double s1[20] = { 0 }, s2[20] = { 0 };
    fmhost::binnedCrossMoments(key.data(), n, bounds, 4, xs, 2, ys, 1, c1, s1);
    if (fmhip_binned_cross_moments_host(key.data(), n, bounds, 4, xs, 2, ys, 1, c2, s2) != FMHIP_OK) return 2;
    if (std::memcmp(c1, c2, sizeof c1) || std::memcmp(s1, s2, sizeof s1)) return 3;
    fmhost::binnedEvaluate(key.data(), n, bounds, 4, xs, 2, coef, e1.data());
    if (fmhip_binned_evaluate_host(key.data(), n, bounds, 4, xs, 2, coef, e2.data()) != FMHIP_OK) return 4;
    if (std::memcmp(e1.data(), e2.data(), n * 4)) return 5;
    try { fmhost::binnedCheckBins(coef + 6, 0); return 6; } catch (const std::invalid_argument&) {}
    // the estimator is a template-free class: naming its members makes the compiler check every body
    auto p1 = &fmhost::MonteCarloConditionalExpectationLocalizedRegression::getLinearRegressionParameters;
    auto p2 = &fmhost::MonteCarloConditionalExpectationLocalizedRegression::getConditionalExpectationHandle;
    std::printf("mirror ok %d\n", (int)(p1 != nullptr) + (int)(p2 != nullptr));
    return 0;
}
''')
    exe = tmp_path / "mirror"
    lib = os.path.dirname(fm._native.LIB_PATH)
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I", os.path.join(ROOT, "include"), "-I", host,
                        str(src), "-o", str(exe), "-L", lib, "-lfmhip", f"-Wl,-rpath,{lib}"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "mirror ok 2" in out.stdout, (out.returncode, out.stdout, out.stderr[-1000:])


def test_kernels_compile_for_gfx950_without_scratch():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc): pytest.skip("needs hipcc")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                        "-c", os.path.join(CSRC, "binned_kernel.hip"), "-o", os.devnull], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    blocks = re.split(r"remark: Function Name: ", r.stderr)[1:]
    seen = {}
    for blk in blocks:
        name = blk.split()[0]
        seen[name] = (int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", blk).group(1)), int(re.search(r"LDS Size \[bytes/block\]: (\d+)", blk).group(1)))
    kernels = {k: v for k, v in seen.items() if "fm_binned_xmom_kernel" in k or "fm_binned_eval_kernel" in k}
    assert len(kernels) == 2, seen
    for name, (scratch, lds) in kernels.items():
        assert scratch == 0, (name, scratch)
        assert lds <= 160 * 1024, (name, lds)                        # a CU's LDS (one workgroup may declare all of it)
