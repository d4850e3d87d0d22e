"""The host side of the device regression, without a GPU: the pivoted Cholesky of the normal equations (regression.py) on fixed matrices
and on a singular one, the estimator's product-by-product path on the CPU twin's vectors against numpy's least squares, the Bermudan
driver on the twin (one exercise date = the European option of the same paths), and the engine's cross-moments pass against the null
device under AddressSanitizer / UBSan and ThreadSanitizer (tests/nulldev: the null device plus a stand-in for the launcher, null_xmom.cpp,
and a driver of its own, drive_xmom.cpp) on one engine, behind a device list and with thread engines, a second thread releasing handles meanwhile."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NULLDEV = os.path.join(ROOT, "tests", "nulldev")


def test_entry_point_is_bound(fm):
    assert "fmhip_cross_moments" in fm._native.SYMBOLS and hasattr(fm.lib(), "fmhip_cross_moments")
    assert callable(fm.cross_moments) and callable(fm.covariance_matrix)


def test_solver_on_fixed_matrices(fm):
    A = np.array([[4.0, 2.0, 2.0], [2.0, 3.0, 1.0], [2.0, 1.0, 5.0]])
    A = A @ A.T
    b = np.array([1.0, 2.0, 3.0])
    assert np.abs(fm.solve_normal_equations(A, b) - np.linalg.solve(A, b)).max() <= 1e-13
    B = np.stack([b, 2.0 * b, b[::-1]], axis=1)
    assert np.abs(fm.solve_normal_equations(A, B) - np.linalg.solve(A, B)).max() <= 1e-13
    H = np.array([[1.0 / (i + j + 1) for j in range(5)] for i in range(5)])          # Hilbert: condition 5e5, still above the pivot rule
    assert np.abs(H @ fm.solve_normal_equations(H, H @ np.ones(5)) - H @ np.ones(5)).max() <= 1e-12


def test_solver_drops_what_the_pivot_rule_says(fm):
    rng = np.random.default_rng(0)
    X = rng.standard_normal((200, 4))
    X[:, 3] = X[:, 0] + X[:, 1]                                                      # collinear
    X = np.c_[X, np.zeros(200)]                                                      # the indicator of an empty bin
    y = X @ np.array([1.0, 2.0, 3.0, 0.0, 0.0]) + 0.1 * rng.standard_normal(200)
    beta = fm.solve_normal_equations(X.T @ X, X.T @ y)
    assert np.isfinite(beta).all() and beta[4] == 0.0 and (beta == 0.0).sum() == 2
    assert np.abs(X @ beta - X @ np.linalg.lstsq(X, y, rcond=None)[0]).max() <= 1e-10   # the same fitted values as the minimum-norm solution
    assert (fm.solve_normal_equations(np.zeros((3, 3)), np.ones(3)) == 0.0).all()       # nothing to regress on
    # the first of equal pivots is taken: of two identical functions the second is dropped
    Z = np.c_[X[:, 0], X[:, 0]]
    beta = fm.solve_normal_equations(Z.T @ Z, Z.T @ y)
    assert beta[1] == 0.0 and beta[0] != 0.0


def test_generic_path_on_the_twin_against_lstsq(fm, oracle):
    rng = np.random.default_rng(3)
    n = 20_000
    z = rng.standard_normal(n).astype(np.float32)
    y = (1.0 + 0.5 * z - 0.25 * z * z + 0.3 * rng.standard_normal(n)).astype(np.float32)
    f = oracle.RandomVariableFloatFactory()
    Z, Y = f.createRandomVariable(0.0, z), f.createRandomVariable(0.0, y)
    est = fm.MonteCarloConditionalExpectationRegression([f.createRandomVariable(1.0), Z, Z.mult(Z)])
    beta = est.getLinearRegressionParameters(Y)
    X = np.stack([np.ones(n), z, z * z], axis=1).astype(np.float64)
    want = np.linalg.lstsq(X, y.astype(np.float64), rcond=None)[0]
    assert np.abs(beta - want).max() <= 1e-5                                          # fp32 products, condition number ≈ 9
    ce = est.getConditionalExpectation(Y).getRealizations()
    assert np.abs(ce - X @ want).max() <= 1e-5
    both = est.getLinearRegressionParameters([Y, Y.mult(2.0)])
    assert both.shape == (3, 2) and np.abs(both[:, 1] - 2.0 * both[:, 0]).max() <= 1e-6


class ArrayBrownianMotion:
    def __init__(self, td, factory, increments):
        self.td, self.factory = td, factory
        self.inc = [[factory.createRandomVariable(td.getTime(t + 1), a) for a in row] for t, row in enumerate(increments)]
    def getTimeDiscretization(self): return self.td
    def getBrownianIncrement(self, t, f): return self.inc[t][f]
    def getRandomVariableForConstant(self, v): return self.factory.createRandomVariable(v)


def test_bermudan_driver_on_the_twin(fm, oracle):
    from importlib import import_module
    mc = import_module("finmath-lib-cuda-extensions_amd.montecarlo")
    n, r, sigma, strike = 20_000, 0.05, 0.30, 1.05
    td = fm.TimeDiscretization(0.0, 10, 0.2)
    bm = ArrayBrownianMotion(td, oracle.RandomVariableFloatFactory(), oracle.bm_generate(99, [0.2] * 10, 1, n))
    x = bm.getRandomVariableForConstant(0.0)
    for i in range(10):
        x = x.add((r - 0.5 * sigma * sigma) * 0.2).addProduct(bm.getBrownianIncrement(i, 0), sigma)
    european = x.exp().bus(strike).floor(0.0).div(math.exp(r * 2.0)).getAverage()
    one_date, _ = mc.bermudan_option_mc(bm, 1.0, r, sigma, [2.0], strike)
    assert one_date == european
    bermudan, value = mc.bermudan_option_mc(bm, 1.0, r, sigma, [0.2 * k for k in range(1, 11)], strike)
    assert european < bermudan < 0.17 and value.size() == n                            # the tree with these ten dates: 0.1535
    call, _ = mc.bermudan_option_mc(bm, 1.0, r, sigma, [1.0, 2.0], strike, call=True)
    european_call = x.exp().sub(strike).floor(0.0).div(math.exp(r * 2.0)).getAverage()
    assert abs(call - european_call) <= 0.02 * european_call                           # no dividends: early exercise of a call is worth nothing


@pytest.fixture(scope="module")
def built():
    if not shutil.which("g++") or not os.path.exists("/opt/rocm/include/hip/hip_runtime_api.h"):
        pytest.skip("needs g++ and the HIP headers")
    r = subprocess.run(["make", "-C", NULLDEV, "-j8", "xmom_asan", "xmom_tsan"], capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return os.path.join(NULLDEV, "build")


@pytest.mark.parametrize("env", [{}, {"FMNULL_DEVICES": "2"}, {"FMNULL_DEVICES": "3"}, {"FMNULL_THREAD_ENGINES": "1"}])
def test_engine_pass_is_clean_under_the_sanitizers(built, tmp_path, env):
    full = dict(os.environ, FMHIP_JIT_CACHE_DIR=str(tmp_path / "code_objects"), FMHIP_JIT_PACK_DIR="off", FMHIP_RING_BYTES="16384", FMHIP_ARENA_BYTES="4096",
                ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1", TSAN_OPTIONS="halt_on_error=1", **env)
    a = subprocess.run([os.path.join(built, "drive_xmom_asan")], capture_output=True, text=True, timeout=600, env=full)
    assert a.returncode == 0 and "Sanitizer" not in a.stderr and "runtime error" not in a.stderr, a.stdout[-500:] + a.stderr[-6000:]
    assert a.stdout.count("xmom done") == 2
    t = subprocess.run([os.path.join(built, "drive_xmom_tsan")], capture_output=True, text=True, timeout=600, env=full)
    assert t.returncode == 0 and "ThreadSanitizer" not in t.stderr, t.stdout[-500:] + t.stderr[-6000:]
    assert t.stdout.count("xmom done") == 2
