"""The wide regression without a GPU: Engine::xmom_wide_pass (csrc/xmom_wide_engine.hpp) against the null device under AddressSanitizer /
UBSan and ThreadSanitizer — HOST builds of stand-alone programs only (tests/nulldev/wide.mk) —, the row-operation solver beyond 12 unknowns,
the routing between fmhip_cross_moments and fmhip_cross_moments_wide, and the max-call driver on the CPU twin."""
import math
import os
import shutil
import subprocess
from importlib import import_module

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NULLDEV = os.path.join(ROOT, "tests", "nulldev")


@pytest.fixture(scope="module")
def built():
    if not shutil.which("g++") or not os.path.exists("/opt/rocm/include/hip/hip_runtime_api.h"):
        pytest.skip("needs g++ and the HIP headers")
    r = subprocess.run(["make", "-C", NULLDEV, "-f", "wide.mk", "-j8", "xmom_wide_asan", "xmom_wide_tsan", "xmom_wide_absent_asan"], capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return os.path.join(NULLDEV, "build")


def _env(tmp_path, env):
    return dict(os.environ, FMHIP_JIT_CACHE_DIR=str(tmp_path / "code_objects"), FMHIP_JIT_PACK_DIR="off", FMHIP_RING_BYTES="16384", FMHIP_ARENA_BYTES="4096",
                ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1", TSAN_OPTIONS="halt_on_error=1", **env)


@pytest.mark.parametrize("env", [{}, {"FMNULL_DEVICES": "2"}, {"FMNULL_DEVICES": "3"}, {"FMNULL_THREAD_ENGINES": "1"}])
def test_engine_pass_is_clean_under_the_sanitizers(built, tmp_path, env):
    """drive_xmom_wide: 1 … 64 vectors stored, pending and shared, the constant 1 in the first and the fourth group, a second thread releasing
    the inputs of pending operands during the call, every argument error — on one engine, behind 2 and 3 shards, with thread engines."""
    full = _env(tmp_path, env)
    a = subprocess.run([os.path.join(built, "drive_xmom_wide_asan")], capture_output=True, text=True, timeout=600, env=full)
    assert a.returncode == 0 and "Sanitizer" not in a.stderr and "runtime error" not in a.stderr, a.stdout[-500:] + a.stderr[-6000:]
    assert a.stdout.count("xmom wide done") == 2
    t = subprocess.run([os.path.join(built, "drive_xmom_wide_tsan")], capture_output=True, text=True, timeout=600, env=full)
    assert t.returncode == 0 and "ThreadSanitizer" not in t.stderr, t.stdout[-500:] + t.stderr[-6000:]
    assert t.stdout.count("xmom wide done") == 2


@pytest.mark.parametrize("env", [{}, {"FMNULL_DEVICES": "2"}, {"FMNULL_THREAD_ENGINES": "1"}])
def test_a_build_without_the_kernel_answers_unsupported(built, tmp_path, env):
    a = subprocess.run([os.path.join(built, "drive_xmom_wide_absent_asan")], capture_output=True, text=True, timeout=600, env=_env(tmp_path, env))
    assert a.returncode == 0 and "Sanitizer" not in a.stderr and "runtime error" not in a.stderr, a.stdout[-500:] + a.stderr[-6000:]
    assert a.stdout.count("xmom wide absent done") == 2


# ------------------------------------------------------------------ solve_normal_equations beyond 12 unknowns
def _parent_solve(A, b):
    """The loops solve_normal_equations runs for K <= 12, as they stood before the row-operation path was added beside them."""
    A = np.asarray(A, dtype=np.float64); B = np.asarray(b, dtype=np.float64).reshape(A.shape[0], -1)
    K = A.shape[0]
    perm = list(range(K)); d = [float(A[i, i]) for i in range(K)]
    tol = 1e-12 * max(d)
    L = np.zeros((K, K)); rank = K
    for k in range(K):
        p = k
        for q in range(k + 1, K):
            if d[perm[q]] > d[perm[p]]: p = q
        if d[perm[p]] <= tol: rank = k; break
        perm[k], perm[p] = perm[p], perm[k]
        i = perm[k]
        L[i, k] = math.sqrt(d[i])
        for q in range(k + 1, K):
            j = perm[q]
            s = float(A[j, i])
            for t in range(k): s -= L[j, t] * L[i, t]
            L[j, k] = s / L[i, k]
            d[j] -= L[j, k] * L[j, k]
    x = np.zeros((K, B.shape[1]))
    for m in range(B.shape[1]):
        z = [0.0] * rank
        for k in range(rank):
            s = float(B[perm[k], m])
            for t in range(k): s -= L[perm[k], t] * z[t]
            z[k] = s / L[perm[k], k]
        for k in range(rank - 1, -1, -1):
            s = z[k]
            for t in range(k + 1, rank): s -= L[perm[t], k] * x[perm[t], m]
            x[perm[k], m] = s / L[perm[k], k]
    return x


def _spd(K, seed):
    """XᵀX/n of K standard normals over n = 50 K paths plus the identity: eigenvalues within [1, ~3], condition number < 4."""
    X = np.random.default_rng(seed).standard_normal((50 * K, K))
    return X.T @ X / (50 * K) + np.eye(K)


@pytest.mark.parametrize("K", [13, 30, 56])
def test_solver_beyond_twelve_unknowns(fm, K):
    A = _spd(K, K)
    assert np.linalg.cond(A) < 4
    rng = np.random.default_rng(100 + K)
    b = rng.standard_normal((K, 3))
    x = fm.solve_normal_equations(A, b)
    assert np.abs(x - np.linalg.solve(A, b)).max() <= 1e-11
    assert np.abs(fm.solve_normal_equations(A, b[:, 0]) - x[:, 0]).max() <= 1e-13       # one column or three: BLAS orders the dot products differently, K·2^-53·κ·max|x| < 1e-13
    assert np.abs(x - _parent_solve(A, b)).max() <= 1e-12                       # the same algorithm, dot products in another order
    # a collinear column (twice column 2) and an empty one: coefficient 0 for the later of the pair and for the empty one, as at K <= 12
    X = rng.standard_normal((40 * K, K))
    X[:, 7] = 2.0 * X[:, 2]
    X[:, 11] = 0.0
    y = X @ rng.standard_normal(K)
    G, g = X.T @ X / X.shape[0], X.T @ y / X.shape[0]
    beta = fm.solve_normal_equations(G, g)
    ref = _parent_solve(G, g)[:, 0]
    assert beta[11] == 0.0 and (beta[2] == 0.0) != (beta[7] == 0.0)
    assert [c == 0.0 for c in beta] == [c == 0.0 for c in ref]
    assert np.abs(X @ beta - y).max() <= 1e-9 and np.abs(beta - ref).max() <= 1e-9


def test_solver_at_twelve_unknowns_is_the_parent_bit_for_bit(fm):
    A = _spd(12, 5)
    b = np.random.default_rng(6).standard_normal((12, 2))
    assert (fm.solve_normal_equations(A, b).view(np.uint64) == _parent_solve(A, b).view(np.uint64)).all()


# ------------------------------------------------------------------ routing
class _Recorder:
    """Stands in for the native library: records (symbol, n_x, n_y) and answers with sums of a diagonal S = n and T = 0."""
    def __init__(self): self.calls = []
    def _answer(self, name):
        def call(hx, n_x, hy, n_y, out):
            self.calls.append((name, n_x, n_y))
            at = 0
            for i in range(n_x):
                for j in range(i, n_x): out[at] = 1000.0 if i == j else 0.0; at += 1
            for k in range(n_x * n_y): out[at + k] = 0.0
            return 0
        return call
    def __getattr__(self, name):
        if name in ("fmhip_cross_moments", "fmhip_cross_moments_wide"): return self._answer(name)
        raise AttributeError(name)


class _Vec:
    def __init__(self, handle): self.handle, self.n = handle, 1000


def test_routing_between_the_narrow_and_the_wide_call(fm, monkeypatch):
    reg = import_module("finmath-lib-cuda-extensions_amd.regression")
    lib = _Recorder()
    monkeypatch.setattr(reg.N, "lib", lambda: lib)
    v = [_Vec(100 + i) for i in range(70)]
    reg.cross_moments(v[:12], v[12:16])
    reg.cross_moments(v[:13], v[13:14])
    S, T = reg.cross_moments(v[:60], v[60:64])
    assert S.shape == (60, 60) and T.shape == (60, 4)
    reg.cross_moments([None] + v[:11], v[12:13])
    assert lib.calls == [("fmhip_cross_moments", 12, 4), ("fmhip_cross_moments_wide", 13, 1), ("fmhip_cross_moments_wide", 60, 4), ("fmhip_cross_moments", 12, 1)]
    with pytest.raises(ValueError):
        reg.cross_moments(v[:61], v[61:65])
    assert len(lib.calls) == 4
    assert reg.covariance_matrix(v[:63]).shape == (63, 63) and lib.calls[-1] == ("fmhip_cross_moments_wide", 64, 0)
    assert reg.covariance_matrix(v[:11]).shape == (11, 11) and lib.calls[-1] == ("fmhip_cross_moments", 12, 0)


def test_estimator_chunks_dependents_by_what_the_wide_call_has_left(fm, monkeypatch):
    reg = import_module("finmath-lib-cuda-extensions_amd.regression")
    lib = _Recorder()
    monkeypatch.setattr(reg.N, "lib", lambda: lib)

    class RV(fm.RandomVariableHip):                                 # a stochastic RandomVariableHip without a device behind it
        def __init__(self, handle): self.realizations = _Vec(handle)
        def isDeterministic(self): return False
        def _sample_size(self): return 1000

    for K, M, want in ((12, 9, [4, 4, 1]), (13, 9, [9]), (56, 20, [8, 8, 4]), (60, 9, [4, 4, 1])):
        del lib.calls[:]
        est = reg.MonteCarloConditionalExpectationRegression([RV(10 + i) for i in range(K)])
        beta = est.getLinearRegressionParameters([RV(200 + m) for m in range(M)])
        assert beta.shape == (K, M)
        symbol = "fmhip_cross_moments" if K <= 12 else "fmhip_cross_moments_wide"
        assert lib.calls == [(symbol, K, m) for m in want], (K, lib.calls)
    est = reg.MonteCarloConditionalExpectationRegression([RV(10 + i) for i in range(61)])
    assert not est._one_pass([RV(1)])                               # beyond 60 basis functions: pair by pair
    est = reg.MonteCarloConditionalExpectationRegression([RV(10 + i) for i in range(20)])
    assert est._one_pass([RV(1)])
    monkeypatch.setenv("FMHIP_DEVICE_WIDE_MOMENTS", "0")            # read per call
    assert not est._one_pass([RV(1)])
    assert reg.MonteCarloConditionalExpectationRegression([RV(10 + i) for i in range(12)])._one_pass([RV(1)])


# ------------------------------------------------------------------ the max-call driver on the CPU twin
class ArrayBrownianMotion:
    def __init__(self, td, factory, increments):
        self.td, self.factory = td, factory
        self.inc = [[factory.createRandomVariable(td.getTime(t + 1), a) for a in row] for t, row in enumerate(increments)]
    def getTimeDiscretization(self): return self.td
    def getNumberOfFactors(self): return len(self.inc[0])
    def getBrownianIncrement(self, t, f): return self.inc[t][f]
    def getRandomVariableForConstant(self, v): return self.factory.createRandomVariable(v)


def test_max_call_driver_on_the_twin(fm, oracle, monkeypatch):
    mc = import_module("finmath-lib-cuda-extensions_amd.montecarlo")
    reg = import_module("finmath-lib-cuda-extensions_amd.regression")
    n, dates = 4096, [3.0 * k / 9 for k in range(1, 10)]
    td = fm.TimeDiscretization(0.0, 9, 3.0 / 9)
    bm = ArrayBrownianMotion(td, oracle.RandomVariableFloatFactory(), oracle.bm_generate(7, [3.0 / 9] * 9, 2, n))
    sizes = []
    init = reg.MonteCarloConditionalExpectationRegression.__init__
    monkeypatch.setattr(reg.MonteCarloConditionalExpectationRegression, "__init__", lambda self, basis, *a: (sizes.append(len(basis)), init(self, basis, *a))[1])
    bermudan, error = mc.bermudan_max_call_mc(bm, [100.0, 100.0], 0.05, 0.10, 0.20, dates, 100.0, basis_order=3)
    assert sizes == [10] * 8                                        # C(2 + 3, 3) functions, one regression per date but the last
    european, _ = mc.bermudan_max_call_mc(bm, [100.0, 100.0], 0.05, 0.10, 0.20, dates[-1:], 100.0, basis_order=3)
    assert european < bermudan and 0.0 < error < 1.0
    assert [len(mc.monomial_exponents(a, d)) for a, d in ((2, 3), (3, 3), (5, 2), (5, 3))] == [10, 20, 21, 56]
    assert len(set(mc.monomial_exponents(5, 3))) == 56 and all(sum(e) <= 3 for e in mc.monomial_exponents(5, 3))
