"""Polynomial regression in one pass without a device (include/fmhip.h: fmhip_polynomial_cross_moments_host, fmhip_polynomial_evaluate_host;
DESIGN.md §4.15): the host definition is exact on small integers and is the fp32 chain written out here; the argument checks answer with
their statuses; the Python estimator with the knob off is MonteCarloConditionalExpectationRegression on the materialised basis, and its
routing is what the docstring says; the engine's side of the two passes is clean under the sanitizers on the null device — stand-alone
host programs only."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess
from importlib import import_module

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NULLDEV = os.path.join(ROOT, "tests", "nulldev")


def _lib(fm):
    return fm._native.lib()


def _ptrs(arrays):
    keep = [None if a is None else np.ascontiguousarray(a, dtype=np.float32) for a in arrays]
    return keep, (C.c_void_p * max(len(keep), 1))(*[None if a is None else a.ctypes.data for a in keep])


def host_moments(fm, states, exponents, extra=(), ys=(), n=None, n_states=None, n_terms=None):
    """(status, S upper triangle, T) of fmhip_polynomial_cross_moments_host."""
    ks, ps = _ptrs(states); kx, px = _ptrs(extra); ky, py = _ptrs(ys)
    e = np.ascontiguousarray(exponents, dtype=np.uint8)
    ns = len(states) if n_states is None else n_states
    nt = (e.size // max(len(states), 1)) if n_terms is None else n_terms
    nx = nt + len(extra)
    out = np.full(max(nx * (nx + 1) // 2 + nx * len(ys), 1), -1.0)
    rc = _lib(fm).fmhip_polynomial_cross_moments_host(ps, ks[0].size if n is None else n, ns, e.ctypes.data_as(C.POINTER(C.c_uint8)), nt, px if extra else None, len(extra),
                                                      py if ys else None, len(ys), out.ctypes.data_as(C.POINTER(C.c_double)))
    return rc, out[: nx * (nx + 1) // 2], out[nx * (nx + 1) // 2:].reshape(nx, len(ys)) if rc == 0 else None


def host_evaluate(fm, states, exponents, coefficients, extra=()):
    ks, ps = _ptrs(states); kx, px = _ptrs(extra)
    e = np.ascontiguousarray(exponents, dtype=np.uint8)
    c = np.ascontiguousarray(coefficients, dtype=np.float64)
    out = np.empty(ks[0].size, dtype=np.float32)
    rc = _lib(fm).fmhip_polynomial_evaluate_host(ps, ks[0].size, len(states), e.ctypes.data_as(C.POINTER(C.c_uint8)), e.size // len(states), px if extra else None, len(extra),
                                                 c.ctypes.data_as(C.POINTER(C.c_double)), out.ctypes.data)
    return rc, out


def f32_monomial(arrays, e):
    """The contract, in numpy float32: u^e = ((u·u)·u)…, the non-trivial powers multiplied in ascending state index."""
    t = None
    for s, es in enumerate(e):
        if not es: continue
        p = arrays[s]
        for _ in range(es - 1): p = (p * arrays[s]).astype(np.float32)
        t = p if t is None else (t * p).astype(np.float32)
    return np.ones_like(arrays[0]) if t is None else t


@pytest.mark.parametrize("n", [1, 5, 64, 1000])
def test_host_moments_are_exact_on_small_integers(fm, n):
    mc = import_module("finmath-lib-cuda-extensions_amd.montecarlo")
    rng = np.random.default_rng(2000 + n)
    a = rng.integers(-3, 4, (3, n))
    y = rng.integers(-3, 4, n)
    table = mc.monomial_exponents(3, 3)
    assert len(table) == 20
    rc, S, T = host_moments(fm, a.astype(np.float32), table, (), [y.astype(np.float32)])
    assert rc == 0
    cols = [[int(np.prod([int(a[s, p]) ** e[s] for s in range(3)])) for p in range(n)] for e in table] + [[int(v) for v in y]]       # Python integers
    at = 0
    for i in range(20):
        for j in range(i, 20):
            assert S[at] == sum(u * v for u, v in zip(cols[i], cols[j])), (i, j)
            at += 1
        assert T[i, 0] == sum(u * v for u, v in zip(cols[i], cols[20])), i
    assert S[0] == n                                                          # the all-zero tuple against itself


def test_all_zero_tuple_gives_plain_sums_and_n(fm):
    rng = np.random.default_rng(3)
    a = rng.standard_normal((2, 777)).astype(np.float32)
    rc, S, T = host_moments(fm, a, [(0, 0), (1, 0), (0, 1)], [None], [a[1]])
    assert rc == 0
    # regressors: 1, a0, a1, 1 (the NULL extra)
    full = np.zeros((4, 4)); full[np.triu_indices(4)] = S
    assert full[0, 0] == 777 == full[0, 3] == full[3, 3]
    assert full[0, 1] == float(np.sum(a[0].astype(np.float64))) or abs(full[0, 1] - math.fsum(a[0].astype(np.float64).tolist())) <= 777 * 2.0 ** -53 * float(np.abs(a[0]).sum())
    assert full[0, 1] == full[1, 3] and full[0, 2] == full[2, 3] and T[0, 0] == T[3, 0] == full[0, 2]


def test_exponent_zero_keeps_an_infinite_state_out(fm):
    a = np.array([[1.5, 2.0, -0.5, 3.0], [np.inf, 1.0, -np.inf, 2.0], [0.0, 0.0, 1.0, 2.0]], dtype=np.float32)
    rc, S, T = host_moments(fm, a, [(1, 0, 0), (2, 0, 1), (0, 1, 1)])
    assert rc == 0
    full = np.zeros((3, 3)); full[np.triu_indices(3)] = S
    assert np.isfinite(full[:2, :2]).all() and full[0, 0] == 1.5 ** 2 + 4.0 + 0.25 + 9.0          # inf⁰ met no 0
    assert np.isnan(full[2, 2]) and np.isnan(full[0, 2])                                         # inf·0 where the state does take part
    rc, r = host_evaluate(fm, a, [(1, 0, 0), (2, 0, 1)], [2.0, -1.0])
    assert rc == 0 and np.isfinite(r).all()


def test_host_evaluate_is_the_fp32_chain_bit_for_bit(fm):
    mc = import_module("finmath-lib-cuda-extensions_amd.montecarlo")
    rng = np.random.default_rng(11)
    n = 4099
    a = [np.exp(0.3 * rng.standard_normal(n)).astype(np.float32) for _ in range(4)]
    extra = [rng.standard_normal(n).astype(np.float32), None]
    table = mc.monomial_exponents(4, 3) + [(6, 0, 0, 1), (0, 5, 6, 0)]
    beta = rng.standard_normal(len(table) + 2)
    rc, got = host_evaluate(fm, a, table, beta, extra)
    assert rc == 0
    cols = [f32_monomial(a, e) for e in table] + [extra[0], np.ones(n, dtype=np.float32)]
    r = (cols[0] * np.float32(beta[0])).astype(np.float32)
    for i in range(1, len(cols)):
        r = (r + (cols[i] * np.float32(beta[i])).astype(np.float32)).astype(np.float32)
    assert np.array_equal(got.view(np.uint32), r.view(np.uint32))
    # … and the moments are those of the same fp32 monomials
    rc, S, _ = host_moments(fm, a, table[:10])
    assert rc == 0
    at = 0
    for i in range(10):
        for j in range(i, 10):
            prod = cols[i].astype(np.float64) * cols[j].astype(np.float64)
            assert abs(S[at] - math.fsum(prod.tolist())) <= n * 2.0 ** -53 * float(np.abs(prod).sum()), (i, j)
            at += 1


def test_host_argument_checks(fm):
    N = fm._native
    a = np.ones((9, 10), dtype=np.float32)
    ok = [(1, 0), (0, 1)]
    bad = N.ERR_INVALID_ARGUMENT
    assert host_moments(fm, a[:2], ok)[0] == 0
    assert host_moments(fm, a[:2], [(7, 0)])[0] == bad                                           # exponent 7
    assert host_moments(fm, a[:2], ok, n_states=0)[0] == bad
    assert host_moments(fm, a[:9], [(1,) * 9])[0] == bad                                         # nine states
    assert host_moments(fm, a[:2], [(1, 1)] * 60, [a[0]] * 3, [a[1]] * 2)[0] == bad              # 65 slots
    assert host_moments(fm, a[:2], [(1, 1)] * 60, [a[0]] * 3, [a[1]])[0] == 0                    # 64
    assert host_moments(fm, [a[0], None], ok)[0] == bad                                          # a NULL among the states
    assert host_moments(fm, a[:2], ok, (), [None])[0] == bad                                     # … among y
    assert host_moments(fm, a[:2], ok, [None])[0] == 0                                           # … among extra_x: the constant 1
    assert host_moments(fm, a[:2], ok, n=0)[0] == bad
    assert host_moments(fm, a[:2], ok, n_terms=0)[0] == bad
    lib = _lib(fm)
    e = (C.c_uint8 * 4)(1, 0, 0, 1)
    _, ps = _ptrs(a[:2])
    out = (C.c_double * 8)()
    assert lib.fmhip_polynomial_cross_moments_host(None, 10, 2, e, 2, None, 0, None, 0, out) == bad
    assert lib.fmhip_polynomial_cross_moments_host(ps, 10, 2, None, 2, None, 0, None, 0, out) == bad
    assert lib.fmhip_polynomial_cross_moments_host(ps, 10, 2, e, 2, None, 1, None, 0, out) == bad
    assert lib.fmhip_polynomial_cross_moments_host(ps, 10, 2, e, 2, None, 0, None, 1, out) == bad
    assert lib.fmhip_polynomial_cross_moments_host(ps, 10, 2, e, 2, None, 0, None, 0, None) == bad
    c = (C.c_double * 64)()
    r = np.empty(10, dtype=np.float32)
    assert lib.fmhip_polynomial_evaluate_host(ps, 10, 2, e, 2, None, 0, c, r.ctypes.data) == 0
    assert lib.fmhip_polynomial_evaluate_host(ps, 10, 2, e, 2, None, 0, None, r.ctypes.data) == bad
    assert lib.fmhip_polynomial_evaluate_host(ps, 10, 2, e, 2, None, 0, c, None) == bad
    e61 = (C.c_uint8 * 122)(*([1, 0] * 61))
    assert lib.fmhip_polynomial_evaluate_host(ps, 10, 2, e61, 61, None, 0, c, r.ctypes.data) == bad          # 60 regressors at the most


# ------------------------------------------------------------------ the Python estimator
def test_knob_off_is_the_materialised_estimator_on_the_twin(fm, oracle, monkeypatch):
    reg = import_module("finmath-lib-cuda-extensions_amd.regression")
    factory = oracle.RandomVariableFloatFactory()
    rng = np.random.default_rng(17)
    n = 2000
    states = [factory.createRandomVariable(0.0, np.exp(0.2 * rng.standard_normal(n))) for _ in range(2)]
    extra = [factory.createRandomVariable(0.0, rng.standard_normal(n))]
    ys = [factory.createRandomVariable(0.0, rng.standard_normal(n)) for _ in range(2)]
    one = factory.createRandomVariable(1.0)
    for env in ("0", "1"):                                                     # the twin's vectors are no RandomVariableHip: materialised either way
        monkeypatch.setenv("FMHIP_DEVICE_POLYNOMIAL_MOMENTS", env)
        est = reg.MonteCarloConditionalExpectationPolynomialRegression(states, order=3, extra_basis=extra, one=one)
        assert est.exponents.shape == (10, 2) and not est._one_pass(ys)
        basis = reg.monomial_basis(states, est.exponents, one) + extra
        assert basis[0] is one and len(basis) == 11
        parent = reg.MonteCarloConditionalExpectationRegression(basis)
        assert np.array_equal(est.getLinearRegressionParameters(ys), parent.getLinearRegressionParameters(ys))
        assert np.array_equal(est.getLinearRegressionParameters(ys[0]), parent.getLinearRegressionParameters(ys[0]))
        for a, b in zip(est.getConditionalExpectation(ys), parent.getConditionalExpectation(ys)):
            assert np.array_equal(np.asarray(a.getRealizations()), np.asarray(b.getRealizations()))
    # the chain of monomial_basis is the contract's: u·u, (u·u)·u, powers multiplied in ascending state index
    u, w = [np.asarray(s.getRealizations(), dtype=np.float32) for s in states]
    got = np.asarray(reg.monomial_basis(states, [(3, 2)], one)[0].getRealizations(), dtype=np.float32)
    want = ((((u * u).astype(np.float32) * u).astype(np.float32)) * (w * w).astype(np.float32)).astype(np.float32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


class _Recorder:
    """Stands in for the native library: records the two polynomial calls and answers S = n on the diagonal, T = 0, and a fresh handle."""
    def __init__(self): self.calls = []
    def fmhip_polynomial_cross_moments(self, hs, n_states, e, n_terms, hx, n_extra, hy, n_y, out):
        self.calls.append(("moments", n_states, n_terms, n_extra, n_y))
        n_x, at = n_terms + n_extra, 0
        for i in range(n_x):
            for j in range(i, n_x): out[at] = 1000.0 if i == j else 0.0; at += 1
        for k in range(n_x * n_y): out[at + k] = 0.0
        return 0
    def fmhip_polynomial_evaluate(self, hs, n_states, e, n_terms, hx, n_extra, c, out):
        self.calls.append(("evaluate", n_states, n_terms, n_extra))
        C.cast(out, C.POINTER(C.c_int64))[0] = 4242
        return 0


class _Vec:
    def __init__(self, handle): self.handle, self.n = handle, 1000


def test_routing_of_the_estimator(fm, monkeypatch):
    reg = import_module("finmath-lib-cuda-extensions_amd.regression")
    lib = _Recorder()
    monkeypatch.setattr(reg.N, "lib", lambda: lib)
    monkeypatch.setattr(fm.DeviceVector, "__del__", lambda self: None, raising=False)

    class RV(fm.RandomVariableHip):                                 # a stochastic RandomVariableHip without a device behind it
        def __init__(self, handle): self.realizations, self.time = _Vec(handle), 0.0
        def isDeterministic(self): return False
        def _sample_size(self): return 1000

    monkeypatch.delenv("FMHIP_DEVICE_POLYNOMIAL_MOMENTS", raising=False)
    states = [RV(10 + i) for i in range(5)]
    est = reg.MonteCarloConditionalExpectationPolynomialRegression(states, order=3)              # K = 56
    beta = est.getLinearRegressionParameters([RV(200 + m) for m in range(20)])
    assert beta.shape == (56, 20)
    assert lib.calls == [("moments", 5, 56, 0, 8), ("moments", 5, 56, 0, 8), ("moments", 5, 56, 0, 4)]      # dependents in chunks of 64 − K
    del lib.calls[:]
    est = reg.MonteCarloConditionalExpectationPolynomialRegression(states[:2], order=2, extra_basis=[RV(50)])
    ce = est.getConditionalExpectation(RV(200))
    assert lib.calls == [("moments", 2, 6, 1, 1), ("evaluate", 2, 6, 1)] and ce.realizations.handle == 4242
    # K <= 60, the knob, every operand a stochastic RandomVariableHip
    assert not reg.MonteCarloConditionalExpectationPolynomialRegression(states, order=3, extra_basis=[RV(60 + i) for i in range(5)])._one_pass([RV(1)])
    assert reg.MonteCarloConditionalExpectationPolynomialRegression(states, order=3, extra_basis=[RV(60 + i) for i in range(4)])._one_pass([RV(1)])
    assert not est._one_pass([fm.RandomVariableHip(0.0, 2.0)])
    assert not reg.MonteCarloConditionalExpectationPolynomialRegression(states[:2], order=2, extra_basis=[fm.RandomVariableHip(0.0, 1.0)])._one_pass([RV(1)])
    assert not reg.MonteCarloConditionalExpectationPolynomialRegression(states[:1], exponents=[(7,)])._one_pass([RV(1)])
    assert est._one_pass([RV(1)])
    monkeypatch.setenv("FMHIP_DEVICE_POLYNOMIAL_MOMENTS", "0")      # read per call
    assert not est._one_pass([RV(1)])


# ------------------------------------------------------------------ the engine's side on the null device: stand-alone host programs
@pytest.fixture(scope="module")
def built():
    if not shutil.which("g++") or not os.path.exists("/opt/rocm/include/hip/hip_runtime_api.h"):
        pytest.skip("needs g++ and the HIP headers")
    r = subprocess.run(["make", "-C", NULLDEV, "-f", "poly.mk", "-j8", "xmom_poly_asan", "xmom_poly_tsan", "xmom_poly_absent_asan"], capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return os.path.join(NULLDEV, "build")


def _env(tmp_path, env):
    return dict(os.environ, FMHIP_JIT_CACHE_DIR=str(tmp_path / "code_objects"), FMHIP_JIT_PACK_DIR="off", FMHIP_RING_BYTES="16384", FMHIP_ARENA_BYTES="4096",
                ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1", TSAN_OPTIONS="halt_on_error=1", **env)


@pytest.mark.parametrize("env", [{}, {"FMNULL_DEVICES": "2"}, {"FMNULL_DEVICES": "3"}, {"FMNULL_THREAD_ENGINES": "1"}])
def test_engine_passes_are_clean_under_the_sanitizers(built, tmp_path, env):
    """drive_xmom_poly: 1 … 8 states, 1 … 64 slots, stored and pending operands, the constant 1 as a tuple and as an extra vector, a second
    thread releasing the inputs of pending operands during the call, the evaluation read back, every argument error with its status from the
    device entry points — on one engine, behind 2 and 3 shards, with thread engines."""
    full = _env(tmp_path, env)
    a = subprocess.run([os.path.join(built, "drive_xmom_poly_asan")], capture_output=True, text=True, timeout=600, env=full)
    assert a.returncode == 0 and "Sanitizer" not in a.stderr and "runtime error" not in a.stderr, a.stdout[-500:] + a.stderr[-6000:]
    assert a.stdout.count("xmom poly done") == 2
    t = subprocess.run([os.path.join(built, "drive_xmom_poly_tsan")], capture_output=True, text=True, timeout=600, env=full)
    assert t.returncode == 0 and "ThreadSanitizer" not in t.stderr, t.stdout[-500:] + t.stderr[-6000:]
    assert t.stdout.count("xmom poly done") == 2


@pytest.mark.parametrize("env", [{}, {"FMNULL_DEVICES": "2"}, {"FMNULL_DEVICES": "3"}, {"FMNULL_THREAD_ENGINES": "1"}])
def test_a_build_without_the_kernels_answers_unsupported(built, tmp_path, env):
    a = subprocess.run([os.path.join(built, "drive_xmom_poly_absent_asan")], capture_output=True, text=True, timeout=600, env=_env(tmp_path, env))
    assert a.returncode == 0 and "Sanitizer" not in a.stderr and "runtime error" not in a.stderr, a.stdout[-500:] + a.stderr[-6000:]
    assert a.stdout.count("xmom poly absent done") == 2


def test_a_failing_allocation_inside_a_polynomial_evaluation_leaves_nothing_behind(built, tmp_path):
    """One fmhip_polynomial_evaluate takes ONE buffer from the pool, its output.  The hook FMHIP_TEST_FAIL_ALLOC_AT is set on it (its position
    from a counting run), and once where nothing reaches it: the call answers FMHIP_OK or FMHIP_ERR_OUT_OF_MEMORY, a result it gives is the
    definition's, a failed call leaves its handle as it was, live vectors and bytes in use are what they were, the same call succeeds
    afterwards (the driver checks all of it), and the process ends without a leak."""
    exe = os.path.join(built, "drive_xmom_poly_asan")
    env = dict(os.environ, FMHIP_JIT_CACHE_DIR=str(tmp_path / "code_objects"), FMHIP_JIT_PACK_DIR="off", FMHIP_RING_BYTES="16384", FMHIP_ARENA_BYTES="4096",
               ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    counting = subprocess.run([exe, "failure"], capture_output=True, text=True, timeout=600, env=env)
    assert counting.returncode == 0 and "Sanitizer" not in counting.stderr, counting.stdout[-500:] + counting.stderr[-6000:]
    before, inside, status = map(int, re.search(r"failure: (\d+) allocations before the call, (\d+) in it, status (-?\d+)", counting.stdout).groups())
    assert inside == 1 and status == 0
    for at in list(range(before + 1, before + inside + 1)) + [10**9]:
        r = subprocess.run([exe, "failure"], capture_output=True, text=True, timeout=600, env=dict(env, FMHIP_TEST_FAIL_ALLOC_AT=str(at)))
        assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr and r.stderr == "", (at, r.stdout[-500:] + r.stderr[-6000:])
        assert "failure done" in r.stdout
        failed = int(re.search(r"status (-?\d+)", r.stdout).group(1)) != 0
        assert failed == (at <= before + inside), (at, r.stdout)
