"""Nested simulation without a GPU (include/fmhip.h: fmhip_block_moments_host; host/block_moments.hpp): the DEFINITION of
the block moments — S1 and S2 in one association that is a function of the block length alone — against numpy for EQUALITY on dyadic data
(every order gives the same bits there), against math.fsum within the published bound on wide-range data, for its independence of where a
block sits, and at its edges; the host half in a stand-alone program under AddressSanitizer / UBSan (tests/cpp/test_block_moments_host.cpp);
the engine's side of the two calls (csrc/nested_engine.hpp, the fronts of csrc/sharded.cpp and csrc/abi.cpp) on the test-only null device
under AddressSanitizer + UBSan and ThreadSanitizer (tests/nulldev/nested.mk: drive_nested.cpp with the stand-in launchers of
null_nested.cpp, drive_nested_absent.cpp without them).  Stand-alone programs only: nothing sanitized is loaded into this process.
And a numpy restatement of montecarlo.bermudan_option_bounds_mc: the reference of the acceptance numbers of tests/test_gpu_nested.py."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NULLDEV = os.path.join(ROOT, "tests", "nulldev")

SEGMENT, LEAVES, SMALL = 2048, 64, 64
# the issue's list, and every regime boundary of the implementation (64 | 65: small | medium; 2048 | 2049: medium | large) with its neighbours
BLOCKS = sorted({1, 2, 3, 7, 63, 64, 65, 66, 100, 511, 512, 513, 2047, 2048, 2049, 2050, 4097})


def chain(block):
    """fm_block_chain of host/block_moments.hpp, restated: the longest chain of additions behind a block's sum."""
    c = -(-min(block, SEGMENT) // LEAVES) - 1 + 6
    if block > SEGMENT: c += -(-(-(-block // SEGMENT)) // LEAVES) - 1 + 6
    return c


def test_the_constants_are_the_headers():
    text = open(os.path.join(ROOT, "finmath-lib-cuda-extensions_amd", "host", "block_moments.hpp")).read()
    assert int(re.search(r"FM_BLOCK_SEGMENT = (\d+)", text).group(1)) == SEGMENT and int(re.search(r"FM_BLOCK_LEAVES = (\d+)", text).group(1)) == LEAVES
    kernel = open(os.path.join(ROOT, "finmath-lib-cuda-extensions_amd", "csrc", "nested_kernel.h")).read()
    assert int(re.search(r"FM_NESTED_SMALL = (\d+)", kernel).group(1)) == SMALL
    assert {SMALL, SMALL + 1, SEGMENT, SEGMENT + 1} <= set(BLOCKS)


def wide_range(n, rng):
    """Signed magnitudes over sixteen decades: without them every fp64 sum of fp32 data of one scale is exact, and a wrong tree passes."""
    a = (10.0 ** rng.uniform(-8.0, 8.0, n)).astype(np.float32)
    return (a * np.where(rng.random(n) < 0.5, -1.0, 1.0)).astype(np.float32)


def dyadic(n, rng):
    """Integers in ±2^10: sums of up to 2^31 of them and of their squares are exact in fp64 in every order."""
    return rng.integers(-(1 << 10), (1 << 10) + 1, n).astype(np.float32)


def same_f32(a, b):
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def shape(block):
    return min(5, max(1, (1 << 16) // block))


@pytest.mark.parametrize("block", BLOCKS)
def test_on_dyadic_data_the_definition_equals_numpy(fm, block):
    m = shape(block)
    a = dyadic(m * block, np.random.default_rng(block))
    s, mean, var = fm.block_moments_host(a, block, ("sum", "mean", "variance"))
    a64 = a.astype(np.float64).reshape(m, block)
    s1, s2 = a64.sum(axis=1), (a64 * a64).sum(axis=1)
    assert same_f32(s, s1.astype(np.float32)) and same_f32(mean, (s1 / block).astype(np.float32))
    assert same_f32(var, np.maximum(0.0, s2 / block - (s1 / block) * (s1 / block)).astype(np.float32))
    # every mask gives the same columns, in ascending bit order whatever the order of the names
    for names in (("variance", "sum"), ("mean",), ("variance",), ("mean", "sum")):
        got = fm.block_moments_host(a, block, names)
        for name, column in zip(names, got): assert same_f32(column, {"sum": s, "mean": mean, "variance": var}[name]), names


@pytest.mark.parametrize("block", BLOCKS + [3 * SEGMENT + 5, 65 * SEGMENT + 1])
def test_the_definition_is_within_its_bound_of_the_exact_sum(fm, block):
    m = 3 if block < 10000 else 1
    a = wide_range(m * block, np.random.default_rng(block + 1))
    # the fp64 sums themselves are not exported (the stand-alone program of test_host_half_under_the_sanitizers holds them to the bound in
    # fp64): here the fp32 sum is the rounding of a value within the bound of fsum
    s, = fm.block_moments_host(a, block, ("sum",))
    a64 = a.astype(np.float64).reshape(m, block)
    for q in range(m):
        exact, mass = math.fsum(a64[q]), math.fsum(np.abs(a64[q]))
        slack = (chain(block) + 1) * 2.0 ** -53 * mass
        lo, hi = np.float32(exact - slack), np.float32(exact + slack)
        assert min(lo, hi) <= s[q] <= max(lo, hi), (block, q, s[q], exact, slack)


@pytest.mark.parametrize("block", BLOCKS)
def test_a_blocks_moments_do_not_depend_on_where_it_sits(fm, block):
    rng = np.random.default_rng(block + 2)
    one = wide_range(block, rng)
    alone = fm.block_moments_host(one, block, ("sum", "mean", "variance"))                       # m = 1
    for m, q in ((2, 1), (3, 0), (5, 3)):
        a = wide_range(m * block, rng)
        a[q * block:(q + 1) * block] = one
        got = fm.block_moments_host(a, block, ("sum", "mean", "variance"))
        for j in range(3): assert same_f32(got[j][q:q + 1], alone[j]), (block, m, q, j)


def test_edges_of_the_definition(fm):
    rng = np.random.default_rng(7)
    v = wide_range(1000, rng)
    mean, var = fm.block_moments_host(v, 1, ("mean", "variance"))
    assert same_f32(mean, v) and (var == 0).all()
    s, mean = fm.block_moments_host(v, 1000, ("sum", "mean"))                                    # block = n
    assert s.size == 1 and abs(float(s[0]) - math.fsum(v.astype(np.float64))) <= np.spacing(np.float32(abs(s[0]))) and mean.size == 1
    for block in (4, 100, 250):
        a = wide_range(1000, rng)
        clean = fm.block_moments_host(a, block, ("sum", "mean", "variance"))
        for bad, where in ((np.nan, 1), (np.inf, 2), (-np.inf, 0)):
            b = a.copy(); b[where * block + block // 2] = bad
            got = fm.block_moments_host(b, block, ("sum", "mean", "variance"))
            for j in range(3):
                others = np.arange(1000 // block) != where
                assert same_f32(got[j][others], clean[j][others])                               # the other blocks are untouched
            if np.isnan(bad): assert all(np.isnan(got[j][where]) for j in range(3))
            else: assert got[0][where] == bad and got[1][where] == bad and np.isnan(got[2][where])
    zeros = np.full(6, -0.0, dtype=np.float32)
    s, var = fm.block_moments_host(zeros, 3, ("sum", "variance"))
    assert np.signbit(s).all() and not np.signbit(var).any()


def test_the_definition_refuses_on_the_host(fm):
    lib, bad = fm.lib(), fm._native.ERR_INVALID_ARGUMENT
    a = np.zeros(12, dtype=np.float32); out = np.zeros(36, dtype=np.float32)
    pa, po = a.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    assert lib.fmhip_block_moments_host(pa, 12, 3, 7, po) == 0
    for n, block, mask, x, o in ((12, 3, 0, pa, po), (12, 3, 8, pa, po), (12, 0, 1, pa, po), (12, -1, 1, pa, po), (12, 5, 1, pa, po), (12, 24, 1, pa, po),
                                 (0, 1, 1, pa, po), (12, 3, 1, None, po), (12, 3, 1, pa, None)):
        assert lib.fmhip_block_moments_host(x, n, block, mask, o) == bad, (n, block, mask)
    with pytest.raises(ValueError): fm.block_moments_host(a, 3, ())
    with pytest.raises(ValueError): fm.block_moments_host(a, 3, ("mean", "mean"))
    with pytest.raises(ValueError): fm.block_moments_host(a, 3, ("median",))
    with pytest.raises(fm.FmhipError): fm.block_moments_host(a, 5)
    if not lib.fmhip_is_initialized():
        h = (C.c_int64 * 3)(); one = (C.c_int64 * 1)(1); r = C.c_int64(0)
        assert lib.fmhip_block_moments(one, 1, 3, 7, h) == fm._native.ERR_NOT_INITIALIZED
        assert lib.fmhip_vec_repeat(1, 2, 2, C.byref(r)) == fm._native.ERR_NOT_INITIALIZED


def test_the_knob_is_read_per_call(fm, monkeypatch):
    monkeypatch.delenv("FMHIP_DEVICE_NESTED", raising=False)
    assert fm.device_nested()
    monkeypatch.setenv("FMHIP_DEVICE_NESTED", "0")
    assert not fm.device_nested()
    monkeypatch.setenv("FMHIP_DEVICE_NESTED", "1")
    assert fm.device_nested()


def test_deterministic_variables_stay_deterministic(fm):
    c = fm.RandomVariableHip(1.5, 0.25)
    (s, mean, var), = fm.block_moments([c], 8, ("sum", "mean", "variance"))
    assert mean.isDeterministic() and mean.doubleValue() == 0.25 and s.doubleValue() == 2.0 and var.doubleValue() == 0.0 and mean.getFiltrationTime() == 1.5
    assert fm.block_means(c, 3).doubleValue() == 0.25
    for r in (fm.repeat_each(c, 5), fm.tile(c, 5)): assert r.isDeterministic() and r.doubleValue() == 0.25 and r.getFiltrationTime() == 1.5
    with pytest.raises(TypeError): fm.block_means(np.zeros(4), 2)
    with pytest.raises(ValueError): fm.block_means(c, 0)
    with pytest.raises(ValueError): fm.repeat_each(c, 0)


def test_host_half_under_the_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("needs g++")
    exe = tmp_path / "block_moments_host"
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-ffp-contract=off",
                        os.path.join(ROOT, "tests", "cpp", "test_block_moments_host.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "block moments host ok" in r.stdout and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stdout[-1500:] + r.stderr[-3000:]


def test_the_kernels_are_in_the_library(fm):
    """A missing kernel is an error, never a fallback: the launchers are weak references, so the library must be shown to hold them."""
    out = subprocess.check_output(["nm", "-D", "--defined-only", fm._native.LIB_PATH], text=True) + subprocess.check_output(["nm", "--defined-only", fm._native.LIB_PATH], text=True, stderr=subprocess.DEVNULL)
    for name in ("launch_block_moments", "launch_repeat", "launch_sort_done"):
        assert name in out, name
    blob = open(fm._native.LIB_PATH, "rb").read()
    for kernel in (b"fm_block_moments_kernel", b"fm_block_combine_kernel", b"fm_repeat_kernel"):
        assert kernel in blob, kernel


# ---------------------------------------------------------------- the engine's side on the null device
@pytest.fixture(scope="module")
def built():
    if not shutil.which("g++") or not os.path.exists("/opt/rocm/include/hip/hip_runtime_api.h"):
        pytest.skip("needs g++ and the HIP headers")
    r = subprocess.run(["make", "-C", NULLDEV, "-f", "nested.mk", "-j8", "nested_asan", "nested_tsan", "nested_absent_asan"], capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return os.path.join(NULLDEV, "build")


def _env(tmp_path, env):
    return dict(os.environ, FMHIP_JIT_CACHE_DIR=str(tmp_path / "code_objects"), FMHIP_JIT_PACK_DIR="off", FMHIP_RING_BYTES="16384", FMHIP_ARENA_BYTES="4096",
                ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1", TSAN_OPTIONS="halt_on_error=1", **env)


@pytest.mark.parametrize("env", [{}, {"FMNULL_DEVICES": "2"}, {"FMNULL_DEVICES": "3"}, {"FMNULL_THREAD_ENGINES": "1"}])
def test_engine_pass_is_clean_under_the_sanitizers(built, tmp_path, env):
    """drive_nested: both calls on vectors of real data, blocks of the three regimes and around their boundaries and small again behind
    the large ones, every mask, one and four vectors per call, repeats with NaN payloads and -0.0, checked against the definition;
    pending operands, a second thread releasing the inputs of pending operands during the call, every argument error — on one engine and
    behind a device list of one shard, behind 2 and 3 shards (FMHIP_ERR_UNSUPPORTED, nothing left behind), with thread engines (a caller
    that does not own the vectors)."""
    full = _env(tmp_path, env)
    a = subprocess.run([os.path.join(built, "drive_nested_asan")], capture_output=True, text=True, timeout=600, env=full)
    assert a.returncode == 0 and "Sanitizer" not in a.stderr and "runtime error" not in a.stderr, a.stdout[-500:] + a.stderr[-6000:]
    assert a.stdout.count("nested done") == 2 and a.stderr == ""
    assert ("a device list of one shard: checked" in a.stdout) == (not env)
    t = subprocess.run([os.path.join(built, "drive_nested_tsan")], capture_output=True, text=True, timeout=600, env=full)
    assert t.returncode == 0 and "ThreadSanitizer" not in t.stderr, t.stdout[-500:] + t.stderr[-6000:]
    assert t.stdout.count("nested done") == 2 and t.stderr == ""


def test_a_failing_allocation_inside_a_block_moments_pass_leaves_nothing_behind(built, tmp_path):
    """One fmhip_block_moments of two vectors and three outputs takes SIX buffers from the pool, its outputs.  The hook
    FMHIP_TEST_FAIL_ALLOC_AT is set on each of them (their positions from a counting run), and once where nothing reaches it: the call
    answers FMHIP_OK or FMHIP_ERR_OUT_OF_MEMORY, a result it gives is right, outputs of a failed call are not written, live vectors and bytes
    in use are what they were, the same call succeeds afterwards (the driver checks all of it), and the process ends without a leak."""
    exe = os.path.join(built, "drive_nested_asan")
    counting = subprocess.run([exe, "failure"], capture_output=True, text=True, timeout=600, env=_env(tmp_path, {}))
    assert counting.returncode == 0 and "Sanitizer" not in counting.stderr, counting.stdout[-500:] + counting.stderr[-6000:]
    before, inside, status = map(int, re.search(r"failure: (\d+) allocations before the call, (\d+) in it, status (-?\d+)", counting.stdout).groups())
    assert inside == 6 and status == 0
    for at in list(range(before + 1, before + inside + 1)) + [10**9]:
        r = subprocess.run([exe, "failure"], capture_output=True, text=True, timeout=600, env=_env(tmp_path, {"FMHIP_TEST_FAIL_ALLOC_AT": str(at)}))
        assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr and r.stderr == "", (at, r.stdout[-500:] + r.stderr[-6000:])
        assert "failure done" in r.stdout
        failed = int(re.search(r"status (-?\d+)", r.stdout).group(1)) != 0
        assert failed == (at <= before + inside), (at, r.stdout)


@pytest.mark.parametrize("env", [{}, {"FMNULL_DEVICES": "2"}, {"FMNULL_THREAD_ENGINES": "1"}])
def test_a_build_without_the_kernel_answers_unsupported(built, tmp_path, env):
    a = subprocess.run([os.path.join(built, "drive_nested_absent_asan")], capture_output=True, text=True, timeout=600, env=_env(tmp_path, env))
    assert a.returncode == 0 and "Sanitizer" not in a.stderr and "runtime error" not in a.stderr, a.stdout[-500:] + a.stderr[-6000:]
    assert a.stdout.count("nested absent done") == 2


# ---------------------------------------------------------------- the driver, restated in numpy
S0, R, SIGMA, T, K = 1.0, 0.05, 0.30, 2.0, 1.05                      # the constants of tests/test_gpu_regression.py
DATES = [0.2 * k for k in range(1, 11)]
TREE = 0.153540                                                      # crr_bermudan_put(DATES) of tests/test_gpu_regression.py
FIT_PATHS, OUTER_PATHS = 1 << 16, 4096
SEED_FIT, SEED_OUTER, SEED_INNER = 31415, 27182, 1000                # the seeds of the acceptance test (tests/test_gpu_nested.py)


def european_put():
    d1 = (math.log(S0 / K) + (R + 0.5 * SIGMA ** 2) * T) / (SIGMA * math.sqrt(T)); d2 = d1 - SIGMA * math.sqrt(T)
    cdf = lambda z: 0.5 * (1.0 + math.erf(z / math.sqrt(2.0)))
    return K * math.exp(-R * T) * cdf(-d2) - S0 * cdf(-d1)


def bounds_numpy(seed_fit, seed_outer, inner_seed, inner_paths, fit_paths=FIT_PATHS, outer_paths=OUTER_PATHS, basis_order=3):
    """montecarlo.bermudan_option_bounds_mc in float64 numpy, step for step: the policy from the fit sample, the lower bound on the outer
    sample, the martingale of the upper bound from inner simulations at the root and at every date but the last."""
    dt, J = DATES[0], len(DATES)
    drift = (R - 0.5 * SIGMA ** 2) * dt

    def advance(x, rng, steps):
        out = []
        for _ in range(steps):
            x = x + drift + SIGMA * math.sqrt(dt) * rng.standard_normal(x.size)
            out.append(np.exp(x))
        return out, x

    h = lambda s, j: np.maximum(K - s, 0.0) * math.exp(-R * DATES[j])
    basis = lambda s: np.vander(s, basis_order + 1, increasing=True)

    def policy_value(states, first):
        value = h(states[-1], J - 1)
        for k in range(J - 2, first - 1, -1):
            e = h(states[k - first], k)
            value = np.where(e - basis(states[k - first]) @ betas[k] >= 0.0, e, value)
        return value

    fit, _ = advance(np.full(fit_paths, math.log(S0)), np.random.default_rng(seed_fit), J)
    betas = [None] * J
    value = h(fit[-1], J - 1)
    for k in range(J - 2, -1, -1):
        A = basis(fit[k])
        betas[k] = np.linalg.solve(A.T @ A, A.T @ value)
        e = h(fit[k], k)
        value = np.where(e - A @ betas[k] >= 0.0, e, value)

    rng = np.random.default_rng(seed_outer)
    outer, xs = [], []
    x = np.full(outer_paths, math.log(S0))
    for _ in range(J):
        (s,), x = advance(x, rng, 1)
        outer.append(s); xs.append(x)
    lower = policy_value(outer, 0)

    previous_c, martingale, worst = None, 0.0, None
    for j in range(-1, J):
        c = None
        if j < J - 1:
            start = np.full(outer_paths * inner_paths, math.log(S0)) if j < 0 else np.repeat(xs[j], inner_paths)
            inner, _ = advance(start, np.random.default_rng(inner_seed + j + 1), J - 1 - j)
            c = policy_value(inner, j + 1).reshape(outer_paths, inner_paths).mean(axis=1)
        if j >= 0:
            e = h(outer[j], j)
            v = e if c is None else np.where(e - basis(outer[j]) @ betas[j] >= 0.0, e, c)
            martingale = martingale + v - previous_c
            worst = e - martingale if worst is None else np.maximum(worst, e - martingale)
        previous_c = c
    se = lambda a: float(a.std() / math.sqrt(a.size))
    return dict(lower=float(lower.mean()), lower_se=se(lower), upper=float(worst.mean()), upper_se=se(worst))


def check_bounds(at64, at16):
    """The conditions of the issue on a pair of runs with 64 and 16 inner paths."""
    print("bounds, 64 inner paths:", at64, "16 inner paths:", at16)
    assert at64["lower"] - 3 * at64["lower_se"] <= TREE <= at64["upper"] + 3 * at64["upper_se"]
    assert at16["lower"] - 3 * at16["lower_se"] <= TREE <= at16["upper"] + 3 * at16["upper_se"]
    assert at64["upper"] < at16["upper"]                             # the inner noise biases the bound upwards
    assert at64["upper"] - TREE <= 0.010
    assert at64["lower"] >= european_put() - 3 * at64["lower_se"]


def test_the_restated_driver_satisfies_the_acceptance_conditions_at_the_tests_seeds():
    check_bounds(bounds_numpy(SEED_FIT, SEED_OUTER, SEED_INNER, 64), bounds_numpy(SEED_FIT, SEED_OUTER, SEED_INNER, 16))
