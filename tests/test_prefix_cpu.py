"""The device prefix sums without a GPU (include/fmhip.h: fmhip_prefix_sums_host; csrc/prefix_host.hpp): the DEFINITION —
P[r] in one tree that is a function of n and r alone — against math.fsum within the published bound, against numpy's float64 cumsum for
EQUALITY on dyadic data (every order gives the same bits there), for monotonicity on wide-range weights, and at its edges (a leading -0.0,
a NaN at each kind of boundary, +inf followed by -inf); the host half of the kernels (chunk arithmetic, a model of the three kernels) in
a stand-alone program under AddressSanitizer / UBSan (tests/cpp/test_prefix_host.cpp); and the engine's side of the three calls
(csrc/prefix_engine.hpp, the fronts of csrc/sharded.cpp and csrc/abi.cpp) on the test-only null device under AddressSanitizer + UBSan and
ThreadSanitizer (tests/nulldev/prefix.mk: drive_prefix.cpp with the stand-in launchers of null_prefix.cpp, drive_prefix_absent.cpp without
them).  Stand-alone programs only: nothing sanitized is loaded into this process."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from test_sort_cpu import inputs as sort_inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NULLDEV = os.path.join(ROOT, "tests", "nulldev")


def header_constants():
    text = open(os.path.join(ROOT, "finmath-lib-cuda-extensions_amd", "csrc", "prefix_host.hpp")).read()
    env = {}
    for name, expr in re.findall(r"constexpr int (FM_PREFIX_\w+) = ([^;,]+)[;,]", text):
        env[name] = int(eval(expr, {"__builtins__": {}}, env))
    return env


K = header_constants()
ITEMS, GROUP, GROUPS, WAVES, TILE = K["FM_PREFIX_ITEMS"], K["FM_PREFIX_GROUP"], K["FM_PREFIX_GROUPS"], K["FM_PREFIX_WAVES"], K["FM_PREFIX_TILE"]
WAVE = K["FM_PREFIX_WAVE_ELEMS"]
assert GROUP * GROUPS == 64 and WAVE == 64 * ITEMS and TILE == WAVES * WAVE == K["FM_PREFIX_BLOCK"] * ITEMS


def chunk_tiles(n):
    return max(K["FM_PREFIX_MIN_CHUNK_TILES"], -(-(-(-n // TILE)) // K["FM_PREFIX_MAX_BLOCKS"]))


def blocks(n):
    return -(-(-(-n // TILE)) // chunk_tiles(n))


def chain(n):
    """prefix_chain(n) of prefix_host.hpp: the longest chain of additions behind any P[r]."""
    return (ITEMS - 1) + (GROUP - 1) + (GROUPS - 1) + (WAVES - 1) + (chunk_tiles(n) - 1) + (blocks(n) - 1)


def wide_range(n, rng, signed=False):
    """Magnitudes over sixteen decades, 1e-8 … 1e8: without them every fp64 sum of fp32 data of one scale is exact, and a wrong tree passes."""
    a = (10.0 ** rng.uniform(-8.0, 8.0, n)).astype(np.float32)
    return (a * np.where(rng.random(n) < 0.5, -1.0, 1.0)).astype(np.float32) if signed else a


def dyadic(n, rng):
    """Integers below 2^12 times 2^-30: every order of summation gives the same bits (n · 2^12 < 2^53)."""
    return (rng.integers(0, 1 << 12, n).astype(np.float64) * 2.0 ** -30).astype(np.float32)


def inputs(n, rng):
    """The sort tests' families, and the two that tell one tree from another."""
    yield from sort_inputs(n, rng)
    yield "wide range", wide_range(n, rng)
    yield "wide range, signed", wide_range(n, rng, signed=True)
    yield "dyadic", dyadic(n, rng)
    yield "half zeros, wide range", (wide_range(n, rng) * (rng.random(n) < 0.5)).astype(np.float32)


def definition(fm, a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    out = np.full(a.size, -1.0, dtype=np.float64)
    st = fm.lib().fmhip_prefix_sums_host(a.ctypes.data_as(C.c_void_p), a.size, out.ctypes.data_as(C.POINTER(C.c_double)))
    assert st == 0, fm.lib().fmhip_last_error()
    return out


def same_f64(a, b):
    """Bit for bit; of a NaN only that it is one."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))).all())


SIZES = [1, 2, ITEMS - 1, ITEMS, ITEMS + 1, 63, 64, 65, WAVE - 1, WAVE, WAVE + 1, TILE - 1, TILE, TILE + 1, 2 * TILE + 1, 4 * TILE + 77, 100_003]


@pytest.mark.parametrize("n", SIZES)
def test_the_definition_is_within_its_bound_of_the_exact_sum(fm, n):
    rng = np.random.default_rng(n)
    bound = (chain(n) + 1) * 2.0 ** -53
    for name, a in inputs(n, rng):
        p = definition(fm, a)
        with np.errstate(invalid="ignore"):
            a64 = a.astype(np.float64)
        finite = np.isfinite(a64)
        upto = n if finite.all() else int(np.argmin(finite))                   # the prefixes before the first inf or NaN
        mass = np.cumsum(np.abs(a64[:upto]))
        for r in sorted({0, upto - 1, upto // 2, upto // 3, min(upto - 1, TILE), min(upto - 1, TILE - 1)} | set(rng.integers(0, max(upto, 1), 8).tolist())):
            if not 0 <= r < upto: continue
            exact = math.fsum(a64[:r + 1])
            assert abs(p[r] - exact) <= bound * mass[r] * (1 + 2.0 ** -30), (name, n, r, p[r], exact)
        if upto < n and not np.isnan(a[upto]) and not np.isinf(a[upto + 1:]).any() and not np.isnan(a[upto + 1:]).any():
            assert (p[upto:] == a64[upto]).all(), (name, n)                      # one infinity, nothing against it
        if name == "all NaN": assert np.isnan(p).all()


@pytest.mark.parametrize("n", SIZES)
def test_on_dyadic_data_the_definition_equals_numpys_cumsum(fm, n):
    a = dyadic(n, np.random.default_rng(n + 1))
    assert (definition(fm, a) == np.cumsum(a, dtype=np.float64)).all()
    i = np.random.default_rng(n).integers(-40, 40, n).astype(np.float32)          # signed integers
    assert (definition(fm, i) == np.cumsum(i, dtype=np.float64)).all()


@pytest.mark.parametrize("n", [WAVE + 1, TILE + 1, 4 * TILE + 77, 100_003])
def test_the_definition_is_monotone_on_wide_range_weights(fm, n):
    """A cumulative weight is a CDF.  (A Kogge–Stone association breaks this on most such vectors.)"""
    for seed in range(8):
        rng = np.random.default_rng(1000 * seed + n)
        w = wide_range(n, rng)
        if seed % 2: w[rng.random(n) < 0.5] = 0.0
        assert (np.diff(definition(fm, w)) >= 0).all(), (n, seed)


def test_edges_of_the_definition(fm):
    n = 4 * TILE + 9
    z = np.zeros(n, dtype=np.float32); z[:3] = -0.0
    p = definition(fm, z)
    assert np.signbit(p[:3]).all() and not np.signbit(p[3:]).any() and (p == 0).all()       # a leading -0.0 stays -0.0: it is not added to 0
    assert np.signbit(definition(fm, np.full(n, -0.0, dtype=np.float32))).all()
    base = np.random.default_rng(4).random(n, dtype=np.float32)
    for at in (0, ITEMS - 1, ITEMS, 63, 64, WAVE - 1, WAVE, TILE - 1, TILE, 2 * TILE - 1, 2 * TILE, 4 * TILE, n - 1):      # each kind of boundary
        a = base.copy(); a[at] = np.nan
        p = definition(fm, a)
        assert (np.isnan(p) == (np.arange(n) >= at)).all(), at
        assert same_f64(p[:at], definition(fm, base)[:at])
        if at + 1 < n:
            a[at] = np.inf; a[at + 1] = -np.inf
            p = definition(fm, a)
            assert p[at] == np.inf and np.isnan(p[at + 1:]).all() and np.isfinite(p[:at]).all(), at


def test_the_definition_refuses_on_the_host(fm):
    lib = fm.lib()
    a = np.ones(4, dtype=np.float32)
    out = np.zeros(4, dtype=np.float64)
    po = out.ctypes.data_as(C.POINTER(C.c_double))
    bad = fm._native.ERR_INVALID_ARGUMENT
    assert lib.fmhip_prefix_sums_host(None, 4, po) == bad
    assert lib.fmhip_prefix_sums_host(a.ctypes.data_as(C.c_void_p), 4, None) == bad
    assert lib.fmhip_prefix_sums_host(a.ctypes.data_as(C.c_void_p), 0, po) == bad
    assert lib.fmhip_prefix_sums_host(a.ctypes.data_as(C.c_void_p), 1 << 31, po) == bad
    assert (fm.prefix_sums_host([1.0, 2.0, 3.5]) == [1.0, 3.0, 6.5]).all()
    # the device calls need an engine: without one they say so, they do not scan on the host
    if not lib.fmhip_is_initialized():
        h, total = C.c_int64(0), C.c_double(0)
        pos = np.zeros(1, dtype=np.int64)
        assert lib.fmhip_prefix_sums(1, 0, C.byref(h), C.byref(total)) == fm._native.ERR_NOT_INITIALIZED
        assert lib.fmhip_prefix_sums_at(1, pos.ctypes.data_as(C.POINTER(C.c_int64)), 1, po) == fm._native.ERR_NOT_INITIALIZED
        assert lib.fmhip_prefix_search(1, po, 1, 0, pos.ctypes.data_as(C.POINTER(C.c_int64)), po, C.byref(total)) == fm._native.ERR_NOT_INITIALIZED


def test_host_half_under_the_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("needs g++")
    exe = tmp_path / "prefix_host"
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-ffp-contract=off",
                        os.path.join(ROOT, "tests", "cpp", "test_prefix_host.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "prefix host ok" in r.stdout and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stdout[-1500:] + r.stderr[-3000:]


def test_the_kernels_are_in_the_library(fm):
    """A missing kernel is an error, never a fallback: the launchers are weak references, so the library must be shown to hold them."""
    out = subprocess.check_output(["nm", "-D", "--defined-only", fm._native.LIB_PATH], text=True) + subprocess.check_output(["nm", "--defined-only", fm._native.LIB_PATH], text=True, stderr=subprocess.DEVNULL)
    for name in ("launch_prefix_sums", "launch_prefix_queries", "launch_sort_done"):
        assert name in out, name
    blob = open(fm._native.LIB_PATH, "rb").read()
    for kernel in (b"fm_prefix_totals_kernel", b"fm_prefix_carry_kernel", b"fm_prefix_apply_kernel", b"fm_prefix_query_kernel"):
        assert kernel in blob, kernel


# ---------------------------------------------------------------- the engine's side on the null device
@pytest.fixture(scope="module")
def built():
    if not shutil.which("g++") or not os.path.exists("/opt/rocm/include/hip/hip_runtime_api.h"):
        pytest.skip("needs g++ and the HIP headers")
    r = subprocess.run(["make", "-C", NULLDEV, "-f", "prefix.mk", "-j8", "prefix_asan", "prefix_tsan", "prefix_absent_asan"], capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return os.path.join(NULLDEV, "build")


def _env(tmp_path, env):
    return dict(os.environ, FMHIP_JIT_CACHE_DIR=str(tmp_path / "code_objects"), FMHIP_JIT_PACK_DIR="off", FMHIP_RING_BYTES="16384", FMHIP_ARENA_BYTES="4096",
                ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1", TSAN_OPTIONS="halt_on_error=1", **env)


@pytest.mark.parametrize("env", [{}, {"FMNULL_DEVICES": "2"}, {"FMNULL_DEVICES": "3"}, {"FMNULL_THREAD_ENGINES": "1"}])
def test_engine_pass_is_clean_under_the_sanitizers(built, tmp_path, env):
    """drive_prefix: the three calls on vectors of real data at n = 1 … 300 007 and small again, checked against the definition; both modes,
    boundary positions and 4096 of them, thresholds at, below and above prefixes, relative ones and NaN; pending operands, a second thread
    releasing the inputs of pending operands during the call, every argument error — on one engine and behind a device list of one shard,
    behind 2 and 3 shards (FMHIP_ERR_UNSUPPORTED, nothing left behind), with thread engines (a caller that does not own the vector)."""
    full = _env(tmp_path, env)
    a = subprocess.run([os.path.join(built, "drive_prefix_asan")], capture_output=True, text=True, timeout=600, env=full)
    assert a.returncode == 0 and "Sanitizer" not in a.stderr and "runtime error" not in a.stderr, a.stdout[-500:] + a.stderr[-6000:]
    assert a.stdout.count("prefix done") == 2 and a.stderr == ""
    assert ("a device list of one shard: checked" in a.stdout) == (not env)
    t = subprocess.run([os.path.join(built, "drive_prefix_tsan")], capture_output=True, text=True, timeout=600, env=full)
    assert t.returncode == 0 and "ThreadSanitizer" not in t.stderr, t.stdout[-500:] + t.stderr[-6000:]
    assert t.stdout.count("prefix done") == 2 and t.stderr == ""


def test_a_failing_allocation_inside_a_prefix_pass_leaves_nothing_behind(built, tmp_path):
    """One fmhip_prefix_sums takes ONE buffer from the pool, its output (the query calls take none).  The hook FMHIP_TEST_FAIL_ALLOC_AT is
    set on it (its position from a counting run), and once where nothing reaches it: the call answers FMHIP_OK or FMHIP_ERR_OUT_OF_MEMORY,
    a result it gives is right, live vectors and bytes in use are what they were, the same call succeeds afterwards (the driver checks all
    of it), and the process ends without a leak."""
    exe = os.path.join(built, "drive_prefix_asan")
    counting = subprocess.run([exe, "failure"], capture_output=True, text=True, timeout=600, env=_env(tmp_path, {}))
    assert counting.returncode == 0 and "Sanitizer" not in counting.stderr, counting.stdout[-500:] + counting.stderr[-6000:]
    before, inside, status = map(int, re.search(r"failure: (\d+) allocations before the call, (\d+) in it, status (-?\d+)", counting.stdout).groups())
    assert inside == 1 and status == 0
    for at in list(range(before + 1, before + inside + 1)) + [10**9]:
        r = subprocess.run([exe, "failure"], capture_output=True, text=True, timeout=600, env=_env(tmp_path, {"FMHIP_TEST_FAIL_ALLOC_AT": str(at)}))
        assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr and r.stderr == "", (at, r.stdout[-500:] + r.stderr[-6000:])
        assert "failure done" in r.stdout
        failed = int(re.search(r"status (-?\d+)", r.stdout).group(1)) != 0
        assert failed == (at <= before + inside), (at, r.stdout)


@pytest.mark.parametrize("env", [{}, {"FMNULL_DEVICES": "2"}, {"FMNULL_THREAD_ENGINES": "1"}])
def test_a_build_without_the_kernel_answers_unsupported(built, tmp_path, env):
    a = subprocess.run([os.path.join(built, "drive_prefix_absent_asan")], capture_output=True, text=True, timeout=600, env=_env(tmp_path, env))
    assert a.returncode == 0 and "Sanitizer" not in a.stderr and "runtime error" not in a.stderr, a.stdout[-500:] + a.stderr[-6000:]
    assert a.stdout.count("prefix absent done") == 2
