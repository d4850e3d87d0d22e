"""The device sort without a GPU (include/fmhip.h: fmhip_argsort_host; csrc/sort_host.hpp): the DEFINITION of the order —
ascending in the 32-bit key of the order statistics, ties in path order — against numpy's stable argsort of the same keys; the host
half of the kernels (chunk arithmetic, offsets, a model of a pass) in a stand-alone program under AddressSanitizer / UBSan
(tests/cpp/test_sort_host.cpp); and the engine's side of the four calls (csrc/sort_engine.hpp, the fronts of csrc/sharded.cpp and
csrc/abi.cpp) on the test-only null device under AddressSanitizer + UBSan and ThreadSanitizer (tests/nulldev/sort.mk: drive_sort.cpp with
the stand-in launchers of null_sort.cpp, drive_sort_absent.cpp without them).  Stand-alone programs only: nothing sanitized is loaded
into this process."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NULLDEV = os.path.join(ROOT, "tests", "nulldev")


def keys(a):
    u = np.asarray(a, dtype=np.float32).view(np.uint32)
    k = np.where(u >> 31 != 0, ~u, u | np.uint32(0x80000000)).astype(np.uint32)
    k[(u & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)] = np.uint32(0xFFFFFFFF)
    return k


def inputs(n, rng):
    """The input families of tests/test_gpu_order_statistics.py …"""
    u = rng.random(n, dtype=np.float32)
    yield "uniform", u
    yield "normal", rng.standard_normal(n).astype(np.float32)
    yield "clustered", np.clip(np.exp(0.3 * rng.standard_normal(n)), 0.5, 1.999).astype(np.float32)
    yield "payoff", np.maximum(rng.standard_normal(n) - 0.2, 0.0).astype(np.float32)
    yield "payoff with signed zeros", (np.maximum(rng.standard_normal(n) - 0.2, 0.0) * np.where(u < 0.5, -1.0, 1.0)).astype(np.float32)
    yield "constant", np.full(n, 1.25, dtype=np.float32)
    yield "two values", np.where(u < 0.3, np.float32(-3.5), np.float32(7.0)).astype(np.float32)
    yield "denormals", (rng.integers(-40, 40, n) * np.float32(1e-45)).astype(np.float32)
    yield "signed zeros", np.where(u < 0.5, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
    special = rng.standard_normal(n).astype(np.float32)
    special[::7] = np.inf; special[3::11] = -np.inf
    bits = special.view(np.uint32)
    bits[5::13] = 0x7FC00000; bits[6::17] = 0xFFC00001; bits[1::19] = 0x7F800123        # NaNs of both signs, several payloads
    yield "specials", special
    yield "all NaN", np.full(n, np.nan, dtype=np.float32)
    yield from byte_families(n, rng)


def byte_families(n, rng):
    """… and one per pass: a vector in which only ONE byte of the key varies, over all 256 values (for n >= 256: a permutation of them, then
    repeats).  The other bytes are 0xBF 12 34 56 (floats in [0.5, 1)); under a varying top byte they are 80 00 00, the one choice for which
    all 256 keys are keys of floats that are no NaN: 0x00800000 is -FLT_MAX's and 0xFF800000 is +inf's."""
    for byte in range(4):
        fixed = np.uint32(0x00800000) if byte == 3 else np.uint32(0xBF123456) & ~np.uint32(0xFF << (8 * byte))
        d = np.concatenate([rng.permutation(256), rng.integers(0, 256, max(n - 256, 0))])[:n].astype(np.uint32)
        k = (fixed | (d << np.uint32(8 * byte))).astype(np.uint32)
        a = np.where(k >> 31 != 0, k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32).view(np.float32)      # the float of a key
        assert not np.isnan(a).any() and (keys(a) == k).all()
        yield f"only byte {byte} varies", a


def argsort_host(fm, a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    out = np.full(a.size, -1, dtype=np.int64)
    st = fm.lib().fmhip_argsort_host(a.ctypes.data_as(C.c_void_p), a.size, out.ctypes.data_as(C.POINTER(C.c_int64)))
    assert st == 0, fm.lib().fmhip_last_error()
    return out


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 2049, 10_007])
def test_the_definition_is_numpys_stable_argsort_of_the_keys(fm, n):
    rng = np.random.default_rng(n)
    for name, a in inputs(n, rng):
        want = np.argsort(keys(a), kind="stable")
        got = argsort_host(fm, a)
        assert (got == want).all(), (name, n)
        if name in ("constant", "all NaN"):
            assert (got == np.arange(n)).all(), (name, n)                     # stability: equal keys keep path order


def test_the_python_keys_are_the_definitions(fm):
    a = np.concatenate([x for _, x in inputs(513, np.random.default_rng(5))])
    from importlib import import_module
    assert (import_module(fm.__name__ + ".sorting").sort_keys(a) == keys(a)).all()


def test_the_definition_refuses_on_the_host(fm):
    lib = fm.lib()
    a = np.ones(4, dtype=np.float32)
    out = np.zeros(4, dtype=np.int64)
    bad = fm._native.ERR_INVALID_ARGUMENT
    assert lib.fmhip_argsort_host(None, 4, out.ctypes.data_as(C.POINTER(C.c_int64))) == bad
    assert lib.fmhip_argsort_host(a.ctypes.data_as(C.c_void_p), 4, None) == bad
    assert lib.fmhip_argsort_host(a.ctypes.data_as(C.c_void_p), 0, out.ctypes.data_as(C.POINTER(C.c_int64))) == bad
    assert lib.fmhip_argsort_host(a.ctypes.data_as(C.c_void_p), 1 << 31, out.ctypes.data_as(C.POINTER(C.c_int64))) == bad
    # the device calls need an engine: without one they say so, they do not sort on the host
    if not lib.fmhip_is_initialized():
        h = C.c_int64(0)
        assert lib.fmhip_argsort(1, out.ctypes.data_as(C.POINTER(C.c_int64))) == fm._native.ERR_NOT_INITIALIZED
        assert lib.fmhip_rank_scores(1, C.byref(h)) == fm._native.ERR_NOT_INITIALIZED
        assert lib.fmhip_sort_by_key(1, None, 0, C.byref(h), None) == fm._native.ERR_NOT_INITIALIZED
        assert lib.fmhip_vec_read_elements(1, out.ctypes.data_as(C.POINTER(C.c_int64)), 1, (C.c_double * 1)()) == fm._native.ERR_NOT_INITIALIZED


def test_host_half_under_the_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("needs g++")
    exe = tmp_path / "sort_host"
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        os.path.join(ROOT, "tests", "cpp", "test_sort_host.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "sort host ok" in r.stdout and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stdout[-1500:] + r.stderr[-3000:]


def test_the_kernels_are_in_the_library(fm):
    """A missing kernel is an error, never a fallback: the launchers are weak references, so the library must be shown to hold them."""
    out = subprocess.check_output(["nm", "-D", "--defined-only", fm._native.LIB_PATH], text=True) + subprocess.check_output(["nm", "--defined-only", fm._native.LIB_PATH], text=True, stderr=subprocess.DEVNULL)
    for name in ("launch_sort_pass", "launch_sort_gather", "launch_sort_scores", "launch_sort_read_elements", "launch_sort_done"):
        assert name in out, name
    blob = open(fm._native.LIB_PATH, "rb").read()
    for kernel in (b"fm_sort_count_kernel", b"fm_sort_offsets_kernel", b"fm_sort_scatter_kernel", b"fm_sort_gather_kernel", b"fm_sort_scores_kernel", b"fm_sort_read_elements_kernel"):
        assert kernel in blob, kernel


# ---------------------------------------------------------------- the engine's side on the null device
@pytest.fixture(scope="module")
def built():
    if not shutil.which("g++") or not os.path.exists("/opt/rocm/include/hip/hip_runtime_api.h"):
        pytest.skip("needs g++ and the HIP headers")
    r = subprocess.run(["make", "-C", NULLDEV, "-f", "sort.mk", "-j8", "sort_asan", "sort_tsan", "sort_absent_asan"], capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return os.path.join(NULLDEV, "build")


def _env(tmp_path, env):
    return dict(os.environ, FMHIP_JIT_CACHE_DIR=str(tmp_path / "code_objects"), FMHIP_JIT_PACK_DIR="off", FMHIP_RING_BYTES="16384", FMHIP_ARENA_BYTES="4096",
                ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1", TSAN_OPTIONS="halt_on_error=1", **env)


@pytest.mark.parametrize("env", [{}, {"FMNULL_DEVICES": "2"}, {"FMNULL_DEVICES": "3"}, {"FMNULL_THREAD_ENGINES": "1"}])
def test_engine_pass_is_clean_under_the_sanitizers(built, tmp_path, env):
    """drive_sort: the four calls on vectors of real data at n = 1 … 300 007 and small again, checked against the definition; 0, 1 and 8
    companions, pending operands, a second thread releasing the inputs of pending operands during the call, every argument error — on one
    engine and behind a device list of one shard, behind 2 and 3 shards (FMHIP_ERR_UNSUPPORTED, nothing left behind), with thread engines
    (a caller that owns none of the vectors, owners mixed in one call)."""
    full = _env(tmp_path, env)
    a = subprocess.run([os.path.join(built, "drive_sort_asan")], capture_output=True, text=True, timeout=600, env=full)
    assert a.returncode == 0 and "Sanitizer" not in a.stderr and "runtime error" not in a.stderr, a.stdout[-500:] + a.stderr[-6000:]
    assert a.stdout.count("sort done") == 2 and a.stderr == ""
    assert ("a device list of one shard: checked" in a.stdout) == (not env)
    t = subprocess.run([os.path.join(built, "drive_sort_tsan")], capture_output=True, text=True, timeout=600, env=full)
    assert t.returncode == 0 and "ThreadSanitizer" not in t.stderr, t.stdout[-500:] + t.stderr[-6000:]
    assert t.stdout.count("sort done") == 2 and t.stderr == ""


def test_a_failing_allocation_inside_a_sort_leaves_nothing_behind(built, tmp_path):
    """One fmhip_sort_by_key with 8 companions takes 13 buffers from the pool: the 4 ping-pong buffers, then the 9 outputs.  The hook
    FMHIP_TEST_FAIL_ALLOC_AT is swept over them (positions from a counting run), and once set where nothing reaches it: the call answers FMHIP_OK or
    FMHIP_ERR_OUT_OF_MEMORY, a result it gives is right, live vectors and bytes in use are what they were, the same call succeeds
    afterwards (the driver checks all of it), and the process ends without a leak."""
    import re
    exe = os.path.join(built, "drive_sort_asan")
    counting = subprocess.run([exe, "failure"], capture_output=True, text=True, timeout=600, env=_env(tmp_path, {}))
    assert counting.returncode == 0 and "Sanitizer" not in counting.stderr, counting.stdout[-500:] + counting.stderr[-6000:]
    before, inside, status = map(int, re.search(r"failure: (\d+) allocations before the call, (\d+) in it, status (-?\d+)", counting.stdout).groups())
    assert inside == 13 and status == 0
    for at in list(range(before + 1, before + inside + 1)) + [10**9]:
        r = subprocess.run([exe, "failure"], capture_output=True, text=True, timeout=600, env=_env(tmp_path, {"FMHIP_TEST_FAIL_ALLOC_AT": str(at)}))
        assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr and r.stderr == "", (at, r.stdout[-500:] + r.stderr[-6000:])
        assert "failure done" in r.stdout
        failed = int(re.search(r"status (-?\d+)", r.stdout).group(1)) != 0
        assert failed == (at <= before + inside), (at, r.stdout)      # every one of the 13 is THIS call's allocation: it fails, and says so


@pytest.mark.parametrize("env", [{}, {"FMNULL_DEVICES": "2"}, {"FMNULL_THREAD_ENGINES": "1"}])
def test_a_build_without_the_kernel_answers_unsupported(built, tmp_path, env):
    a = subprocess.run([os.path.join(built, "drive_sort_absent_asan")], capture_output=True, text=True, timeout=600, env=_env(tmp_path, env))
    assert a.returncode == 0 and "Sanitizer" not in a.stderr and "runtime error" not in a.stderr, a.stdout[-500:] + a.stderr[-6000:]
    assert a.stdout.count("sort absent done") == 2
