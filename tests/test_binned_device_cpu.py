"""The engine's side of the localized regression without a GPU: Engine::binned_xmom_pass and Engine::binned_eval (csrc/binned_engine.hpp)
against the null device under AddressSanitizer / UBSan and ThreadSanitizer — HOST builds only.  The stand-ins (tests/nulldev/null_binned.cpp)
compute with the host definition in the layout the engine asked for, and the driver (drive_binned.cpp) compares counts, sums and the estimate
with fmhip_binned_*_host bit for bit: one engine, device lists of 2 and 3 shards, thread engines, a second thread releasing the inputs of
pending operands during the calls, every argument error, and a build without the launchers (drive_binned_absent.cpp): FMHIP_ERR_UNSUPPORTED."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NULLDEV = os.path.join(ROOT, "tests", "nulldev")


@pytest.fixture(scope="module")
def built():
    if not shutil.which("g++") or not os.path.exists("/opt/rocm/include/hip/hip_runtime_api.h"):
        pytest.skip("needs g++ and the HIP headers")
    r = subprocess.run(["make", "-C", NULLDEV, "-j8", "binned_asan", "binned_tsan", "binned_absent_asan"], capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return os.path.join(NULLDEV, "build")


@pytest.mark.parametrize("env", [{}, {"FMNULL_DEVICES": "2"}, {"FMNULL_DEVICES": "3"}, {"FMNULL_THREAD_ENGINES": "1"}])
def test_engine_passes_are_clean_under_the_sanitizers(built, tmp_path, env):
    full = dict(os.environ, FMHIP_JIT_CACHE_DIR=str(tmp_path / "code_objects"), FMHIP_JIT_PACK_DIR="off", FMHIP_RING_BYTES="16384", FMHIP_ARENA_BYTES="4096",
                ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1", TSAN_OPTIONS="halt_on_error=1", **env)
    a = subprocess.run([os.path.join(built, "drive_binned_asan")], capture_output=True, text=True, timeout=600, env=full)
    assert a.returncode == 0 and "Sanitizer" not in a.stderr and "runtime error" not in a.stderr, a.stdout[-500:] + a.stderr[-6000:]
    assert a.stdout.count("binned done") == 2
    t = subprocess.run([os.path.join(built, "drive_binned_tsan")], capture_output=True, text=True, timeout=600, env=full)
    assert t.returncode == 0 and "ThreadSanitizer" not in t.stderr, t.stdout[-500:] + t.stderr[-6000:]
    assert t.stdout.count("binned done") == 2


@pytest.mark.parametrize("env", [{}, {"FMNULL_DEVICES": "2"}, {"FMNULL_THREAD_ENGINES": "1"}])
def test_a_build_without_the_kernels_answers_unsupported(built, tmp_path, env):
    """drive_binned_absent links NO stand-in for the two launchers (weak references that stay null): both device entry points answer
    FMHIP_ERR_UNSUPPORTED behind their argument checks — on one engine, behind a device list and with thread engines — and leave no handle;
    the host definition works without them."""
    full = dict(os.environ, FMHIP_JIT_CACHE_DIR=str(tmp_path / "code_objects"), FMHIP_JIT_PACK_DIR="off", ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", **env)
    a = subprocess.run([os.path.join(built, "drive_binned_absent_asan")], capture_output=True, text=True, timeout=600, env=full)
    assert a.returncode == 0 and "Sanitizer" not in a.stderr, a.stdout[-500:] + a.stderr[-3000:]
    assert a.stdout.count("binned absent done") == 2


def test_the_cross_moments_driver_is_unaffected(built, tmp_path):
    """drive_xmom links the cross-moments stand-in only: the existing driver still builds and passes beside the new passes."""
    r = subprocess.run(["make", "-C", NULLDEV, "-j8", "xmom_asan"], capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    full = dict(os.environ, FMHIP_JIT_CACHE_DIR=str(tmp_path / "code_objects"), FMHIP_JIT_PACK_DIR="off", ASAN_OPTIONS="detect_leaks=1:abort_on_error=0")
    a = subprocess.run([os.path.join(built, "drive_xmom_asan")], capture_output=True, text=True, timeout=600, env=full)
    assert a.returncode == 0 and a.stdout.count("xmom done") == 2, a.stdout[-500:] + a.stderr[-3000:]


def test_a_failing_allocation_inside_a_binned_evaluation_leaves_nothing_behind(built, tmp_path):
    """One fmhip_binned_evaluate takes ONE buffer from the pool, its output.  The hook FMHIP_TEST_FAIL_ALLOC_AT is set on it (its position
    from a counting run), and once where nothing reaches it: the call answers FMHIP_OK or FMHIP_ERR_OUT_OF_MEMORY, a result it gives is the
    definition's, a failed call leaves its handle as it was, live vectors and bytes in use are what they were, the same call succeeds
    afterwards (the driver checks all of it), and the process ends without a leak."""
    exe = os.path.join(built, "drive_binned_asan")
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
