"""The engine's side of the transform option value per path (csrc/transform_engine.hpp) on the TEST-ONLY null device under
the sanitizers: stand-alone programs (tests/nulldev/drive_transform*.cpp, transform.mk) with a stand-in launcher that walks the groups the
kernel's way, on one engine, behind a device list of two and with thread engines; a failing allocation on each of the call's allocations;
a build without the kernel answers FMHIP_ERR_UNSUPPORTED."""
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
    r = subprocess.run(["make", "-C", NULLDEV, "-f", "transform.mk", "-j8", "transform_asan", "transform_tsan", "transform_absent_asan", "transform_absent_tsan"],
                       capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return os.path.join(NULLDEV, "build")


def _env(tmp_path, env):
    return dict(os.environ, FMHIP_JIT_CACHE_DIR=str(tmp_path / "code_objects"), FMHIP_JIT_PACK_DIR="off", FMHIP_RING_BYTES="16384", FMHIP_ARENA_BYTES="4096",
                ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1", TSAN_OPTIONS="halt_on_error=1", **env)


@pytest.mark.parametrize("env", [{}, {"FMNULL_DEVICES": "2"}, {"FMNULL_THREAD_ENGINES": "1"}])
def test_engine_pass_is_clean_under_the_sanitizers(built, tmp_path, env):
    """drive_transform: fmhip_transform_option on vectors of real data at n = 1 … 100 003, 0 … 2 states, 1 … 256 nodes, checked against the host
    entry point; pending operands; every argument refusal with nothing flushed, launched or allocated — on one engine, behind a device list
    of two (every shard its block), with thread engines (a caller that does not own the vectors)."""
    full = _env(tmp_path, env)
    a = subprocess.run([os.path.join(built, "drive_transform_asan")], capture_output=True, text=True, timeout=600, env=full)
    assert a.returncode == 0 and "Sanitizer" not in a.stderr and "runtime error" not in a.stderr, a.stdout[-500:] + a.stderr[-6000:]
    assert "transform option done" in a.stdout and a.stderr == ""
    t = subprocess.run([os.path.join(built, "drive_transform_tsan")], capture_output=True, text=True, timeout=600, env=full)
    assert t.returncode == 0 and "ThreadSanitizer" not in t.stderr, t.stdout[-500:] + t.stderr[-6000:]
    assert "transform option done" in t.stdout and t.stderr == ""


def test_a_failing_allocation_leaves_nothing_behind(built, tmp_path):
    """One fmhip_transform_option of three outputs: its pool allocations are counted by a first run, and FMHIP_TEST_FAIL_ALLOC_AT is set on
    each of them, and once where nothing reaches it: the call answers FMHIP_OK or FMHIP_ERR_OUT_OF_MEMORY, a failed call writes no handle,
    live vectors and bytes in use are what they were, the same call succeeds afterwards (the driver checks all of it), and the process ends
    without a leak."""
    exe = os.path.join(built, "drive_transform_asan")
    counting = subprocess.run([exe, "failure"], capture_output=True, text=True, timeout=600, env=_env(tmp_path, {}))
    assert counting.returncode == 0 and "Sanitizer" not in counting.stderr, counting.stdout[-500:] + counting.stderr[-6000:]
    before, inside, status = map(int, re.search(r"failure: (\d+) allocations before the call, (\d+) in it, status (-?\d+)", counting.stdout).groups())
    assert inside >= 3 and status == 0                                       # the three outputs at least
    for at in list(range(before + 1, before + inside + 1)) + [10**9]:
        r = subprocess.run([exe, "failure"], capture_output=True, text=True, timeout=600, env=_env(tmp_path, {"FMHIP_TEST_FAIL_ALLOC_AT": str(at)}))
        assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr and r.stderr == "", (at, r.stdout[-500:] + r.stderr[-6000:])
        assert "failure done" in r.stdout
        failed = int(re.search(r"status (-?\d+)", r.stdout).group(1)) != 0
        assert failed == (at <= before + inside), (at, r.stdout)


@pytest.mark.parametrize("env", [{}, {"FMNULL_DEVICES": "2"}, {"FMNULL_THREAD_ENGINES": "1"}])
def test_a_build_without_the_kernel_answers_unsupported(built, tmp_path, env):
    a = subprocess.run([os.path.join(built, "drive_transform_absent_asan")], capture_output=True, text=True, timeout=600, env=_env(tmp_path, env))
    assert a.returncode == 0 and "Sanitizer" not in a.stderr and "runtime error" not in a.stderr, a.stdout[-500:] + a.stderr[-6000:]
    assert "transform option absent done" in a.stdout
    t = subprocess.run([os.path.join(built, "drive_transform_absent_tsan")], capture_output=True, text=True, timeout=600, env=_env(tmp_path, env))
    assert t.returncode == 0 and "ThreadSanitizer" not in t.stderr, t.stdout[-500:] + t.stderr[-6000:]
    assert "transform option absent done" in t.stdout
