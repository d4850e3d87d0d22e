"""The engine's side of the inverse-CDF increments without a GPU: the generation pass (csrc/mt_generate_engine.hpp) against the null
device under AddressSanitizer / UBSan and ThreadSanitizer (tests/nulldev: the null device, the jump stand-in and the stand-in for
the launcher of fm_mt_icdf_kernel, null_mt.cpp, which generates with the host code from the state, the descriptors and the tables the
engine hands it, and a driver of its own, drive_increments.cpp) on one engine, behind device lists and with thread
engines — blocks behind path offsets reproduce fmhip_increments_host exactly there, which pins the engine's seeding, jump distances, the
sharing of tables between equal means, and the layout of descriptors, tables and slab."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NULLDEV = os.path.join(ROOT, "tests", "nulldev")


@pytest.fixture(scope="module")
def built():
    if not shutil.which("g++") or not os.path.exists("/opt/rocm/include/hip/hip_runtime_api.h"):
        pytest.skip("needs g++ and the HIP headers")
    r = subprocess.run(["make", "-C", NULLDEV, "-j8", "increments_asan", "increments_tsan"], capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return os.path.join(NULLDEV, "build")


@pytest.mark.parametrize("env", [{}, {"FMNULL_DEVICES": "2"}, {"FMNULL_DEVICES": "3"}, {"FMNULL_THREAD_ENGINES": "1"}])
def test_engine_pass_is_clean_under_the_sanitizers(built, tmp_path, env):
    full = dict(os.environ, FMHIP_JIT_CACHE_DIR=str(tmp_path / "code_objects"), FMHIP_JIT_PACK_DIR="off", FMHIP_RING_BYTES="16384", FMHIP_ARENA_BYTES="4096",
                ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1", TSAN_OPTIONS="halt_on_error=1", **env)
    a = subprocess.run([os.path.join(built, "drive_increments_asan")], capture_output=True, text=True, timeout=600, env=full)
    assert a.returncode == 0 and "Sanitizer" not in a.stderr and "runtime error" not in a.stderr, a.stdout[-500:] + a.stderr[-6000:]
    assert a.stdout.count("increments done") == 2
    t = subprocess.run([os.path.join(built, "drive_increments_tsan")], capture_output=True, text=True, timeout=600, env=full)
    assert t.returncode == 0 and "ThreadSanitizer" not in t.stderr, t.stdout[-500:] + t.stderr[-6000:]
    assert t.stdout.count("increments done") == 2
