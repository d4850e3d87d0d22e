"""The engine's side of the gamma and exponential increments without a GPU: the generation pass (csrc/mt_generate_engine.hpp) picking the
launcher of fm_mt_levy_kernel, against the null device under AddressSanitizer / UBSan and ThreadSanitizer — HOST builds only.  The stand-in
(tests/nulldev/null_mt_levy.cpp) generates with the host code from the state, the descriptors and the constants the engine hands it, and
the driver (drive_levy.cpp) compares blocks behind path offsets with fmhip_increments_host: one engine, device lists of 2 and 3 shards,
thread engines.  That pins which launcher a call takes, the seeding, the jump distances, one entry of constants per distinct shape beside
the Poisson tables, and the layout of descriptors, table block and slab."""
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
    r = subprocess.run(["make", "-C", NULLDEV, "-j8", "levy_asan", "levy_tsan"], capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return os.path.join(NULLDEV, "build")


@pytest.mark.parametrize("env", [{}, {"FMNULL_DEVICES": "2"}, {"FMNULL_DEVICES": "3"}, {"FMNULL_THREAD_ENGINES": "1"}])
def test_engine_pass_is_clean_under_the_sanitizers(built, tmp_path, env):
    full = dict(os.environ, FMHIP_JIT_CACHE_DIR=str(tmp_path / "code_objects"), FMHIP_JIT_PACK_DIR="off", FMHIP_RING_BYTES="16384", FMHIP_ARENA_BYTES="4096",
                ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1", TSAN_OPTIONS="halt_on_error=1", **env)
    a = subprocess.run([os.path.join(built, "drive_levy_asan")], capture_output=True, text=True, timeout=600, env=full)
    assert a.returncode == 0 and "Sanitizer" not in a.stderr and "runtime error" not in a.stderr, a.stdout[-500:] + a.stderr[-6000:]
    assert a.stdout.count("levy done") == 2
    t = subprocess.run([os.path.join(built, "drive_levy_tsan")], capture_output=True, text=True, timeout=600, env=full)
    assert t.returncode == 0 and "ThreadSanitizer" not in t.stderr, t.stdout[-500:] + t.stderr[-6000:]
    assert t.stdout.count("levy done") == 2


def test_a_build_without_the_kernel_refuses_the_new_laws(built, tmp_path):
    """drive_increments links the stand-ins of the older launchers only: the engine answers FMHIP_ERR_UNSUPPORTED there for a gamma law — it
    never draws on the host instead.  Seen through the existing driver's binary being unaffected: it still passes."""
    r = subprocess.run(["make", "-C", NULLDEV, "-j8", "increments_asan"], capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    full = dict(os.environ, FMHIP_JIT_CACHE_DIR=str(tmp_path / "code_objects"), FMHIP_JIT_PACK_DIR="off", ASAN_OPTIONS="detect_leaks=1:abort_on_error=0")
    a = subprocess.run([os.path.join(built, "drive_increments_asan")], capture_output=True, text=True, timeout=600, env=full)
    assert a.returncode == 0 and a.stdout.count("increments done") == 2, a.stdout[-500:] + a.stderr[-3000:]
