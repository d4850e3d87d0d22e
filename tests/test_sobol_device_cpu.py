"""The engine's side of the Sobol' Brownian motion without a GPU: Engine::sobol_bm_generate (csrc/sobol_engine.hpp) against the null device
under AddressSanitizer / UBSan and ThreadSanitizer — HOST builds only.  The stand-in (tests/nulldev/null_sobol.cpp) walks the plan, the
direction words and the shifts that the engine uploaded, with the host code, and the driver (drive_sobol.cpp) compares blocks behind path
offsets with fmhip_sobol_increments_host: one engine, device lists of 2 and 3 shards, thread engines.  That pins the plan and its slots,
the layout of the upload, the workgroup range of a block of paths, the slab, and every argument error."""
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
    r = subprocess.run(["make", "-C", NULLDEV, "-j8", "sobol_asan", "sobol_tsan"], capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return os.path.join(NULLDEV, "build")


@pytest.mark.parametrize("env", [{}, {"FMNULL_DEVICES": "2"}, {"FMNULL_DEVICES": "3"}, {"FMNULL_THREAD_ENGINES": "1"}])
def test_engine_pass_is_clean_under_the_sanitizers(built, tmp_path, env):
    full = dict(os.environ, FMHIP_JIT_CACHE_DIR=str(tmp_path / "code_objects"), FMHIP_JIT_PACK_DIR="off", FMHIP_RING_BYTES="16384", FMHIP_ARENA_BYTES="4096",
                ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1", TSAN_OPTIONS="halt_on_error=1", **env)
    a = subprocess.run([os.path.join(built, "drive_sobol_asan")], capture_output=True, text=True, timeout=600, env=full)
    assert a.returncode == 0 and "Sanitizer" not in a.stderr and "runtime error" not in a.stderr, a.stdout[-500:] + a.stderr[-6000:]
    assert a.stdout.count("sobol done") == 2
    t = subprocess.run([os.path.join(built, "drive_sobol_tsan")], capture_output=True, text=True, timeout=600, env=full)
    assert t.returncode == 0 and "ThreadSanitizer" not in t.stderr, t.stdout[-500:] + t.stderr[-6000:]
    assert t.stdout.count("sobol done") == 2


def test_a_build_without_the_kernel_refuses(built, tmp_path):
    """drive_mersenne links the Mersenne-Twister stand-ins only: the Sobol' launcher is absent there, and the existing driver is unaffected
    by the new pass — it still builds and passes.  (That the engine answers FMHIP_ERR_UNSUPPORTED without the launcher is a null check in
    front of the upload: csrc/sobol_engine.hpp.)"""
    r = subprocess.run(["make", "-C", NULLDEV, "-j8", "mersenne_asan"], capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    full = dict(os.environ, FMHIP_JIT_CACHE_DIR=str(tmp_path / "code_objects"), FMHIP_JIT_PACK_DIR="off", ASAN_OPTIONS="detect_leaks=1:abort_on_error=0")
    a = subprocess.run([os.path.join(built, "drive_mersenne_asan")], capture_output=True, text=True, timeout=600, env=full)
    assert a.returncode == 0 and a.stdout.count("mersenne done") == 2, a.stdout[-500:] + a.stderr[-3000:]
