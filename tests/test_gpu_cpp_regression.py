"""Builds (g++) and runs tests/cpp/test_regression.cpp: the C++ host mirror's MonteCarloConditionalExpectationRegression (normal equations
from one fmhip_cross_moments call) against the CPU twin's pair-by-pair path through the common C++ interface — eager and fused, with
FMHIP_DEVICE_CROSS_MOMENTS=0, and the solver's pivot rule."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_mirror_regression(fm, oracle, tmp_path):
    exe = str(tmp_path / "test_regression")
    libdir = os.path.join(ROOT, "finmath-lib-cuda-extensions_amd", "lib")
    orcdir = os.path.join(ROOT, "oracle")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_regression.cpp"),
                           f"-L{libdir}", "-lfmhip", f"-L{orcdir}", "-lfm_oracle", f"-Wl,-rpath,{libdir}", f"-Wl,-rpath,{orcdir}", "-lm"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().splitlines()[-1].startswith("OK")
