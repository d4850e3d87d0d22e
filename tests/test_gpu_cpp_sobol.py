"""Builds (g++) and runs tests/cpp/test_sobol.cpp in its `device` mode: the C++ host mirror's BrownianMotionFromSobolSequenceHip (generated
on the device by fm_sobol_bm_kernel) against BrownianMotionFromSobolSequence over the device factory (drawn by host/sobol.hpp, uploaded) —
every draw equal, both constructions, with and without the digital shift, and a block behind a path offset."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_mirror_sobol(fm, oracle, tmp_path):
    exe = str(tmp_path / "test_sobol")
    libdir = os.path.join(ROOT, "finmath-lib-cuda-extensions_amd", "lib")
    orcdir = os.path.join(ROOT, "oracle")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_sobol.cpp"),
                           f"-L{libdir}", "-lfmhip", f"-L{orcdir}", "-lfm_oracle", f"-Wl,-rpath,{libdir}", f"-Wl,-rpath,{orcdir}", "-lm"])
    out = subprocess.run([exe, "device"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().splitlines()[-1] == "OK device"
