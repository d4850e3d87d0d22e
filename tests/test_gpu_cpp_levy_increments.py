"""Builds (g++) and runs tests/cpp/test_levy_increments.cpp in its `device` mode: the C++ host mirror's IndependentIncrementsFromICDFHip
(generated on the device by fm_mt_levy_kernel) against IndependentIncrementsFromICDF over the device factory (drawn by host/increments.hpp,
uploaded) with gamma, normal and exponential factors — every draw, gamma and exponential draws equal — a block behind a path offset, and a
variance-gamma path written against the RandomVariable interface on both."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_mirror_levy_increments(fm, oracle, tmp_path):
    exe = str(tmp_path / "test_levy_increments")
    libdir = os.path.join(ROOT, "finmath-lib-cuda-extensions_amd", "lib")
    orcdir = os.path.join(ROOT, "oracle")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_levy_increments.cpp"),
                           f"-L{libdir}", "-lfmhip", f"-L{orcdir}", "-lfm_oracle", f"-Wl,-rpath,{libdir}", f"-Wl,-rpath,{orcdir}", "-lm"])
    out = subprocess.run([exe, "device"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().splitlines()[-1] == "OK device"
