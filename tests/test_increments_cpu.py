"""CPU-only: independent increments with a law per (time step, factor) — the host definition fmhip_increments_host (host/increments.hpp),
its argument checks, the bindings, the Python mirror's switch and the Merton series.  The Poisson tables themselves (first entry exp(−mean)
to the bit, rising, ending in 1.0, a uniform one ulp either side of an entry) are checked where they can be seen, in
tests/cpp/test_increments.cpp, which this file builds and runs."""
import ctypes as C
import math
import os
import subprocess
from importlib import import_module

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NORMAL, UNIFORM, POISSON = 0, 1, 2
INVALID, NOT_INITIALIZED = -5, -6


def call_host(fm, seed, laws, n_paths, steps=None, factors=None):
    """laws: [step][factor] of (kind, a, b) → (status, [step·factors + factor][path] doubles)"""
    flat = [law for row in laws for law in row]
    kinds = np.array([k for k, _, _ in flat], dtype=np.int32)
    a = np.array([v for _, v, _ in flat], dtype=np.float64)
    b = np.array([v for _, _, v in flat], dtype=np.float64)
    out = np.zeros((len(flat), max(n_paths, 0)), dtype=np.float64)
    rc = fm.lib().fmhip_increments_host(seed, len(laws) if steps is None else steps, len(laws[0]) if factors is None else factors, n_paths,
                                        kinds.ctypes.data_as(C.POINTER(C.c_int32)), a.ctypes.data_as(C.POINTER(C.c_double)),
                                        b.ctypes.data_as(C.POINTER(C.c_double)), out.ctypes.data_as(C.POINTER(C.c_double)))
    return rc, out


def test_entry_points_are_bound(fm):
    for name in ("fmhip_increments_host", "fmhip_increments_generate_device"):
        assert name in fm._native.SYMBOLS and hasattr(fm.lib(), name)
    header = open(os.path.join(ROOT, "include", "fmhip.h"), encoding="utf-8").read()
    assert "enum { FMHIP_LAW_NORMAL = 0, FMHIP_LAW_UNIFORM = 1, FMHIP_LAW_POISSON = 2 };" in header
    assert fm.lib().fmhip_abi_version() == 1


@pytest.mark.parametrize("seed", [3141, 0, -1])
def test_all_normal_laws_are_the_mersenne_brownian_motion(fm, seed):
    dt = np.array([0.25, 0.0, 1.5, 0.1])
    want = fm.mersenne_increments(seed, dt, 3, 4001)
    got = fm.host_increments(seed, lambda i, f: fm.NormalLaw(math.sqrt(dt[i])), 4, 3, 4001)
    assert got.shape == want.shape and (got.view(np.uint64) == want.view(np.uint64)).all()


def test_uniform_known_answers(fm):
    """MT19937 seeded as finmath seeds it; nextDouble = ((next(26) << 26) | next(26)) · 2^-52: a uniform law on [0, 1) returns the doubles
    themselves, which the all-normal law above has tied to fmhip_mersenne_increments through the inverse normal CDF."""
    u = fm.host_increments(31415, lambda i, f: fm.UniformLaw(0.0, 1.0), 2, 3, 50)
    assert ((u >= 0) & (u < 1)).all() and (u * 2.0 ** 52 == np.floor(u * 2.0 ** 52)).all()
    z = fm.host_increments(31415, lambda i, f: fm.NormalLaw(1.0), 2, 3, 50)
    assert (z == np.vectorize(fm.lib().fmhip_inverse_normal_cdf)(u)).all()
    v = fm.host_increments(31415, lambda i, f: fm.UniformLaw(-1.0, 3.0), 2, 3, 50)
    assert (v == -1.0 + 4.0 * u).all()
    mixed = fm.host_increments(31415, lambda i, f: [fm.UniformLaw(0.0, 1.0), fm.PoissonLaw(1.0), fm.UniformLaw(2.0, 2.0)][f], 2, 3, 50)
    assert (mixed[:, 0] == u[:, 0]).all() and (mixed[:, 2] == 2.0).all()
    # the Poisson law of the same uniform: exp(-1) = F[0], 2 exp(-1) = F[1], 2.5 exp(-1) = F[2]
    F = np.cumsum([math.exp(-1.0), math.exp(-1.0), math.exp(-1.0) / 2])
    sure = np.abs(u[:, 1, :, None] - F).min(axis=-1) > 1e-12
    assert ((mixed[:, 1] == np.searchsorted(F, u[:, 1]))[sure & (u[:, 1] < F[-1])]).all()


@pytest.mark.parametrize("mean", [0.02, 1.0, 30.0, 128.0])
def test_poisson_sample_moments(fm, mean):
    n = 1_000_000
    x = fm.host_increments(7, lambda i, f: fm.PoissonLaw(mean), 1, 1, n)[0, 0]
    assert (x == np.floor(x)).all() and x.min() >= 0
    assert abs(x.mean() - mean) <= 5 * math.sqrt(mean / n)
    # the variance of the sample variance of a Poisson variable: (mean + 2 mean^2 ... ) / n, fourth central moment mean + 3 mean^2
    assert abs(x.var() - mean) <= 5 * math.sqrt((mean + 2 * mean * mean) / n)


def test_poisson_mean_zero_and_shared_means(fm):
    x = fm.host_increments(1, lambda i, f: fm.PoissonLaw(0.0), 3, 2, 1000)
    assert (x == 0).all()
    a = fm.host_increments(5, lambda i, f: fm.PoissonLaw(2.0), 4, 1, 500)                      # one table for four laws
    b = fm.host_increments(5, lambda i, f: fm.PoissonLaw(2.0 if i != 2 else 3.0), 4, 1, 500)
    assert (a[[0, 1, 3]] == b[[0, 1, 3]]).all() and (b[2] >= a[2]).all() and (b[2] > a[2]).any()      # the same uniforms, a larger mean


def test_argument_errors(fm):
    nan, inf = float("nan"), float("inf")
    ok = [[(NORMAL, 1.0, 0.0), (UNIFORM, 0.0, 1.0), (POISSON, 1.0, 0.0)]]
    assert call_host(fm, 1, ok, 10)[0] == 0 and call_host(fm, 1, ok, 0)[0] == 0
    bad = [
        [[(3, 1.0, 0.0)]], [[(-1, 1.0, 0.0)]],
        [[(NORMAL, -1.0, 0.0)]], [[(NORMAL, nan, 0.0)]], [[(POISSON, -0.5, 0.0)]], [[(POISSON, nan, 0.0)]], [[(POISSON, 128.0000001, 0.0)]], [[(POISSON, inf, 0.0)]],
        [[(UNIFORM, 2.0, 1.0)]], [[(UNIFORM, 0.0, inf)]], [[(UNIFORM, -inf, 0.0)]], [[(UNIFORM, nan, 1.0)]], [[(UNIFORM, 0.0, nan)]],
        [[(POISSON, 100.0 + 1e-3 * i, 0.0)] for i in range(400)],                      # more than 2^16 table doubles over all distinct means
    ]
    for laws in bad:
        rc, _ = call_host(fm, 1, laws, 10)
        assert rc == INVALID, laws[0]
        assert len(fm.lib().fmhip_last_error()) > 10
    assert call_host(fm, 1, ok, -1)[0] == INVALID and call_host(fm, 1, ok, 10, steps=0)[0] == INVALID and call_host(fm, 1, ok, 10, factors=0)[0] == INVALID
    assert call_host(fm, 1, ok, 1, steps=1 << 20, factors=1 << 5)[0] == INVALID         # more than 2^24 laws: the count is checked before a law is read
    assert b"2^24" in fm.lib().fmhip_last_error()
    assert call_host(fm, 1, [[(POISSON, 128.0, 0.0)]], 10)[0] == 0
    # the 2^44-word limit: the check comes before anything is drawn (no output is touched: a null pointer is enough to see that)
    lib = fm.lib()
    k, a, b = (C.c_int32 * 1)(NORMAL), (C.c_double * 1)(1.0), (C.c_double * 1)(0.0)
    assert lib.fmhip_increments_host(1, 1, 1, (1 << 31), k, a, b, None) == INVALID
    assert lib.fmhip_increments_host(1, 1, 1, 10, None, a, b, (C.c_double * 10)()) == INVALID
    with pytest.raises(fm.FmhipError):
        fm.host_increments(1, lambda i, f: fm.PoissonLaw(500.0), 1, 1, 10)


def test_device_entry_point_without_a_device_fails_loudly(fm):
    try:
        import torch
        has_gpu = torch.cuda.is_available()
    except Exception:
        has_gpu = False
    lib = fm.lib()
    if has_gpu or lib.fmhip_is_initialized():
        pytest.skip("a GPU is present")
    k, a, b, out = (C.c_int32 * 1)(POISSON), (C.c_double * 1)(1.0), (C.c_double * 1)(0.0), (C.c_int64 * 1)()
    assert lib.fmhip_increments_generate_device(1, 1, 1, 10, 0, k, a, b, out) == NOT_INITIALIZED and out[0] == 0
    assert b"fmhip_init" in lib.fmhip_last_error()


def test_mirror_switch_and_classes(fm, monkeypatch):
    inc = import_module("finmath-lib-cuda-extensions_amd.increments")
    monkeypatch.delenv("FMHIP_DEVICE_INCREMENTS", raising=False)
    assert inc._device_increments()
    monkeypatch.setenv("FMHIP_DEVICE_INCREMENTS", "0")
    assert not inc._device_increments()
    td = fm.TimeDiscretization(0.0, 2, 0.5)
    laws = lambda i, f: fm.PoissonLaw(0.5) if f else fm.NormalLaw(1.0)
    x = fm.IndependentIncrementsFromICDF(td, 2, 10, 7, laws, None, 40)
    assert x.pathOffset == 40 and x.getCloneWithModifiedSeed(8).pathOffset == 40 and x.getCloneWithModifiedSeed(8).getSeed() == 8
    assert x == fm.IndependentIncrementsFromICDF(td, 2, 10, 7, laws, None, 40) and hash(x) == hash(fm.IndependentIncrementsFromICDF(td, 2, 10, 7, laws, None, 40))
    assert x != fm.IndependentIncrementsFromICDF(td, 2, 10, 7, lambda i, f: fm.NormalLaw(1.0), None, 40)
    assert x.getCloneWithModifiedTimeDiscretization(fm.TimeDiscretization(0.0, 4, 0.25)).getTimeDiscretization().getNumberOfTimeSteps() == 4
    j = fm.JumpProcessIncrements(td, [2.0, 4.0], 10, 7)
    assert j.getNumberOfFactors() == 2 and j._law_table()[1][1] == fm.PoissonLaw(2.0) and isinstance(j.getCloneWithModifiedSeed(1), fm.JumpProcessIncrements)
    assert fm.NormalLaw(2.0).kind == NORMAL and fm.UniformLaw(0, 1).kind == UNIFORM and fm.PoissonLaw(1).kind == POISSON


def test_mirror_over_the_cpu_twin_and_the_merton_series(fm, oracle, monkeypatch):
    """A factory that is not the device's is handed host-drawn increments (no device is touched): Merton's call on the CPU twin against the series."""
    mc = import_module("finmath-lib-cuda-extensions_amd.montecarlo")
    td = fm.TimeDiscretization(0.0, 10, 0.1)
    par = dict(initial_value=100.0, risk_free_rate=0.05, volatility=0.2, jump_intensity=1.0, jump_size_mean=-0.1, jump_size_stddev=0.15, maturity=1.0, strike=100.0)
    inc = fm.merton_increments(td, 200_000, 3141, par["jump_intensity"], oracle.RandomVariableFloatFactory())
    value, rv = mc.merton_call_mc(inc, **par)
    exact = mc.merton_call_analytic(**par)
    assert abs(value - exact) <= 3 * rv.getStandardError() and 12.5 < exact < 13.0
    assert inc.getIncrement(3, 2).getFiltrationTime() == td.getTime(4)
    # no jumps: the series is Black–Scholes; jumps of size zero too
    bs = mc.black_scholes_call_analytic(100.0, 0.05, 0.2, 1.0, 100.0)
    assert mc.merton_call_analytic(**dict(par, jump_intensity=0.0)) == bs
    assert abs(mc.merton_call_analytic(**dict(par, jump_size_mean=0.0, jump_size_stddev=0.0)) - bs) <= 1e-12 * bs


def test_cpp_definition_and_mirror(tmp_path):
    exe = str(tmp_path / "test_increments")
    libdir = os.path.join(ROOT, "finmath-lib-cuda-extensions_amd", "lib")
    orcdir = os.path.join(ROOT, "oracle")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_increments.cpp"),
                           f"-L{libdir}", "-lfmhip", f"-L{orcdir}", "-lfm_oracle", f"-Wl,-rpath,{libdir}", f"-Wl,-rpath,{orcdir}", "-lm"])
    out = subprocess.run([exe, "cpu"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().splitlines()[-1] == "OK cpu"
