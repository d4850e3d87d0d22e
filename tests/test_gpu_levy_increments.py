"""Gamma and exponential increments on the device (fm_mt_levy_kernel in mt_bm_kernel.hip) against the definition,
fmhip_increments_host (host/gamma_icdf.hpp compiled for the host) narrowed to fp32.  EVERY draw is compared.

The contract: gamma and exponential streams are EQUAL, no share left out — the device compiles the host's text, which uses + − × /, sqrt
and integer operations only.  Poisson and uniform streams in the same call are equal; normal streams stay under the contract of
mt_bm_kernel.hip (a central draw equal, a tail draw at most one fp32 ulp off, a handful in 10^8).  A call without the new laws runs the
kernel it ran before.  Tests that need another environment or another engine mode run in a child process."""
import ctypes as C
import hashlib
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CENTRAL = 1.4395
NORMAL, UNIFORM, POISSON, GAMMA, EXPONENTIAL = 0, 1, 2, 4, 5
INVALID = -5


def arrays(laws):
    flat = [law for row in laws for law in row]
    return (np.array([k for k, _, _ in flat], dtype=np.int32), np.array([a for _, a, _ in flat], dtype=np.float64),
            np.array([b for _, _, b in flat], dtype=np.float64))


def pointers(kinds, a, b):
    return kinds.ctypes.data_as(C.POINTER(C.c_int32)), a.ctypes.data_as(C.POINTER(C.c_double)), b.ctypes.data_as(C.POINTER(C.c_double))


def generate(fm, seed, laws, n_paths, path_offset=0):
    N = fm._native
    kinds, a, b = arrays(laws)
    handles = (C.c_int64 * kinds.size)()
    N.check(N.lib().fmhip_increments_generate_device(seed, len(laws), len(laws[0]), n_paths, path_offset, *pointers(kinds, a, b), handles))
    vecs = [fm.DeviceVector(handles[k], n_paths) for k in range(kinds.size)]
    return np.stack([v.to_float32() for v in vecs]) if n_paths else np.zeros((kinds.size, 0), dtype=np.float32)


def host(fm, seed, laws, n_paths, path_offset=0):
    N = fm._native
    kinds, a, b = arrays(laws)
    out = np.empty((kinds.size, path_offset + n_paths), dtype=np.float64)
    N.check(N.lib().fmhip_increments_host(seed, len(laws), len(laws[0]), path_offset + n_paths, *pointers(kinds, a, b), out.ctypes.data_as(C.POINTER(C.c_double))))
    return out[:, path_offset:]


def compare(fm, got, seed, laws, n_paths, path_offset=0):
    """Everything but the normal streams equal — gamma and exponential among it, a hard condition; normal streams under §4.9's contract.
    Returns the number of normal tail draws one ulp off."""
    kinds, a, _ = arrays(laws)
    want64 = host(fm, seed, laws, n_paths, path_offset)
    want = want64.astype(np.float32)
    assert got.shape == want.shape
    differ = got.view(np.uint32) != want.view(np.uint32)
    for kind, name in ((GAMMA, "gamma"), (EXPONENTIAL, "exponential"), (POISSON, "Poisson"), (UNIFORM, "uniform")):
        assert not differ[kinds == kind].any(), f"{differ[kinds == kind].sum()} {name} draws differ"
    if not differ.any():
        return 0
    scale = np.where(a > 0, a, 1.0)[:, None]
    central = np.abs(want64) / scale < CENTRAL
    assert not (differ & central).any(), f"{(differ & central).sum()} central normal draws differ"
    ulps = np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))[differ]
    assert ulps.max() == 1, f"a tail draw differs by {ulps.max()} fp32 ulps"
    assert differ.sum() <= 2 + got.size * 1e-7, f"{differ.sum()} of {got.size} draws differ by one ulp"
    return int(differ.sum())


def variance_gamma_laws(steps, dt, nu):
    return [[(GAMMA, dt / nu, nu), (NORMAL, 1.0, 0.0)] for _ in range(steps)]


GAMMA_SHAPES = [0.01, 0.02, 0.06, 0.0625, 0.3, 0.5, 0.99, 1.0, 1.01, 2.5, 7.0, 30.0, 99.5, 300.0, 999.0, 1000.0]
SHAPES = {
    "variance-gamma 40 x 2": (variance_gamma_laws(40, 0.0125, 0.2), 100_003),
    "gamma only, a shape per step": ([[(GAMMA, shape, 0.5 + i)] for i, shape in enumerate(GAMMA_SHAPES)], 20_011),
    "exponential only 3 x 2": ([[(EXPONENTIAL, 0.5 * (i + 1), 0.0), (EXPONENTIAL, 1e-3, 0.0)] for i in range(3)], 100_003),
    "all five laws": ([[(NORMAL, 0.5, 0.0), (UNIFORM, -1.0, 3.0), (POISSON, 2.5 * (i + 1), 0.0), (GAMMA, 0.06 * (i + 1), 0.2), (EXPONENTIAL, 3.0, 0.0)] for i in range(3)], 50_021),
    "903 streams (element-wise stores)": ([[(GAMMA, 0.05 + 0.01 * i, 1.0), (NORMAL, 1.0, 0.0), (EXPONENTIAL, 1.0 + i, 0.0)] for i in range(301)], 50),
}


@pytest.mark.parametrize("name", list(SHAPES))
def test_shapes_against_the_host_definition(gpu, name):
    laws, n = SHAPES[name]
    got = generate(gpu, 31415, laws, n)
    n_ulp = compare(gpu, got, 31415, laws, n)
    kinds = arrays(laws)[0]
    assert np.isfinite(got).all() and (got[(kinds == GAMMA) | (kinds == EXPONENTIAL)] >= 0).all()
    print(f"{name}: {got.size} draws, {n_ulp} normal tail draws one fp32 ulp off")


@pytest.mark.parametrize("n", [0, 1, 63, 1 << 20])
def test_path_counts(gpu, n):
    laws = [[(GAMMA, 0.06, 0.2), (NORMAL, 1.0, 0.0)], [(EXPONENTIAL, 2.0, 0.0), (GAMMA, 3.5, 1.0)]]
    for seed in (0, -1):
        got = generate(gpu, seed, laws, n)
        assert got.shape == (4, n)
        compare(gpu, got, seed, laws, n)


def test_path_offset_blocks_are_slices_of_the_whole(gpu):
    laws = variance_gamma_laws(4, 0.25, 0.2)
    n = 800_000
    whole = generate(gpu, 77, laws, n)
    compare(gpu, whole, 77, laws, n)
    for off, cnt in ((0, 5_000), (12_345, 5_001), (777_777, 22_223)):
        block = generate(gpu, 77, laws, cnt, off)
        assert (block.view(np.uint32) == whole[:, off:off + cnt].view(np.uint32)).all(), off


def test_which_kernel_runs_and_what_the_counters_say(gpu):
    """Old laws only: one launch (two behind a path offset) and 4 bytes written per draw, as before this kernel existed.  A call with a
    new law: the same — fm_mt_levy_kernel once, plus the jump kernel behind a path offset.  That it IS the other kernel is seen in the
    numbers: the old kernel knows no gamma law, and every draw is compared."""
    n = 10_007
    old = [[(NORMAL, 1.0, 0.0), (POISSON, 1.0, 0.0)]]
    new = [[(GAMMA, 0.5, 1.0), (NORMAL, 1.0, 0.0)]]
    moved = {}
    for name, laws in (("old", old), ("new", new)):
        for offset, launches in ((0, 1), (5, 2)):
            before, s0 = gpu.pool_stats().n_kernel_launches, gpu.engine_stats()
            N = gpu._native
            kinds, a, b = arrays(laws)
            handles = (C.c_int64 * 2)()
            N.check(N.lib().fmhip_increments_generate_device(3, 1, 2, n, offset, *pointers(kinds, a, b), handles))
            s1 = gpu.engine_stats()
            assert gpu.pool_stats().n_kernel_launches - before == launches, (name, offset)
            moved[name, offset] = {k: s1[k] - s0[k] for k in s1 if s1[k] != s0[k] and "peak" not in k}
            got = np.stack([gpu.DeviceVector(h, n).to_float32() for h in handles])
            compare(gpu, got, 3, laws, n, offset)
    print(moved)
    assert moved["new", 0] == moved["old", 0] and moved["new", 5] == moved["old", 5]
    assert 4 * n * 2 in moved["old", 0].values()                         # the bytes written: 4 per draw


def test_argument_errors_launch_nothing(gpu):
    lib = gpu._native.lib()
    out = (C.c_int64 * 8)()
    before = gpu.engine_stats()
    launches = gpu.pool_stats().n_kernel_launches
    live = gpu.pool_stats().n_live_vectors
    nan, inf = float("nan"), float("inf")

    def call(laws, n_paths=10):
        kinds, a, b = arrays(laws)
        return lib.fmhip_increments_generate_device(1, len(laws), len(laws[0]), n_paths, 0, *pointers(kinds, a, b), out)
    bad = [
        [[(3, 1.0, 0.0)]],
        [[(GAMMA, 0.0, 1.0)]], [[(GAMMA, -1.0, 1.0)]], [[(GAMMA, nan, 1.0)]], [[(GAMMA, inf, 1.0)]], [[(GAMMA, 0.0099, 1.0)]], [[(GAMMA, 1000.5, 1.0)]],
        [[(GAMMA, 1.0, 0.0)]], [[(GAMMA, 1.0, -2.0)]], [[(GAMMA, 1.0, nan)]], [[(GAMMA, 1.0, inf)]],
        [[(EXPONENTIAL, 0.0, 0.0)]], [[(EXPONENTIAL, -1.0, 0.0)]], [[(EXPONENTIAL, nan, 0.0)]], [[(EXPONENTIAL, inf, 0.0)]],
        [[(GAMMA, 1.0 + 1e-4 * i, 1.0)] for i in range(11_000)],                       # 11 000 distinct shapes of 6 constants: more than 2^16 doubles
    ]
    for laws in bad:
        assert call(laws) == INVALID, laws[0]
        assert lib.fmhip_last_error()
    assert b"step 10922" in lib.fmhip_last_error()
    assert gpu.engine_stats() == before and gpu.pool_stats().n_kernel_launches == launches
    assert call([[(GAMMA, 0.01, 1e-300), (GAMMA, 1000.0, 1e300), (EXPONENTIAL, 1e-300, 0.0)]]) == 0
    for h in list(out)[:3]:
        lib.fmhip_vec_release(h)
    assert gpu.pool_stats().n_kernel_launches - launches == 1
    assert gpu.pool_stats().n_live_vectors == live


def test_gamma_sample_moments(gpu):
    """10^6 paths, the engine's own getAverage / getVariance: the mean within 4 standard errors of shape·scale, the variance within 4 of
    shape·scale² (variance of a sample variance: (μ4 − σ⁴)/n, μ4 = 3 k (k + 2) θ⁴ for Gamma(k, θ))."""
    n = 1_000_000
    td = gpu.TimeDiscretization(0.0, 3, 0.1)
    for shape_per_time, scale in ((0.6, 0.2), (10.0, 1.0), (300.0, 2.0)):
        g = gpu.GammaProcess(td, n, 99, shape_per_time, scale)
        for i in range(3):
            k = shape_per_time * td.getTimeStep(i)
            x = g.getIncrement(i, 0)
            mean, var = k * scale, k * scale * scale
            mu4 = 3.0 * k * (k + 2.0) * scale ** 4
            assert abs(x.getAverage() - mean) <= 4 * math.sqrt(var / n), (shape_per_time, i)
            assert abs(x.getVariance() - var) <= 4 * math.sqrt((mu4 - var * var) / n), (shape_per_time, i)


def test_python_mirror(gpu):
    td = gpu.TimeDiscretization(0.0, 4, 0.25)
    vg = gpu.VarianceGammaProcess(td, 3000, 4711, 0.2, -0.14, 0.2)
    before = gpu.pool_stats().n_kernel_launches
    got = np.stack([vg.increments.getIncrement(i, f).realizations.to_float32() for i in range(4) for f in range(2)])
    assert gpu.pool_stats().n_kernel_launches - before == 1
    laws = [[(GAMMA, td.getTimeStep(i) / 0.2, 0.2), (NORMAL, 1.0, 0.0)] for i in range(4)]
    assert compare(gpu, got, 4711, laws, 3000) == 0
    g, z = got[2].astype(np.float32), got[3].astype(np.float32)
    want = (np.float32(-0.14) * g + np.float32(0.2) * (np.sqrt(g) * z)).astype(np.float32)
    mine = vg.getIncrement(1, 0).realizations.to_float32()
    assert np.allclose(mine, want, rtol=1e-6, atol=1e-7)
    assert vg.getIncrement(1, 0).getFiltrationTime() == 0.5
    part = gpu.VarianceGammaProcess(td, 1999, 4711, 0.2, -0.14, 0.2, None, 1001)
    blk = np.stack([part.increments.getIncrement(i, f).realizations.to_float32() for i in range(4) for f in range(2)])
    assert (blk.view(np.uint32) == got[:, 1001:].view(np.uint32)).all()
    assert vg == vg.getCloneWithModifiedSeed(4711) and vg != vg.getCloneWithModifiedSeed(1) and hash(vg) == hash(vg.getCloneWithModifiedSeed(4711))
    gp = gpu.GammaProcess(td, 3000, 4711, 5.0, 0.2)
    got = np.stack([gp.getIncrement(i, 0).realizations.to_float32() for i in range(4)])
    compare(gpu, got, 4711, [[(GAMMA, 5.0 * td.getTimeStep(i), 0.2)] for i in range(4)], 3000)
    assert isinstance(gp.getCloneWithModifiedTimeDiscretization(gpu.TimeDiscretization(0.0, 2, 0.5)), gpu.GammaProcess)


VG = dict(sigma=0.2, theta=-0.14, nu=0.2)
CALL = dict(initial_value=100.0, risk_free_rate=0.05, maturity=1.0, strike=100.0)


def test_variance_gamma_call_against_the_quadrature(gpu):
    from importlib import import_module
    mc = import_module("finmath-lib-cuda-extensions_amd.montecarlo")
    td = gpu.TimeDiscretization(0.0, 10, 0.1)
    n = 1_000_000
    value, rv = mc.variance_gamma_call_mc(gpu.VarianceGammaProcess(td, n, 3141, **VG), **CALL)
    exact = mc.variance_gamma_call_analytic(100.0, 0.05, VG["sigma"], VG["theta"], VG["nu"], 1.0, 100.0)
    err = rv.getStandardError()
    print(f"variance-gamma call: Monte-Carlo {value!r} +- {err!r}, quadrature {exact!r}")
    assert abs(value - exact) <= 3 * err and 0.005 < err < 0.05
    # θ = 0 and ν as small as the shape cap allows (dt/ν = 1000): the gamma clock is almost the calendar, the model almost Black–Scholes
    nu = max(td.getTimeStep(i) for i in range(10)) / 1000.0
    v0, rv0 = mc.variance_gamma_call_mc(gpu.VarianceGammaProcess(td, n, 3141, 0.2, 0.0, nu), **CALL)
    bs = mc.black_scholes_call_analytic(100.0, 0.05, 0.2, 1.0, 100.0)
    print(f"variance-gamma call, theta 0, nu {nu!r}: Monte-Carlo {v0!r} +- {rv0.getStandardError()!r}, Black-Scholes {bs!r}")
    assert abs(v0 - bs) <= 3 * rv0.getStandardError()


_CHILD = r'''
import hashlib, importlib, json, math, os, sys, threading
sys.path.insert(0, %(root)r)
sys.path.insert(0, os.path.join(%(root)r, "tests"))
import numpy as np
fm = importlib.import_module("finmath-lib-cuda-extensions_amd")
import test_gpu_levy_increments as T
mode = sys.argv[1]
digest = lambda x: hashlib.sha256(np.ascontiguousarray(x).view(np.uint32).tobytes()).hexdigest()
out = {}
if mode == "devices":
    fm.init_devices([0, 0])
else:
    fm.init(0)
if mode == "threads":
    fm.set_thread_engines(True)
if mode == "model":
    mc = importlib.import_module("finmath-lib-cuda-extensions_amd.montecarlo")
    before = fm.pool_stats().n_kernel_launches
    vg = fm.VarianceGammaProcess(fm.TimeDiscretization(0.0, 10, 0.1), 1_000_000, 3141, **T.VG)
    vg.increments.getIncrement(0, 0)
    out["generation_launches"] = fm.pool_stats().n_kernel_launches - before
    value, rv = mc.variance_gamma_call_mc(vg, **T.CALL)
    out["value"] = value.hex()
    out["values"] = digest(rv.realizations.to_float32())
else:
    def cases():
        for name, n, off in T.CHILD_CASES:
            out[f"{name}/{n}/{off}"] = digest(T.generate(fm, 99, T.SHAPES[name][0], n, off))
    if mode == "threads":
        t = threading.Thread(target=cases); t.start(); t.join()
    else:
        cases()
    if mode == "devices":
        kinds, a, b = T.arrays([[(T.GAMMA, 2000.0, 1.0)]])
        out["rc_bad"] = fm._native.lib().fmhip_increments_generate_device(1, 1, 1, 10, 0, *T.pointers(kinds, a, b), (T.C.c_int64 * 1)())
print("RESULT " + json.dumps(out))
fm.shutdown()
'''

CHILD_CASES = [("variance-gamma 40 x 2", 30_011, 0), ("all five laws", 50_021, 7), ("gamma only, a shape per step", 1, 0), ("exponential only 3 x 2", 4_099, 12_345)]


def child(tmp_path, mode, env):
    script = tmp_path / "child.py"
    script.write_text(_CHILD % {"root": ROOT})
    r = subprocess.run([sys.executable, str(script), mode], capture_output=True, text=True, timeout=900, env=dict(os.environ, **env))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return json.loads([line for line in r.stdout.splitlines() if line.startswith("RESULT ")][-1][7:])


def digest(x):
    return hashlib.sha256(np.ascontiguousarray(x).view(np.uint32).tobytes()).hexdigest()


def expected_cases(gpu):
    want = {}
    for name, n, off in CHILD_CASES:
        got = generate(gpu, 99, SHAPES[name][0], n, off)
        compare(gpu, got, 99, SHAPES[name][0], n, off)
        want[f"{name}/{n}/{off}"] = digest(got)
    return want


@pytest.mark.parametrize("env", [{"FMHIP_MT_SEGMENT_LOG2": "9"}, {"FMHIP_MT_SEGMENT_LOG2": "14", "FMHIP_MT_TILE": "0"}, {"FMHIP_MT_SEGMENT_LOG2": "43"}],
                         ids=lambda e: ",".join(f"{k[6:]}={v}" for k, v in e.items()))
def test_bits_do_not_depend_on_segment_length_or_stores(gpu, tmp_path, env):
    assert child(tmp_path, "single", env) == expected_cases(gpu)


@pytest.mark.parametrize("mode", ["devices", "threads"])
def test_device_list_and_thread_engines(gpu, tmp_path, mode):
    out = child(tmp_path, mode, {})
    if mode == "devices":
        assert out.pop("rc_bad") == INVALID
    assert out == expected_cases(gpu)


def test_variance_gamma_value_identical_with_host_drawn_increments(gpu, tmp_path):
    """FMHIP_DEVICE_INCREMENTS=0: the increments are drawn by the host definition and uploaded.  The gamma draws are equal, so the value is
    the same to the last bit (the normal draws one ulp off, which §4.9's contract allows for, are counted over all 2 x 10^7 draws and printed)."""
    device = child(tmp_path, "model", {"FMHIP_DEVICE_INCREMENTS": "1"})
    host_drawn = child(tmp_path, "model", {"FMHIP_DEVICE_INCREMENTS": "0"})
    assert device["generation_launches"] == 1 and host_drawn["generation_launches"] == 0
    td = gpu.TimeDiscretization(0.0, 10, 0.1)
    laws = [[(GAMMA, td.getTimeStep(i) / VG["nu"], VG["nu"]), (NORMAL, 1.0, 0.0)] for i in range(10)]
    n_ulp = compare(gpu, generate(gpu, 3141, laws, 1_000_000), 3141, laws, 1_000_000)
    print(f"variance-gamma call: device {float.fromhex(device['value'])!r}, host-drawn {float.fromhex(host_drawn['value'])!r}; {n_ulp} normal draws one ulp off")
    assert device == dict(host_drawn, generation_launches=1)
