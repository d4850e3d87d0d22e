"""fmhip_increments_generate_device (fm_mt_icdf_kernel in mt_bm_kernel.hip, increments_device_engine.hpp): increments with a
law per (time step, factor) generated on the device from finmath-lib's MT19937 stream, against the definition — fmhip_increments_host
(one host core, host/increments.hpp) narrowed to fp32.  Every draw is compared.

The contract: Poisson and uniform streams are EQUAL (the device only compares the uniform with the host's table, or multiplies and
adds); normal streams obey the contract of mt_bm_kernel.hip (a central draw equal, a tail draw at most one fp32 ulp off, and no more than
a handful in 10^8 are) — `compare` enforces exactly that and returns the number of such draws.  An all-normal call equals
fmhip_bm_generate_mersenne_device bit for bit.  Tests that need another environment or another engine mode run in a child process."""
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
CENTRAL = 1.4395                      # |z| below this is a central draw for sure (the branch point is Φ⁻¹(0.925) = 1.43953…)
NORMAL, UNIFORM, POISSON = 0, 1, 2
INVALID = -5                          # FMHIP_ERR_INVALID_ARGUMENT


def arrays(laws):
    """laws: [step][factor] of (kind, a, b) → the three flat arrays of the C-ABI"""
    flat = [law for row in laws for law in row]
    return (np.array([k for k, _, _ in flat], dtype=np.int32), np.array([a for _, a, _ in flat], dtype=np.float64),
            np.array([b for _, _, b in flat], dtype=np.float64))


def pointers(kinds, a, b):
    return kinds.ctypes.data_as(C.POINTER(C.c_int32)), a.ctypes.data_as(C.POINTER(C.c_double)), b.ctypes.data_as(C.POINTER(C.c_double))


def generate(fm, seed, laws, n_paths, path_offset=0):
    """[step·n_factors + factor][path] fp32, through the C-ABI."""
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
    """Poisson and uniform streams equal; normal streams under the contract.  Returns the number of normal tail draws one ulp off."""
    kinds, a, _ = arrays(laws)
    want64 = host(fm, seed, laws, n_paths, path_offset)
    want = want64.astype(np.float32)
    assert got.shape == want.shape
    differ = got.view(np.uint32) != want.view(np.uint32)
    exact = kinds != NORMAL
    assert not differ[exact].any(), f"{differ[exact].sum()} Poisson or uniform draws differ"
    if not differ.any():
        return 0
    scale = np.where(a > 0, a, 1.0)[:, None]
    central = np.abs(want64) / scale < CENTRAL
    assert not (differ & central).any(), f"{(differ & central).sum()} central normal draws differ"
    ulps = np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))[differ]
    assert ulps.max() == 1, f"a tail draw differs by {ulps.max()} fp32 ulps"
    assert differ.sum() <= 2 + got.size * 1e-7, f"{differ.sum()} of {got.size} draws differ by one ulp"
    return int(differ.sum())


def merton_laws(steps, dt, intensity):
    return [[(NORMAL, math.sqrt(dt), 0.0), (NORMAL, 1.0, 0.0), (POISSON, intensity * dt, 0.0)] for _ in range(steps)]


def mirror_merton_laws(td, intensity):
    """as merton_increments states them: the time steps are differences of the times"""
    steps = [td.getTimeStep(i) for i in range(td.getNumberOfTimeSteps())]
    return [[(NORMAL, math.sqrt(dt), 0.0), (NORMAL, 1.0, 0.0), (POISSON, intensity * dt, 0.0)] for dt in steps]


def poisson_laws(steps, means):
    return [[(POISSON, m, 0.0) for m in means] for _ in range(steps)]


SHAPES = {
    "merton 40 x 3": (merton_laws(40, 0.125, 1.5), 100_003),
    "poisson 5 x 2": (poisson_laws(5, [0.02, 30.0]), 100_003),
    "poisson 1 x 1": (poisson_laws(1, [1.0]), 100_003),
    "poisson 1 x 1, mean 128": (poisson_laws(1, [128.0]), 50_000),
    "poisson 1 x 1, mean 0": (poisson_laws(1, [0.0]), 5_000),
    "uniform and poisson 3 x 2": ([[(UNIFORM, -1.0, 3.0), (POISSON, 2.5 * (i + 1), 0.0)] for i in range(3)], 20_011),
    "mixed 301 x 3 (element-wise stores)": ([[(NORMAL, 0.5, 0.0), (UNIFORM, 0.0, 1.0), (POISSON, 0.01 * (i + 1), 0.0)] for i in range(301)], 50),
    "a mean per step: 60 tables": ([[(POISSON, 0.5 + 2.0 * i, 0.0)] for i in range(60)], 4_099),
    "uniform 2 x 1 degenerate": ([[(UNIFORM, 2.0, 2.0)], [(UNIFORM, -1e300, 1e300)]], 1_000),
}


@pytest.mark.parametrize("name", list(SHAPES))
def test_shapes_against_the_host_definition(gpu, name):
    laws, n = SHAPES[name]
    got = generate(gpu, 31415, laws, n)
    n_ulp = compare(gpu, got, 31415, laws, n)
    print(f"{name}: {got.size} draws, {n_ulp} normal tail draws one fp32 ulp off")
    if name == "poisson 1 x 1, mean 0":
        assert (got == 0).all()


@pytest.mark.parametrize("n", [0, 1, 3, 100_003, 1 << 20])
def test_path_counts(gpu, n):
    laws = [[(NORMAL, 0.5, 0.0), (POISSON, 0.3, 0.0)], [(UNIFORM, 1.0, 2.0), (POISSON, 7.0, 0.0)]]
    for seed in (0, -1):
        got = generate(gpu, seed, laws, n)
        assert got.shape == (4, n)
        compare(gpu, got, seed, laws, n)


def test_all_normal_equals_the_brownian_kernel(gpu):
    N = gpu._native
    dt = np.array([0.5, 0.0, 1e-3, 2.0, 0.125])
    n, factors = 60_013, 3
    laws = [[(NORMAL, math.sqrt(v), 0.0)] * factors for v in dt]
    got = generate(gpu, 1234, laws, n, 17)
    handles = (C.c_int64 * (dt.size * factors))()
    N.check(N.lib().fmhip_bm_generate_mersenne_device(1234, dt.size, factors, n, 17, dt.ctypes.data_as(C.POINTER(C.c_double)), handles))
    bm = np.stack([gpu.DeviceVector(h, n).to_float32() for h in handles])
    assert (got.view(np.uint32) == bm.view(np.uint32)).all()
    compare(gpu, got, 1234, laws, n, 17)


def test_path_offset_blocks_are_slices_of_the_whole(gpu):
    laws = merton_laws(4, 0.25, 2.0)
    n = 800_000
    whole = generate(gpu, 77, laws, n)
    compare(gpu, whole, 77, laws, n)
    for off, cnt in ((0, 5_000), (12_345, 5_001), (777_777, 22_223), (1, 1), (799_999, 1)):
        block = generate(gpu, 77, laws, cnt, off)
        assert (block.view(np.uint32) == whole[:, off:off + cnt].view(np.uint32)).all(), off


def test_argument_errors_launch_nothing(gpu):
    lib = gpu._native.lib()
    out = (C.c_int64 * 6)()
    before = gpu.engine_stats()
    launches = gpu.pool_stats().n_kernel_launches
    live = gpu.pool_stats().n_live_vectors
    nan, inf = float("nan"), float("inf")

    def call(laws, n_paths=10, path_offset=0, steps=None, factors=None, out_ptr=out):
        kinds, a, b = arrays(laws)
        return lib.fmhip_increments_generate_device(1, len(laws) if steps is None else steps, len(laws[0]) if factors is None else factors,
                                                    n_paths, path_offset, *pointers(kinds, a, b), out_ptr)
    ok = [[(NORMAL, 1.0, 0.0), (UNIFORM, 0.0, 1.0), (POISSON, 1.0, 0.0)]]
    bad = [
        [[(3, 1.0, 0.0)]], [[(-1, 1.0, 0.0)]],
        [[(NORMAL, -1.0, 0.0)]], [[(NORMAL, nan, 0.0)]], [[(POISSON, -0.5, 0.0)]], [[(POISSON, nan, 0.0)]], [[(POISSON, 128.5, 0.0)]], [[(POISSON, inf, 0.0)]],
        [[(UNIFORM, 2.0, 1.0)]], [[(UNIFORM, 0.0, inf)]], [[(UNIFORM, -inf, 0.0)]], [[(UNIFORM, nan, 1.0)]],
        [[(POISSON, 100.0 + 1e-3 * i, 0.0)] for i in range(400)],                      # 400 tables of some 250 entries: more than 2^16 doubles
    ]
    for laws in bad:
        assert call(laws) == INVALID, laws[0]
        assert lib.fmhip_last_error()
    assert call(ok, n_paths=-1) == INVALID and call(ok, path_offset=-1) == INVALID and call(ok, steps=0) == INVALID and call(ok, factors=0) == INVALID
    assert call(ok, out_ptr=C.POINTER(C.c_int64)()) == INVALID
    assert call(ok, path_offset=(1 << 44) // 6) == INVALID                              # the last word would lie beyond 2^44
    assert call(ok, steps=1 << 20, factors=1 << 5, n_paths=1) == INVALID                # more than 2^24 laws (the count is checked before a law is read)
    after = gpu.engine_stats()
    assert after == before and gpu.pool_stats().n_kernel_launches == launches
    assert call(ok, path_offset=(1 << 44) // 6 - 10) == 0                               # the last paths that fit
    for h in list(out)[:3]:
        lib.fmhip_vec_release(h)
    assert gpu.pool_stats().n_kernel_launches - launches == 2                           # one jump, one generation
    assert gpu.pool_stats().n_live_vectors == live


def test_python_mirror(gpu):
    td = gpu.TimeDiscretization(0.0, 4, 0.25)
    inc = gpu.merton_increments(td, 3000, 4711, 2.0)
    laws = merton_laws(4, 0.25, 2.0)
    before = gpu.pool_stats().n_kernel_launches
    got = np.stack([inc.getIncrement(i, f).realizations.to_float32() for i in range(4) for f in range(3)])
    assert gpu.pool_stats().n_kernel_launches - before == 1
    assert compare(gpu, got, 4711, laws, 3000) == 0
    assert inc.getIncrement(2, 1).getFiltrationTime() == 0.75
    part = gpu.merton_increments(td, 1999, 4711, 2.0, None, 1001)
    blk = np.stack([part.getIncrement(i, f).realizations.to_float32() for i in range(4) for f in range(3)])
    assert (blk.view(np.uint32) == got[:, 1001:].view(np.uint32)).all()
    jumps = gpu.JumpProcessIncrements(td, [2.0, 40.0], 3000, 4711)
    got = np.stack([jumps.getIncrement(i, f).realizations.to_float32() for i in range(4) for f in range(2)])
    compare(gpu, got, 4711, poisson_laws(4, [0.5, 10.0]), 3000)
    assert jumps == jumps.getCloneWithModifiedSeed(4711) and jumps != jumps.getCloneWithModifiedSeed(1) and hash(jumps) == hash(jumps.getCloneWithModifiedSeed(4711))
    assert isinstance(jumps.getCloneWithModifiedTimeDiscretization(gpu.TimeDiscretization(0.0, 2, 0.5)), gpu.JumpProcessIncrements)


MERTON = dict(initial_value=100.0, risk_free_rate=0.05, volatility=0.2, jump_intensity=1.0, jump_size_mean=-0.1, jump_size_stddev=0.15, maturity=1.0, strike=100.0)


def test_merton_call_against_the_series(gpu):
    from importlib import import_module
    mc = import_module("finmath-lib-cuda-extensions_amd.montecarlo")
    td = gpu.TimeDiscretization(0.0, 10, 0.1)
    n = 1_000_000
    inc = gpu.merton_increments(td, n, 3141, MERTON["jump_intensity"])
    value, rv = mc.merton_call_mc(inc, **MERTON)
    exact = mc.merton_call_analytic(**MERTON)
    err = rv.getStandardError()
    print(f"Merton call: Monte-Carlo {value!r} +- {err!r}, series {exact!r}")
    assert abs(value - exact) <= 3 * err and 0.005 < err < 0.05
    # no jumps: the Black–Scholes driver fed the same increments, operation for operation
    calm = gpu.merton_increments(td, n, 3141, 0.0)
    no_jumps = dict(MERTON, jump_intensity=0.0)
    v0, rv0 = mc.merton_call_mc(calm, **no_jumps)
    assert (calm.getIncrement(3, 2).realizations.to_float32() == 0).all()
    vbs, rvbs = mc.black_scholes_call_mc(calm, 100.0, 0.05, 0.2, 1.0, 100.0)
    assert v0 == vbs and (rv0.realizations.to_float32().view(np.uint32) == rvbs.realizations.to_float32().view(np.uint32)).all()
    assert abs(v0 - mc.black_scholes_call_analytic(100.0, 0.05, 0.2, 1.0, 100.0)) <= 3 * rv0.getStandardError()


_CHILD = r'''
import hashlib, importlib, json, math, os, sys, threading
sys.path.insert(0, %(root)r)
sys.path.insert(0, os.path.join(%(root)r, "tests"))
import numpy as np
fm = importlib.import_module("finmath-lib-cuda-extensions_amd")
import test_gpu_increments as T
mode = sys.argv[1]
digest = lambda x: hashlib.sha256(np.ascontiguousarray(x).view(np.uint32).tobytes()).hexdigest()
out = {}
if mode == "devices":
    fm.init_devices([0, 0])
else:
    fm.init(0)
if mode == "threads":
    fm.set_thread_engines(True)
if mode == "merton":
    mc = importlib.import_module("finmath-lib-cuda-extensions_amd.montecarlo")
    before = fm.pool_stats().n_kernel_launches
    inc = fm.merton_increments(fm.TimeDiscretization(0.0, 10, 0.1), 1_000_000, 3141, T.MERTON["jump_intensity"])
    inc.getIncrement(0, 0)
    out["generation_launches"] = fm.pool_stats().n_kernel_launches - before
    value, rv = mc.merton_call_mc(inc, **T.MERTON)
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
        kinds, a, b = T.arrays([[(T.POISSON, 200.0, 0.0)]])
        out["rc_bad"] = fm._native.lib().fmhip_increments_generate_device(1, 1, 1, 10, 0, *T.pointers(kinds, a, b), (T.C.c_int64 * 1)())
print("RESULT " + json.dumps(out))
fm.shutdown()
'''

CHILD_CASES = [("merton 40 x 3", 30_011, 0), ("uniform and poisson 3 x 2", 100_003, 7), ("poisson 5 x 2", 1, 0), ("a mean per step: 60 tables", 4_099, 12_345)]


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


@pytest.mark.parametrize("env", [{"FMHIP_MT_SEGMENT_LOG2": "9"}, {"FMHIP_MT_SEGMENT_LOG2": "14", "FMHIP_MT_TILE": "0"}, {"FMHIP_MT_SEGMENT_LOG2": "43"},
                                 {"FMHIP_ICDF_LINEAR_MAX": "0"}, {"FMHIP_ICDF_LINEAR_MAX": "512"}], ids=lambda e: ",".join(f"{k[6:]}={v}" for k, v in e.items()))
def test_bits_do_not_depend_on_segment_length_stores_or_search(gpu, tmp_path, env):
    """Segments of 512 words (most workgroups own one path or none), one workgroup for everything, element-wise stores, every Poisson
    table bisected, every table walked from 0: the same bits."""
    assert child(tmp_path, "single", env) == expected_cases(gpu)


@pytest.mark.parametrize("mode", ["devices", "threads"])
def test_device_list_and_thread_engines(gpu, tmp_path, mode):
    """A device list {0, 0}: every shard generates its own block of paths, the front's vectors are the whole; thread engines: a second thread
    generates on its own engine.  In a process of its own; compared with this process's single engine."""
    out = child(tmp_path, mode, {})
    if mode == "devices":
        assert out.pop("rc_bad") == INVALID
    assert out == expected_cases(gpu)


def test_merton_value_identical_with_host_drawn_increments(gpu, tmp_path):
    """FMHIP_DEVICE_INCREMENTS=0: the increments are drawn by the host definition and uploaded; the value is the same to the last bit
    whenever no normal tail draw is one ulp off (counted here over all 3 x 10^7 draws)."""
    device = child(tmp_path, "merton", {"FMHIP_DEVICE_INCREMENTS": "1"})
    host_drawn = child(tmp_path, "merton", {"FMHIP_DEVICE_INCREMENTS": "0"})
    assert device["generation_launches"] == 1 and host_drawn["generation_launches"] == 0
    laws = mirror_merton_laws(gpu.TimeDiscretization(0.0, 10, 0.1), MERTON["jump_intensity"])
    n_ulp = compare(gpu, generate(gpu, 3141, laws, 1_000_000), 3141, laws, 1_000_000)
    print(f"Merton call: device {float.fromhex(device['value'])!r}, host-drawn {float.fromhex(host_drawn['value'])!r}; {n_ulp} draws one ulp off")
    if n_ulp == 0:
        assert device == dict(host_drawn, generation_launches=1)
    else:
        assert abs(float.fromhex(device["value"]) - float.fromhex(host_drawn["value"])) <= 1e-9 * n_ulp * abs(float.fromhex(host_drawn["value"]))
