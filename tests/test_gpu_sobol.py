"""fmhip_bm_generate_sobol_device (fm_sobol_bm_kernel in sobol_kernel.hip, sobol_engine.hpp): Brownian increments from
Sobol' points through a Brownian bridge or increment by increment, generated on the device, against the definition —
fmhip_sobol_increments_host (host/sobol.hpp compiled for the host) narrowed to fp32.  EVERY draw is compared and NONE may differ: the host
and the device compile the point, the normal quantile and the bridge node from one text that uses + − × / sqrt and integer operations only.
Tests that need another environment or another engine mode run in a child process."""
import ctypes as C
import importlib
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -5
S0, RATE, SIGMA, MATURITY, STRIKE = 100.0, 0.05, 0.2, 1.0, 100.0          # the Asian call of DESIGN.md §4.12


def generate(fm, seed, randomize, construction, dt, n_factors, n_paths, path_offset=0):
    """[step·n_factors + factor][path] fp32, through the C-ABI."""
    N = fm._native
    dt = np.ascontiguousarray(dt, dtype=np.float64)
    count = dt.size * n_factors
    handles = (C.c_int64 * count)()
    N.check(N.lib().fmhip_bm_generate_sobol_device(seed, randomize, construction, dt.size, n_factors, n_paths, path_offset, dt.ctypes.data_as(C.POINTER(C.c_double)), handles))
    vecs = [fm.DeviceVector(handles[k], n_paths) for k in range(count)]
    return np.stack([v.to_float32() for v in vecs]) if n_paths else np.zeros((count, 0), dtype=np.float32)


def definition(fm, seed, randomize, construction, dt, n_factors, n_paths, path_offset=0):
    dt = np.asarray(dt, dtype=np.float64)
    return fm.sobol_increments(seed, dt, n_factors, n_paths, construction, bool(randomize), path_offset).reshape(dt.size * n_factors, n_paths).astype(np.float32)


def assert_equal(got, want, what):
    assert got.shape == want.shape, what
    differ = got.view(np.uint32) != want.view(np.uint32)
    print(f"{what}: {got.size} draws, {int(differ.sum())} differ")
    assert not differ.any(), f"{what}: {int(differ.sum())} of {got.size} draws differ, first at {np.argwhere(differ)[0].tolist()}"


UNEQUAL = [0.5, 0.01, 1e-3, 2.0, 0.125, 7.0, 0.3]


@pytest.mark.parametrize("construction", [0, 1])
@pytest.mark.parametrize("randomize", [0, 1])
@pytest.mark.parametrize("shape", [(40, 5, 100_003), (200, 5, 1 << 16), (7, 3, 4099), (1, 1, 1000), (64, 1, 1 << 20),
                                   (3, 2, 0), (3, 2, 1), (3, 2, 63), (3, 2, 257)])
def test_every_draw_equals_the_definition(gpu, shape, randomize, construction):
    """40 x 5 is the LMM shape, 200 x 5 its 1000-dimension form, 7 x 3 has unequal time steps; path counts around the edges of a wave and of a
    workgroup."""
    steps, factors, paths = shape
    dt = UNEQUAL if steps == 7 else np.full(steps, 0.25)
    got = generate(gpu, 31415, randomize, construction, dt, factors, paths)
    assert_equal(got, definition(gpu, 31415, randomize, construction, dt, factors, paths), f"{shape} randomize={randomize} construction={construction}")


@pytest.mark.parametrize("construction", [0, 1])
def test_blocks_behind_an_offset_are_slices_of_the_whole(gpu, construction):
    dt = [0.1, 0.4, 0.9, 0.2, 0.3]
    n = 800_000
    whole = generate(gpu, 77, 1, construction, dt, 2, n)
    assert_equal(whole, definition(gpu, 77, 1, construction, dt, 2, n), "whole")
    for offset, count in ((0, 1000), (12_345, 5000), (777_777, 22_223), (255, 2), (256, 1), (799_999, 1)):
        block = generate(gpu, 77, 1, construction, dt, 2, count, offset)
        assert (block.view(np.uint32) == whole[:, offset:offset + count].view(np.uint32)).all(), (offset, count)
    far = (1 << 30) - 5001                                   # the end of the sequence
    assert_equal(generate(gpu, 77, 1, construction, dt, 2, 5000, far), definition(gpu, 77, 1, construction, dt, 2, 5000, far), "far block")


def test_counters_move_as_for_the_mersenne_generator_and_not_on_errors(gpu):
    N = gpu._native
    lib = N.lib()
    dt = (C.c_double * 3)(0.1, 0.2, 0.3)
    out = (C.c_int64 * 6)()

    def counters():
        e = gpu.engine_stats()
        return np.array([gpu.pool_stats().n_kernel_launches, e["kernel_launches"], e["algorithmic_bytes"], e["algorithmic_bytes_written"], gpu.traffic_stats()[0]])

    base = counters()
    assert lib.fmhip_bm_generate_mersenne_device(1, 3, 2, 1000, 0, dt, out) == 0
    for h in out: lib.fmhip_vec_release(h)
    mersenne = counters() - base
    base = counters()
    assert lib.fmhip_bm_generate_sobol_device(1, 1, 1, 3, 2, 1000, 0, dt, out) == 0
    for h in out: lib.fmhip_vec_release(h)
    sobol = counters() - base
    print("mersenne", mersenne.tolist(), "sobol", sobol.tolist())
    assert (sobol == mersenne).all() and sobol[0] == 1 and sobol[2] == 4 * 6 * 1000
    # a block behind an offset: still one launch (no jump-ahead prologue)
    base = counters()
    assert lib.fmhip_bm_generate_sobol_device(1, 1, 1, 3, 2, 1000, 12_345, dt, out) == 0
    for h in out: lib.fmhip_vec_release(h)
    assert (counters() - base)[0] == 1

    live = gpu.pool_stats().n_live_vectors
    base = counters()
    bad_dt, nan_dt, zero_dt = (C.c_double * 3)(0.1, -0.2, 0.3), (C.c_double * 3)(0.1, float("nan"), 0.3), (C.c_double * 3)(0.1, 0.0, 0.3)
    null_d, null_v = C.POINTER(C.c_double)(), C.POINTER(C.c_int64)()
    calls = [(1, 1, 1, 0, 2, 10, 0, dt, out), (1, 1, 1, 3, 0, 10, 0, dt, out), (1, 1, 1, 3, 2, -1, 0, dt, out), (1, 1, 1, 3, 2, 10, -1, dt, out),
             (1, 2, 1, 3, 2, 10, 0, dt, out), (1, -1, 1, 3, 2, 10, 0, dt, out), (1, 1, 2, 3, 2, 10, 0, dt, out), (1, 1, -1, 3, 2, 10, 0, dt, out),
             (1, 1, 1, 3, 2, 10, 0, null_d, out), (1, 1, 1, 3, 2, 10, 0, dt, null_v), (1, 1, 1, 3, 2, 10, 0, bad_dt, out), (1, 1, 0, 3, 2, 10, 0, bad_dt, out),
             (1, 1, 1, 3, 2, 10, 0, nan_dt, out), (1, 1, 0, 3, 2, 10, 0, nan_dt, out), (1, 1, 1, 3, 2, 10, 0, zero_dt, out),
             (1, 1, 1, 3, 2, 10, (1 << 30) - 10, dt, out), (1, 1, 1, 3, 2, 1 << 30, 0, dt, out), (1, 1, 1, 3, 342, 10, 0, dt, out)]
    for args in calls:
        assert lib.fmhip_bm_generate_sobol_device(*args) == INVALID, args[:7]
        assert lib.fmhip_last_error()
    assert (counters() == base).all() and gpu.pool_stats().n_live_vectors == live
    assert lib.fmhip_bm_generate_sobol_device(1, 1, 0, 3, 2, 10, 0, zero_dt, out) == 0          # a zero step is an increment of zero without a bridge
    for h in out: lib.fmhip_vec_release(h)
    assert lib.fmhip_bm_generate_sobol_device(1, 1, 1, 3, 2, 10, (1 << 30) - 11, dt, out) == 0   # the last path that fits
    for h in out: lib.fmhip_vec_release(h)


def pseudo_random_standard_error(fm, mc, td, n, payoff):
    bm = fm.BrownianMotionFromMersenneRandomNumbers(td, 1, n, 1)
    value, rv = payoff(bm)
    return value, math.sqrt(rv.getSampleVariance() / n)


def test_asian_call_with_a_bridge_beats_pseudo_random_by_five(gpu):
    """64 steps, 2^20 paths, bridge, seed 1: the error against the closed form is at most 1/5 of the pseudo-random standard error at the same
    N, computed here from the same payoff under BrownianMotionFromMersenneRandomNumbers.  The price with FMHIP_DEVICE_SOBOL=0 is the same
    to the last bit."""
    mc = importlib.import_module("finmath-lib-cuda-extensions_amd.montecarlo")
    n = 1 << 20
    td = gpu.TimeDiscretization(0.0, 64, 1.0 / 64)
    exact = mc.geometric_asian_call_analytic(S0, RATE, SIGMA, [td.getTime(k + 1) for k in range(64)], STRIKE)
    payoff = lambda bm: mc.geometric_asian_call_mc(bm, S0, RATE, SIGMA, MATURITY, STRIKE)
    pseudo, se = pseudo_random_standard_error(gpu, mc, td, n, payoff)
    prices = {}
    try:
        for knob in ("1", "0"):
            os.environ["FMHIP_DEVICE_SOBOL"] = knob
            before = gpu.pool_stats().n_kernel_launches
            prices[knob] = payoff(gpu.BrownianMotionFromSobolSequence(td, 1, n, 1))[0]
            assert gpu.pool_stats().n_kernel_launches > before
    finally:
        os.environ.pop("FMHIP_DEVICE_SOBOL", None)
    incremental = payoff(gpu.BrownianMotionFromSobolSequence(td, 1, n, 1, construction="incremental"))[0]
    print(f"closed form {exact!r}; Sobol' bridge {prices['1']!r} (error {prices['1'] - exact:.3e}); host path {prices['0']!r}; "
          f"incremental error {incremental - exact:.3e}; pseudo-random {pseudo!r} (error {pseudo - exact:.3e}, standard error {se:.3e}); gate {se / 5:.3e}")
    assert abs(exact - 5.620434) < 1e-6 and 5e-3 < se < 1e-2
    assert prices["1"] == prices["0"]
    assert abs(prices["1"] - exact) <= se / 5


def test_black_scholes_call_is_closer_than_with_the_mersenne_class(gpu):
    """black_scholes_call_mc fed the new class (10 steps, README's parameters, 2^20 paths) against the Mersenne class at the same N."""
    mc = importlib.import_module("finmath-lib-cuda-extensions_amd.montecarlo")
    n = 1 << 20
    td = gpu.TimeDiscretization(0.0, 10, 0.1)
    args = (100.0, 0.05, 0.2, 1.0, 105.0)
    exact = mc.black_scholes_call_analytic(*args)
    sobol = mc.black_scholes_call_mc(gpu.BrownianMotionFromSobolSequence(td, 1, n, 1), *args)[0]
    mersenne = mc.black_scholes_call_mc(gpu.BrownianMotionFromMersenneRandomNumbers(td, 1, n, 1), *args)[0]
    print(f"closed form {exact!r}; Sobol' {sobol!r} (error {sobol - exact:.3e}); Mersenne {mersenne!r} (error {mersenne - exact:.3e})")
    assert abs(sobol - exact) < abs(mersenne - exact)


def test_python_mirror(gpu):
    td = gpu.TimeDiscretization([0.0, 0.5, 0.6, 2.0])
    steps = [td.getTimeStep(i) for i in range(3)]
    want = gpu.sobol_increments(4711, steps, 2, 3000, "bridge").astype(np.float32).reshape(6, 3000)
    got = {}
    try:
        for knob in ("1", "0"):
            os.environ["FMHIP_DEVICE_SOBOL"] = knob
            before = gpu.pool_stats().n_kernel_launches
            bm = gpu.BrownianMotionFromSobolSequence(td, 2, 3000, 4711)
            got[knob] = np.stack([bm.getBrownianIncrement(i, f).realizations.to_float32() for i in range(3) for f in range(2)])
            assert (gpu.pool_stats().n_kernel_launches - before >= 1) == (knob == "1")
            part = gpu.BrownianMotionFromSobolSequence(td, 2, 1999, 4711, path_offset=1001)
            blk = np.stack([part.getBrownianIncrement(i, f).realizations.to_float32() for i in range(3) for f in range(2)])
            assert (blk.view(np.uint32) == got[knob][:, 1001:].view(np.uint32)).all()
            clone = bm.getCloneWithModifiedSeed(5)
            assert isinstance(clone, gpu.BrownianMotionFromSobolSequence) and clone.construction == bm.construction and clone.getSeed() == 5
            assert bm.getBrownianIncrement(2, 1).getFiltrationTime() == 2.0
            other = bm.getCloneWithModifiedTimeDiscretization(gpu.TimeDiscretization(0.0, 2, 0.5))
            assert isinstance(other, gpu.BrownianMotionFromSobolSequence) and other.getTimeDiscretization().getNumberOfTimeSteps() == 2
    finally:
        os.environ.pop("FMHIP_DEVICE_SOBOL", None)
    assert (got["1"].view(np.uint32) == want.view(np.uint32)).all() and (got["0"].view(np.uint32) == want.view(np.uint32)).all()
    plain = gpu.BrownianMotionFromSobolSequence(td, 2, 100, 4711, construction="incremental", randomize=False)
    assert (plain.getBrownianIncrement(0, 0).realizations.to_float32().view(np.uint32)
            == gpu.sobol_increments(0, steps, 2, 100, "incremental", False).astype(np.float32)[0, 0].view(np.uint32)).all()


_OTHER_MODES = r'''
import importlib, json, os, sys, threading
sys.path.insert(0, %(root)r)
import numpy as np
import ctypes as C
fm = importlib.import_module("finmath-lib-cuda-extensions_amd")
mode = sys.argv[1]
N = fm._native

def gen(seed, construction, dt, nf, n, off=0):
    dt = np.ascontiguousarray(dt, dtype=np.float64)
    handles = (C.c_int64 * (dt.size * nf))()
    N.check(N.lib().fmhip_bm_generate_sobol_device(seed, 1, construction, dt.size, nf, n, off, dt.ctypes.data_as(C.POINTER(C.c_double)), handles))
    return np.stack([fm.DeviceVector(h, n).to_float32() for h in handles])

dt = [0.1, 0.4, 0.9]
out = {}
if mode == "devices":
    fm.init_devices([0, 0])
    for c in (0, 1):
        for n, off in ((100_003, 0), (1, 0), (20_001, 7)):
            out[f"{c}/{n}/{off}"] = gen(99, c, dt, 2, n, off).view(np.uint32).tolist()
    bad = (C.c_int64 * 6)()
    out["rc_bad"] = N.lib().fmhip_bm_generate_sobol_device(99, 1, 7, 3, 2, 10, 0, (C.c_double * 3)(*dt), bad)
else:
    fm.init(0)
    fm.set_thread_engines(True)
    def other():
        for c in (0, 1): out[f"{c}/100003/0"] = gen(99, c, dt, 2, 100_003).view(np.uint32).tolist()     # on this thread's own engine
    t = threading.Thread(target=other); t.start(); t.join()
    for c in (0, 1):
        out[f"{c}/1/0"] = gen(99, c, dt, 2, 1).view(np.uint32).tolist()
        out[f"{c}/20001/7"] = gen(99, c, dt, 2, 20_001, 7).view(np.uint32).tolist()
    out["rc_bad"] = 1
print("RESULT " + json.dumps(out))
fm.shutdown()
'''


@pytest.mark.parametrize("mode", ["devices", "threads"])
def test_device_list_and_thread_engines(gpu, mode, tmp_path):
    """A device list {0, 0}: the front checks once, every shard generates its own block at its own offset; thread engines: a second thread
    generates on its own engine.  In a process of its own, under a time limit; compared with the definition."""
    script = tmp_path / "modes.py"
    script.write_text(_OTHER_MODES % {"root": ROOT})
    r = subprocess.run([sys.executable, str(script), mode], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = json.loads([line for line in r.stdout.splitlines() if line.startswith("RESULT ")][-1][7:])
    assert out["rc_bad"] != 0
    dt = [0.1, 0.4, 0.9]
    for c in (0, 1):
        for n, off in ((100_003, 0), (1, 0), (20_001, 7)):
            want = definition(gpu, 99, 1, c, dt, 2, n, off)
            assert (np.array(out[f"{c}/{n}/{off}"], dtype=np.uint32).reshape(want.shape) == want.view(np.uint32)).all(), (mode, c, n, off)
