"""fmhip_bm_generate_mersenne_device (mt_bm_kernel.hip, mersenne_device_engine.hpp): finmath-lib's Mersenne-Twister
Brownian increments generated on the device, against the definition — fmhip_mersenne_increments (one host core) narrowed to fp32.

The contract: the uniforms are the host's bit for bit; a draw with |u − 0.5| <= 0.425 goes through + − × / only and is EQUAL; a tail draw
goes through log, where the device library and glibc may differ by an fp64 ulp, so a tail draw may differ by ONE fp32 ulp, and no more
than a handful in 10^8 do.  `compare` enforces exactly that and returns the number of such draws, which the tests print."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CENTRAL = 1.4395                      # |z| below this is a central draw for sure (the branch point is Φ⁻¹(0.925) = 1.43953…)


def generate(fm, seed, dt, n_factors, n_paths, path_offset=0):
    """[step·n_factors + factor][path] fp32, through the C-ABI."""
    N = fm._native
    dt = np.ascontiguousarray(dt, dtype=np.float64)
    count = dt.size * n_factors
    handles = (C.c_int64 * count)()
    N.check(N.lib().fmhip_bm_generate_mersenne_device(seed, dt.size, n_factors, n_paths, path_offset, dt.ctypes.data_as(C.POINTER(C.c_double)), handles))
    vecs = [fm.DeviceVector(handles[k], n_paths) for k in range(count)]
    return np.stack([v.to_float32() for v in vecs]) if n_paths else np.zeros((count, 0), dtype=np.float32)


def compare(fm, got, seed, dt, n_factors, n_paths, path_offset=0):
    dt = np.asarray(dt, dtype=np.float64)
    host = fm.mersenne_increments(seed, dt, n_factors, path_offset + n_paths)[:, :, path_offset:].reshape(dt.size * n_factors, n_paths)
    want = host.astype(np.float32)
    assert got.shape == want.shape
    differ = got.view(np.uint32) != want.view(np.uint32)
    if not differ.any():
        return 0
    sq = np.repeat(np.sqrt(dt), n_factors)[:, None]
    unit = np.abs(host) / np.where(sq > 0, sq, 1.0)
    assert not (differ & (unit < CENTRAL)).any(), f"{(differ & (unit < CENTRAL)).sum()} central draws differ"
    ulps = np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))[differ]
    assert ulps.max() == 1, f"a tail draw differs by {ulps.max()} fp32 ulps"
    assert differ.sum() <= 2 + got.size * 1e-7, f"{differ.sum()} of {got.size} draws differ by one ulp"
    return int(differ.sum())


@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 1, 311), (1, 1, 312), (1, 1, 313), (3, 2, 1000), (1, 1, 16385), (7, 3, 4099),
                                   (40, 5, 100_003), (2, 1, (1 << 24) + 3), (301, 3, 50), (1000, 1, 37)])
def test_shapes_against_the_host_generator(gpu, shape):
    """Block edges of the twister (312 draws), of a segment, of a store tile; 40 x 5 is the LMM shape, 903 and 1000 vectors are too large
    for a store tile of four paths (element-wise stores)."""
    steps, factors, paths = shape
    dt = np.full(steps, 0.25)
    got = generate(gpu, 31415, dt, factors, paths)
    n_ulp = compare(gpu, got, 31415, dt, factors, paths)
    print(f"{shape}: {got.size} draws, {n_ulp} tail draws one fp32 ulp off")


@pytest.mark.parametrize("seed", [0, 1, 1234, -1, -2147483648, 2147483647])
def test_seeds_and_non_uniform_steps(gpu, seed):
    dt = np.array([0.5, 0.0, 1e-3, 2.0, 0.125, 7.0])
    got = generate(gpu, seed, dt, 3, 20_011)
    compare(gpu, got, seed, dt, 3, 20_011)
    assert (got[3:6] == 0).all()                         # dt = 0: zeros (of either sign, as on the host — compare() looked at the bits)


def test_path_offset_blocks_concatenate_to_the_whole(gpu):
    dt = np.array([0.1, 0.2, 0.3])
    n = 50_021
    whole = generate(gpu, 77, dt, 2, n)
    compare(gpu, whole, 77, dt, 2, n)
    cuts = [0, 1, 3, 4, 1001, 1002, 16_387, 30_000, n]   # offsets that are no multiple of 4, blocks of one path
    blocks = [generate(gpu, 77, dt, 2, b - a, a) for a, b in zip(cuts, cuts[1:])]
    assert (np.concatenate(blocks, axis=1).view(np.uint32) == whole.view(np.uint32)).all()
    # far into the stream: 2^30 paths in front, checked by composition (two jumps against one) and against the neighbouring block
    far = 1 << 30
    a = generate(gpu, 77, dt, 2, 2000, far)
    b = generate(gpu, 77, dt, 2, 1000, far + 1000)
    assert (a[:, 1000:].view(np.uint32) == b.view(np.uint32)).all()
    assert generate(gpu, 77, dt, 2, 0, 5).shape == (6, 0)


def test_result_does_not_depend_on_the_segment_length(gpu):
    dt = np.full(5, 0.5)
    n = 30_011                                           # 5 x 2 x 30011 draws = 600 220 words
    want = generate(gpu, -5, dt, 2, n)
    compare(gpu, want, -5, dt, 2, n)
    try:
        for j in (1, 5, 10, 11, 14, 17, 20, 30, 43):     # j = 1 … 5: most workgroups own no path; 20 on: one workgroup
            os.environ["FMHIP_MT_SEGMENT_LOG2"] = str(j)
            if (2 * 10 * n) >> j > 1 << 20:
                with pytest.raises(Exception):
                    generate(gpu, -5, dt, 2, n)
                continue
            got = generate(gpu, -5, dt, 2, n)
            assert (got.view(np.uint32) == want.view(np.uint32)).all(), f"segment length 2^{j}"
        os.environ["FMHIP_MT_SEGMENT_LOG2"] = "15"
        os.environ["FMHIP_MT_TILE"] = "0"                # element-wise stores write the same numbers
        assert (generate(gpu, -5, dt, 2, n).view(np.uint32) == want.view(np.uint32)).all()
    finally:
        os.environ.pop("FMHIP_MT_SEGMENT_LOG2", None)
        os.environ.pop("FMHIP_MT_TILE", None)


def test_argument_errors_launch_nothing(gpu):
    N = gpu._native
    lib = N.lib()
    dt = (C.c_double * 3)(0.1, 0.2, 0.3)
    bad_dt = (C.c_double * 3)(0.1, -0.2, 0.3)
    nan_dt = (C.c_double * 3)(0.1, float("nan"), 0.3)
    out = (C.c_int64 * 6)()
    before = gpu.pool_stats().n_kernel_launches
    live = gpu.pool_stats().n_live_vectors
    INVALID = -5                                          # FMHIP_ERR_INVALID_ARGUMENT
    null_d, null_v = C.POINTER(C.c_double)(), C.POINTER(C.c_int64)()
    calls = [
        (1, 0, 2, 10, 0, dt, out), (1, 3, 0, 10, 0, dt, out), (1, -1, 2, 10, 0, dt, out), (1, 3, 2, -1, 0, dt, out), (1, 3, 2, 10, -1, dt, out),
        (1, 3, 2, (1 << 31) + 1, 0, dt, out), (1, 3, 2, 10, 0, null_d, out), (1, 3, 2, 10, 0, dt, null_v), (1, 3, 2, 10, 0, bad_dt, out), (1, 3, 2, 10, 0, nan_dt, out),
        (1, 3, 2, 10, (1 << 44) // 12, dt, out),          # the last word would lie beyond 2^44
        (1, 3, 2, 10, 1 << 62, dt, out),
        (1, 1 << 20, 1 << 5, 1, 0, dt, out),              # more than 2^24 increments per path (dt is not read that far: the count is checked first)
    ]
    for args in calls:
        rc = lib.fmhip_bm_generate_mersenne_device(*args)
        assert rc == INVALID, args[:5]
    assert lib.fmhip_bm_generate_mersenne_device(1, 3, 2, 10, (1 << 44) // 12 - 10, dt, out) == 0      # the last path that fits
    for h in out:
        lib.fmhip_vec_release(h)
    after = gpu.pool_stats()
    assert after.n_kernel_launches - before == 2          # the accepted call alone: one jump, one generation
    assert after.n_live_vectors == live


def test_python_mirror_with_the_knob_on_and_off(gpu):
    td = gpu.TimeDiscretization(0.0, 4, 0.25)
    host = gpu.mersenne_increments(4711, [0.25] * 4, 2, 3000).astype(np.float32)
    got = {}
    try:
        for knob in ("1", "0"):
            os.environ["FMHIP_DEVICE_MERSENNE"] = knob
            before = gpu.pool_stats().n_kernel_launches
            bm = gpu.BrownianMotionFromMersenneRandomNumbers(td, 2, 3000, 4711)
            got[knob] = np.stack([bm.getBrownianIncrement(i, f).realizations.to_float32() for i in range(4) for f in range(2)])
            assert (gpu.pool_stats().n_kernel_launches - before >= 1) == (knob == "1")      # the device path launches, the host path uploads
            # a rank's block (parallel.py): paths 1001 … 3000 of the same motion, on either path
            part = gpu.BrownianMotionFromMersenneRandomNumbers(td, 2, 1999, 4711, None, 1001)
            blk = np.stack([part.getBrownianIncrement(i, f).realizations.to_float32() for i in range(4) for f in range(2)])
            assert (blk.view(np.uint32) == got[knob][:, 1001:].view(np.uint32)).all()
            assert isinstance(bm.getCloneWithModifiedSeed(5), gpu.BrownianMotionFromMersenneRandomNumbers)
    finally:
        os.environ.pop("FMHIP_DEVICE_MERSENNE", None)
    assert (got["0"].view(np.uint32) == host.reshape(8, 3000).view(np.uint32)).all()
    assert compare(gpu, got["1"], 4711, [0.25] * 4, 2, 3000) == 0      # 24 000 draws: none of the one-in-10^8 kind


def test_black_scholes_value_equal_between_both_paths(gpu):
    """10^6 paths, 5 steps: a European call valued on the device-generated and on the host-generated motion.  The vectors obey the contract
    (all draws compared), so the values agree to the rounding of at most a handful of one-ulp differences."""
    td = gpu.TimeDiscretization(0.0, 5, 0.4)
    n = 1_000_000
    values, incs = {}, {}
    try:
        for knob in ("1", "0"):
            os.environ["FMHIP_DEVICE_MERSENNE"] = knob
            bm = gpu.BrownianMotionFromMersenneRandomNumbers(td, 1, n, 31415)
            x = None
            for i in range(5):
                w = bm.getBrownianIncrement(i, 0)
                x = w if x is None else x.add(w)
            s = x.mult(0.3).add((0.05 - 0.5 * 0.09) * 2.0).exp().mult(100.0)
            values[knob] = s.sub(105.0).floor(0.0).getAverage() * np.exp(-0.05 * 2.0)
            incs[knob] = np.stack([bm.getBrownianIncrement(i, 0).realizations.to_float32() for i in range(5)])
    finally:
        os.environ.pop("FMHIP_DEVICE_MERSENNE", None)
    n_ulp = compare(gpu, incs["1"], 31415, [0.4] * 5, 1, n)
    assert (incs["0"].view(np.uint32) == gpu.mersenne_increments(31415, [0.4] * 5, 1, n).astype(np.float32).reshape(5, n).view(np.uint32)).all()
    print(f"Black-Scholes call: device {values['1']!r}, host {values['0']!r}; {n_ulp} of {5 * n} draws one ulp off")
    assert abs(values["1"] - values["0"]) <= (1e-9 * n_ulp + 1e-15) * abs(values["0"]) and 10.0 < values["0"] < 20.0
    if n_ulp == 0:
        assert values["1"] == values["0"]


_OTHER_MODES = r'''
import importlib, json, os, sys, threading
sys.path.insert(0, %(root)r)
import numpy as np
import ctypes as C
fm = importlib.import_module("finmath-lib-cuda-extensions_amd")
mode = sys.argv[1]
N = fm._native

def gen(seed, dt, nf, n, off=0):
    dt = np.ascontiguousarray(dt, dtype=np.float64)
    handles = (C.c_int64 * (dt.size * nf))()
    N.check(N.lib().fmhip_bm_generate_mersenne_device(seed, dt.size, nf, n, off, dt.ctypes.data_as(C.POINTER(C.c_double)), handles))
    return np.stack([fm.DeviceVector(h, n).to_float32() for h in handles])

dt = [0.1, 0.4, 0.9]
out = {}
if mode == "devices":
    fm.init_devices([0, 0])
    for n, off in ((100_003, 0), (1, 0), (20_001, 7)):       # blocks of 50 002 + 50 001 paths; a vector shorter than the shards are many; an odd offset
        out[f"{n}/{off}"] = gen(99, dt, 2, n, off).view(np.uint32).tolist()
    bad = (C.c_int64 * 6)()
    out["rc_bad"] = N.lib().fmhip_bm_generate_mersenne_device(99, 3, 2, 10, -1, (C.c_double * 3)(*dt), bad)
else:
    fm.init(0)
    fm.set_thread_engines(True)
    def other():
        out["100003/0"] = gen(99, dt, 2, 100_003).view(np.uint32).tolist()     # on this thread's own engine
    t = threading.Thread(target=other); t.start(); t.join()
    out["1/0"] = gen(99, dt, 2, 1).view(np.uint32).tolist()
    out["20001/7"] = gen(99, dt, 2, 20_001, 7).view(np.uint32).tolist()
    out["rc_bad"] = 1
print("RESULT " + json.dumps(out))
fm.shutdown()
'''


@pytest.mark.parametrize("mode", ["devices", "threads"])
def test_device_list_and_thread_engines(gpu, mode, tmp_path):
    """A device list {0, 0}: every shard generates its own block of paths (no host vector, no upload), the front's vectors are the whole;
    thread engines: a second thread generates on its own engine.  In a process of its own; compared with this process's single engine."""
    import json
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / "modes.py"
    script.write_text(_OTHER_MODES % {"root": root})
    r = subprocess.run([sys.executable, str(script), mode], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = json.loads([line for line in r.stdout.splitlines() if line.startswith("RESULT ")][-1][7:])
    assert out["rc_bad"] != 0
    dt = [0.1, 0.4, 0.9]
    for n, off in ((100_003, 0), (1, 0), (20_001, 7)):
        want = generate(gpu, 99, dt, 2, n, off)
        assert (np.array(out[f"{n}/{off}"], dtype=np.uint32).reshape(want.shape) == want.view(np.uint32)).all(), (mode, n, off)
    compare(gpu, generate(gpu, 99, dt, 2, 100_003), 99, dt, 2, 100_003)
