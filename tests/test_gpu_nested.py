"""Nested simulation on the device (include/fmhip.h: fmhip_block_moments, fmhip_vec_repeat; csrc/nested_kernel.hip) on a real
MI355X: the three outputs EQUAL the host definition's bit for bit on wide-range random data at every block length of the three regimes and
around their boundaries, for one and four vectors per call and every mask; one vector's outputs do not depend on its slot; dyadic data give
numpy's exact values; the repeat against numpy on bit patterns; the frame (pending operands, pool statistics, refusals, a given-up
vector, small–large–small, the knob), a device list and thread engines in a process of their own; and the primal–dual bounds of a Bermudan
put against the tree.

Every test prints the figures it asserts on before it asserts (run with -s).  No test asks the device for anything out of range: bad
arguments are refused on the host before a launch."""
import ctypes as C
import json
import os
import subprocess
import sys
from importlib import import_module

import numpy as np
import pytest

from test_gpu_kernel_regression import limit
from test_nested_cpu import (BLOCKS, DATES, FIT_PATHS, K, OUTER_PATHS, R, S0, SEED_FIT, SEED_INNER, SEED_OUTER, SEGMENT, SIGMA, TREE, chain, check_bounds,
                             dyadic, same_f32, wide_range)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("sum", "mean", "variance")
LARGE = (1 << 21) + 3                           # 1025 segments: several workgroups per block, the second stage over more than 64 partials per lane group
MS = (1, 2, 3, 5, 257)
MAX_N = 1 << 22
MASKS = [tuple(n for k, n in enumerate(NAMES) if mask >> k & 1) for mask in range(1, 8)]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def ms_of(block):
    return sorted({min(m, MAX_N // block) for m in MS})


class knob_off:
    def __enter__(self):
        self.prev = os.environ.get("FMHIP_DEVICE_NESTED")
        os.environ["FMHIP_DEVICE_NESTED"] = "0"
    def __exit__(self, *a):
        if self.prev is None: del os.environ["FMHIP_DEVICE_NESTED"]
        else: os.environ["FMHIP_DEVICE_NESTED"] = self.prev


def check_against_the_definition(gpu, arrays, block, masks):
    """Every mask of `masks` on the vectors of `arrays` in ONE call each, against the definition computed once per vector."""
    want = [dict(zip(NAMES, gpu.block_moments_host(a, block, NAMES))) for a in arrays]
    vs = [gpu.DeviceVector.from_host(a) for a in arrays]
    m = arrays[0].size // block
    for names in masks:
        got = gpu.block_moments(vs, block, names)
        assert len(got) == len(vs)
        for i, row in enumerate(got):
            for name, rv in zip(names, row):
                assert rv.size() == m and same_f32(rv.realizations.to_float32(), want[i][name]), (block, m, len(vs), names, i, name)
    for v, a in zip(vs, arrays): assert (bits(v.to_float32()) == bits(a)).all()


@pytest.mark.parametrize("block", BLOCKS + [LARGE])
def test_the_outputs_are_the_definitions_bit_for_bit(gpu, block):
    rng = np.random.default_rng(block)
    with limit(120):
        for m in ms_of(block):
            n = m * block
            arrays = [wide_range(n, rng) for _ in range(4 if n <= 1 << 20 else 2)]
            check_against_the_definition(gpu, arrays[:1], block, MASKS)
            check_against_the_definition(gpu, arrays, block, MASKS if n <= 1 << 16 else [NAMES, ("variance",)])


@pytest.mark.parametrize("block,m", [(3, (1 << 18) + 1), (65, (1 << 14) + 5), (SEGMENT + 1, 8200)])
def test_more_tasks_than_waves_in_the_grid(gpu, block, m):
    """The wave-stride loop wraps: more tasks than the capped grid has waves (16384), in each regime."""
    with limit(120):
        check_against_the_definition(gpu, [wide_range(m * block, np.random.default_rng(m))], block, [NAMES])


def test_one_vectors_outputs_do_not_depend_on_its_slot_or_its_company(gpu):
    rng = np.random.default_rng(5)
    with limit(120):
        for block, m in ((7, 33), (100, 5), (SEGMENT + 1, 3)):
            n = block * m
            a, others = wide_range(n, rng), [gpu.DeviceVector.from_host(wide_range(n, rng)) for _ in range(3)]
            others[1] = gpu.DeviceVector.from_host(np.full(n, np.nan, dtype=np.float32))
            v = gpu.DeviceVector.from_host(a)
            alone = [rv.realizations.to_float32() for rv in gpu.block_moments([v], block, NAMES)[0]]
            for slot in range(4):
                call = others[:slot] + [v] + others[slot:]
                got = gpu.block_moments(call, block, NAMES)[slot]
                for j in range(3): assert (bits(got[j].realizations.to_float32()) == bits(alone[j])).all(), (block, slot, j)
            twice = gpu.block_moments([v, v], block, ("mean",))
            assert (bits(twice[0][0].realizations.to_float32()) == bits(alone[1])).all() and (bits(twice[1][0].realizations.to_float32()) == bits(alone[1])).all()


@pytest.mark.parametrize("block", [1, 3, 64, 65, 2048, 2049, 4097])
def test_on_dyadic_data_the_outputs_are_numpys_exact_values(gpu, block):
    m = ms_of(block)[-1]
    a = dyadic(m * block, np.random.default_rng(block))
    with limit(60):
        s, mean, var = [rv.realizations.to_float32() for rv in gpu.block_moments([gpu.DeviceVector.from_host(a)], block, NAMES)[0]]
    a64 = a.astype(np.float64).reshape(m, block)
    s1, s2 = a64.sum(axis=1), (a64 * a64).sum(axis=1)
    assert same_f32(s, s1.astype(np.float32)) and same_f32(mean, (s1 / block).astype(np.float32))
    assert same_f32(var, np.maximum(0.0, s2 / block - (s1 / block) * (s1 / block)).astype(np.float32))


def test_nan_and_infinity_stay_inside_their_block(gpu):
    rng = np.random.default_rng(9)
    with limit(60):
        for block in (4, 100, SEGMENT + 1):
            a = wide_range(5 * block, rng)
            a[block + block // 2] = np.nan; a[3 * block] = np.inf; a[5 * block - 1] = -np.inf
            check_against_the_definition(gpu, [a], block, [NAMES])
            s, = gpu.block_moments([gpu.DeviceVector.from_host(a)], block, ("sum",))[0]
            s = s.realizations.to_float32()
            assert np.isnan(s[1]) and s[3] == np.inf and s[4] == -np.inf and np.isfinite(s[[0, 2]]).all()


# ---------------------------------------------------------------- the repeat
def special(n, rng):
    a = wide_range(n, rng).view(np.uint32).copy()
    a[0] = 0x7fc12345                                                # a NaN with a payload
    if n > 1: a[n - 1] = 0x80000000                                  # -0.0
    if n > 2: a[n // 2] = 0xffa00001                                 # a negative NaN with another payload
    return a.view(np.float32)


@pytest.mark.parametrize("n", [1, 3, 64, 65, 4097])
def test_tile_and_repeat_each_are_numpys_on_bit_patterns(gpu, n):
    a = special(n, np.random.default_rng(n))
    v = gpu.DeviceVector.from_host(a)
    with limit(120):
        for k in (1, 2, 3, 64, 65, 1000):
            assert (bits(gpu.repeat_each(v, k).realizations.to_float32()) == np.repeat(bits(a), k)).all(), (n, k)
            assert (bits(gpu.tile(v, k).realizations.to_float32()) == np.tile(bits(a), k)).all(), (n, k)
        if n == 4097:                                                # both at once through the C-ABI, and more quads than the capped grid has lanes
            h = C.c_int64(0)
            for each, times in ((3, 5), (1000, 2)):
                assert gpu.lib().fmhip_vec_repeat(v.handle, each, times, C.byref(h)) == 0
                out = gpu.DeviceVector(h.value, n * each * times)
                assert (bits(out.to_float32()) == np.tile(np.repeat(bits(a), each), times)).all()
    assert (bits(v.to_float32()) == bits(a)).all()


@pytest.mark.parametrize("k", [1, 2, 3, 63, 64, 65, 100, 2048, 2049, 4096])
def test_the_block_means_of_a_repeat_are_the_vector(gpu, k):
    """k·x is exact in fp64 for an fp32 x and k <= 4096 … but its tree is a sum, not a product: sums of equal terms over the leaves are exact
    as long as every partial sum j·x fits 53 bits, which 24 + 12 bits do."""
    a = wide_range(257, np.random.default_rng(k))
    v = gpu.RandomVariableHip(0.75, a)
    with limit(60):
        back = gpu.block_means(gpu.repeat_each(v, k), k)
    assert back.getFiltrationTime() == 0.75 and (bits(back.realizations.to_float32()) == bits(a)).all()
    variance, = gpu.block_moments([gpu.repeat_each(v, k)], k, ("variance",))[0]
    # S1 = k·x is exact, S2 = k·x² is not (48 + 12 bits): the variance's documented bound, (chain + 1)·2^-53·S2/k, and its rounding to fp32
    bound = (chain(k) + 1) * 2.0 ** -53 * np.square(a.astype(np.float64)) * (1 + 2.0 ** -23)
    got = variance.realizations.to_float32().astype(np.float64)
    print("block", k, "largest variance / bound", float((got / bound).max()))
    assert (got <= bound).all()


# ---------------------------------------------------------------- the engine's behaviour
def test_pending_operands_give_the_bits_of_materialised_ones(gpu):
    block, m = 100, 41
    a = wide_range(block * m, np.random.default_rng(3))
    prev = gpu.set_fusion(True)
    try:
        with limit(60):
            stored = gpu.DeviceVector.from_host(a)
            doubled = gpu.DeviceVector.from_host((a * np.float32(2.0)).astype(np.float32))
            want = [rv.realizations.to_float32() for rv in gpu.block_moments([doubled], block, NAMES)[0]] + [gpu.repeat_each(doubled, 3).realizations.to_float32()]
            got = [rv.realizations.to_float32() for rv in gpu.block_moments([stored.v1s1("MULT_S", 2.0)], block, NAMES)[0]] + [gpu.repeat_each(stored.v1s1("MULT_S", 2.0), 3).realizations.to_float32()]
            two = gpu.block_moments([stored.v1s1("MULT_S", 2.0), stored.v1s1("ADD_S", 0.0)], block, ("mean",))
        for g, w in zip(got, want): assert (bits(g) == bits(w)).all()
        assert (bits(two[0][0].realizations.to_float32()) == bits(want[1])).all()
        assert (bits(stored.to_float32()) == bits(a)).all()
    finally:
        gpu.set_fusion(prev)


def test_pool_statistics_show_only_the_outputs(gpu):
    block, m = 128, 1024
    n = block * m
    a = np.random.default_rng(8).random(n, dtype=np.float32)
    with limit(60):
        v = gpu.DeviceVector.from_host(a)
        gpu.block_moments([v], block, NAMES); gpu.block_moments([v], n, NAMES); gpu.repeat_each(v, 2)      # warm: scratch and pinned blocks are the engine's for good
        sizes = {}
        for count in (m, 2 * n):
            before = gpu.pool_stats().bytes_in_use
            probe = gpu.DeviceVector.from_host(np.zeros(count, dtype=np.float32))
            sizes[count] = gpu.pool_stats().bytes_in_use - before
            del probe
        for call, n_out, per in ((lambda: gpu.block_moments([v], block, NAMES), 3, sizes[m]), (lambda: gpu.block_moments([v, v], block, ("mean",)), 2, sizes[m]),
                                 (lambda: gpu.repeat_each(v, 2), 1, sizes[2 * n]), (lambda: gpu.tile(v, 2), 1, sizes[2 * n])):
            before = gpu.pool_stats()
            kept = call()
            after = gpu.pool_stats()
            assert after.n_live_vectors - before.n_live_vectors == n_out
            assert after.bytes_in_use - before.bytes_in_use == n_out * per
            assert after.n_kernel_launches == before.n_kernel_launches + 1          # ONE armed launch per call
            del kept


def test_refusals_are_made_on_the_host(gpu):
    N = gpu._native
    lib = gpu.lib()
    n = 1000
    v = gpu.DeviceVector.from_host(np.arange(n, dtype=np.float32))
    other = gpu.DeviceVector.from_host(np.arange(n + 1, dtype=np.float32))
    before = gpu.pool_stats()
    outs, h = (C.c_int64 * 12)(), C.c_int64(0)
    vs = lambda *hs: (C.c_int64 * len(hs))(*hs)
    bad = N.ERR_INVALID_ARGUMENT
    assert lib.fmhip_block_moments(vs(v.handle), 0, 10, 1, outs) == bad
    assert lib.fmhip_block_moments(vs(*[v.handle] * 5), 5, 10, 1, outs) == bad
    assert lib.fmhip_block_moments(vs(v.handle), 1, 10, 0, outs) == bad
    assert lib.fmhip_block_moments(vs(v.handle), 1, 10, 8, outs) == bad
    assert lib.fmhip_block_moments(vs(v.handle), 1, 0, 7, outs) == bad
    assert lib.fmhip_block_moments(vs(v.handle), 1, -5, 7, outs) == bad
    assert lib.fmhip_block_moments(vs(v.handle), 1, 7, 7, outs) == bad              # 1000 is no multiple of 7
    assert lib.fmhip_block_moments(vs(v.handle), 1, 2000, 7, outs) == bad
    assert lib.fmhip_block_moments(None, 1, 10, 7, outs) == bad
    assert lib.fmhip_block_moments(vs(v.handle), 1, 10, 7, None) == bad
    assert lib.fmhip_block_moments(vs(v.handle, 0), 2, 10, 7, outs) == bad
    assert lib.fmhip_block_moments(vs(v.handle, other.handle), 2, 1, 7, outs) == N.ERR_SIZE_MISMATCH
    assert lib.fmhip_block_moments(vs(v.handle + 12345), 1, 10, 7, outs) == N.ERR_INVALID_HANDLE
    assert lib.fmhip_vec_repeat(v.handle, 0, 1, C.byref(h)) == bad
    assert lib.fmhip_vec_repeat(v.handle, 1, 0, C.byref(h)) == bad
    assert lib.fmhip_vec_repeat(v.handle, -2, 3, C.byref(h)) == bad
    assert lib.fmhip_vec_repeat(v.handle, 1 << 22, 1, C.byref(h)) == bad            # 1000·2^22 > 2^31 − 1
    assert lib.fmhip_vec_repeat(v.handle, 1 << 11, 1 << 11, C.byref(h)) == bad
    assert lib.fmhip_vec_repeat(v.handle, 1 << 40, 1 << 40, C.byref(h)) == bad
    assert lib.fmhip_vec_repeat(v.handle, 2, 2, None) == bad
    assert lib.fmhip_vec_repeat(0, 2, 2, C.byref(h)) == bad
    assert lib.fmhip_vec_repeat(v.handle + 12345, 2, 2, C.byref(h)) == N.ERR_INVALID_HANDLE
    with pytest.raises(ValueError): gpu.block_means(v, 7)
    with pytest.raises(ValueError): gpu.block_moments([v, other], 1)
    with pytest.raises(ValueError): gpu.repeat_each(v, 1 << 22)
    after = gpu.pool_stats()
    assert after.n_kernel_launches == before.n_kernel_launches and after.n_live_vectors == before.n_live_vectors      # nothing was launched for any of it
    assert h.value == 0 and all(x == 0 for x in outs)
    # under an expectation communicator both calls act on this rank's own vector
    try:
        gpu.set_expectation_comm(2, 0, lambda local: np.stack([local, local]))
        with limit(60):
            mean = gpu.block_means(v, 10).realizations.to_float32()
            rep = gpu.repeat_each(v, 2).realizations.to_float32()
    finally:
        gpu.set_expectation_comm(1, 0, None)
    assert (mean == np.arange(n, dtype=np.float64).reshape(100, 10).mean(axis=1).astype(np.float32)).all() and (rep == np.repeat(np.arange(n, dtype=np.float32), 2)).all()


def test_a_given_up_vector_is_the_error_a_read_is(gpu):
    prev = gpu.set_fusion(True)
    try:
        with limit(60):
            base = gpu.DeviceVector.from_host(np.arange(4096, dtype=np.float32))
            ys = [base.v1s1("ADD_S", float(k)) for k in range(1, 4)]
            gpu.give_up_values(ys)
            gpu.reduce_moments_batch_end(gpu.reduce_moments_batch_begin(ys), len(ys))
            for y in ys:
                try:
                    y.to_float32()
                    read_error = None
                except gpu.FmhipError as e:
                    read_error = e.code
                for call in (lambda: gpu.block_means(y, 64), lambda: gpu.repeat_each(y, 2), lambda: gpu.block_moments([base, y], 4096, NAMES)):
                    if read_error is None:
                        call()
                    else:
                        with pytest.raises(gpu.FmhipError) as info:
                            call()
                        assert info.value.code == read_error and "given up" in str(info.value)
    finally:
        gpu.set_fusion(prev)


def test_small_large_small_on_one_engine(gpu):
    """The side-pass scratch grows for the partials of a large block and serves the small shapes again."""
    rng = np.random.default_rng(12)
    small, large = dyadic(65 * 4, rng), dyadic(2 * LARGE, rng)
    with limit(120):
        vs, vl = gpu.DeviceVector.from_host(small), gpu.DeviceVector.from_host(large)
        for _ in range(2):
            assert (gpu.block_means(vs, 65).realizations.to_float32() == small.astype(np.float64).reshape(4, 65).mean(axis=1).astype(np.float32)).all()
            assert (gpu.block_moments([vl, vl], LARGE, ("sum",))[1][0].realizations.to_float32() == large.astype(np.float64).reshape(2, LARGE).sum(axis=1).astype(np.float32)).all()
            assert (gpu.block_means(vs, 4).realizations.to_float32() == small.astype(np.float64).reshape(65, 4).mean(axis=1).astype(np.float32)).all()
            assert (bits(gpu.repeat_each(vs, 3).realizations.to_float32()) == np.repeat(bits(small), 3)).all()


def test_the_host_switch_gives_identical_results(gpu):
    rng = np.random.default_rng(6)
    a, b = wide_range(SEGMENT * 3 + 300, rng), special(4097, rng)
    def everything():
        v, w = gpu.RandomVariableHip(1.25, a), gpu.DeviceVector.from_host(b)
        out = []
        for block in (1, 4, 6444 // 4, 6444):
            for row in gpu.block_moments([v, v.mult(2.0)], block, ("variance", "sum", "mean")):
                out += [bits(rv.realizations.to_float32()) for rv in row]
                assert all(rv.getFiltrationTime() == 1.25 for rv in row)
        return out + [bits(gpu.repeat_each(w, 5).realizations.to_float32()), bits(gpu.tile(w, 3).realizations.to_float32())]
    with limit(120):
        launches = gpu.pool_stats().n_kernel_launches
        device = everything()
        assert gpu.pool_stats().n_kernel_launches >= launches + 6
        with knob_off():
            launches = gpu.pool_stats().n_kernel_launches
            host = everything()
    for k, (d, h) in enumerate(zip(device, host)):
        assert d.shape == h.shape and (d == h).all(), k


# ---------------------------------------------------------------- the fronts: a device list, thread engines
_FRONTS = r'''
import ctypes as C, importlib, json, os, sys, threading
import numpy as np
sys.path.insert(0, %(root)r)
fm = importlib.import_module("finmath-lib-cuda-extensions_amd")
mode, out_path = sys.argv[1], sys.argv[2]
N = fm._native
block, m = 2049, 37
rng = np.random.default_rng(77)
a = ((10.0 ** rng.uniform(-8.0, 8.0, block * m)) * np.where(rng.random(block * m) < 0.5, -1.0, 1.0)).astype(np.float32)
res, info = {}, {}

def everything(tag, v):
    for bl in (3, 2049):
        row = fm.block_moments([v, v], bl, ("sum", "mean", "variance"))[1]
        for name, rv in zip(("sum", "mean", "variance"), row): res["%%s_%%d_%%s" %% (tag, bl, name)] = rv.realizations.to_float32()
    res[tag + "_repeat"] = fm.repeat_each(fm.block_means(v, 2049), 5).realizations.to_float32()
    res[tag + "_in"] = v.to_float32()

if mode == "devices_one":
    fm.init_devices([0])
    fm.set_fusion(True)
    V = fm.DeviceVector.from_host(a)
    everything("stored", V)
    everything("pending", V.v1s1("MULT_S", 2.0))
elif mode == "devices_two":
    fm.init_devices([0, 0])
    lib = fm.lib()
    V = fm.DeviceVector.from_host(a)
    V.to_float32()
    before = fm.pool_stats()
    outs, h = (C.c_int64 * 6)(), C.c_int64(0)
    two = (C.c_int64 * 2)(V.handle, V.handle)
    info["status"] = [lib.fmhip_block_moments(two, 2, 3, 7, outs), lib.fmhip_block_moments(two, 1, 2049, 2, outs), lib.fmhip_vec_repeat(V.handle, 2, 3, C.byref(h))]
    info["unsupported"] = N.ERR_UNSUPPORTED
    info["message"] = lib.fmhip_last_error().decode("utf-8", "replace")
    after = fm.pool_stats()
    info["launches"] = [before.n_kernel_launches, after.n_kernel_launches]
    info["live"] = [before.n_live_vectors, after.n_live_vectors]
    info["outputs"] = [h.value] + list(outs)
    os.environ["FMHIP_DEVICE_NESTED"] = "0"                  # the documented fallback: through reads and uploads, on any device list
    everything("host", V)
elif mode == "threads":
    fm.init(0)
    fm.set_thread_engines(True)
    fm.set_fusion(True)
    V = fm.DeviceVector.from_host(a)
    pend = V.v1s1("MULT_S", 2.0)                               # pending, owned by the main thread's engine
    kept = {}
    def other():
        kept["stored"] = fm.block_moments([V, V], 2049, ("sum", "mean", "variance"))[1]
        kept["pending"] = fm.block_moments([pend, V], 3, ("sum", "mean", "variance"))[0]
        kept["repeat"] = fm.repeat_each(pend, 2)
    t = threading.Thread(target=other); t.start(); t.join()
    for name, rv in zip(("sum", "mean", "variance"), kept["stored"]): res["stored_2049_" + name] = rv.realizations.to_float32()      # read back on the main thread
    for name, rv in zip(("sum", "mean", "variance"), kept["pending"]): res["pending_3_" + name] = rv.realizations.to_float32()
    res["pending_repeat2"] = kept["repeat"].realizations.to_float32()
    res["stored_in"], res["pending_in"] = V.to_float32(), pend.to_float32()
    kept.clear()
np.savez(out_path, **res)
print("RESULT " + json.dumps(info))
fm.shutdown()
'''


def _run_front(tmp_path, mode):
    script = tmp_path / "fronts.py"
    script.write_text(_FRONTS % {"root": ROOT})
    out_path = tmp_path / (mode + ".npz")
    r = subprocess.run([sys.executable, str(script), mode, str(out_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    info = json.loads([line for line in r.stdout.splitlines() if line.startswith("RESULT ")][-1][7:])
    return info, dict(np.load(out_path))


def _check_everything(gpu, res, tag, a):
    for bl in (3, 2049):
        for name, want in zip(NAMES, gpu.block_moments_host(a, bl, NAMES)): assert same_f32(res[f"{tag}_{bl}_{name}"], want), (tag, bl, name)
    assert (bits(res[tag + "_repeat"]) == np.repeat(bits(gpu.block_moments_host(a, 2049, ("mean",))[0]), 5)).all(), tag


@pytest.mark.parametrize("mode", ["devices_one", "devices_two", "threads"])
def test_device_list_and_thread_engines(gpu, mode, tmp_path):
    """In a process of its own.  A device list of ONE shard is that shard's call: everything equals the definition, on stored and on pending
    operands.  A list of two answers FMHIP_ERR_UNSUPPORTED for both calls — nothing launched, nothing left behind — and the mirror's host
    path (FMHIP_DEVICE_NESTED=0) gives the definition's results there.  Thread engines: a thread that owns neither the vector nor the
    pending one reduces and repeats them; the outputs are read on the main thread."""
    block, m = 2049, 37
    rng = np.random.default_rng(77)
    a = ((10.0 ** rng.uniform(-8.0, 8.0, block * m)) * np.where(rng.random(block * m) < 0.5, -1.0, 1.0)).astype(np.float32)
    doubled = (a * np.float32(2.0)).astype(np.float32)
    info, res = _run_front(tmp_path, mode)
    if mode == "devices_one":
        assert (bits(res["stored_in"]) == bits(a)).all() and (bits(res["pending_in"]) == bits(doubled)).all()
        _check_everything(gpu, res, "stored", a)
        _check_everything(gpu, res, "pending", doubled)
    elif mode == "devices_two":
        assert info["status"] == [info["unsupported"]] * 3 and info["unsupported"] == gpu._native.ERR_UNSUPPORTED
        assert "shards" in info["message"]
        assert info["launches"][0] == info["launches"][1] and info["live"][0] == info["live"][1] and info["outputs"] == [0] * 7
        assert (bits(res["host_in"]) == bits(a)).all()
        _check_everything(gpu, res, "host", a)
    else:
        assert (bits(res["stored_in"]) == bits(a)).all() and (bits(res["pending_in"]) == bits(doubled)).all()
        for name, want in zip(NAMES, gpu.block_moments_host(a, 2049, NAMES)): assert same_f32(res["stored_2049_" + name], want), name
        for name, want in zip(NAMES, gpu.block_moments_host(doubled, 3, NAMES)): assert same_f32(res["pending_3_" + name], want), name
        assert (bits(res["pending_repeat2"]) == np.repeat(bits(doubled), 2)).all()


# ---------------------------------------------------------------- the driver
def test_primal_dual_bounds_of_a_bermudan_put_against_the_tree(gpu):
    """montecarlo.bermudan_option_bounds_mc with the constants of tests/test_gpu_regression.py: 10 dates, 2^16 fit paths, 4096 outer paths,
    64 and 16 inner paths, a cubic.  lower − 3·se <= tree <= upper + 3·se; upper(64) < upper(16) (the inner noise biases the bound upwards);
    upper(64) − tree <= 0.010; lower >= european − 3·se.  tests/test_nested_cpu.py holds the numpy restatement to the same conditions at
    the same seeds (there, over five seeds: lower 0.1507 … 0.1530 ± 0.0024, upper(64) 0.1574 … 0.1580 ± 0.0003, upper(16) 0.1661 … 0.1674 ±
    0.0007).  Measured on one MI355X: lower 0.15178 ± 0.00237, upper(64) 0.15714 ± 0.00032, upper(16) 0.16689 ± 0.00067."""
    mc = import_module("finmath-lib-cuda-extensions_amd.montecarlo")
    from test_gpu_regression import crr_bermudan_put
    assert abs(crr_bermudan_put(DATES) - TREE) < 5e-7
    td = gpu.TimeDiscretization(0.0, 10, 0.2)
    prev = gpu.set_fusion(True)
    try:
        with limit(240):
            fit, outer = gpu.BrownianMotionHip(td, 1, FIT_PATHS, SEED_FIT), gpu.BrownianMotionHip(td, 1, OUTER_PATHS, SEED_OUTER)
            at64 = mc.bermudan_option_bounds_mc(fit, outer, 64, SEED_INNER, S0, R, SIGMA, DATES, K)
            at16 = mc.bermudan_option_bounds_mc(fit, outer, 16, SEED_INNER, S0, R, SIGMA, DATES, K)
            small = lambda: mc.bermudan_option_bounds_mc(gpu.BrownianMotionHip(td, 1, 1 << 12, 5), gpu.BrownianMotionHip(td, 1, 300, 6), 7, 70, S0, R, SIGMA, DATES, K)
            on = small()
            with knob_off(): off = small()
    finally:
        gpu.set_fusion(prev)
    check_bounds(at64, at16)
    print("knob on:", on, "knob off:", off)
    assert on == off                                                 # to the last bit: the host definition is the device's
