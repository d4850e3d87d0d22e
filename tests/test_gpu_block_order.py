"""Block order statistics on the device (include/fmhip.h: fmhip_block_order_statistics, fmhip_block_sort; csrc/block_order_kernel.hip;
DESIGN.md §4.23) on a real MI355X: ranks, range means and the block sort EQUAL the host definition's bit for bit at every block length of
the issue's list — both regimes, every padded size with its neighbours — for one and four vectors per call, on wide-range data, ties,
constant, ascending and descending blocks, ±0, ±inf, denormals and NaNs of both signs at 0 %, about 10 % and 100 % of a block; one vector's
outputs do not depend on its slot or on the other selectors; the grid-stride loops wrap; the frame (inputs unchanged, pending operands, a
given-up vector, refusals, pool statistics, the knob), a device list and thread engines in a process of their own; and the nested initial
margin of a forward against its closed-form bracket.

Every test prints the figures it asserts on before it asserts (run with -s).  No test asks the device for anything out of range: bad
arguments are refused on the host before a launch."""
import ctypes as C
import json
import os
import re
import subprocess
import sys
from importlib import import_module

import numpy as np
import pytest

from test_block_order_cpu import (BLOCKS, DELTA, FAMILIES, INNER_PATHS, MATURITY, OUTER_PATHS, QUANTILE, QUIET_NAN, R, S0, SEED_INNER, SEED_OUTER, SIGMA, STRIKE, T_MARGIN,
                                  bits, check_margin, family, quantile_index, selectors)
from test_gpu_kernel_regression import limit
from test_gpu_nested import knob_off
from test_nested_cpu import wide_range

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MS = (1, 2, 3, 5, 257)
MAX_N = 1 << 20


def ms_of(block):
    return sorted({min(m, MAX_N // block) for m in MS})


def check_against_the_definition(gpu, arrays, block, sort=True, wanted=None):
    """The issue's ranks and ranges on the vectors of `arrays` in ONE call, and the block sort of each, against the definition (computed once
    per array where the caller keeps `wanted`)."""
    ranks, ranges = selectors(block)
    wanted = {} if wanted is None else wanted
    m = arrays[0].size // block
    vs = [gpu.DeviceVector.from_host(a) for a in arrays]
    got = gpu.block_order_statistics(vs, block, ranks, ranges)
    assert len(got) == len(vs)
    for i, (a, row) in enumerate(zip(arrays, got)):
        if id(a) not in wanted: wanted[id(a)] = gpu.block_order_statistics_host(a, block, ranks, ranges)
        want = wanted[id(a)]
        assert len(row) == len(want) == len(ranks) + len(ranges)
        for j, (rv, w) in enumerate(zip(row, want)):
            g = rv.realizations.to_float32()
            assert g.shape == (m,) and (bits(g) == bits(w)).all(), (block, m, len(vs), i, j, int((bits(g) != bits(w)).sum()))
        if sort:
            assert (bits(gpu.block_sort(vs[i], block).realizations.to_float32()) == bits(gpu.block_sort_host(a, block))).all(), (block, m, i)
    for v, a in zip(vs, arrays): assert (bits(v.to_float32()) == bits(a)).all()                    # inputs unchanged


@pytest.mark.parametrize("block", BLOCKS)
def test_ranks_ranges_and_the_sort_are_the_definitions_bit_for_bit(gpu, block):
    rng = np.random.default_rng(block)
    with limit(120):
        for m in ms_of(block):
            n = m * block
            arrays, wanted = [family(name, n, block, rng) for name in FAMILIES], {}
            for at in range(0, len(arrays), 4):
                group = (arrays + arrays)[at:at + 4]                                                # four vectors per call (the list wraps)
                check_against_the_definition(gpu, group, block, sort=False, wanted=wanted)
            for a in arrays: check_against_the_definition(gpu, [a], block, wanted=wanted)           # one vector per call, and its sort


def test_nans_infinities_and_zeros_come_back_as_the_definition_says(gpu):
    with limit(60):
        for block in (4, 100, 1000):
            a = np.arange(3 * block, dtype=np.float32)
            u = bits(a).copy()
            u[0], u[1], u[2] = 0x80000000, 0x00000000, 0x00000001                                   # -0.0, +0.0, the smallest denormal
            u[block], u[block + 1], u[block + 2] = 0xffc00001, 0x7f800001, 0x7f800000               # two NaNs with payloads, +inf
            u[2 * block], u[2 * block + 1] = 0xff800000, 0x7f800000                                 # -inf and +inf in one block
            a = u.view(np.float32)
            v = gpu.DeviceVector.from_host(a)
            lo, second, top, below = [bits(rv.realizations.to_float32()) for rv in gpu.block_order_statistics([v], block, ranks=[0, 1, block - 1, block - 3])[0]]
            mean_all, = [bits(rv.realizations.to_float32()) for rv in gpu.block_order_statistics([v], block, ranges=[(0, block - 1)])[0]]
            s = bits(gpu.block_sort(v, block).realizations.to_float32())
            print(block, [hex(x) for x in (lo[0], second[0], top[1], below[1], mean_all[1], mean_all[2])])
            assert lo[0] == 0x80000000 and second[0] == 0x00000000 and s[2] == 0x00000001          # -0.0 before +0.0, the denormal bit for bit
            assert top[1] == QUIET_NAN and s[2 * block - 2] == QUIET_NAN and below[1] == 0x7f800000  # the NaN tail is quiet; +inf just before it
            assert mean_all[1] == QUIET_NAN and mean_all[2] == QUIET_NAN                             # a range into the NaN tail; both infinities
            assert bits(gpu.block_min(v, block).realizations.to_float32())[2] == 0xff800000 and bits(gpu.block_max(v, block).realizations.to_float32())[2] == 0x7f800000


def test_one_vectors_outputs_do_not_depend_on_its_slot_or_the_other_selectors(gpu):
    rng = np.random.default_rng(5)
    with limit(120):
        for block, m in ((7, 33), (100, 5), (2049, 3)):
            n = block * m
            ranks, ranges = selectors(block)
            a, others = family("nan10", n, block, rng), [gpu.DeviceVector.from_host(wide_range(n, rng)) for _ in range(3)]
            others[1] = gpu.DeviceVector.from_host(np.full(n, np.nan, dtype=np.float32))
            v = gpu.DeviceVector.from_host(a)
            alone = [bits(gpu.block_order_statistics([v], block, ranks=[r])[0][0].realizations.to_float32()) for r in ranks]
            alone += [bits(gpu.block_order_statistics([v], block, ranges=[g])[0][0].realizations.to_float32()) for g in ranges]
            for slot in range(4):
                call = others[:slot] + [v] + others[slot:]
                got = gpu.block_order_statistics(call, block, ranks, ranges)[slot]
                for j in range(len(alone)): assert (bits(got[j].realizations.to_float32()) == alone[j]).all(), (block, slot, j)
            twice = gpu.block_order_statistics([v, v], block, ranges=ranges[::-1])
            for row in twice:
                for j, g in enumerate(ranges[::-1]): assert (bits(row[j].realizations.to_float32()) == alone[len(ranks) + ranges.index(g)]).all(), (block, g)


@pytest.mark.parametrize("block,m", [(3, (1 << 18) + 1), (65, (1 << 14) + 5), (4096, 300)])
def test_more_blocks_than_the_grid_takes_at_once(gpu, block, m):
    """The wave-stride loop (small regime: 16384 waves of 16 blocks of 3) and the workgroup-stride loop (8192 workgroups at P = 128, 256 at
    P = 4096) wrap."""
    kernel = open(os.path.join(ROOT, "finmath-lib-cuda-extensions_amd", "csrc", "block_order_kernel.h")).read()
    sweep, small_cap = int(re.search(r"FM_ORDER_SWEEP = 1 << (\d+)", kernel).group(1)), int(re.search(r"FM_ORDER_SMALL_MAX_BLOCKS = (\d+)", kernel).group(1))
    padded = 1 << max(7, (block - 1).bit_length())
    assert (m > small_cap * 4 * (64 // 4)) if block == 3 else (m > min(max((1 << sweep) // padded, 256), 8192))
    with limit(120):
        check_against_the_definition(gpu, [family("nan10", m * block, block, np.random.default_rng(m))], block)


# ---------------------------------------------------------------- the engine's behaviour
def test_pending_operands_give_the_bits_of_materialised_ones(gpu):
    block, m = 100, 41
    ranks, ranges = selectors(block)
    a = wide_range(block * m, np.random.default_rng(3))
    doubled = (a * np.float32(2.0)).astype(np.float32)
    prev = gpu.set_fusion(True)
    try:
        with limit(60):
            stored = gpu.DeviceVector.from_host(a)
            got = [rv.realizations.to_float32() for rv in gpu.block_order_statistics([stored.v1s1("MULT_S", 2.0), stored.v1s1("ADD_S", 0.0)], block, ranks, ranges)[0]]
            got_sort = gpu.block_sort(stored.v1s1("MULT_S", 2.0), block).realizations.to_float32()
        for g, w in zip(got, gpu.block_order_statistics_host(doubled, block, ranks, ranges)): assert (bits(g) == bits(w)).all()
        assert (bits(got_sort) == bits(gpu.block_sort_host(doubled, block))).all()
        assert (bits(stored.to_float32()) == bits(a)).all()
    finally:
        gpu.set_fusion(prev)


def test_pool_statistics_show_only_the_outputs(gpu):
    block, m = 128, 1024
    n = block * m
    a = np.random.default_rng(8).random(n, dtype=np.float32)
    with limit(60):
        v = gpu.DeviceVector.from_host(a)
        gpu.block_order_statistics([v], block, ranks=[0]); gpu.block_sort(v, block)                 # warm: the pinned block is the engine's for good
        sizes = {}
        for count in (m, n // 16, n):
            before = gpu.pool_stats().bytes_in_use
            probe = gpu.DeviceVector.from_host(np.zeros(count, dtype=np.float32))
            sizes[count] = gpu.pool_stats().bytes_in_use - before
            del probe
        for call, n_out, per in ((lambda: gpu.block_order_statistics([v], block, [0, 5, 5], [(0, 3)]), 4, sizes[m]),
                                 (lambda: gpu.block_order_statistics([v, v], 16, ranges=[(0, 15)]), 2, sizes[n // 16]),
                                 (lambda: gpu.block_sort(v, block), 1, sizes[n])):
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
    long = gpu.DeviceVector.from_host(np.zeros(2 * 4097, dtype=np.float32))
    before = gpu.pool_stats()
    outs, h = (C.c_int64 * 48)(), C.c_int64(0)
    vs = lambda *hs: (C.c_int64 * len(hs))(*hs)
    i64 = lambda *xs: (C.c_int64 * max(len(xs), 1))(*xs)
    bad, f = N.ERR_INVALID_ARGUMENT, lib.fmhip_block_order_statistics
    assert f(vs(v.handle), 0, 10, i64(0), 1, None, None, 0, outs) == bad
    assert f(vs(*[v.handle] * 5), 5, 10, i64(0), 1, None, None, 0, outs) == bad
    assert f(vs(v.handle), 1, 10, None, 0, None, None, 0, outs) == bad                              # no selector
    assert f(vs(v.handle), 1, 10, i64(*range(9)), 9, None, None, 0, outs) == bad
    assert f(vs(v.handle), 1, 10, i64(0), -1, None, None, 0, outs) == bad
    assert f(vs(v.handle), 1, 10, None, 0, i64(0, 0, 0, 0, 0), i64(1, 1, 1, 1, 1), 5, outs) == bad
    assert f(vs(v.handle), 1, 10, i64(10), 1, None, None, 0, outs) == bad
    assert f(vs(v.handle), 1, 10, i64(-1), 1, None, None, 0, outs) == bad
    assert f(vs(v.handle), 1, 10, None, 0, i64(0), i64(10), 1, outs) == bad
    assert f(vs(v.handle), 1, 10, None, 0, i64(5), i64(4), 1, outs) == bad
    assert f(vs(v.handle), 1, 0, i64(0), 1, None, None, 0, outs) == bad
    assert f(vs(v.handle), 1, -5, i64(0), 1, None, None, 0, outs) == bad
    assert f(vs(v.handle), 1, 7, i64(0), 1, None, None, 0, outs) == bad                             # 1000 is no multiple of 7
    assert f(vs(v.handle), 1, 2000, i64(0), 1, None, None, 0, outs) == bad
    assert f(None, 1, 10, i64(0), 1, None, None, 0, outs) == bad
    assert f(vs(v.handle), 1, 10, i64(0), 1, None, None, 0, None) == bad
    assert f(vs(v.handle), 1, 10, None, 1, None, None, 0, outs) == bad
    assert f(vs(v.handle), 1, 10, None, 0, i64(0), None, 1, outs) == bad
    assert f(vs(v.handle, 0), 2, 10, i64(0), 1, None, None, 0, outs) == bad
    assert f(vs(v.handle, other.handle), 2, 1, i64(0), 1, None, None, 0, outs) == N.ERR_SIZE_MISMATCH
    assert f(vs(v.handle + 12345), 1, 10, i64(0), 1, None, None, 0, outs) == N.ERR_INVALID_HANDLE
    assert f(vs(long.handle), 1, 4097, i64(0), 1, None, None, 0, outs) == N.ERR_UNSUPPORTED
    message = lib.fmhip_last_error().decode()
    assert "fmhip_select_ranks_batch" in message and "fmhip_sort_by_key" in message
    assert lib.fmhip_block_sort(v.handle, 0, C.byref(h)) == bad
    assert lib.fmhip_block_sort(v.handle, 7, C.byref(h)) == bad
    assert lib.fmhip_block_sort(v.handle, 10, None) == bad
    assert lib.fmhip_block_sort(0, 10, C.byref(h)) == bad
    assert lib.fmhip_block_sort(v.handle + 12345, 10, C.byref(h)) == N.ERR_INVALID_HANDLE
    assert lib.fmhip_block_sort(long.handle, 4097, C.byref(h)) == N.ERR_UNSUPPORTED
    with pytest.raises(ValueError): gpu.block_min(v, 7)
    with pytest.raises(ValueError): gpu.block_order_statistics([v, other], 1, ranks=[0])
    with pytest.raises(ValueError): gpu.block_sort(v, 7)
    after = gpu.pool_stats()
    assert after.n_kernel_launches == before.n_kernel_launches and after.n_live_vectors == before.n_live_vectors and after.bytes_in_use == before.bytes_in_use
    assert h.value == 0 and all(x == 0 for x in outs)
    # under an expectation communicator both calls act on this rank's own vector
    try:
        gpu.set_expectation_comm(2, 0, lambda local: np.stack([local, local]))
        with limit(60):
            top = gpu.block_max(v, 10).realizations.to_float32()
            s = gpu.block_sort(v.v1s1("MULT_S", -1.0), 10).realizations.to_float32()
    finally:
        gpu.set_expectation_comm(1, 0, None)
    assert (top == np.arange(n, dtype=np.float32).reshape(100, 10).max(axis=1)).all() and (s == np.sort(-np.arange(n, dtype=np.float32).reshape(100, 10), axis=1).ravel()).all()


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
                for call in (lambda: gpu.block_min(y, 64), lambda: gpu.block_sort(y, 2), lambda: gpu.block_order_statistics([base, y], 4096, ranges=[(0, 4095)])):
                    if read_error is None:
                        call()
                    else:
                        with pytest.raises(gpu.FmhipError) as info:
                            call()
                        assert info.value.code == read_error and "given up" in str(info.value)
    finally:
        gpu.set_fusion(prev)


def test_the_host_switch_gives_identical_results(gpu):
    rng = np.random.default_rng(6)
    a = family("nan10", 4096 * 3, 4096, rng)
    def everything():
        v = gpu.RandomVariableHip(1.25, a)
        out = []
        for block in (1, 4, 96, 4096):
            ranks, ranges = selectors(block)
            for row in gpu.block_order_statistics([v, v.mult(2.0)], block, ranks * 2, ranges * 2):      # 10 ranks, 8 ranges: taken in groups
                assert len(row) == 18 and all(rv.getFiltrationTime() == 1.25 for rv in row)
                out += [bits(rv.realizations.to_float32()) for rv in row]
            out += [bits(rv.realizations.to_float32()) for rv in gpu.block_quantiles(v, block, [0.99, 0.5]) + gpu.block_quantile_expectations(v, block, [(0.0, 0.05), (0.9, 0.5)])]
            out += [bits(gpu.block_sort(v, block).realizations.to_float32()), bits(gpu.block_min(v, block).realizations.to_float32()), bits(gpu.block_max(v, block).realizations.to_float32())]
        return out
    with limit(120):
        launches = gpu.pool_stats().n_kernel_launches
        device = everything()
        assert gpu.pool_stats().n_kernel_launches >= launches + 4 * 7
        with knob_off():
            host = everything()
    assert len(device) == len(host)
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
a[::11] = np.nan
res, info = {}, {}
SELECT = {3: ([0, 2, 1], [(0, 2), (1, 1)]), 2049: ([0, 2048, 1024, 19], [(0, 2048), (0, 102), (1024, 2048)])}

def everything(tag, v):
    for bl in (3, 2049):
        row = fm.block_order_statistics([v, v], bl, *SELECT[bl])[1]
        for j, rv in enumerate(row): res["%%s_%%d_%%d" %% (tag, bl, j)] = rv.realizations.to_float32()
        res["%%s_%%d_sort" %% (tag, bl)] = fm.block_sort(v, bl).realizations.to_float32()
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
    ranks, lo, hi = (C.c_int64 * 2)(0, 2), (C.c_int64 * 1)(0), (C.c_int64 * 1)(2)
    info["status"] = [lib.fmhip_block_order_statistics(two, 2, 3, ranks, 2, lo, hi, 1, outs), lib.fmhip_block_order_statistics(two, 1, 2049, ranks, 1, None, None, 0, outs),
                      lib.fmhip_block_sort(V.handle, 3, C.byref(h))]
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
        kept["stored"] = fm.block_order_statistics([V, V], 2049, *SELECT[2049])[1]
        kept["pending"] = fm.block_order_statistics([pend, V], 3, *SELECT[3])[0]
        kept["sort"] = fm.block_sort(pend, 2049)
    t = threading.Thread(target=other); t.start(); t.join()
    for j, rv in enumerate(kept["stored"]): res["stored_2049_%%d" %% j] = rv.realizations.to_float32()      # read back on the main thread
    for j, rv in enumerate(kept["pending"]): res["pending_3_%%d" %% j] = rv.realizations.to_float32()
    res["pending_2049_sort"] = kept["sort"].realizations.to_float32()
    res["stored_in"], res["pending_in"] = V.to_float32(), pend.to_float32()
    kept.clear()
np.savez(out_path, **res)
print("RESULT " + json.dumps(info))
fm.shutdown()
'''
SELECT = {3: ([0, 2, 1], [(0, 2), (1, 1)]), 2049: ([0, 2048, 1024, 19], [(0, 2048), (0, 102), (1024, 2048)])}


def _run_front(tmp_path, mode):
    script = tmp_path / "fronts.py"
    script.write_text(_FRONTS % {"root": ROOT})
    out_path = tmp_path / (mode + ".npz")
    r = subprocess.run([sys.executable, str(script), mode, str(out_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    info = json.loads([line for line in r.stdout.splitlines() if line.startswith("RESULT ")][-1][7:])
    return info, dict(np.load(out_path))


def _check_statistics(gpu, res, tag, a, bl):
    for j, want in enumerate(gpu.block_order_statistics_host(a, bl, *SELECT[bl])): assert (bits(res[f"{tag}_{bl}_{j}"]) == bits(want)).all(), (tag, bl, j)


def _check_everything(gpu, res, tag, a):
    for bl in (3, 2049):
        _check_statistics(gpu, res, tag, a, bl)
        assert (bits(res[f"{tag}_{bl}_sort"]) == bits(gpu.block_sort_host(a, bl))).all(), (tag, bl)


@pytest.mark.parametrize("mode", ["devices_one", "devices_two", "threads"])
def test_device_list_and_thread_engines(gpu, mode, tmp_path):
    """In a process of its own.  A device list of ONE shard is that shard's call: everything equals the definition, on stored and on pending
    operands.  A list of two ({0, 0}) answers FMHIP_ERR_UNSUPPORTED for both calls — nothing launched, nothing left behind — and the
    mirror's host path (FMHIP_DEVICE_NESTED=0) gives the definition's results there.  Thread engines: a thread that owns neither the vector
    nor the pending one selects and sorts; the outputs are read on the main thread."""
    block, m = 2049, 37
    rng = np.random.default_rng(77)
    a = ((10.0 ** rng.uniform(-8.0, 8.0, block * m)) * np.where(rng.random(block * m) < 0.5, -1.0, 1.0)).astype(np.float32)
    a[::11] = np.nan
    doubled = (a * np.float32(2.0)).astype(np.float32)
    same_in = lambda got, want: bool(((bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))).all())
    info, res = _run_front(tmp_path, mode)
    if mode == "devices_one":
        assert same_in(res["stored_in"], a) and same_in(res["pending_in"], doubled)
        _check_everything(gpu, res, "stored", a)
        _check_everything(gpu, res, "pending", doubled)
    elif mode == "devices_two":
        assert info["status"] == [info["unsupported"]] * 3 and info["unsupported"] == gpu._native.ERR_UNSUPPORTED
        assert "shards" in info["message"]
        assert info["launches"][0] == info["launches"][1] and info["live"][0] == info["live"][1] and info["outputs"] == [0] * 7
        assert same_in(res["host_in"], a)
        _check_everything(gpu, res, "host", a)
    else:
        assert same_in(res["stored_in"], a) and same_in(res["pending_in"], doubled)
        _check_statistics(gpu, res, "stored", a, 2049)
        _check_statistics(gpu, res, "pending", doubled, 3)
        assert (bits(res["pending_2049_sort"]) == bits(gpu.block_sort_host(doubled, 2049))).all()


# ---------------------------------------------------------------- the driver
def test_nested_initial_margin_of_a_forward_against_its_closed_form(gpu):
    """montecarlo.nested_initial_margin_mc: 4096 outer paths at t = 1, 256 inner paths each over δ = 0.04, S0 = 100, r = 5 %, σ = 20 %, T = 2,
    K = 100, the 99 % quantile (rank 2 of 256).  The estimate lies in [IM_cf(3/256) − 4·SE, IM_cf(2/256) + 4·SE] = [9.186, 9.766] widened by
    four standard errors (tests/test_block_order_cpu.py holds the numpy restatement to the same bracket: 9.394 … 9.398 ± 0.033), and the
    same run with the knob off gives the same two numbers to the last bit; so does a smaller run with a block that is no power of two."""
    mc = import_module("finmath-lib-cuda-extensions_amd.montecarlo")
    def run(m, k, seed_outer, seed_inner):
        outer = gpu.BrownianMotionHip(gpu.TimeDiscretization(0.0, 1, T_MARGIN), 1, m, seed_outer)
        inner = gpu.BrownianMotionHip(gpu.TimeDiscretization(T_MARGIN, 1, DELTA), 1, m * k, seed_inner)
        return mc.nested_initial_margin_mc(outer, inner, S0, R, SIGMA, T_MARGIN, DELTA, MATURITY, STRIKE, k, QUANTILE)
    assert quantile_index(INNER_PATHS, QUANTILE) == 2
    prev = gpu.set_fusion(True)
    try:
        with limit(120):
            launches = gpu.pool_stats().n_kernel_launches
            estimate, se = run(OUTER_PATHS, INNER_PATHS, SEED_OUTER, SEED_INNER)
            assert gpu.pool_stats().n_kernel_launches > launches
            on = run(300, 100, 5, 6)
            with knob_off():
                host = run(OUTER_PATHS, INNER_PATHS, SEED_OUTER, SEED_INNER)
                off = run(300, 100, 5, 6)
    finally:
        gpu.set_fusion(prev)
    print("4096 x 256, knob on:", (estimate, se), "knob off:", host)
    print("300 x 100, knob on:", on, "knob off:", off)
    check_margin(estimate, se)
    assert (estimate, se) == host                                    # to the last bit: the host definition is the device's
    assert on == off
