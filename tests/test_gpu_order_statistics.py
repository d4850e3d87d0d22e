"""Order statistics on the device (include/fmhip.h: fmhip_select_ranks_batch, fmhip_rank_sums_batch, fmhip_count_not_above) through the
C-ABI: a selected value is an element of the vector, so the answers are those of a sort — bit for bit; the oracle is numpy's sort on the
keys of java.util.Arrays.sort(float[]) (-0 before +0, every NaN equal and last).  No test here asks the device for anything out of
range: bad arguments are refused on the host before a launch."""
import math
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def keys(a):
    u = np.asarray(a, dtype=np.float32).view(np.uint32)
    k = np.where(u >> 31 != 0, ~u, u | np.uint32(0x80000000)).astype(np.uint32)
    k[(u & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)] = np.uint32(0xFFFFFFFF)
    return k


def java_sorted(a):
    a = np.asarray(a, dtype=np.float32)
    return a[np.argsort(keys(a), kind="stable")]


def same_bits(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float32).astype(np.float64)
    return bool(np.all((got.view(np.uint64) == want.view(np.uint64)) | (np.isnan(got) & np.isnan(want))))


def rank_sweep(n, rng):
    return np.unique(np.clip(np.concatenate([[0, 1, n // 2, n - 2, n - 1], rng.integers(0, n, 11)]), 0, n - 1)).astype(np.int64)


def inputs(n, rng):
    u = rng.random(n, dtype=np.float32)
    yield "uniform", u
    yield "normal", rng.standard_normal(n).astype(np.float32)
    yield "clustered", np.clip(np.exp(0.3 * rng.standard_normal(n)), 0.5, 1.999).astype(np.float32)
    yield "payoff", np.maximum(rng.standard_normal(n) - 0.2, 0.0).astype(np.float32)
    yield "constant", np.full(n, 1.25, dtype=np.float32)
    yield "two values", np.where(u < 0.3, np.float32(-3.5), np.float32(7.0)).astype(np.float32)
    yield "denormals", (rng.integers(-40, 40, n) * np.float32(1e-45)).astype(np.float32)
    z = np.where(u < 0.5, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
    yield "signed zeros", z
    special = rng.standard_normal(n).astype(np.float32)
    special[::7] = np.inf; special[3::11] = -np.inf
    bits = special.view(np.uint32)
    bits[5::13] = 0x7FC00000; bits[6::17] = 0xFFC00001; bits[1::19] = 0x7F800123        # NaNs of both signs, several payloads
    yield "specials", special
    yield "all NaN", np.full(n, np.nan, dtype=np.float32)


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 2047, 2048, 2049, 50_001])
def test_select_is_the_sorted_sample(gpu, n):
    rng = np.random.default_rng(n)
    for name, a in inputs(n, rng):
        v = gpu.DeviceVector.from_host(a)
        ranks = rank_sweep(n, rng)
        got = v.select_ranks(ranks)
        want = java_sorted(a)[ranks]
        assert same_bits(got, want), (name, n)
        if name == "signed zeros":
            assert (np.signbit(got) == np.signbit(want)).all()


@pytest.mark.parametrize("n", [1_000_000, (1 << 24) + 3])
def test_select_large(gpu, n):
    rng = np.random.default_rng(7)
    for name in ("normal", "payoff"):
        a = rng.standard_normal(n).astype(np.float32)
        if name == "payoff": a = np.maximum(a, 0.0)
        ranks = rank_sweep(n, rng)
        assert same_bits(gpu.DeviceVector.from_host(a).select_ranks(ranks), java_sorted(a)[ranks]), (name, n)


def test_batch_is_the_single_calls_and_four_launches(gpu):
    rng = np.random.default_rng(11)
    n, count = 20_001, 200
    data = [np.maximum(rng.standard_normal(n) + 0.01 * k, 0.0).astype(np.float32) if k % 2 else rng.standard_normal(n).astype(np.float32) for k in range(count)]
    vs = [gpu.DeviceVector.from_host(a) for a in data]
    q95 = min(max(int(math.floor((n + 1) * (1 - 0.95) - 1 + 0.5)), 0), n - 1)      # the position getQuantile(0.95) returns
    ranks = np.array([q95, n // 2, n - 1 - n // 20], dtype=np.int64)
    gpu.synchronize()
    before = gpu.pool_stats().n_kernel_launches
    got = gpu.select_ranks_batch(vs, ranks)
    assert gpu.pool_stats().n_kernel_launches - before <= 4           # independent of the number of vectors
    for k in range(count):
        assert same_bits(got[k], java_sorted(data[k])[ranks]), k
    for k in (0, 1, 57, 199):
        assert same_bits(vs[k].select_ranks(ranks), got[k])
    q = gpu.quantiles(vs, 0.95)
    assert same_bits(q, got[:, 0])


def test_rank_sums(gpu):
    rng = np.random.default_rng(3)
    n = 50_001
    a = rng.standard_normal(n).astype(np.float32)
    a[::3] = np.float32(0.5)                                            # ties that straddle both ends of a range
    v = gpu.DeviceVector.from_host(a)
    s = java_sorted(a).astype(np.float64)
    scale = np.abs(s).sum()
    lo, hi = int(np.searchsorted(s, 0.5, "left")), int(np.searchsorted(s, 0.5, "right")) - 1
    for i0, i1 in [(0, n - 1), (0, 0), (n - 1, n - 1), (17, 17), (100, 40_000), (lo + 5, hi - 5), (lo - 3, lo + 3), (hi - 3, hi + 3), (lo + 1, n - 1), (0, hi - 1)]:
        assert abs(v.rank_sum(i0, i1) - math.fsum(s[i0:i1 + 1])) <= 1e-13 * scale, (i0, i1)
    assert abs(v.rank_sum(0, n - 1) - v.moments().sum) <= 1e-13 * scale
    ints = gpu.DeviceVector.from_host((np.arange(5000) % 17 - 8).astype(np.float32))
    si = np.sort((np.arange(5000) % 17 - 8).astype(np.float64))
    for i0, i1 in [(0, 4999), (10, 20), (2500, 4000)]:
        assert ints.rank_sum(i0, i1) == si[i0:i1 + 1].sum()
    # NaN tail, and +inf with -inf inside
    b = a.copy(); b[5] = np.nan
    vb = gpu.DeviceVector.from_host(b)
    assert math.isnan(vb.rank_sum(0, n - 1)) and math.isnan(vb.rank_sum(n - 1, n - 1)) and not math.isnan(vb.rank_sum(0, n - 2))
    c = a.copy(); c[7] = np.inf; c[9] = -np.inf
    vc = gpu.DeviceVector.from_host(c)
    assert math.isnan(vc.rank_sum(0, n - 1)) and vc.rank_sum(1, n - 1) == math.inf and vc.rank_sum(0, n - 2) == -math.inf
    assert math.isfinite(vc.rank_sum(1, n - 2))


def test_rank_sum_bits_do_not_depend_on_where_the_vector_came_from(gpu):
    rng = np.random.default_rng(5)
    n = 30_000
    a = rng.standard_normal(n).astype(np.float32)
    x = gpu.DeviceVector.from_host(a)
    stored = x.v1s1("MULT_S", 2.0); stored.to_float32()
    prev = gpu.set_fusion(True)
    try:
        pending = x.v1s1("MULT_S", 2.0)
        rows = [x.v1s1("MULT_S", 2.0) for _ in range(4)]
        want = stored.rank_sum(100, 25_000)
        assert pending.rank_sum(100, 25_000) == want
        import ctypes as C
        h = (C.c_int64 * 4)(*[r.handle for r in rows]); out = (C.c_double * 4)()
        gpu._native.check(gpu.lib().fmhip_rank_sums_batch(h, 4, 100, 25_000, out))
        assert list(out) == [want] * 4
    finally:
        gpu.set_fusion(prev)


def test_count_not_above(gpu):
    rng = np.random.default_rng(9)
    n = 50_001
    a = rng.standard_normal(n).astype(np.float32)
    a[::50] = np.nan
    v = gpu.DeviceVector.from_host(a)
    s = np.sort(a[~np.isnan(a)]).astype(np.float64)
    e = float(s[1234])
    between = (e + float(np.nextafter(np.float32(e), np.float32(np.inf)))) / 2            # a double between two adjacent floats
    bounds = np.array([0.3, -1.0, e, between, np.nextafter(e, -np.inf), 0.3, np.nan, np.inf, -np.inf, 2.5, -1.0])      # unsorted, duplicates, NaN
    got = v.count_not_above(bounds)
    want = np.searchsorted(s, bounds, side="right"); want[np.isnan(bounds)] = 0
    assert (got == want).all()
    assert v.count_not_above([0.0])[0] == np.searchsorted(s, 0.0, side="right")
    many = np.sort(rng.standard_normal(4096))
    assert (v.count_not_above(many) == np.searchsorted(s, many, side="right")).all()
    more = rng.standard_normal(5000)                                   # more than one launch holds
    assert (v.count_not_above(more) == np.searchsorted(s, more, side="right")).all()


def test_arguments_are_checked_on_the_host(gpu):
    import ctypes as C
    lib, N = gpu.lib(), gpu._native
    v = gpu.DeviceVector.from_host(np.arange(10, dtype=np.float32))
    w = gpu.DeviceVector.from_host(np.arange(11, dtype=np.float32))
    out = (C.c_double * 4)()
    for bad in (-1, 10):
        assert lib.fmhip_select_ranks_batch((C.c_int64 * 1)(v.handle), 1, (C.c_int64 * 1)(bad), 1, out) == N.ERR_INVALID_ARGUMENT
    assert lib.fmhip_select_ranks_batch((C.c_int64 * 2)(v.handle, w.handle), 2, (C.c_int64 * 1)(0), 1, out) == N.ERR_SIZE_MISMATCH
    assert lib.fmhip_rank_sums_batch((C.c_int64 * 1)(v.handle), 1, 5, 4, out) == N.ERR_INVALID_ARGUMENT
    assert lib.fmhip_select_ranks_batch((C.c_int64 * 1)(12345678), 1, (C.c_int64 * 1)(0), 1, out) == N.ERR_INVALID_HANDLE
    empty = gpu.DeviceVector.from_host(np.zeros(0, dtype=np.float32))
    assert lib.fmhip_select_ranks_batch((C.c_int64 * 1)(empty.handle), 1, (C.c_int64 * 1)(0), 1, out) == N.ERR_INVALID_ARGUMENT
    assert v.select_ranks([9])[0] == 9.0                                # … and the engine is as it was


def test_mirror_device_path_equals_host_path(gpu, oracle, monkeypatch):
    d = oracle.java_random_doubles(99, 40_001) * 4.0 - 1.0
    f = gpu.RandomVariableHipFactory()
    for fused in (False, True):
        prev = gpu.set_fusion(fused)
        try:
            res = {}
            for knob in ("0", "1"):
                monkeypatch.setenv("FMHIP_DEVICE_ORDER_STATS", knob)
                x = f.createRandomVariable(0.0, d)
                y = x.exp().sub(1.5).floor(0.0)                         # a pending expression, never read
                res[knob] = ([x.getQuantile(q) for q in (0.0, 0.01, 0.05, 0.5, 0.95, 1.0)], [y.getQuantile(q) for q in (0.05, 0.5, 0.99)],
                             x.getQuantileExpectation(0.05, 0.95), y.getQuantileExpectation(0.9, 0.2), x.getHistogram([2.0, -0.5, 0.1, 0.1, 1.0]),
                             y.getHistogram(7, 2.0))
            a, b = res["0"], res["1"]
            assert a[0] == b[0] and a[1] == b[1]
            assert abs(a[2] - b[2]) <= 1e-13 * (1 + abs(a[2])) and abs(a[3] - b[3]) <= 1e-13 * (1 + abs(a[3]))
            assert (a[4] == b[4]).all() and (a[5][0] == b[5][0]).all() and (a[5][1] == b[5][1]).all()
        finally:
            gpu.set_fusion(prev)
    assert f.createRandomVariable(3.0).getQuantile(0.3) == 3.0          # deterministic: as before


def test_given_up_values_are_the_documented_error(gpu):
    """fmhip_vec_give_up_values is a statement about the caller, not an order: where the engine did not store the value, asking for its
    order statistics is the error a read is; where it kept it, the right answer."""
    prev = gpu.set_fusion(True)
    try:
        x = gpu.DeviceVector.from_host(np.arange(4096, dtype=np.float32))
        ys = [x.v1s1("ADD_S", float(k)) for k in range(1, 5)]
        gpu.give_up_values(ys)
        gpu.reduce_moments_batch_end(gpu.reduce_moments_batch_begin(ys), len(ys))
        for k, y in enumerate(ys, start=1):
            try:
                assert y.select_ranks([0, 4095]).tolist() == [float(k), 4095.0 + k]
            except gpu.FmhipError as e:
                assert e.code == gpu._native.ERR_INVALID_ARGUMENT and "given up" in str(e)
    finally:
        gpu.set_fusion(prev)


def test_communicator_answers_for_the_global_sample(gpu):
    rng = np.random.default_rng(21)
    n = 40_000
    a = np.maximum(rng.standard_normal(n), -0.5).astype(np.float32)
    whole = gpu.DeviceVector.from_host(a)
    shards = [gpu.DeviceVector.from_host(a[: n // 2]), gpu.DeviceVector.from_host(a[n // 2:])]
    ranks = np.array([0, 17, n // 2, n - 1], dtype=np.int64)
    bounds = np.array([0.0, -0.5, 1.0])
    want = (whole.select_ranks(ranks), whole.rank_sum(1000, 30_000), whole.count_not_above(bounds))
    s = java_sorted(a)
    try:
        for rank in (0, 1):
            # the other rank's part of every gather, computed the way its engine would: from its shard and the prefixes this rank sends along
            other = a[n // 2:] if rank == 0 else a[: n // 2]
            state = {"calls": 0}

            def gather(local, rank=rank, other=other):
                state["calls"] += 1
                theirs = state["next"](local)
                return np.stack([local, theirs] if rank == 0 else [theirs, local])

            gpu.set_expectation_comm(2, rank, gather)
            mine = shards[rank]
            # select: the other rank's histogram of a pass = total histogram of the whole vector minus this rank's
            passes = []

            def select_theirs(local):
                # local holds this rank's counts; the whole vector's counts of the same pass come from a run without a communicator
                return passes.pop(0) - local

            # record the whole vector's per-pass histograms by asking it with a world of one rank that logs what it gathers
            log = []
            gpu.set_expectation_comm(2, 0, lambda local: (log.append(local.copy()), np.stack([local, np.zeros_like(local)]))[1])
            whole.select_ranks(ranks)
            passes[:] = log; del log[:]
            gpu.set_expectation_comm(2, rank, gather)
            state["next"] = select_theirs
            got = mine.select_ranks(ranks)
            assert same_bits(got, s[ranks]) and same_bits(got, want[0]) and not passes
            # counts
            gpu.set_expectation_comm(2, 0, lambda local: (log.append(local.copy()), np.stack([local, np.zeros_like(local)]))[1])
            whole.count_not_above(bounds)
            passes[:] = log; del log[:]
            gpu.set_expectation_comm(2, rank, gather)
            assert (mine.count_not_above(bounds) == want[2]).all()
            # rank sum: two selected ends (passes as above), then the inner sums in rank order
            gpu.set_expectation_comm(2, 0, lambda local: (log.append(local.copy()), np.stack([local, np.zeros_like(local)]))[1])
            whole.rank_sum(1000, 30_000)
            passes[:] = log; del log[:]
            gpu.set_expectation_comm(2, rank, gather)
            got_sum = mine.rank_sum(1000, 30_000)
            assert abs(got_sum - want[1]) <= 1e-13 * np.abs(a).astype(np.float64).sum()
    finally:
        gpu.set_expectation_comm(1, 0, None)
    assert same_bits(shards[0].select_ranks([0]), java_sorted(a[: n // 2])[[0]])      # local again without one


_OTHER_MODES = r'''
import importlib, json, sys, threading
import numpy as np
sys.path.insert(0, %(root)r)
fm = importlib.import_module("finmath-lib-cuda-extensions_amd")
mode = sys.argv[1]
rng = np.random.default_rng(31)
n = 100_003
a = np.maximum(rng.standard_normal(n), -0.25).astype(np.float32)
ranks = [0, 5, n // 2, n - 2, n - 1]
bounds = [0.0, -0.25, 1.0, -3.0]

def ask(v):
    return {"select": v.select_ranks(ranks).tolist(), "sum": v.rank_sum(1000, 90_000), "counts": v.count_not_above(bounds).tolist()}

if mode == "devices":
    fm.init_devices([0, 0])
    fm.set_fusion(True)
    x = fm.DeviceVector.from_host(a)
    out = {"stored": ask(x), "pending": ask(x.v1s1("MULT_S", 2.0))}
    tiny = fm.DeviceVector.from_host(a[:3])                  # a vector shorter than the shards are many paths apart
    out["tiny"] = tiny.select_ranks([0, 1, 2]).tolist()
else:
    fm.init(0)
    fm.set_thread_engines(True)
    fm.set_fusion(True)
    x = fm.DeviceVector.from_host(a)
    y = x.v1s1("MULT_S", 2.0)                                # pending, owned by the main thread's engine
    out = {}
    def other():
        out["stored"] = ask(x); out["pending"] = ask(y)
    t = threading.Thread(target=other); t.start(); t.join()
print("RESULT " + json.dumps(out))
fm.shutdown()
'''


@pytest.mark.parametrize("mode", ["devices", "threads"])
def test_device_list_and_thread_engines(mode, tmp_path):
    """A device list {0, 0} (every shard runs the pass on its block, the front adds the counts) and a vector of another thread's engine: the
    answers of the whole vector — select and counts exactly, the rank sum within the reassociation bound.  In a process of its own."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / "modes.py"
    script.write_text(_OTHER_MODES % {"root": root})
    r = subprocess.run([sys.executable, str(script), mode], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = json.loads([line for line in r.stdout.splitlines() if line.startswith("RESULT ")][-1][7:])
    rng = np.random.default_rng(31)
    n = 100_003
    a = np.maximum(rng.standard_normal(n), -0.25).astype(np.float32)
    ranks = [0, 5, n // 2, n - 2, n - 1]
    for key, data in (("stored", a), ("pending", a * np.float32(2.0))):
        s = java_sorted(data)
        assert same_bits(out[key]["select"], s[ranks]), key
        assert abs(out[key]["sum"] - math.fsum(s[1000:90_001].astype(np.float64))) <= 1e-13 * np.abs(s).astype(np.float64).sum(), key
        assert out[key]["counts"] == [int(np.searchsorted(np.sort(data).astype(np.float64), b, side="right")) for b in (0.0, -0.25, 1.0, -3.0)], key
    if mode == "devices":
        assert same_bits(out["tiny"], java_sorted(a[:3]))
