"""Block order statistics without a GPU (include/fmhip.h: fmhip_block_order_statistics_host, fmhip_block_sort_host; host/block_order.hpp;
DESIGN.md §4.23): the DEFINITION against numpy — every block sorted by the uint32 key, ranks as bit patterns, range means against
block_moments_host of the sorted slice taken as one block and against math.fsum within the published bound — on data with ties, ±0,
±inf, denormals and NaNs of both signs; every refusal; the Python mirror's fallback path on host arrays; the host half in a stand-alone
program under AddressSanitizer / UBSan (tests/cpp/test_block_order_host.cpp); the engine's side of the two calls
(csrc/block_order_engine.hpp, the fronts of csrc/sharded.cpp and csrc/abi.cpp) on the test-only null device under AddressSanitizer + UBSan
and ThreadSanitizer (tests/nulldev/block_order.mk: drive_block_order.cpp with the stand-in launcher of null_block_order.cpp,
drive_block_order_absent.cpp without it).  Stand-alone programs only: nothing sanitized is loaded into this process.
And a numpy restatement of montecarlo.nested_initial_margin_mc with the closed-form bracket of tests/test_gpu_block_order.py."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess
from statistics import NormalDist

import numpy as np
import pytest

from test_nested_cpu import chain, wide_range

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NULLDEV = os.path.join(ROOT, "tests", "nulldev")

MAX_BLOCK, MAX_RANKS, MAX_RANGES, SMALL = 4096, 8, 4, 64
QUIET_NAN = 0x7fc00000
# the issue's list: every power of two the padding takes with its neighbours, the regime boundary 64 | 65, the segment boundary 2048 | 2049
BLOCKS = [1, 2, 3, 5, 31, 32, 33, 63, 64, 65, 100, 127, 128, 129, 255, 256, 257, 1000, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096]
FAMILIES = ("wide", "ties", "constant", "ascending", "descending", "zeros", "infinities", "denormals", "nan10", "nan100")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def quantile_index(n, q):
    """random_variable.quantile_index, restated: the position getQuantile(q) returns."""
    return min(max(int(math.floor((n + 1) * (1 - q) - 1 + 0.5)), 0), n - 1)


def selectors(block):
    """The ranks (with a duplicate) and the ranges of the issue."""
    ranks = [0, block - 1, block // 2, quantile_index(block, 0.99), 0]
    ranges = [(0, 0), (0, block - 1), (0, block // 20), (block // 2, block - 1)]
    return ranks, ranges


def family(name, n, block, rng):
    """n float32 of one of FAMILIES; NaNs carry both signs and several payloads."""
    def nans(count):
        payload = rng.integers(1, 1 << 23, count).astype(np.uint32)
        return (np.uint32(0x7f800000) | payload | (rng.integers(0, 2, count).astype(np.uint32) << np.uint32(31))).view(np.float32)
    if name == "wide": return wide_range(n, rng)
    if name == "ties": return rng.choice(np.array([-1.5, 0.25, 3.0], dtype=np.float32), n)
    if name == "constant": return np.full(n, 2.75, dtype=np.float32)
    if name == "ascending": return (np.arange(n, dtype=np.float32) - np.float32(n // 2)) * np.float32(0.37)
    if name == "descending": return ((np.arange(n, dtype=np.float32) - np.float32(n // 2)) * np.float32(0.37))[::-1].copy()
    if name == "zeros":
        a = wide_range(n, rng)
        a[rng.random(n) < 0.6] = 0.0
        a[rng.random(n) < 0.3] = -0.0
        return a
    if name == "infinities":
        a = wide_range(n, rng)
        a[rng.random(n) < 0.05] = np.inf
        a[(np.arange(n) // block) % 2 == 0] = np.where(rng.random(n) < 0.05, -np.inf, a)[(np.arange(n) // block) % 2 == 0]      # every other block has both
        return a
    if name == "denormals":
        a = (rng.integers(0, 1 << 23, n).astype(np.uint32) | (rng.integers(0, 2, n).astype(np.uint32) << np.uint32(31))).view(np.float32).copy()
        some = rng.random(n) < 0.3
        a[some] = wide_range(n, rng)[some]
        return a
    if name == "nan10":
        a = wide_range(n, rng)
        at = rng.random(n) < 0.1
        a[at] = nans(int(at.sum()))
        return a
    if name == "nan100": return nans(n)
    raise KeyError(name)


def keys_of(a):
    u = bits(a).astype(np.uint32)
    k = np.where(u >> 31 != 0, ~u, u | np.uint32(0x80000000)).astype(np.uint32)
    return np.where((u & np.uint32(0x7fffffff)) > np.uint32(0x7f800000), np.uint32(0xffffffff), k).astype(np.uint32)


def sorted_blocks(a, block):
    """[m, block] uint32: every block in ascending key order as bit patterns, NaNs as the quiet NaN — numpy's restatement of s_q."""
    k = np.sort(keys_of(a).reshape(-1, block), axis=1)
    u = np.where(k >> 31 != 0, k & np.uint32(0x7fffffff), ~k).astype(np.uint32)
    return np.where(k == np.uint32(0xffffffff), np.uint32(QUIET_NAN), u).astype(np.uint32)


def check_definition_against_numpy(fm, a, block):
    """The host definition on `a` against the numpy restatement: ranks and the sort as bit patterns; a range mean against block_moments_host
    of the sorted slice taken as one block (bits; NaN for NaN) and within (chain + 1)·2⁻⁵³·Σ|terms| of math.fsum."""
    ranks, ranges = selectors(block)
    s = sorted_blocks(a, block)
    got = fm.block_order_statistics_host(a, block, ranks, ranges)
    assert len(got) == len(ranks) + len(ranges)
    for r, g in zip(ranks, got): assert (bits(g) == s[:, r]).all(), (block, r)
    assert (bits(fm.block_sort_host(a, block)) == s.ravel()).all(), block
    for (lo, hi), g in zip(ranges, got[len(ranks):]):
        count = hi - lo + 1
        piece = np.ascontiguousarray(s[:, lo:hi + 1]).view(np.float32)
        want = fm.block_moments_host(piece.ravel(), count, ("mean",))[0]
        assert (bits(g) == np.where(np.isnan(want), np.uint32(QUIET_NAN), bits(want))).all(), (block, lo, hi)
        for q in range(piece.shape[0]):
            terms = [float(x) for x in piece[q]]
            if not all(math.isfinite(t) for t in terms):
                both = any(t == math.inf for t in terms) and any(t == -math.inf for t in terms)
                if any(math.isnan(t) for t in terms) or both: assert bits(g)[q] == QUIET_NAN, (block, lo, hi, q)
                else: assert math.isinf(float(g[q])), (block, lo, hi, q)
                continue
            exact, bound = math.fsum(terms), (chain(count) + 1) * 2.0 ** -53 * math.fsum(abs(t) for t in terms)
            mean = exact / count
            # the output is fl32(fl64(S / count)): the sum's bound, the division's rounding and half an ulp of fp32 (of a denormal: 2⁻¹⁵⁰)
            slack = bound / count + abs(mean) * (2.0 ** -24 + 2.0 ** -52) + 2.0 ** -150
            assert abs(float(g[q]) - mean) <= slack, (block, lo, hi, q, float(g[q]), mean, slack)


def test_the_constants_are_the_headers():
    text = open(os.path.join(ROOT, "finmath-lib-cuda-extensions_amd", "host", "block_order.hpp")).read()
    assert int(re.search(r"FM_BLOCK_ORDER_MAX = (\d+)", text).group(1)) == MAX_BLOCK
    assert int(re.search(r"FM_BLOCK_ORDER_MAX_RANKS = (\d+)", text).group(1)) == MAX_RANKS and int(re.search(r"FM_BLOCK_ORDER_MAX_RANGES = (\d+)", text).group(1)) == MAX_RANGES
    kernel = open(os.path.join(ROOT, "finmath-lib-cuda-extensions_amd", "csrc", "block_order_kernel.h")).read()
    assert int(re.search(r"FM_ORDER_SMALL = (\d+)", kernel).group(1)) == SMALL
    assert {SMALL, SMALL + 1, 2048, 2049, MAX_BLOCK} <= set(BLOCKS)


def test_the_key_is_the_order_statistics_key(fm):
    """host/block_order.hpp restates key_of_bits of csrc/order_stats.hpp: on a block with every kind of value the order is that of
    java.util.Arrays.sort(float[]), and the definition's sort is numpy's sort by the restated key."""
    rng = np.random.default_rng(1)
    a = np.concatenate([family(f, 64, 64, rng) for f in FAMILIES])
    s = sorted_blocks(a, a.size)[0].view(np.float32)
    finite = s[~np.isnan(s)]
    assert (finite[1:] >= finite[:-1]).all()                                                       # ascending values …
    zeros = np.flatnonzero(finite == 0)
    signs = bits(finite[zeros]) >> 31
    assert (np.diff(signs.astype(np.int64)) <= 0).all()                                            # … −0.0 before +0.0 …
    assert np.isnan(s[finite.size:]).all()                                                         # … NaNs last
    assert (bits(fm.block_sort_host(a, a.size)) == bits(s)).all()


@pytest.mark.parametrize("block", BLOCKS)
def test_the_definition_equals_numpy(fm, block):
    rng = np.random.default_rng(block)
    for k, name in enumerate(FAMILIES):
        m = (1, 2, 3, 5)[k % 4] if block > 256 else 5
        check_definition_against_numpy(fm, family(name, m * block, block, rng), block)


def test_a_block_is_a_function_of_its_multiset(fm):
    rng = np.random.default_rng(2)
    for block in (5, 100, 2049):
        a = family("nan10", block, block, rng)
        ranks, ranges = selectors(block)
        alone = fm.block_order_statistics_host(a, block, ranks, ranges)
        moved = np.concatenate([family("wide", block, block, rng), rng.permutation(a), family("ties", block, block, rng)])
        among = fm.block_order_statistics_host(moved, block, ranks, ranges)
        for x, y in zip(alone, among): assert bits(x)[0] == bits(y)[1]
        one_by_one = [fm.block_order_statistics_host(a, block, [r], [])[0] for r in ranks] + [fm.block_order_statistics_host(a, block, [], [g])[0] for g in ranges]
        for x, y in zip(alone, one_by_one): assert (bits(x) == bits(y)).all()


def test_more_selectors_than_a_call_takes_are_taken_in_groups(fm):
    rng = np.random.default_rng(3)
    a = wide_range(3 * 50, rng)
    ranks, ranges = list(range(0, 50, 3)), [(k, k + 5) for k in range(0, 40, 4)]                    # 17 ranks, 10 ranges
    got = fm.block_order_statistics_host(a, 50, ranks, ranges)
    s = sorted_blocks(a, 50)
    for r, g in zip(ranks, got): assert (bits(g) == s[:, r]).all()
    for g, w in zip(got[len(ranks):], [fm.block_order_statistics_host(a, 50, [], [x])[0] for x in ranges]): assert (bits(g) == bits(w)).all()


def test_refusals(fm):
    lib = fm.lib()
    N = fm._native
    a = np.arange(12, dtype=np.float32)
    pa, out = a.ctypes.data_as(C.c_void_p), np.zeros(64, dtype=np.float32)
    po = out.ctypes.data_as(C.c_void_p)
    i64 = lambda *xs: (C.c_int64 * max(len(xs), 1))(*xs)
    bad, unsupported = N.ERR_INVALID_ARGUMENT, N.ERR_UNSUPPORTED
    host = lib.fmhip_block_order_statistics_host
    assert host(pa, 12, 3, i64(0, 2), 2, i64(0), i64(2), 1, po) == 0
    assert host(pa, 12, 3, i64(0, 0), 2, None, None, 0, po) == 0                                     # duplicate ranks are allowed
    assert host(pa, 12, 3, None, 0, None, None, 0, po) == bad                                        # no selector
    assert host(pa, 12, 3, i64(*range(9)), 9, None, None, 0, po) == bad
    assert host(pa, 12, 3, i64(0), -1, None, None, 0, po) == bad
    assert host(pa, 12, 3, None, 0, i64(0, 0, 0, 0, 0), i64(0, 0, 0, 0, 0), 5, po) == bad
    assert host(pa, 12, 3, i64(3), 1, None, None, 0, po) == bad                                      # a rank outside the block
    assert host(pa, 12, 3, i64(-1), 1, None, None, 0, po) == bad
    assert host(pa, 12, 3, None, 0, i64(0), i64(3), 1, po) == bad                                    # a range outside the block
    assert host(pa, 12, 3, None, 0, i64(-1), i64(1), 1, po) == bad
    assert host(pa, 12, 3, None, 0, i64(2), i64(1), 1, po) == bad                                    # from > to
    assert host(pa, 12, 0, i64(0), 1, None, None, 0, po) == bad
    assert host(pa, 12, -4, i64(0), 1, None, None, 0, po) == bad
    assert host(pa, 12, 5, i64(0), 1, None, None, 0, po) == bad                                      # 12 is no multiple of 5
    assert host(None, 12, 3, i64(0), 1, None, None, 0, po) == bad
    assert host(pa, 12, 3, i64(0), 1, None, None, 0, None) == bad
    assert host(pa, 12, 3, None, 1, None, None, 0, po) == bad
    assert host(pa, 12, 3, None, 0, i64(0), None, 1, po) == bad
    long = np.zeros(2 * 4097, dtype=np.float32)
    assert host(long.ctypes.data_as(C.c_void_p), long.size, 4097, i64(0), 1, None, None, 0, po) == unsupported
    message = lib.fmhip_last_error().decode()
    assert "fmhip_select_ranks_batch" in message and "fmhip_sort_by_key" in message
    sort = lib.fmhip_block_sort_host
    assert sort(pa, 12, 4, po) == 0
    for n, block, x, o in ((12, 0, pa, po), (12, -1, pa, po), (12, 5, pa, po), (0, 1, pa, po), (12, 4, None, po), (12, 4, pa, None)):
        assert sort(x, n, block, o) == bad, (n, block)
    assert sort(long.ctypes.data_as(C.c_void_p), long.size, 4097, long.ctypes.data_as(C.c_void_p)) == unsupported
    assert "fmhip_select_ranks_batch" in lib.fmhip_last_error().decode() and "fmhip_sort_by_key" in lib.fmhip_last_error().decode()
    with pytest.raises(fm.FmhipError): fm.block_order_statistics_host(a, 5, [0])
    with pytest.raises(fm.FmhipError): fm.block_order_statistics_host(a, 3, [3])
    with pytest.raises(fm.FmhipError): fm.block_sort_host(a, 5)
    # the device entry points exist and refuse without an engine
    one, h = (C.c_int64 * 1)(1), (C.c_int64 * 12)()
    if not lib.fmhip_is_initialized():
        assert lib.fmhip_block_order_statistics(one, 1, 3, i64(0), 1, None, None, 0, h) == N.ERR_NOT_INITIALIZED
        assert lib.fmhip_block_sort(1, 3, h) == N.ERR_NOT_INITIALIZED


def test_the_mirror_on_deterministic_variables_and_its_checks(fm):
    c = fm.RandomVariableHip(2.5, 3.0)
    row, = fm.block_order_statistics([c], 8, ranks=[0, 7], ranges=[(0, 7)])
    assert all(rv.isDeterministic() and rv.getAverage() == 3.0 and rv.getFiltrationTime() == 2.5 for rv in row) and len(row) == 3
    assert fm.block_min(c, 4).getAverage() == 3.0 and fm.block_max(c, 4).getAverage() == 3.0
    assert fm.block_sort(c, 4).isDeterministic() and fm.block_sort(c, 4).getFiltrationTime() == 2.5
    q, = fm.block_quantiles(c, 100, [0.99])
    e, = fm.block_quantile_expectations(c, 100, [(0.0, 0.05)])
    assert q.getAverage() == 3.0 and e.getAverage() == 3.0
    with pytest.raises(ValueError): fm.block_order_statistics([c], 8)
    with pytest.raises(ValueError): fm.block_order_statistics([c], 8, ranks=[8])
    with pytest.raises(ValueError): fm.block_order_statistics([c], 8, ranges=[(3, 2)])
    with pytest.raises(ValueError): fm.block_order_statistics([c], 0, ranks=[0])
    with pytest.raises(ValueError): fm.block_order_statistics([], 8, ranks=[0])
    with pytest.raises(TypeError): fm.block_min(np.zeros(4), 2)
    with pytest.raises(ValueError): fm.block_sort(c, 0)
    # a block above 4096 elements is UNSUPPORTED for every kind of operand, after the checks of the selectors
    for call in (lambda: fm.block_sort(c, 4097), lambda: fm.block_order_statistics([c], 4097, ranks=[0]), lambda: fm.block_min(c, 10**6)):
        with pytest.raises(fm.FmhipError) as info: call()
        assert info.value.code == fm._native.ERR_UNSUPPORTED and "fmhip_sort_by_key" in str(info.value)
    with pytest.raises(ValueError): fm.block_order_statistics([c], 4097, ranks=[4097])
    assert fm.block_sort(c, 4096).isDeterministic()


def test_the_quantile_conventions_are_getquantiles(fm):
    """block_quantiles and block_quantile_expectations name their selectors by the index formulas of getQuantile and getQuantileExpectation:
    on host arrays (the definition) they give what numpy gives with those formulas."""
    nested = __import__("importlib").import_module("finmath-lib-cuda-extensions_amd.nested")
    assert nested.quantile_index(256, 0.99) == 2 and quantile_index(256, 0.99) == 2
    rng = np.random.default_rng(4)
    block, m = 100, 7
    a = wide_range(block * m, rng)
    s = np.sort(a.reshape(m, block), axis=1)
    for q in (0.0, 0.01, 0.5, 0.95, 1.0):
        assert (fm.block_order_statistics_host(a, block, [nested.quantile_index(block, q)])[0] == s[:, quantile_index(block, q)]).all()
    position = lambda q: min(max(int(math.floor((block + 1) * q - 1 + 0.5)), 0), block - 1)
    got = fm.block_order_statistics_host(a, block, [], [(position(0.0), position(0.05))])[0]
    assert np.allclose(got, s[:, 0:position(0.05) + 1].astype(np.float64).mean(axis=1), rtol=1e-6)


def test_host_half_under_the_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("needs g++")
    exe = tmp_path / "block_order_host"
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-ffp-contract=off",
                        os.path.join(ROOT, "tests", "cpp", "test_block_order_host.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "block order host ok" in r.stdout and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stdout[-1500:] + r.stderr[-3000:]


def test_the_kernels_are_in_the_library(fm):
    """A missing kernel is an error, never a fallback: the launcher is a weak reference, so the library must be shown to hold it."""
    out = subprocess.check_output(["nm", "-D", "--defined-only", fm._native.LIB_PATH], text=True) + subprocess.check_output(["nm", "--defined-only", fm._native.LIB_PATH], text=True, stderr=subprocess.DEVNULL)
    for name in ("launch_block_order", "launch_sort_done"):
        assert name in out, name
    blob = open(fm._native.LIB_PATH, "rb").read()
    for kernel in (b"fm_block_order_small_kernel", b"fm_block_order_medium_kernel"):
        assert kernel in blob, kernel


# ---------------------------------------------------------------- the engine's side on the null device
@pytest.fixture(scope="module")
def built():
    if not shutil.which("g++") or not os.path.exists("/opt/rocm/include/hip/hip_runtime_api.h"):
        pytest.skip("needs g++ and the HIP headers")
    r = subprocess.run(["make", "-C", NULLDEV, "-f", "block_order.mk", "-j8", "block_order_asan", "block_order_tsan", "block_order_absent_asan"], capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return os.path.join(NULLDEV, "build")


def _env(tmp_path, env):
    return dict(os.environ, FMHIP_JIT_CACHE_DIR=str(tmp_path / "code_objects"), FMHIP_JIT_PACK_DIR="off", FMHIP_RING_BYTES="16384", FMHIP_ARENA_BYTES="4096",
                ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1", TSAN_OPTIONS="halt_on_error=1", **env)


@pytest.mark.parametrize("env", [{}, {"FMNULL_DEVICES": "2"}, {"FMNULL_DEVICES": "3"}, {"FMNULL_THREAD_ENGINES": "1"}])
def test_engine_pass_is_clean_under_the_sanitizers(built, tmp_path, env):
    """drive_block_order: both calls on vectors of real data with NaNs, infinities and signed zeros, blocks of both regimes and around
    their boundaries, one and four vectors per call, checked against the definition (the stand-in sums a range as a wave does); pending
    operands, a second thread releasing the inputs of pending operands during the call, every argument error — on one engine and behind a
    device list of one shard, behind 2 and 3 shards (FMHIP_ERR_UNSUPPORTED, nothing left behind), with thread engines (a caller that does
    not own the vectors)."""
    full = _env(tmp_path, env)
    a = subprocess.run([os.path.join(built, "drive_block_order_asan")], capture_output=True, text=True, timeout=600, env=full)
    assert a.returncode == 0 and "Sanitizer" not in a.stderr and "runtime error" not in a.stderr, a.stdout[-500:] + a.stderr[-6000:]
    assert a.stdout.count("block order done") == 2 and a.stderr == ""
    assert ("a device list of one shard: checked" in a.stdout) == (not env)
    t = subprocess.run([os.path.join(built, "drive_block_order_tsan")], capture_output=True, text=True, timeout=600, env=full)
    assert t.returncode == 0 and "ThreadSanitizer" not in t.stderr, t.stdout[-500:] + t.stderr[-6000:]
    assert t.stdout.count("block order done") == 2 and t.stderr == ""


def test_a_failing_allocation_inside_a_block_order_pass_leaves_nothing_behind(built, tmp_path):
    """One fmhip_block_order_statistics of two vectors, two ranks and one range takes SIX buffers from the pool, its outputs.  The hook
    FMHIP_TEST_FAIL_ALLOC_AT is set on each of them (their positions from a counting run), and once where nothing reaches it: the call
    answers FMHIP_OK or FMHIP_ERR_OUT_OF_MEMORY, a result it gives is right, outputs of a failed call are not written, live vectors and bytes
    in use are what they were, the same call succeeds afterwards (the driver checks all of it), and the process ends without a leak."""
    exe = os.path.join(built, "drive_block_order_asan")
    counting = subprocess.run([exe, "failure"], capture_output=True, text=True, timeout=600, env=_env(tmp_path, {}))
    assert counting.returncode == 0 and "Sanitizer" not in counting.stderr, counting.stdout[-500:] + counting.stderr[-6000:]
    before, inside, status = map(int, re.search(r"failure: (\d+) allocations before the call, (\d+) in it, status (-?\d+)", counting.stdout).groups())
    assert inside == 6 and status == 0
    for at in list(range(before + 1, before + inside + 1)) + [10**9]:
        r = subprocess.run([exe, "failure"], capture_output=True, text=True, timeout=600, env=_env(tmp_path, {"FMHIP_TEST_FAIL_ALLOC_AT": str(at)}))
        assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr and r.stderr == "", (at, r.stdout[-500:] + r.stderr[-6000:])
        assert "failure done" in r.stdout
        failed = int(re.search(r"status (-?\d+)", r.stdout).group(1)) != 0
        assert failed == (at <= before + inside), (at, r.stdout)


@pytest.mark.parametrize("env", [{}, {"FMNULL_DEVICES": "2"}, {"FMNULL_THREAD_ENGINES": "1"}])
def test_a_build_without_the_kernel_answers_unsupported(built, tmp_path, env):
    a = subprocess.run([os.path.join(built, "drive_block_order_absent_asan")], capture_output=True, text=True, timeout=600, env=_env(tmp_path, env))
    assert a.returncode == 0 and "Sanitizer" not in a.stderr and "runtime error" not in a.stderr, a.stdout[-500:] + a.stderr[-6000:]
    assert a.stdout.count("block order absent done") == 2


# ---------------------------------------------------------------- the driver, restated in numpy
S0, R, SIGMA, T_MARGIN, DELTA, MATURITY, STRIKE = 100.0, 0.05, 0.2, 1.0, 0.04, 2.0, 100.0
OUTER_PATHS, INNER_PATHS, QUANTILE = 4096, 256, 0.99
SEED_OUTER, SEED_INNER = 27182, 1000


def closed_form_margin(p):
    """IM_cf(p): the margin at level p for the MEAN outer state S0·e^{rt} — the p-quantile of the inner P&L of a forward, negated."""
    z = NormalDist().inv_cdf(p)
    growth = math.exp((R - 0.5 * SIGMA * SIGMA) * DELTA + SIGMA * math.sqrt(DELTA) * z) - 1.0
    return -(S0 * math.exp(R * T_MARGIN) * growth - STRIKE * math.exp(-R * MATURITY) * (math.exp(R * (T_MARGIN + DELTA)) - math.exp(R * T_MARGIN)))


def check_margin(estimate, standard_error):
    """The bracket of the issue: the order statistic i of k estimates a quantile between the levels i/k and (i + 1)/k; the margin is linear
    in the outer state, so its mean over the outer paths is the closed form at the mean state."""
    i = quantile_index(INNER_PATHS, QUANTILE)
    low, high = closed_form_margin((i + 1) / INNER_PATHS), closed_form_margin(i / INNER_PATHS)
    print(f"E[IM] = {estimate:.4f} +- {standard_error:.4f}; bracket [{low:.3f}, {high:.3f}] widened by 4 SE")
    assert i == 2 and low < high
    assert low - 4 * standard_error <= estimate <= high + 4 * standard_error


def test_the_numpy_restatement_of_the_initial_margin_lies_in_the_closed_form_bracket(fm):
    """montecarlo.nested_initial_margin_mc restated on numpy's draws (the same law, other numbers than the device's Philox), over four seeds,
    the quantile per outer path taken by the DEFINITION (block_quantiles' rank through fmhip_block_order_statistics_host on the fp32 P&L)
    and, beside it, by numpy's sort: the same margins bit for bit, and their mean inside [9.186, 9.766] widened by four standard errors."""
    assert abs(closed_form_margin(3 / 256) - 9.186) < 2e-3 and abs(closed_form_margin(2 / 256) - 9.766) < 2e-3
    drift = R - 0.5 * SIGMA * SIGMA
    for seed in (1, 2, 3, 4):
        rng = np.random.default_rng(seed)
        x = math.log(S0) + drift * T_MARGIN + SIGMA * math.sqrt(T_MARGIN) * rng.standard_normal(OUTER_PATHS)
        inner = np.repeat(x, INNER_PATHS) + drift * DELTA + SIGMA * math.sqrt(DELTA) * rng.standard_normal(OUTER_PATHS * INNER_PATHS)
        change = STRIKE * (math.exp(-R * (MATURITY - T_MARGIN - DELTA)) - math.exp(-R * (MATURITY - T_MARGIN)))
        pnl = (np.exp(inner) - np.repeat(np.exp(x), INNER_PATHS) - change).astype(np.float32)
        rank = quantile_index(INNER_PATHS, QUANTILE)
        margin = -fm.block_order_statistics_host(pnl, INNER_PATHS, [rank])[0].astype(np.float64)
        assert (bits(-np.sort(pnl.reshape(OUTER_PATHS, INNER_PATHS), axis=1)[:, rank]) == bits(margin.astype(np.float32))).all()
        check_margin(float(margin.mean()), float(margin.std() / math.sqrt(OUTER_PATHS)))
