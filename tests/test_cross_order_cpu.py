"""CPU-only: order statistics ACROSS vectors and the selection behind their index (include/fmhip.h: fmhip_cross_order_statistics_host,
fmhip_cross_select_host; host/cross_order.hpp, the definition).  The definition against an independent restatement —
numpy's stable argsort of the keys per path — on the issue's grid of K and n with ±0.0, ±inf, denormals, several NaN payloads, ties across
slots, all-equal paths and the same array in two slots; its bit-level properties; every refusal; the host half as a stand-alone program
under AddressSanitizer / UBSan (tests/cpp/test_cross_order_host.cpp); the engine's side of the two calls (csrc/cross_order_engine.hpp, the
fronts of csrc/sharded.cpp and csrc/abi.cpp) on the test-only null device under AddressSanitizer + UBSan and ThreadSanitizer
(tests/nulldev/cross_order.mk).  Stand-alone programs only: nothing sanitized is loaded into this process.

tests/test_gpu_cross_order.py takes its data and its restatement from here."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NULLDEV = os.path.join(ROOT, "tests", "nulldev")
KS = (1, 2, 3, 5, 8, 9, 16, 17, 31, 32)
NS = (1, 63, 64, 65, 2049)
QUIET_NAN = 0x7fc00000
SPECIALS = np.array([0x00000000, 0x80000000, 0x7f800000, 0xff800000, 0x00000001, 0x80000001, 0x007fffff, 0x7fc00000, 0xffc00001, 0x7f800001, 0x7fc12345, 0xffa00001],
                    dtype=np.uint32)                                   # ±0, ±inf, denormals of both signs, NaNs of both signs with payloads


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def cross_data(k, n, rng):
    """k float32 arrays of n elements: wide-range values; about a sixth of the elements special; ties across slots (a path's slot-0 value copied
    into other slots); all-equal paths; with k >= 2 the last slot IS the first array (the same array in two slots)."""
    rows = ((10.0 ** rng.uniform(-6.0, 6.0, (k, n))) * np.where(rng.random((k, n)) < 0.5, -1.0, 1.0)).astype(np.float32)
    u = rows.view(np.uint32)
    special = rng.random((k, n)) < 1.0 / 6.0
    u[special] = SPECIALS[rng.integers(0, SPECIALS.size, int(special.sum()))]
    tie = rng.random((k, n)) < 0.2
    u[:] = np.where(tie, u[0][None, :], u)
    equal = rng.random(n) < 0.1
    u[:, equal] = u[k // 2][equal][None, :]
    arrays = [np.ascontiguousarray(rows[i]) for i in range(k)]
    if k >= 2: arrays[k - 1] = arrays[0]
    return arrays


def keys_of(u):
    """The 32-bit key of the order statistics, restated: NaN -> 0xffffffff, negative -> ~u, else u | 0x80000000."""
    u = u.astype(np.uint32)
    nan = (u & np.uint32(0x7fffffff)) > np.uint32(0x7f800000)
    return np.where(nan, np.uint32(0xffffffff), np.where((u >> np.uint32(31)) != 0, ~u, u | np.uint32(0x80000000))).astype(np.uint32)


def bits_of_keys(keys):
    return np.where(keys == np.uint32(0xffffffff), np.uint32(QUIET_NAN), np.where((keys >> np.uint32(31)) != 0, keys & np.uint32(0x7fffffff), ~keys)).astype(np.uint32)


def restated(arrays):
    """(value bits [k, n], slots [k, n]) of all ranks: numpy's stable argsort of the keys per path."""
    keys = keys_of(np.stack([bits(a) for a in arrays]))
    order = np.argsort(keys, axis=0, kind="stable")
    return bits_of_keys(np.take_along_axis(keys, order, axis=0)), order


def some_ranks(k):
    return sorted({0, k - 1, k // 2, (k - 1) // 3}) + [k - 1]          # with a duplicate


@pytest.mark.parametrize("k", KS)
def test_the_definition_equals_numpys_stable_argsort(fm, k):
    rng = np.random.default_rng(100 + k)
    for n in NS:
        arrays = cross_data(k, n, rng)
        want_values, want_slots = restated(arrays)
        got = fm.cross_order_statistics_host(arrays, range(k), values=True, indices=True)
        assert len(got) == 2 * k
        values, slots = np.stack([bits(g) for g in got[:k]]), np.stack(got[k:])
        assert (values == want_values).all(), (k, n)
        assert (slots == want_slots.astype(np.float32)).all(), (k, n)
        # the multiset of a path's outputs is the multiset of its inputs, NaNs canonicalised
        canonical = bits_of_keys(keys_of(np.stack([bits(a) for a in arrays])))
        assert (np.sort(values, axis=0) == np.sort(canonical, axis=0)).all()
        # the indices are a permutation of 0 … k − 1
        assert (np.sort(slots, axis=0) == np.arange(k, dtype=np.float32)[:, None]).all()
        # select_across(index_r, vs) is value r wherever that value is no NaN
        for r in sorted({0, k // 2, k - 1}):
            picked = bits(fm.cross_select_host(slots[r], arrays))
            not_nan = values[r] != QUIET_NAN
            assert (picked[not_nan] == values[r][not_nan]).all(), (k, n, r)
            assert (np.isnan(picked.view(np.float32)) == ~not_nan).all()


def test_selectors_and_the_mask_do_not_change_an_outputs_bits(fm):
    rng = np.random.default_rng(7)
    for k, n in ((3, 65), (9, 64), (32, 63)):
        arrays = cross_data(k, n, rng)
        all_values, all_slots = restated(arrays)
        ranks = some_ranks(k)
        for chosen in (ranks, ranks[::-1], [ranks[1]] * 32, [ranks[-1]]):
            both = fm.cross_order_statistics_host(arrays, chosen, True, True)
            only_values = fm.cross_order_statistics_host(arrays, chosen, True, False)
            only_slots = fm.cross_order_statistics_host(arrays, chosen, False, True)
            assert len(both) == 2 * len(chosen) and len(only_values) == len(only_slots) == len(chosen)
            for j, r in enumerate(chosen):
                assert (bits(both[j]) == all_values[r]).all() and (bits(only_values[j]) == all_values[r]).all()
                assert (both[len(chosen) + j] == all_slots[r]).all() and (only_slots[j] == all_slots[r]).all()
        # more selectors than a call takes are taken in groups
        many = [r % k for r in range(70)]
        got = fm.cross_order_statistics_host(arrays, many, True, True)
        for j, r in enumerate(many): assert (bits(got[j]) == all_values[r]).all() and (got[70 + j] == all_slots[r]).all()


def test_an_output_is_a_function_of_the_paths_values_alone(fm):
    rng = np.random.default_rng(8)
    arrays = cross_data(5, 300, rng)
    whole = fm.cross_order_statistics_host(arrays, range(5), True, True)
    perm = rng.permutation(300)
    moved = fm.cross_order_statistics_host([a[perm] for a in arrays], range(5), True, True)
    part = fm.cross_order_statistics_host([a[17:18] for a in arrays], range(5), True, True)
    for w, m, p in zip(whole, moved, part):
        assert (bits(w)[perm] == bits(m)).all() and bits(w)[17] == bits(p)[0]


def test_cross_select_picks_bit_for_bit_and_refuses_every_other_index(fm):
    k, n = 5, 64
    arrays = cross_data(k, n, np.random.default_rng(9))
    for j in range(k):
        assert (bits(fm.cross_select_host(np.full(n, j, dtype=np.float32), arrays)) == bits(arrays[j])).all()      # NaN payloads kept
    assert (bits(fm.cross_select_host(np.full(n, -0.0, dtype=np.float32), arrays)) == bits(arrays[0])).all()
    for bad in (-1.0, float(k), 0.5, np.nan, np.inf, -np.inf, 4.0000005, 1e30, -1e-30):
        assert (bits(fm.cross_select_host(np.full(n, bad, dtype=np.float32), arrays)) == QUIET_NAN).all(), bad
    one = [arrays[0]]
    assert (bits(fm.cross_select_host(np.float32([0, 1, -1, 0.5, np.nan]), [a[:5] for a in one])) == np.array([bits(arrays[0])[0]] + [QUIET_NAN] * 4, dtype=np.uint32)).all()


def test_refusals(fm):
    N, lib = fm._native, fm.lib()
    n = 10
    a = np.arange(n, dtype=np.float32)
    out = [np.full(n, -7.0, dtype=np.float32) for _ in range(64)]
    ptrs = lambda arrays: (C.c_void_p * len(arrays))(*[x.ctypes.data for x in arrays])
    ints = lambda *xs: (C.c_int32 * max(len(xs), 1))(*xs)
    bad, f = N.ERR_INVALID_ARGUMENT, lib.fmhip_cross_order_statistics_host
    vs2, vs33 = ptrs([a, a]), ptrs([a] * 33)
    assert f(vs2, 0, n, ints(0), 1, 1, ptrs(out)) == bad
    assert f(vs33, 33, n, ints(0), 1, 1, ptrs(out)) == bad
    assert f(vs2, 2, n, ints(0), 0, 1, ptrs(out)) == bad
    assert f(vs2, 2, n, ints(*[0] * 33), 33, 1, ptrs(out)) == bad
    assert f(vs2, 2, n, ints(2), 1, 1, ptrs(out)) == bad                                   # rank K
    assert f(vs2, 2, n, ints(-1), 1, 1, ptrs(out)) == bad
    assert f(vs2, 2, n, ints(0), 1, 0, ptrs(out)) == bad                                   # no output
    assert f(vs2, 2, n, ints(0), 1, 4, ptrs(out)) == bad
    assert f(vs2, 2, 0, ints(0), 1, 1, ptrs(out)) == bad
    assert f(vs2, 2, -3, ints(0), 1, 1, ptrs(out)) == bad
    assert f(vs2, 2, 1 << 31, ints(0), 1, 1, ptrs(out)) == bad
    assert f(None, 2, n, ints(0), 1, 1, ptrs(out)) == bad
    assert f(vs2, 2, n, None, 1, 1, ptrs(out)) == bad
    assert f(vs2, 2, n, ints(0), 1, 1, None) == bad
    assert f((C.c_void_p * 2)(a.ctypes.data, None), 2, n, ints(0), 1, 1, ptrs(out)) == bad
    assert f(vs2, 2, n, ints(0), 1, 3, (C.c_void_p * 2)(out[0].ctypes.data, None)) == bad
    g = lib.fmhip_cross_select_host
    assert g(a.ctypes.data_as(C.c_void_p), vs2, 0, n, out[0].ctypes.data_as(C.c_void_p)) == bad
    assert g(a.ctypes.data_as(C.c_void_p), vs33, 33, n, out[0].ctypes.data_as(C.c_void_p)) == bad
    assert g(None, vs2, 2, n, out[0].ctypes.data_as(C.c_void_p)) == bad
    assert g(a.ctypes.data_as(C.c_void_p), None, 2, n, out[0].ctypes.data_as(C.c_void_p)) == bad
    assert g(a.ctypes.data_as(C.c_void_p), vs2, 2, n, None) == bad
    assert g(a.ctypes.data_as(C.c_void_p), vs2, 2, 0, out[0].ctypes.data_as(C.c_void_p)) == bad
    assert all((o == -7.0).all() for o in out)                                             # a refusal writes nothing
    # the device calls without a device: an error, never a host result
    if not lib.fmhip_is_initialized():
        h = (C.c_int64 * 2)()
        assert lib.fmhip_cross_order_statistics((C.c_int64 * 1)(1), 1, ints(0), 1, 1, h) != 0 and h[0] == 0
        assert lib.fmhip_cross_select(1, (C.c_int64 * 1)(1), 1, h) != 0 and h[0] == 0


def test_the_mirror_on_deterministic_variables_and_its_checks(fm):
    rv = lambda x: fm.RandomVariableHip(2.0, x)
    got = fm.order_across([rv(3.0), rv(-1.0), rv(2.0)], [0, 2, 1], values=True, indices=True)
    assert [g.isDeterministic() for g in got] == [True] * 6 and [g.value for g in got] == [-1.0, 3.0, 2.0, 1.0, 0.0, 2.0]
    assert [g.value for g in fm.sort_across([rv(3.0), rv(-1.0), rv(2.0)], descending=True)] == [3.0, 2.0, -1.0]
    assert fm.max_across([rv(1.0), rv(5.0)]).value == 5.0 and fm.min_across([rv(1.0), rv(5.0)]).value == 1.0
    assert fm.median_across([rv(1.0), rv(5.0), rv(3.0), rv(4.0)]).value == 3.0
    assert fm.argmax_across([rv(1.0), rv(5.0), rv(5.0)]).value == 2.0 and fm.argmin_across([rv(1.0), rv(1.0), rv(5.0)]).value == 0.0
    assert fm.select_across(rv(1.0), [rv(7.0), rv(8.0)]).value == 8.0 and np.isnan(fm.select_across(rv(2.0), [rv(7.0), rv(8.0)]).value)
    assert got[0].getFiltrationTime() == 2.0
    with pytest.raises(ValueError): fm.order_across([], [0])
    with pytest.raises(ValueError): fm.order_across([rv(1.0)] * 33, [0])
    with pytest.raises(ValueError): fm.order_across([rv(1.0)], [1])
    with pytest.raises(ValueError): fm.order_across([rv(1.0)], [])
    with pytest.raises(ValueError): fm.order_across([rv(1.0)], [0], values=False, indices=False)
    with pytest.raises(ValueError): fm.select_across(rv(0.0), [])
    with pytest.raises(TypeError): fm.order_across([1.0], [0])


def test_the_constants_are_the_headers(fm):
    header = open(os.path.join(ROOT, "finmath-lib-cuda-extensions_amd", "host", "cross_order.hpp")).read()
    cs = import_cross_section(fm)
    assert int(re.search(r"FM_CROSS_MAX_VECTORS = (\d+)", header).group(1)) == cs.MAX_VECTORS == max(KS)
    assert int(re.search(r"FM_CROSS_MAX_RANKS = (\d+)", header).group(1)) == cs.MAX_RANKS
    public = open(os.path.join(ROOT, "include", "fmhip.h")).read()
    assert int(re.search(r"#define FMHIP_CROSS_VALUES (\d+)", public).group(1)) == cs.VALUES and int(re.search(r"#define FMHIP_CROSS_INDICES (\d+)", public).group(1)) == cs.INDICES


def import_cross_section(fm):
    from importlib import import_module
    return import_module(fm.__name__ + ".cross_section")


def test_host_half_under_the_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("needs g++")
    exe = tmp_path / "cross_order_host"
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-ffp-contract=off",
                        os.path.join(ROOT, "tests", "cpp", "test_cross_order_host.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "cross order host ok" in r.stdout and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stdout[-1500:] + r.stderr[-3000:]


def test_the_kernels_are_in_the_library(fm):
    """A missing kernel is an error, never a fallback: the launchers are weak references, so the library must be shown to hold them."""
    out = subprocess.check_output(["nm", "-D", "--defined-only", fm._native.LIB_PATH], text=True) + subprocess.check_output(["nm", "--defined-only", fm._native.LIB_PATH], text=True, stderr=subprocess.DEVNULL)
    for name in ("launch_cross_order", "launch_cross_select"):
        assert name in out, name
    blob = open(fm._native.LIB_PATH, "rb").read()
    for kernel in (b"fm_cross_order_kernel", b"fm_cross_select_kernel"):
        assert kernel in blob, kernel


# ---------------------------------------------------------------- the engine's side on the null device
@pytest.fixture(scope="module")
def built():
    if not shutil.which("g++") or not os.path.exists("/opt/rocm/include/hip/hip_runtime_api.h"):
        pytest.skip("needs g++ and the HIP headers")
    r = subprocess.run(["make", "-C", NULLDEV, "-f", "cross_order.mk", "-j8", "cross_order_asan", "cross_order_tsan", "cross_order_absent_asan"], capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return os.path.join(NULLDEV, "build")


def _env(tmp_path, env):
    return dict(os.environ, FMHIP_JIT_CACHE_DIR=str(tmp_path / "code_objects"), FMHIP_JIT_PACK_DIR="off", FMHIP_RING_BYTES="16384", FMHIP_ARENA_BYTES="4096",
                ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1", TSAN_OPTIONS="halt_on_error=1", **env)


@pytest.mark.parametrize("env", [{}, {"FMNULL_DEVICES": "2"}, {"FMNULL_THREAD_ENGINES": "1"}])
def test_engine_pass_is_clean_under_the_sanitizers(built, tmp_path, env):
    """drive_cross_order: both calls on vectors of real data with NaNs, infinities, signed zeros and ties, every padded network size and its
    neighbours, checked against the definition (the stand-in sorts with the kernels' network); pending operands, a second thread releasing
    the inputs of pending operands during the call, every argument error — on one engine and behind a device list of one shard, behind two
    shards (per shard), with thread engines (a caller that does not own the vectors)."""
    full = _env(tmp_path, env)
    a = subprocess.run([os.path.join(built, "drive_cross_order_asan")], capture_output=True, text=True, timeout=600, env=full)
    assert a.returncode == 0 and "Sanitizer" not in a.stderr and "runtime error" not in a.stderr, a.stdout[-500:] + a.stderr[-6000:]
    assert a.stdout.count("cross order done") == 2 and a.stderr == ""
    assert ("a device list of one shard: checked" in a.stdout) == (not env)
    t = subprocess.run([os.path.join(built, "drive_cross_order_tsan")], capture_output=True, text=True, timeout=600, env=full)
    assert t.returncode == 0 and "ThreadSanitizer" not in t.stderr, t.stdout[-500:] + t.stderr[-6000:]
    assert t.stdout.count("cross order done") == 2 and t.stderr == ""


def test_a_failing_allocation_inside_a_cross_order_pass_leaves_nothing_behind(built, tmp_path):
    """One fmhip_cross_order_statistics of three ranks with values and indices takes SIX buffers from the pool, its outputs.  The hook
    FMHIP_TEST_FAIL_ALLOC_AT is set on each of them (their positions from a counting run), and once where nothing reaches it: the call
    answers FMHIP_OK or FMHIP_ERR_OUT_OF_MEMORY, a result it gives is right, outputs of a failed call are not written, live vectors and bytes
    in use are what they were, the same call succeeds afterwards (the driver checks all of it), and the process ends without a leak."""
    exe = os.path.join(built, "drive_cross_order_asan")
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
    a = subprocess.run([os.path.join(built, "drive_cross_order_absent_asan")], capture_output=True, text=True, timeout=600, env=_env(tmp_path, env))
    assert a.returncode == 0 and "Sanitizer" not in a.stderr and "runtime error" not in a.stderr, a.stdout[-500:] + a.stderr[-6000:]
    assert a.stdout.count("cross order absent done") == 2
