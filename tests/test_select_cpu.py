"""The device selection without a GPU (include/fmhip.h: fmhip_compress_host, fmhip_expand_host, fmhip_gather_host; csrc/select_host.hpp;
DESIGN.md §4.27): the DEFINITIONS against an independent numpy restatement — np.flatnonzero(mask >= 0) in float32, fancy indexing and
np.where — for EQUALITY of uint32 views, over every mask family at sizes around every boundary of the chunk geometry; every semantics line
of the header as an equality; every refusal of the host twins; the definitions in a stand-alone program under AddressSanitizer / UBSan
(tests/cpp/test_select_host.cpp); the engine's side (csrc/select_engine.hpp, the fronts of csrc/sharded.cpp and csrc/abi.cpp) on the
test-only null device under AddressSanitizer + UBSan and ThreadSanitizer (tests/nulldev/select.mk: drive_select.cpp with the stand-in
launchers of null_select.cpp, drive_select_absent.cpp without them); and the Bermudan driver on the CPU twin, whose default path computes
what it computed before.  Stand-alone programs only: nothing sanitized is loaded into this process."""
import ctypes as C
import importlib
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NULLDEV = os.path.join(ROOT, "tests", "nulldev")
QUIET_NAN = 0x7FC00000
TILE = 2048
CHUNK = 2 * TILE                    # prefix_chunk_elems(n) for every n here
TWO_CHUNKS, THREE_CHUNKS = CHUNK + 1, 2 * CHUNK + 1      # 4097, 8193: the smallest n with two and with three chunks
SIZES = [1, 7, 8, 9, 63, 64, 65, 511, 512, 513, 2047, 2048, 2049, TWO_CHUNKS, THREE_CHUNKS, 3 * 2048 + 5]
FILLS = [0.0, -0.0, np.inf, np.nan]
ODD = np.array([np.nan, -0.0, 0.0, -1e-45, np.inf, -np.inf], dtype=np.float32)
ODD_SELECTED = np.array([False, True, True, False, True, False])         # the semantics line of the header, element by element


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def families(n, rng):
    """(name, mask) for every family of the issue."""
    f32 = np.float32
    idx = np.arange(n)
    yield "all", np.ones(n, dtype=f32)
    yield "none", -np.ones(n, dtype=f32)
    yield "first", np.where(idx == 0, 0.0, -1.0).astype(f32)
    yield "last", np.where(idx == n - 1, 2.0, -2.0).astype(f32)
    yield "alternating", np.where(idx % 2 == 1, 1.0, -1.0).astype(f32)
    yield "one per 64", np.where(idx % 64 == 17 % min(n, 64), 1.0, -1.0).astype(f32)
    yield "half", (rng.random(n) - 0.5).astype(f32)
    yield "one in a hundred", (rng.random(n) - 0.99).astype(f32)
    yield "odd values", ODD[rng.integers(0, ODD.size, n)]


def values_for(n, rng, count=2):
    """Value vectors with NaNs that carry payloads, -0.0 and denormals among them."""
    out = []
    for _ in range(count):
        v = rng.standard_normal(n).astype(np.float32)
        b = v.view(np.uint32)
        k = np.arange(n)
        b[k % 7 == 1] = (0x7FC01234 + (k[k % 7 == 1] & 0xFF)).astype(np.uint32)
        b[k % 7 == 3] = 0x80000000
        b[k % 11 == 5] = 0x00000001
        out.append(v)
    return out


def selected(mask):
    """The restatement of `selected`: >= 0 in float32."""
    return np.asarray(mask, dtype=np.float32) >= np.float32(0.0)


def check_compress(fm, mask, values, what):
    sel = np.flatnonzero(selected(mask))
    outs, pos, count = fm.compress_host(mask, values, positions=True)
    assert count == sel.size, what
    assert pos.dtype == np.int64 and (pos == sel).all(), what
    for o, v in zip(outs, values):
        assert o.size == sel.size and (bits(o) == bits(v)[sel]).all(), what
    outs_only, count_only = fm.compress_host(mask, values)
    assert count_only == count and all((bits(a) == bits(b)).all() for a, b in zip(outs_only, outs)), what
    assert fm.compress_host(mask, [])[1] == count, what
    return outs, pos, count


@pytest.mark.parametrize("n", SIZES)
def test_the_definitions_equal_the_numpy_restatement(fm, n):
    rng = np.random.default_rng(100 + n)
    values = values_for(n, rng, 2)
    for name, mask in families(n, rng):
        outs, pos, count = check_compress(fm, mask, values, (n, name))
        sel = selected(mask)
        # expand(mask, compress(mask, v), fill) == where(selected, v, fill)
        for fill in FILLS:
            back = fm.expand_host(mask, outs, fill)
            for b, v in zip(back, values):
                want = np.where(sel, bits(v), bits(np.float32(fill))).astype(np.uint32)
                assert (bits(b) == want).all(), (n, name, fill)
        # gather(positions_of(mask), v) == compress(mask, v)
        if count:
            for g, o in zip(fm.gather_host(pos.astype(np.float32), values), outs):
                assert (bits(g) == bits(o)).all(), (n, name)


def test_what_is_selected(fm):
    """selected(x) is x >= 0.0f, the trigger of FMHIP_OP_CHOOSE: NaN no, -0.0 yes, +0.0 yes, -1e-45 no, +inf yes, -inf no."""
    v = np.arange(ODD.size, dtype=np.float32)
    (out,), pos, count = fm.compress_host(ODD, [v], positions=True)
    assert pos.tolist() == np.flatnonzero(ODD_SELECTED).tolist() == [1, 2, 4] and count == 3 and out.tolist() == [1.0, 2.0, 4.0]
    (back,) = fm.expand_host(ODD, [out], -9.0)
    assert back.tolist() == [-9.0, 1.0, 2.0, -9.0, 4.0, -9.0]


def test_nan_payloads_survive_bit_for_bit(fm):
    v = np.array([0x7FC01234, 0xFFC00001, 0x7F800001, 0x80000000, 0x00000001, 0x7FFFFFFF], dtype=np.uint32).view(np.float32)
    mask = np.array([1, -1, 1, 1, -1, 1], dtype=np.float32)
    (out,), count = fm.compress_host(mask, [v])
    assert bits(out).tolist() == [0x7FC01234, 0x7F800001, 0x80000000, 0x7FFFFFFF] and count == 4
    (back,) = fm.expand_host(mask, [out], np.nan)
    assert bits(back).tolist() == [0x7FC01234, QUIET_NAN, 0x7F800001, 0x80000000, QUIET_NAN, 0x7FFFFFFF]
    (g,) = fm.gather_host([5, 0, 0, 1, 4], [v])
    assert bits(g).tolist() == [0x7FFFFFFF, 0x7FC01234, 0x7FC01234, 0xFFC00001, 0x00000001]


def test_an_empty_selection_and_a_full_one(fm):
    v = np.arange(5, dtype=np.float32)
    (out,), pos, count = fm.compress_host(-np.ones(5), [v], positions=True)
    assert count == 0 and out.size == 0 and pos.size == 0
    (back,) = fm.expand_host(-np.ones(5), [np.zeros(0, dtype=np.float32)], 7.0)        # nothing selected: the fill everywhere
    assert back.tolist() == [7.0] * 5
    (out,), count = fm.compress_host(np.zeros(5), [v])
    assert count == 5 and out.tolist() == v.tolist()


def test_gather_by_hostile_indices(fm):
    n = 10
    v = np.arange(100, 100 + n, dtype=np.float32)
    index = np.array([-1, -0.0, n - 1, n, 0.5, np.nan, np.inf, -np.inf, 0, 3e38, -1e-45, 4.0000005], dtype=np.float32)
    (g,) = fm.gather_host(index, [v])
    want = np.full(index.size, QUIET_NAN, dtype=np.uint32)
    want[[1, 2, 8]] = bits(v)[[0, n - 1, 0]]
    want[11] = bits(v)[4] if np.float32(4.0000005) == 4 else QUIET_NAN
    assert (bits(g) == want).all(), bits(g)
    # n - 1 = 2^24 + 1 is no float: an index of 2^24 + 2 = n is out of range only because the comparison is made in double.  Two values,
    # no big arrays: the definition reads values[k] for a valid k alone.
    big = (1 << 24) + 2
    (g,) = fm.gather_host(np.array([big, 1.0], dtype=np.float32), [v], n=big)
    assert bits(g).tolist() == [QUIET_NAN, int(bits(v)[1])]


def test_the_host_twins_refuse(fm):
    lib = fm.lib()
    bad, mismatch = fm._native.ERR_INVALID_ARGUMENT, fm._native.ERR_SIZE_MISMATCH
    n = 4
    m = np.array([1, -1, 1, 1], dtype=np.float32); x = np.arange(n, dtype=np.float32)
    out = np.full(n, -7.0, dtype=np.float32); pos = np.full(n, -7, dtype=np.int64); count = C.c_int64(-7)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    vin, vout = (C.c_void_p * 9)(*[x.ctypes.data] * 9), (C.c_void_p * 9)(*[out.ctypes.data] * 9)
    holed = (C.c_void_p * 1)(None)
    pp = pos.ctypes.data_as(C.POINTER(C.c_int64))
    compress = lambda *a: lib.fmhip_compress_host(*a, C.byref(count))
    assert compress(vp(m), n, vin, 9, vout, pp) == bad                                  # n_values outside 0 … 8
    assert compress(vp(m), n, vin, -1, vout, pp) == bad
    for size in (0, -1, 1 << 31):
        assert compress(vp(m), size, vin, 1, vout, pp) == bad                           # n outside 1 … 2^31 - 1
    assert compress(vp(m), (1 << 24) + 1, vin, 1, vout, pp) == bad                      # positions beyond 2^24 (refused before anything is read)
    assert compress(None, n, vin, 1, vout, pp) == bad                                   # NULL pointers
    assert compress(vp(m), n, None, 1, vout, pp) == bad
    assert compress(vp(m), n, vin, 1, None, pp) == bad
    assert compress(vp(m), n, holed, 1, vout, pp) == bad
    assert compress(vp(m), n, vin, 1, holed, pp) == bad
    expand = lib.fmhip_expand_host
    assert expand(vp(m), n, vin, 0, 3, 0.0, vout) == bad                                # n_values outside 1 … 8
    assert expand(vp(m), n, vin, 9, 3, 0.0, vout) == bad
    for size in (0, -1, 1 << 31):
        assert expand(vp(m), size, vin, 1, 3, 0.0, vout) == bad
    assert expand(None, n, vin, 1, 3, 0.0, vout) == bad
    assert expand(vp(m), n, None, 1, 3, 0.0, vout) == bad
    assert expand(vp(m), n, vin, 1, 3, 0.0, None) == bad
    assert expand(vp(m), n, holed, 1, 3, 0.0, vout) == bad
    for wrong in (2, 4, 0, -1):
        assert expand(vp(m), n, vin, 1, wrong, 0.0, vout) == mismatch                   # values that are not `count` long
    gather = lib.fmhip_gather_host
    assert gather(vp(x), n, vin, 0, n, vout) == bad
    assert gather(vp(x), n, vin, 9, n, vout) == bad
    for size in (0, -1, 1 << 31):
        assert gather(vp(x), size, vin, 1, n, vout) == bad
        assert gather(vp(x), n, vin, 1, size, vout) == bad
    assert gather(None, n, vin, 1, n, vout) == bad
    assert gather(vp(x), n, None, 1, n, vout) == bad
    assert gather(vp(x), n, vin, 1, n, None) == bad
    assert gather(vp(x), n, holed, 1, n, vout) == bad
    assert (out == -7.0).all() and (pos == -7).all() and count.value == -7              # a refusal leaves the outputs untouched
    assert compress(vp(m), n, vin, 1, vout, pp) == 0 and count.value == 3 and pos.tolist() == [0, 2, 3, -7] and out.tolist() == [0.0, 2.0, 3.0, -7.0]
    assert compress(vp(m), n, None, 0, None, None) == 0 and count.value == 3            # a call that only wants the count is valid
    # the device calls need an engine: without one they say so, they do not run on the host
    if not lib.fmhip_is_initialized():
        h = C.c_int64(0); hv = (C.c_int64 * 1)(1)
        not_initialized = fm._native.ERR_NOT_INITIALIZED
        assert lib.fmhip_compress(1, hv, 1, C.byref(h), None, None) == not_initialized and h.value == 0
        assert lib.fmhip_expand(1, hv, 1, 0.0, C.byref(h)) == not_initialized and h.value == 0
        assert lib.fmhip_gather(1, hv, 1, C.byref(h)) == not_initialized and h.value == 0


def test_the_mirror_checks_its_arguments(fm):
    with pytest.raises(ValueError): fm.compress_host([1.0, 2.0], [[1.0]])
    with pytest.raises(ValueError): fm.expand_host([1.0, 2.0], [[1.0, 2.0], [1.0]])
    with pytest.raises(ValueError): fm.gather_host([0.0], [[1.0, 2.0], [1.0]])
    with pytest.raises(fm._native.FmhipError) as e: fm.expand_host([1.0, -1.0], [[1.0, 2.0]])
    assert e.value.code == fm._native.ERR_SIZE_MISMATCH
    with pytest.raises(TypeError): fm.compress(np.ones(3), [])
    assert os.environ.get("FMHIP_DEVICE_SELECT", "1") == "0" or fm.device_select()


def test_definition_under_the_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("needs g++")
    exe = tmp_path / "select_host"
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-ffp-contract=off",
                        os.path.join(ROOT, "tests", "cpp", "test_select_host.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "select host ok" in r.stdout and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stdout[-1500:] + r.stderr[-3000:]


def test_the_kernels_are_in_the_library(fm):
    """A missing kernel is an error, never a fallback: the launchers are weak references, so the library must be shown to hold them."""
    out = subprocess.check_output(["nm", "-D", "--defined-only", fm._native.LIB_PATH], text=True) + subprocess.check_output(["nm", "--defined-only", fm._native.LIB_PATH], text=True, stderr=subprocess.DEVNULL)
    for launcher in ("launch_select_count", "launch_select_compress", "launch_select_expand", "launch_select_gather"):
        assert launcher in out, launcher
    blob = open(fm._native.LIB_PATH, "rb").read()
    for kernel in (b"fm_select_count_kernel", b"fm_select_carry_kernel", b"fm_select_compress_kernel", b"fm_select_expand_kernel", b"fm_select_gather_kernel"):
        assert kernel in blob, kernel


# ---------------------------------------------------------------- the engine's side on the null device
@pytest.fixture(scope="module")
def built():
    if not shutil.which("g++") or not os.path.exists("/opt/rocm/include/hip/hip_runtime_api.h"):
        pytest.skip("needs g++ and the HIP headers")
    r = subprocess.run(["make", "-C", NULLDEV, "-f", "select.mk", "-j8", "select_asan", "select_tsan", "select_absent_asan"], capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return os.path.join(NULLDEV, "build")


def _env(tmp_path, env):
    return dict(os.environ, FMHIP_JIT_CACHE_DIR=str(tmp_path / "code_objects"), FMHIP_JIT_PACK_DIR="off", FMHIP_RING_BYTES="16384", FMHIP_ARENA_BYTES="4096",
                ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1", TSAN_OPTIONS="halt_on_error=1", **env)


@pytest.mark.parametrize("env", [{}, {"FMNULL_DEVICES": "2"}, {"FMNULL_DEVICES": "3"}, {"FMNULL_THREAD_ENGINES": "1"}])
def test_engine_passes_are_clean_under_the_sanitizers(built, tmp_path, env):
    """drive_select: the stand-ins' outputs against the host twins' at n = 1 … 300 007 and small again — every mask family, 0, 1 and 8 value
    vectors, positions, the count alone, count == 0 (handles of 0, the pool unchanged), the expand's size mismatch behind the count, hostile
    indices, pending operands, every argument error — on one engine and behind a device list of one shard, behind 2 and 3 shards
    (FMHIP_ERR_UNSUPPORTED, nothing left behind), with thread engines."""
    full = _env(tmp_path, env)
    a = subprocess.run([os.path.join(built, "drive_select_asan")], capture_output=True, text=True, timeout=600, env=full)
    assert a.returncode == 0 and "Sanitizer" not in a.stderr and "runtime error" not in a.stderr, a.stdout[-500:] + a.stderr[-6000:]
    assert a.stdout.count("select done") == 2 and a.stderr == ""
    assert ("a device list of one shard: checked" in a.stdout) == (not env)
    t = subprocess.run([os.path.join(built, "drive_select_tsan")], capture_output=True, text=True, timeout=600, env=full)
    assert t.returncode == 0 and "ThreadSanitizer" not in t.stderr, t.stdout[-500:] + t.stderr[-6000:]
    assert t.stdout.count("select done") == 2 and t.stderr == ""


def test_a_failing_allocation_between_the_phases_leaves_nothing_behind(built, tmp_path):
    """A compress with one value vector and the positions takes TWO buffers from the pool, an expand of one vector ONE — all three BETWEEN
    the phases, behind the count.  The hook FMHIP_TEST_FAIL_ALLOC_AT is set on each (its position from a counting run), and once where
    nothing reaches it: the call answers FMHIP_OK or FMHIP_ERR_OUT_OF_MEMORY, the output handles of a failed call are untouched, live vectors
    and bytes in use are what they were, the same calls succeed afterwards (the driver checks all of it), and the process ends without a
    leak."""
    exe = os.path.join(built, "drive_select_asan")
    counting = subprocess.run([exe, "failure"], capture_output=True, text=True, timeout=600, env=_env(tmp_path, {}))
    assert counting.returncode == 0 and "Sanitizer" not in counting.stderr, counting.stdout[-500:] + counting.stderr[-6000:]
    before, inside, status = map(int, re.search(r"failure: (\d+) allocations before the call, (\d+) in it, status (-?\d+)", counting.stdout).groups())
    assert inside == 3 and status == 0
    for at in list(range(before + 1, before + inside + 1)) + [10**9]:
        r = subprocess.run([exe, "failure"], capture_output=True, text=True, timeout=600, env=_env(tmp_path, {"FMHIP_TEST_FAIL_ALLOC_AT": str(at)}))
        assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr and r.stderr == "", (at, r.stdout[-500:] + r.stderr[-6000:])
        assert "failure done" in r.stdout
        failed = int(re.search(r"status (-?\d+)", r.stdout).group(1)) != 0
        assert failed == (at <= before + inside), (at, r.stdout)


@pytest.mark.parametrize("env", [{}, {"FMNULL_THREAD_ENGINES": "1"}])
def test_a_build_without_the_kernels_answers_unsupported(built, tmp_path, env):
    a = subprocess.run([os.path.join(built, "drive_select_absent_asan")], capture_output=True, text=True, timeout=600, env=_env(tmp_path, env))
    assert a.returncode == 0 and "Sanitizer" not in a.stderr and "runtime error" not in a.stderr, a.stdout[-500:] + a.stderr[-6000:]
    assert a.stdout.count("select absent done") == 2


# ---------------------------------------------------------------- the Bermudan driver on the CPU twin: the default path is what it was
BERMUDAN_BEFORE = 0.15167715261338052       # bermudan_option_mc on the CPU twin at 20 000 paths, seed 777, from the commit before the argument


def test_the_bermudan_driver_without_the_new_argument_computes_what_it_computed(fm, oracle, monkeypatch):
    """The CPU twin's factory runs the driver without a device (as tests/test_gpu_regression.py runs it): in_the_money_only=False is the
    call without the argument, to the last bit, whatever FMHIP_DEVICE_SELECT says — the default path reads neither — and it is the number
    the driver gave before the argument existed (recorded from that commit: same seed, same increments)."""
    from test_gpu_regression import K, R, S0, SIGMA, ArrayBrownianMotion
    mc = importlib.import_module("finmath-lib-cuda-extensions_amd.montecarlo")
    td = fm.TimeDiscretization(0.0, 10, 0.2)
    dates = [0.2 * k for k in range(1, 11)]
    n = 20_000
    inc = oracle.bm_generate(777, [td.getTimeStep(i) for i in range(10)], 1, n)
    bm = ArrayBrownianMotion(td, oracle.RandomVariableFloatFactory(), inc)
    plain, _ = mc.bermudan_option_mc(bm, S0, R, SIGMA, dates, K)
    monkeypatch.setenv("FMHIP_DEVICE_SELECT", "0")
    explicit, _ = mc.bermudan_option_mc(bm, S0, R, SIGMA, dates, K, in_the_money_only=False)
    assert explicit == plain
    assert plain == BERMUDAN_BEFORE, repr(plain)
