"""The device resampling without a GPU (include/fmhip.h: fmhip_resample_host; csrc/resample_host.hpp): the DEFINITION
against an independent numpy restatement — P from fmhip_prefix_sums_host of the cleaned weights, the targets in numpy float64, the ancestors
by a plain linear scan — for EQUALITY of ancestors and gathered bits; every semantics line of the header as an equality; the systematic
offspring counts on dyadic weights; every refusal of the host twin; the definition in a stand-alone program under AddressSanitizer / UBSan
(tests/cpp/test_resample_host.cpp); the engine's side of fmhip_resample (csrc/resample_engine.hpp, the fronts of csrc/sharded.cpp and
csrc/abi.cpp) on the test-only null device under AddressSanitizer + UBSan and ThreadSanitizer (tests/nulldev/resample.mk: drive_resample.cpp
with the stand-in launcher of null_resample.cpp, drive_resample_absent.cpp without it); and the bootstrap particle filter on the host path
against the Kalman filter.  Stand-alone programs only: nothing sanitized is loaded into this process."""
import ctypes as C
import importlib
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NULLDEV = os.path.join(ROOT, "tests", "nulldev")
SYSTEMATIC, STRATIFIED, MULTINOMIAL = 0, 1, 2
QUIET_NAN = 0x7FC00000
TILE = 2048
CHUNK = 2 * TILE                    # prefix_chunk_elems(n) for every n here
TWO_CHUNKS, THREE_CHUNKS = CHUNK + 1, 2 * CHUNK + 1      # the smallest n with prefix_blocks(n) > 1, and with 3 chunks
SIZES = [1, 7, 8, 9, 511, 512, 513, 2047, 2048, 2049, 3 * 2048 + 5, TWO_CHUNKS, THREE_CHUNKS]
BELOW_ONE = np.nextafter(1.0, 0.0)


def outputs_for(n):
    return sorted({1, 63, 64, 65, n, 4 * n, max(1, n // 4)})


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def clean(w):
    w = np.asarray(w, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        return np.where(w > 0, w, np.float32(0.0)).astype(np.float32)


def uniform_in_force(u):
    """(U, dead) of the header, in numpy."""
    u = np.asarray(u, dtype=np.float32).astype(np.float64)
    dead = np.isnan(u)
    with np.errstate(invalid="ignore"):
        return np.where(u < 0, 0.0, np.where(u >= 1, BELOW_ONE, u)), dead


def restatement(fm, w, n, scheme, m, offset, u, values):
    """(outs, ancestors, total) by the text of the definition: every operation one rounded float64 operation of numpy, the ancestor by a
    linear scan of P (the targets taken in ascending order, so that ONE walk along P serves all of them)."""
    if w is None:
        P, total = np.arange(1, n + 1, dtype=np.float64), float(n)
    else:
        P = fm.prefix_sums_host(clean(w))
        total = float(P[-1])
    j = np.arange(m, dtype=np.float64)
    U, dead = (np.zeros(m), np.zeros(m, dtype=bool)) if scheme == SYSTEMATIC else uniform_in_force(u)
    f = U if scheme == MULTINOMIAL else (j + (offset if scheme == SYSTEMATIC else U)) / np.float64(m)
    t = f * np.float64(total)
    a = np.full(m, -1, dtype=np.int64)
    if total > 0 and total != math.inf:
        if w is None:
            a = np.minimum(t.astype(np.int64), n - 1)
        else:
            Pl = P.tolist()
            first_total = next(r for r in range(n) if Pl[r] == total)
            r = 0
            for k in np.argsort(t, kind="stable").tolist():
                tk = t[k]
                while r < n and not Pl[r] > tk: r += 1
                a[k] = r if r < n else first_total
        a[dead] = -1
    outs = []
    for v in values:
        o = np.full(m, QUIET_NAN, dtype=np.uint32)
        o[a >= 0] = bits(v)[a[a >= 0]]
        outs.append(o)
    return outs, a, total


def families(n, rng):
    yield "uniform", rng.random(n, dtype=np.float32)
    concentrated = rng.random(n, dtype=np.float32)
    heavy = rng.random(n) < 0.01
    if heavy.any() and not heavy.all():                       # 99 % of the mass on 1 % of the paths
        concentrated[heavy] *= np.float32(99.0 * concentrated[~heavy].sum() / max(concentrated[heavy].sum(), 1e-30))
    yield "concentrated", concentrated
    half = rng.random(n, dtype=np.float32); half[rng.random(n) < 0.5] = 0.0; half[rng.integers(n)] = 0.5
    yield "half zeros", half
    one = np.zeros(n, dtype=np.float32); one[rng.integers(n)] = 3.0
    yield "one positive", one
    dirty = rng.random(n, dtype=np.float32)
    kind = rng.integers(0, 8, n)
    dirty[kind == 0] = np.nan; dirty[kind == 1] *= -1; dirty[kind == 2] = -0.0; dirty[rng.integers(n)] = 0.25
    yield "NaN, negative, -0.0", dirty
    yield "wide range", (10.0 ** rng.uniform(-8.0, 8.0, n)).astype(np.float32)


def values_for(n, rng, count=2):
    vs = []
    for _ in range(count):
        v = rng.standard_normal(n).astype(np.float32)
        u = v.view(np.uint32)
        u[rng.random(n) < 0.1] = np.uint32(0x7FC01234)          # a NaN with a payload
        u[rng.random(n) < 0.1] = np.uint32(0x80000000)          # -0.0
        vs.append(v)
    return vs


def check(fm, w, n, scheme, m, offset, u, values, what):
    outs, a, total = fm.resample_host(w, values, m, scheme, offset, u) if (w is not None or values) else (None, None, None)
    want_outs, want_a, want_total = restatement(fm, w, n, scheme, m, offset, u, values)
    assert np.float64(total).view(np.uint64) == np.float64(want_total).view(np.uint64) or (math.isnan(total) and math.isnan(want_total)), what
    assert (a == want_a).all(), (what, np.flatnonzero(a != want_a)[:5])
    for o, wo in zip(outs, want_outs):
        assert (bits(o) == wo).all(), what
    if w is not None and (a >= 0).any():
        assert (clean(w)[a[a >= 0]] > 0).all(), what                                 # a path of zero weight is never an ancestor
    assert ((a >= -1) & (a <= n - 1)).all(), what
    return a


@pytest.mark.parametrize("n", SIZES)
def test_the_definition_equals_the_numpy_restatement(fm, n):
    rng = np.random.default_rng(n)
    fams = list(families(n, rng))
    values = values_for(n, rng)
    case = 0
    for m in outputs_for(n):
        u = rng.random(m, dtype=np.float32)
        if m > 4: u[[0, 1, 2, 3]] = [np.nan, -0.5, 1.0, np.nextafter(np.float32(1), np.float32(0))]
        for scheme in (SYSTEMATIC, STRATIFIED, MULTINOMIAL):
            name, w = fams[case % len(fams)]; case += 1
            offset = [0.0, 0.5, float(BELOW_ONE), float(rng.random())][case % 4]
            check(fm, w, n, scheme, m, offset, u, values, (name, n, m, scheme))
        check(fm, None, n, [SYSTEMATIC, STRATIFIED, MULTINOMIAL][case % 3], m, 0.25, u, values, ("equal weights", n, m))


def test_every_family_at_a_size_with_three_chunks(fm):
    n = THREE_CHUNKS + 77
    rng = np.random.default_rng(5)
    values = values_for(n, rng, 1)
    for name, w in families(n, rng):
        for scheme in (SYSTEMATIC, STRATIFIED, MULTINOMIAL):
            check(fm, w, n, scheme, n, 0.375, rng.random(n, dtype=np.float32), values, (name, scheme))


def test_targets_that_equal_a_prefix_pick_the_next_path(fm):
    """Equal dyadic weights with offset 0: every t_j equals a prefix exactly, so the strict > picks the next path — at every chunk boundary too."""
    for n in (8, 512, CHUNK, 4 * CHUNK):                    # powers of two: j/n is exact
        w = np.full(n, 0.25, dtype=np.float32)
        x = np.arange(n, dtype=np.float32)
        (out,), a, total = fm.resample_host(w, [x], n, SYSTEMATIC, 0.0)
        assert total == 0.25 * n and (a == np.arange(n)).all() and (out == x).all()      # t_j = j/4 = P[j-1]: path j, not j - 1
        a = check(fm, w, n, SYSTEMATIC, n, 0.0, None, [x], n)
        assert (a == np.arange(n)).all()
        (out,), a, _ = fm.resample_host(w, [x], 2 * n, SYSTEMATIC, 0.0)                # t_j = j/8: P[j//2 - 1] for even j
        assert (a == np.arange(2 * n) // 2).all()


def test_one_dominant_weight_and_single_positive_weights(fm):
    n, m = THREE_CHUNKS, 1000
    x = np.arange(n, dtype=np.float32)
    w = np.full(n, 1e-30, dtype=np.float32); w[5000] = 1.0                              # fl(sum) carries the small ones; all targets but the edges land on 5000
    u = np.linspace(0.001, 0.999, m).astype(np.float32)
    for scheme in (SYSTEMATIC, STRATIFIED, MULTINOMIAL):
        _, a, _ = fm.resample_host(w, [x], m, scheme, 0.5, u)
        assert (a == 5000).all()
    for at in (0, n - 1, CHUNK - 1, CHUNK):
        w = np.zeros(n, dtype=np.float32); w[at] = 2.0
        for scheme in (SYSTEMATIC, STRATIFIED, MULTINOMIAL):
            for offset in (0.0, float(BELOW_ONE)):
                (out,), a, total = fm.resample_host(w, [x], m, scheme, offset, np.r_[np.float32(0), u[1:-1], np.float32(1)].astype(np.float32))
                assert total == 2.0 and (a == at).all() and (out == at).all(), (at, scheme)


def test_zero_weights_at_the_ends_and_dirty_weights_are_never_ancestors(fm):
    n, m = TWO_CHUNKS + 5, 3000
    rng = np.random.default_rng(3)
    w = rng.random(n, dtype=np.float32)
    w[:700] = 0.0; w[-900:] = 0.0
    u = np.r_[np.float32(0), rng.random(m - 2, dtype=np.float32), np.float32(1)].astype(np.float32)
    for scheme in (SYSTEMATIC, STRATIFIED, MULTINOMIAL):
        _, a, _ = fm.resample_host(w, [], m, scheme, 0.0, u)
        assert a.min() == 700 and a.max() <= n - 901                                  # t = 0 picks the first POSITIVE weight
    base = rng.random(n, dtype=np.float32)
    dirty = base.copy(); zeroed = base.copy()
    for k, bad in enumerate((np.nan, -1.5, -0.0, -np.inf)):
        dirty[k::9] = bad; zeroed[k::9] = 0.0
    for scheme in (SYSTEMATIC, STRATIFIED, MULTINOMIAL):
        _, a1, t1 = fm.resample_host(dirty, [], m, scheme, 0.5, u)
        _, a2, t2 = fm.resample_host(zeroed, [], m, scheme, 0.5, u)
        assert t1 == t2 and (a1 == a2).all()                                          # negative, NaN and -0.0 behave as zero


def test_degenerate_totals_give_the_quiet_nan_and_status_ok(fm):
    n, m = 1000, 777
    x = np.arange(n, dtype=np.float32)
    u = np.random.default_rng(1).random(m, dtype=np.float32)
    inf = np.ones(n, dtype=np.float32); inf[500] = np.inf
    for w, is_total in ((np.zeros(n, dtype=np.float32), lambda t: t == 0.0), (np.full(n, -1.0, dtype=np.float32), lambda t: t == 0.0),
                        (np.full(n, np.nan, dtype=np.float32), lambda t: t == 0.0), (inf, lambda t: t == math.inf)):
        for scheme in (SYSTEMATIC, STRATIFIED, MULTINOMIAL):
            (out,), a, total = fm.resample_host(w, [x], m, scheme, 0.5, u)              # (N.check: the status is FMHIP_OK)
            assert is_total(total) and (a == -1).all() and (bits(out) == QUIET_NAN).all()


def test_uniforms_outside_the_unit_interval_and_nan(fm):
    n = 4097
    rng = np.random.default_rng(2)
    w = rng.random(n, dtype=np.float32)
    x = np.arange(n, dtype=np.float32)
    below = np.nextafter(np.float32(1), np.float32(0))
    u = np.array([np.nan, -0.5, 1.0, below, 0.0, 7.0, -np.inf, np.inf], dtype=np.float32)
    m = u.size
    P = fm.prefix_sums_host(w); total = P[-1]
    for scheme in (STRATIFIED, MULTINOMIAL):
        (out,), a, _ = fm.resample_host(w, [x], m, scheme, None, u)
        assert a[0] == -1 and bits(out)[0] == QUIET_NAN                               # a NaN: the element is dead
        U = np.array([0.0, 0.0, BELOW_ONE, float(below), 0.0, BELOW_ONE, 0.0, BELOW_ONE])
        for j in range(1, m):
            f = U[j] if scheme == MULTINOMIAL else (np.float64(j) + U[j]) / np.float64(m)
            t = f * total
            want = int(np.argmax(P > t)) if (P > t).any() else int(np.argmax(P == total))      # (7 + U rounds up to 8: t = total)
            assert a[j] == want, (scheme, j)
    (out,), a, _ = fm.resample_host(None, [x], m, MULTINOMIAL, None, u)
    assert a.tolist() == [-1, 0, n - 1, int(float(below) * n), 0, n - 1, 0, n - 1]


def test_companions_come_back_bit_for_bit(fm):
    n = 3000
    rng = np.random.default_rng(8)
    vs = values_for(n, rng, 8)
    w = rng.random(n, dtype=np.float32)
    outs, a, _ = fm.resample_host(w, vs, 5000, STRATIFIED, None, rng.random(5000, dtype=np.float32))
    assert len(outs) == 8
    seen = set()
    for v, o in zip(vs, outs):
        assert (bits(o) == bits(v)[a]).all()
        seen |= set(bits(o).tolist())
    assert 0x7FC01234 in seen and 0x80000000 in seen


def test_the_bootstrap(fm):
    for n in (1, 7, 4097, 100_003):
        rng = np.random.default_rng(n)
        x = rng.standard_normal(n).astype(np.float32)
        u = rng.random(2 * n + 3, dtype=np.float32)
        (out,), a, total = fm.resample_host(None, [x], None, MULTINOMIAL, None, u)
        want = np.minimum(np.floor(u.astype(np.float64) * n).astype(np.int64), n - 1)
        assert total == float(n) and (a == want).all() and (bits(out) == bits(x)[want]).all()


def test_systematic_offspring_counts_on_dyadic_weights(fm):
    """Every product is exact: each path's offspring count is floor or ceil of m·w_r/total, and the counts sum to m."""
    for n, m in ((64, 64), (1000, 4096), (TWO_CHUNKS + 7, 8192), (THREE_CHUNKS, 2048)):
        rng = np.random.default_rng(n + m)
        w = (rng.integers(0, 256, n).astype(np.float64) * 2.0 ** -10).astype(np.float32)     # total < 2^22 · 2^-10, m a power of two
        for offset in (0.0, 0.5, 0.8125):
            _, a, total = fm.resample_host(w, [], m, SYSTEMATIC, offset)
            counts = np.bincount(a, minlength=n)
            expected = m * w.astype(np.float64) / total
            assert counts.sum() == m
            assert ((counts == np.floor(expected)) | (counts == np.ceil(expected))).all(), (n, m, offset)


def test_the_host_twin_refuses(fm):
    lib = fm.lib()
    bad = fm._native.ERR_INVALID_ARGUMENT
    n = m = 4
    w = np.ones(n, dtype=np.float32); x = np.arange(n, dtype=np.float32); u = np.full(m, 0.5, dtype=np.float32)
    out = np.full(m, -7.0, dtype=np.float32); anc = np.full(m, -7, dtype=np.int64); total = C.c_double(-7.0)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    vin, vout = (C.c_void_p * 9)(*[x.ctypes.data] * 9), (C.c_void_p * 9)(*[out.ctypes.data] * 9)
    pa = anc.ctypes.data_as(C.POINTER(C.c_int64))
    call = lambda *a: lib.fmhip_resample_host(*a, C.byref(total))
    assert call(vp(w), n, 3, m, 0.5, vp(u), vin, 1, vout, pa) == bad                        # an unknown scheme
    assert call(vp(w), n, -1, m, 0.5, vp(u), vin, 1, vout, pa) == bad
    for size in (0, -1, 1 << 31):
        assert call(vp(w), n, 0, size, 0.5, vp(u), vin, 1, vout, pa) == bad                 # m outside 1 … 2^31 - 1
        assert call(vp(w), size, 0, m, 0.5, vp(u), vin, 1, vout, pa) == bad                 # n
    assert call(vp(w), n, 0, m, 0.5, vp(u), vin, 9, vout, pa) == bad                        # n_values outside 0 … 8
    assert call(vp(w), n, 0, m, 0.5, vp(u), vin, -1, vout, pa) == bad
    assert call(vp(w), n, 0, m, 0.5, vp(u), None, 0, None, None) == bad                     # nothing asked for
    assert call(None, n, 2, m, 0.0, vp(u), None, 0, None, pa) == bad                        # neither weights nor a value vector
    for offset in (1.0, -0.25, math.nan, math.inf, -math.inf):
        assert call(vp(w), n, 0, m, offset, vp(u), vin, 1, vout, pa) == bad                 # an offset outside [0, 1) or not finite
        assert call(vp(w), n, 2, m, offset, vp(u), vin, 1, vout, pa) == bad                 # (whatever the scheme)
    for scheme in (1, 2):
        assert call(vp(w), n, scheme, m, 0.0, None, vin, 1, vout, pa) == bad                # no uniforms with a scheme that needs them
    assert call(vp(w), (1 << 24) + 1, 0, m, 0.5, None, vin, 1, vout, pa) == bad             # ancestors beyond 2^24 (refused before anything is read)
    assert call(vp(w), n, 0, m, 0.5, None, None, 1, vout, pa) == bad                        # NULL pointers
    assert call(vp(w), n, 0, m, 0.5, None, vin, 1, None, pa) == bad
    vin[0] = None
    assert call(vp(w), n, 0, m, 0.5, None, vin, 1, vout, pa) == bad
    assert (out == -7.0).all() and (anc == -7).all() and total.value == -7.0                # a refusal leaves the outputs untouched
    vin[0] = x.ctypes.data
    assert call(vp(w), n, 0, m, 0.5, None, vin, 1, vout, pa) == 0 and total.value == 4.0 and anc.tolist() == [0, 1, 2, 3]
    # the device call needs an engine: without one it says so, it does not resample on the host
    if not lib.fmhip_is_initialized():
        h = C.c_int64(0)
        hv = (C.c_int64 * 1)(1)
        assert lib.fmhip_resample(1, 0, 4, 0.5, 0, hv, 1, C.byref(h), None, None) == fm._native.ERR_NOT_INITIALIZED and h.value == 0


def test_the_mirror_checks_its_arguments(fm):
    with pytest.raises(ValueError): fm.resample_host([1.0], [[1.0]], scheme="residual")
    with pytest.raises(ValueError): fm.resample_host([1.0, 2.0], [[1.0]])
    (out,), a, total = fm.resample_host([1.0, 3.0], [[10.0, 20.0]], 4, "systematic", 0.5)
    assert total == 4.0 and a.tolist() == [0, 1, 1, 1] and out.tolist() == [10.0, 20.0, 20.0, 20.0]
    assert os.environ.get("FMHIP_DEVICE_RESAMPLE", "1") == "0" or fm.device_resample()


def test_definition_under_the_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("needs g++")
    exe = tmp_path / "resample_host"
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-ffp-contract=off",
                        os.path.join(ROOT, "tests", "cpp", "test_resample_host.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "resample host ok" in r.stdout and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stdout[-1500:] + r.stderr[-3000:]


def test_the_kernels_are_in_the_library(fm):
    """A missing kernel is an error, never a fallback: the launcher is a weak reference, so the library must be shown to hold it."""
    out = subprocess.check_output(["nm", "-D", "--defined-only", fm._native.LIB_PATH], text=True) + subprocess.check_output(["nm", "--defined-only", fm._native.LIB_PATH], text=True, stderr=subprocess.DEVNULL)
    assert "launch_resample" in out
    blob = open(fm._native.LIB_PATH, "rb").read()
    for kernel in (b"fm_resample_totals_kernel", b"fm_resample_carry_kernel", b"fm_resample_prefix_kernel", b"fm_resample_gather_kernel"):
        assert kernel in blob, kernel


# ---------------------------------------------------------------- the engine's side on the null device
@pytest.fixture(scope="module")
def built():
    if not shutil.which("g++") or not os.path.exists("/opt/rocm/include/hip/hip_runtime_api.h"):
        pytest.skip("needs g++ and the HIP headers")
    r = subprocess.run(["make", "-C", NULLDEV, "-f", "resample.mk", "-j8", "resample_asan", "resample_tsan", "resample_absent_asan"], capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return os.path.join(NULLDEV, "build")


def _env(tmp_path, env):
    return dict(os.environ, FMHIP_JIT_CACHE_DIR=str(tmp_path / "code_objects"), FMHIP_JIT_PACK_DIR="off", FMHIP_RING_BYTES="16384", FMHIP_ARENA_BYTES="4096",
                ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1", TSAN_OPTIONS="halt_on_error=1", **env)


@pytest.mark.parametrize("env", [{}, {"FMNULL_DEVICES": "2"}, {"FMNULL_DEVICES": "3"}, {"FMNULL_THREAD_ENGINES": "1"}])
def test_engine_pass_is_clean_under_the_sanitizers(built, tmp_path, env):
    """drive_resample: the stand-in's outputs against the host twin's at n = 1 … 300 007 and small again — every scheme and equal weights,
    0, 1 and 8 companions, ancestors, totals, degenerate totals, hostile uniforms, pending operands, every argument error — on one engine and
    behind a device list of one shard, behind 2 and 3 shards (FMHIP_ERR_UNSUPPORTED, nothing left behind), with thread engines."""
    full = _env(tmp_path, env)
    a = subprocess.run([os.path.join(built, "drive_resample_asan")], capture_output=True, text=True, timeout=600, env=full)
    assert a.returncode == 0 and "Sanitizer" not in a.stderr and "runtime error" not in a.stderr, a.stdout[-500:] + a.stderr[-6000:]
    assert a.stdout.count("resample done") == 2 and a.stderr == ""
    assert ("a device list of one shard: checked" in a.stdout) == (not env)
    t = subprocess.run([os.path.join(built, "drive_resample_tsan")], capture_output=True, text=True, timeout=600, env=full)
    assert t.returncode == 0 and "ThreadSanitizer" not in t.stderr, t.stdout[-500:] + t.stderr[-6000:]
    assert t.stdout.count("resample done") == 2 and t.stderr == ""


def test_a_failing_allocation_inside_a_resample_leaves_nothing_behind(built, tmp_path):
    """A weighted fmhip_resample with one companion and the ancestors takes THREE buffers from the pool: two outputs and the temporary of
    P.  The hook FMHIP_TEST_FAIL_ALLOC_AT is set on each (its position from a counting run), and once where nothing reaches it: the call
    answers FMHIP_OK or FMHIP_ERR_OUT_OF_MEMORY, the outputs of a failed call are untouched, live vectors and bytes in use are what they
    were, the same call succeeds afterwards (the driver checks all of it), and the process ends without a leak."""
    exe = os.path.join(built, "drive_resample_asan")
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
def test_a_build_without_the_kernel_answers_unsupported(built, tmp_path, env):
    a = subprocess.run([os.path.join(built, "drive_resample_absent_asan")], capture_output=True, text=True, timeout=600, env=_env(tmp_path, env))
    assert a.returncode == 0 and "Sanitizer" not in a.stderr and "runtime error" not in a.stderr, a.stdout[-500:] + a.stderr[-6000:]
    assert a.stdout.count("resample absent done") == 2


# ---------------------------------------------------------------- the bootstrap filter on the host path against the Kalman filter
A, Q, R, P0, STEPS, PARTICLES, SEEDS = 0.9, 0.25, 0.25, 1.0, 50, 4096, 16


def kalman_observations():
    rng = np.random.default_rng(20261021)
    x = math.sqrt(P0) * rng.standard_normal()
    ys = []
    for _ in range(STEPS):
        x = A * x + math.sqrt(Q) * rng.standard_normal()
        ys.append(x + math.sqrt(R) * rng.standard_normal())
    return ys


def host_filter(fm, observations, seed):
    """particle_filter_log_likelihood with numpy's normals in the Brownian motion's place: float32 states, the weights' total and the
    resampled state from resample_host — what FMHIP_DEVICE_RESAMPLE=0 runs."""
    rng = np.random.default_rng(seed)
    offsets = np.random.Generator(np.random.PCG64(seed + 1000))
    f32 = np.float32
    x = (f32(math.sqrt(P0)) * rng.standard_normal(PARTICLES).astype(f32)).astype(f32)
    ll = 0.0
    for y in observations:
        x = (f32(A) * x + f32(math.sqrt(Q)) * rng.standard_normal(PARTICLES).astype(f32)).astype(f32)
        z = ((x - f32(y)) / f32(math.sqrt(R))).astype(np.float64)
        w = (np.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)).astype(f32)
        (x,), _, total = fm.resample_host(w, [x], PARTICLES, SYSTEMATIC, offsets.random())
        ll += math.log(total / PARTICLES) - 0.5 * math.log(R)
    return ll


def test_the_particle_filter_on_the_host_path_is_unbiased_against_the_kalman_filter(fm):
    """Over 16 seeds the mean of exp(loglik − kalman) lies within 4 of its own standard errors of 1: the likelihood estimate is unbiased,
    its logarithm is not, so the ratio is tested."""
    mc = importlib.import_module("finmath-lib-cuda-extensions_amd.montecarlo")
    ys = kalman_observations()
    exact = mc.kalman_log_likelihood(ys, A, Q, R, P0)
    ratios = np.array([math.exp(host_filter(fm, ys, seed) - exact) for seed in range(SEEDS)])
    mean, error = ratios.mean(), ratios.std(ddof=1) / math.sqrt(SEEDS)
    print(f"exp(loglik - kalman): {mean:.4f} +- {error:.4f}")
    assert abs(mean - 1.0) <= 4.0 * error, (mean, error)


def test_the_kalman_filter_at_one_observation():
    mc = importlib.import_module("finmath-lib-cuda-extensions_amd.montecarlo")
    s = A * A * P0 + Q + R
    assert mc.kalman_log_likelihood([0.7], A, Q, R, P0) == pytest.approx(-0.5 * (math.log(2 * math.pi * s) + 0.49 / s), rel=1e-15)
