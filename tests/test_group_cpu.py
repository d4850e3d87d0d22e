"""The device reduce-by-key without a GPU (include/fmhip.h: fmhip_group_sums_host; csrc/group_host.hpp): the DEFINITION
through ctypes against an independent numpy restatement — np.bincount for the counts, math.fsum per group for the sums, within one fp32
rounding plus the definition's bound (prefix_chain(n) + 1)·2⁻⁵³·Σ|the group's own terms| — over every index family at sizes around every
boundary of the chunk geometry and every m around the one-, two- and three-pass thresholds; every consequence the header states as an
equality (one group is the prefix total, a permutation is the values, other groups' values leave a group's bits alone, slot, n_values and
mask change nothing); hostile indices; every refusal; the mirror's argument checks; the definition in a stand-alone program under
AddressSanitizer / UBSan (tests/cpp/test_group_host.cpp); the engine's side (csrc/group_engine.hpp, the fronts of csrc/sharded.cpp and
csrc/abi.cpp) on the test-only null device under AddressSanitizer + UBSan and ThreadSanitizer (tests/nulldev/group.mk: drive_group.cpp
with the stand-in launchers of null_group.cpp, drive_group_absent.cpp without them); and the Merton driver's comparison on host-drawn
increments and the definition alone, which is where its seed was fixed.  Stand-alone programs only: nothing sanitized is loaded into this
process.  The GPU test imports the helpers below."""
import ctypes as C
import math
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
SIZES = [1, 7, 64, 65, 2047, 2048, 2049, 4095, 4096, 4097, 12_289, 100_003]
SUM, MEAN, VARIANCE = 1, 2, 4
WHAT = {SUM: "sum", MEAN: "mean", VARIANCE: "variance"}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def prefix_chain(n):
    """prefix_chain(n) of csrc/prefix_host.hpp"""
    tiles = (n + TILE - 1) // TILE
    chunk_tiles = max((tiles + 1023) // 1024, 2)
    blocks = max((tiles + chunk_tiles - 1) // chunk_tiles, 1)
    return 7 + 7 + 7 + 3 + (chunk_tiles - 1) + (blocks - 1)


def group_counts_of(n):
    """The m of the issue: around one, two and three radix passes, and m = n."""
    return sorted({1, 2, 255, 256, 257, 65_535, 65_536, 65_537, n})


def families(n, m, rng):
    """(name, index) for every family of the issue."""
    f32 = np.float32
    r = np.arange(n)
    yield "one group", np.zeros(n, dtype=f32)
    yield "permutation", (rng.permutation(n) % m).astype(f32)                       # with m >= n: every group at most one member
    heads = sorted({0} | {b + d for b in (8, 64, 512, 2048, 4096, 8192, 12_288) for d in (-1, 0, 1) if 0 < b + d < n})
    yield "sorted runs", ((np.searchsorted(heads, r, side="right") - 1) % m).astype(f32)      # heads on and either side of lane, group, wave, tile and chunk
    yield "uniform", rng.integers(0, m, n).astype(f32)
    yield "one group holds 99 %", np.where(rng.random(n) < 0.99, m // 2, rng.integers(0, m, n)).astype(f32)
    yield "many empty groups", (rng.integers(0, 3, n) * (m // 3)).astype(f32)


HOSTILE = np.array([np.nan, np.inf, -np.inf, -1.0, 0.5, 2.0 ** 30, -0.0], dtype=np.float32)          # and m itself: added where m is known


def values_for(n, rng, count=1, odd=True):
    """Value vectors; with odd=True NaN, ±inf and -0.0 among them."""
    out = []
    for _ in range(count):
        v = (rng.standard_normal(n) * 100.0).astype(np.float32)
        if odd:
            k = np.arange(n)
            v[k % 1009 == 7] = np.nan
            v[k % 1013 == 9] = np.inf
            v[k % 1019 == 11] = -np.inf
            v[k % 7 == 3] = -0.0
        out.append(v)
    return out


def membership(index, m):
    """(key, grouped): the restatement of the rule in numpy — an integer in [0, m - 1], -0.0 counting as 0."""
    x = np.asarray(index, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        grouped = np.isfinite(x) & (x >= 0) & (x <= m - 1) & (x == np.floor(x))
    return np.where(grouped, x, 0).astype(np.int64), grouped


def check_against_numpy(fm, index, values, m, what):
    """group_sums_host against bincount and fsum; returns what the twin gave."""
    n = index.size
    outs, counts, ungrouped = fm.group_sums_host(index, values, m, what=("sum", "mean", "variance"))
    key, grouped = membership(index, m)
    want_counts = np.bincount(key[grouped], minlength=m)
    assert ungrouped == n - int(grouped.sum()), what
    assert (counts == want_counts.astype(np.float32)).all(), what
    order = np.flatnonzero(grouped)[np.argsort(key[grouped], kind="stable")]
    starts = np.concatenate([[0], np.cumsum(want_counts)])
    eps = (prefix_chain(n) + 1) * 2.0 ** -53
    for v, (s, mean, var) in zip(values, outs):
        empty = want_counts == 0
        assert (bits(s)[empty] == 0).all() and (bits(mean)[empty] == QUIET_NAN).all() and (bits(var)[empty] == QUIET_NAN).all(), what
        x = v.astype(np.float64)[order]
        for k in np.flatnonzero(~empty):
            terms = x[starts[k]:starts[k + 1]]
            c = float(want_counts[k])
            if not np.isfinite(terms).all():
                with np.errstate(invalid="ignore"): ref = terms.sum()
                assert (np.isnan(s[k]) and bits(s)[k] == QUIET_NAN) if np.isnan(ref) else s[k] == ref, (what, k)
                continue
            exact, total = math.fsum(terms), math.fsum(np.abs(terms))
            b1 = eps * total
            assert abs(float(s[k]) - exact) <= b1 + 2.0 ** -24 * (abs(exact) + b1) + 2.0 ** -149, (what, "sum", k, float(s[k]), exact)
            assert abs(float(mean[k]) - exact / c) <= b1 / c + (2.0 ** -24 + 2.0 ** -52) * (abs(exact) + b1) / c + 2.0 ** -149, (what, "mean", k)
            exact2 = math.fsum(terms * terms)
            b2 = eps * exact2
            ref = max(0.0, exact2 / c - (exact / c) ** 2)
            slack = (b2 + 2.0 * abs(exact / c) * b1) / c * 1.01 + 2.0 ** -50 * (exact2 / c + (exact / c) ** 2)
            assert abs(float(var[k]) - ref) <= slack + 2.0 ** -24 * (ref + slack) + 2.0 ** -149, (what, "variance", k, float(var[k]), ref)
    return outs, counts, ungrouped


def cases():
    """(n, m, family names) — every family where it is cheap; above that 'one group' and 'sorted runs' always, and two more per (n, m)
    in rotation."""
    out, turn = [], 0
    names = ["one group", "permutation", "sorted runs", "uniform", "one group holds 99 %", "many empty groups"]
    for n in SIZES:
        for m in group_counts_of(n):
            if n <= 4097 and (m <= 257 or m == n): out.append((n, m, names))
            else: out.append((n, m, [names[0], names[2], names[(1, 3, 4, 5)[turn % 4]], names[(1, 3, 4, 5)[(turn + 2) % 4]]])); turn += 1
    return out


@pytest.mark.parametrize("n,m,names", cases(), ids=lambda v: str(v) if isinstance(v, int) else "f")
def test_definition_against_numpy(fm, n, m, names):
    rng = np.random.default_rng(1000 + 31 * n + m)
    values = values_for(n, rng, 1, odd=(n % 2 == 1))
    for name, index in families(n, m, rng):
        if name not in names: continue
        outs, counts, ungrouped = check_against_numpy(fm, index, values, m, (n, m, name))
        if name == "one group" and np.isfinite(values[0]).all():
            prefix = fm.prefix_sums_host(values[0])
            assert bits(outs[0][0])[0] == bits(np.float32(prefix[-1]))[0] and counts[0] == np.float32(n)      # the prefix total, bit for bit
        if name == "permutation" and m >= n:
            key, _ = membership(index, m)
            assert (bits(outs[0][0])[key] == bits(values[0])).all()                    # the values, bit for bit (-0.0 and NaN payload aside: NaN is canonical)


def test_hostile_indices_belong_to_no_group(fm):
    rng = np.random.default_rng(5)
    for n, m in ((65, 7), (4097, 256), (12_289, 65_537)):
        bad = np.concatenate([HOSTILE[:-1], np.array([m, m + 1, -2 ** 31, 1e30, np.nextafter(np.float32(1), np.float32(2))], dtype=np.float32)])
        index = rng.integers(0, m, n).astype(np.float32)
        where = rng.random(n) < 0.3
        index[where] = bad[rng.integers(0, bad.size, int(where.sum()))]
        index[::11] = -0.0                                                            # -0.0 counts as 0
        values = values_for(n, rng, 1, odd=False)
        outs, counts, ungrouped = check_against_numpy(fm, index, values, m, ("hostile", n, m))
        assert ungrouped == int(where.sum() - (where[::11]).sum()) and counts[0] >= np.float32(len(index[::11]))
        # every element ungrouped: every group empty, and never an error
        outs, counts, ungrouped = fm.group_sums_host(np.full(n, np.nan, dtype=np.float32), values, m, what=("sum", "mean"))
        assert ungrouped == n and (counts == 0).all() and (bits(outs[0][0]) == 0).all() and (bits(outs[0][1]) == QUIET_NAN).all()


def test_other_groups_are_untouched_bit_for_bit(fm):
    """The values of one group change — to other numbers, to NaN, to ±inf — and every other group keeps its bits."""
    rng = np.random.default_rng(6)
    for n, m in ((2049, 5), (12_289, 300), (100_003, 17)):
        index = rng.integers(0, m, n).astype(np.float32)
        (v,) = values_for(n, rng, 1, odd=False)
        base, _, _ = fm.group_sums_host(index, [v], m, what=("sum", "mean", "variance"))
        victim = m // 2
        for poison in (np.nan, np.inf, -np.inf, 1e30, 0.0):
            w = v.copy(); w[index == victim] = poison
            got, _, _ = fm.group_sums_host(index, [w], m, what=("sum", "mean", "variance"))
            others = np.arange(m) != victim
            for a, b in zip(base[0], got[0]): assert (bits(a)[others] == bits(b)[others]).all(), (n, m, poison)
        w = v.copy(); w[np.flatnonzero(index == victim)[0]] = np.nan                   # one NaN: its own group only
        got, _, _ = fm.group_sums_host(index, [w], m, what=("sum",))
        assert np.isnan(got[0][0][victim]) and (bits(got[0][0])[others] == bits(base[0][0])[others]).all()


def test_slot_number_of_vectors_and_mask_change_nothing(fm):
    rng = np.random.default_rng(7)
    n, m = 12_289, 300
    index = rng.integers(0, m + 2, n).astype(np.float32)
    vs = values_for(n, rng, 4)
    alone = [fm.group_sums_host(index, [v], m, what=("sum", "mean", "variance"))[0][0] for v in vs]
    for what in (("sum",), ("mean",), ("variance",), ("sum", "variance"), ("variance", "mean"), ("mean", "sum", "variance")):
        for chosen in ([0, 1, 2, 3], [3, 0], [2], [1, 1, 1, 1]):
            outs, counts, ungrouped = fm.group_sums_host(index, [vs[i] for i in chosen], m, what=what)
            for i, row in zip(chosen, outs):
                for w, o in zip(what, row): assert (bits(o) == bits(alone[i][("sum", "mean", "variance").index(w)])).all(), (what, chosen)
    counts_only = fm.group_sums_host(index, [], m)
    assert counts_only[0] == [] and (counts_only[1] == counts).all() and counts_only[2] == ungrouped


def test_twin_refuses_bad_arguments(fm):
    lib = fm.lib()
    bad = fm._native.ERR_INVALID_ARGUMENT
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    n, m = 4, 3
    index, x = np.float32([0, 1, 2, 7]), np.float32([1, 2, 3, 4])
    out, counts = np.full(m, -7.0, dtype=np.float32), np.full(m, -7.0, dtype=np.float32)
    vin, vout, holed = (C.c_void_p * 5)(*[x.ctypes.data] * 5), (C.c_void_p * 1)(out.ctypes.data), (C.c_void_p * 1)(None)
    u = C.c_int64(-7)
    call = lib.fmhip_group_sums_host
    for groups in (0, -1, (1 << 24) + 1):
        assert call(vp(index), n, groups, vin, 1, SUM, vp(counts), vout, C.byref(u)) == bad      # m outside 1 … 2^24
    for k in (-1, 5):
        assert call(vp(index), n, m, vin, k, SUM, vp(counts), vout, C.byref(u)) == bad           # n_values outside 0 … 4
    assert call(vp(index), n, m, vin, 1, 0, vp(counts), vout, C.byref(u)) == bad                 # a mask of 0 with a value vector
    assert call(vp(index), n, m, vin, 1, 8, vp(counts), vout, C.byref(u)) == bad                 # unknown bits
    assert call(vp(index), n, m, None, 0, 0, None, None, None) == bad                            # nothing asked for
    for size in (0, -1, 1 << 31):
        assert call(vp(index), size, m, vin, 1, SUM, vp(counts), vout, C.byref(u)) == bad        # n outside 1 … 2^31 - 1
    assert call(None, n, m, vin, 1, SUM, vp(counts), vout, C.byref(u)) == bad                    # NULL pointers
    assert call(vp(index), n, m, None, 1, SUM, vp(counts), vout, C.byref(u)) == bad
    assert call(vp(index), n, m, holed, 1, SUM, vp(counts), vout, C.byref(u)) == bad
    assert call(vp(index), n, m, vin, 1, SUM, vp(counts), None, C.byref(u)) == bad
    assert call(vp(index), n, m, vin, 1, SUM, vp(counts), holed, C.byref(u)) == bad
    assert (out == -7.0).all() and (counts == -7.0).all() and u.value == -7                      # a refusal leaves the outputs untouched
    assert call(vp(index), n, m, vin, 1, SUM, vp(counts), vout, C.byref(u)) == 0 and out.tolist() == [1.0, 2.0, 3.0] and counts.tolist() == [1.0, 1.0, 1.0] and u.value == 1
    assert call(vp(index), n, m, None, 0, 0, None, None, C.byref(u)) == 0 and u.value == 1       # a call that only wants the ungrouped count is valid
    assert call(vp(index), n, m, None, 0, 0, vp(counts), None, None) == 0
    # the device call needs an engine: without one it says so, it does not run on the host
    if not lib.fmhip_is_initialized():
        h = C.c_int64(0); hv = (C.c_int64 * 1)(1)
        assert lib.fmhip_group_sums(1, m, hv, 1, SUM, None, C.byref(h), None) == fm._native.ERR_NOT_INITIALIZED and h.value == 0


def test_the_mirror_checks_its_arguments(fm):
    with pytest.raises(ValueError): fm.group_sums_host([0.0, 1.0], [[1.0]], 2)                   # sizes
    with pytest.raises(ValueError): fm.group_sums_host([0.0], [[1.0]], 0)                         # m
    with pytest.raises(ValueError): fm.group_sums_host([0.0], [[1.0]], (1 << 24) + 1)
    with pytest.raises(ValueError): fm.group_sums_host([0.0], [[1.0]], 2.5)
    with pytest.raises(ValueError): fm.group_sums_host([0.0], [[1.0]] * 5, 2)                     # five vectors
    with pytest.raises(ValueError): fm.group_sums_host([0.0], [[1.0]], 2, what=("median",))
    with pytest.raises(ValueError): fm.group_sums_host([0.0], [[1.0]], 2, what=("sum", "sum"))
    with pytest.raises(ValueError): fm.group_sums_host([0.0], [[1.0]], 2, what=())
    with pytest.raises(TypeError): fm.group_moments(np.zeros(3), [], 2, counts=True)              # the mirror takes device vectors
    with pytest.raises(TypeError): fm.group_counts(np.zeros(3), 2)
    assert os.environ.get("FMHIP_DEVICE_GROUP", "1") == "0" or fm.device_group()
    for name in ("fmhip_group_sums", "fmhip_group_sums_host"):
        assert name in fm._native.SYMBOLS and hasattr(fm.lib(), name)
    outs, counts, ungrouped = fm.group_sums_host([2, 0, 2, 5], [[1, 2, 3, 4]], 3, what="mean")   # a single name, plain lists
    assert outs[0][0][2] == 2.0 and outs[0][0][0] == 2.0 and np.isnan(outs[0][0][1]) and counts.tolist() == [1.0, 0.0, 2.0] and ungrouped == 1


def test_definition_under_the_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("needs g++")
    exe = tmp_path / "group_host"
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-ffp-contract=off",
                        os.path.join(ROOT, "tests", "cpp", "test_group_host.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "group host ok" in r.stdout and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stdout[-1500:] + r.stderr[-3000:]


def test_the_kernels_are_in_the_library(fm):
    """A missing kernel is an error, never a fallback: the launchers are weak references, so the library must be shown to hold them."""
    out = subprocess.check_output(["nm", "-D", "--defined-only", fm._native.LIB_PATH], text=True) + subprocess.check_output(["nm", "--defined-only", fm._native.LIB_PATH], text=True, stderr=subprocess.DEVNULL)
    for launcher in ("launch_group_keys", "launch_group_scan"):
        assert launcher in out, launcher
    blob = open(fm._native.LIB_PATH, "rb").read()
    for kernel in (b"fm_group_keys_kernel", b"fm_group_fill_kernel", b"fm_group_totals_kernel", b"fm_group_carry_kernel", b"fm_group_apply_kernel"):
        assert kernel in blob, kernel


# ---------------------------------------------------------------- the engine's side on the null device
@pytest.fixture(scope="module")
def built():
    if not shutil.which("g++") or not os.path.exists("/opt/rocm/include/hip/hip_runtime_api.h"):
        pytest.skip("needs g++ and the HIP headers")
    r = subprocess.run(["make", "-C", NULLDEV, "-f", "group.mk", "-j8", "group_asan", "group_tsan", "group_absent_asan"], capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return os.path.join(NULLDEV, "build")


def _env(tmp_path, env):
    return dict(os.environ, FMHIP_JIT_CACHE_DIR=str(tmp_path / "code_objects"), FMHIP_JIT_PACK_DIR="off", FMHIP_RING_BYTES="16384", FMHIP_ARENA_BYTES="4096",
                ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1", TSAN_OPTIONS="halt_on_error=1", **env)


@pytest.mark.parametrize("env", [{}, {"FMNULL_DEVICES": "2"}, {"FMNULL_DEVICES": "3"}, {"FMNULL_THREAD_ENGINES": "1"}])
def test_engine_pass_is_clean_under_the_sanitizers(built, tmp_path, env):
    """drive_group: the stand-ins' outputs against the host twin's at n = 1 … 40 007 and small again — every index family, m on either
    side of one, two and three radix passes, 0, 1 and 4 value vectors, every mask, counts and the ungrouped count on and off, hostile
    indices, pending operands, every argument error — on one engine and behind a device list of one shard, behind 2 and 3 shards
    (FMHIP_ERR_UNSUPPORTED, nothing left behind), with thread engines."""
    full = _env(tmp_path, env)
    a = subprocess.run([os.path.join(built, "drive_group_asan")], capture_output=True, text=True, timeout=900, env=full)
    assert a.returncode == 0 and "Sanitizer" not in a.stderr and "runtime error" not in a.stderr, a.stdout[-500:] + a.stderr[-6000:]
    assert a.stdout.count("group done") == 2 and a.stderr == ""
    assert ("a device list of one shard: checked" in a.stdout) == (not env)
    t = subprocess.run([os.path.join(built, "drive_group_tsan")], capture_output=True, text=True, timeout=900, env=full)
    assert t.returncode == 0 and "ThreadSanitizer" not in t.stderr, t.stdout[-500:] + t.stderr[-6000:]
    assert t.stdout.count("group done") == 2 and t.stderr == ""


def test_a_failing_allocation_leaves_nothing_behind(built, tmp_path):
    """A call with one value vector, two outputs and the counts takes SEVEN buffers from the pool: the sort's two key and two index
    buffers, then the counts and the outputs.  The hook FMHIP_TEST_FAIL_ALLOC_AT is set on each (its position from a counting run), and
    once where nothing reaches it: the call answers FMHIP_OK or FMHIP_ERR_OUT_OF_MEMORY, the output handles of a failed call are untouched,
    live vectors and bytes in use are what they were, the same call succeeds afterwards (the driver checks all of it), and the process
    ends without a leak."""
    exe = os.path.join(built, "drive_group_asan")
    counting = subprocess.run([exe, "failure"], capture_output=True, text=True, timeout=600, env=_env(tmp_path, {}))
    assert counting.returncode == 0 and "Sanitizer" not in counting.stderr, counting.stdout[-500:] + counting.stderr[-6000:]
    before, inside, status = map(int, re.search(r"failure: (\d+) allocations before the call, (\d+) in it, status (-?\d+)", counting.stdout).groups())
    assert inside == 7 and status == 0
    for at in list(range(before + 1, before + inside + 1)) + [10**9]:
        r = subprocess.run([exe, "failure"], capture_output=True, text=True, timeout=600, env=_env(tmp_path, {"FMHIP_TEST_FAIL_ALLOC_AT": str(at)}))
        assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr and r.stderr == "", (at, r.stdout[-500:] + r.stderr[-6000:])
        assert "failure done" in r.stdout
        failed = int(re.search(r"status (-?\d+)", r.stdout).group(1)) != 0
        assert failed == (at <= before + inside), (at, r.stdout)


@pytest.mark.parametrize("env", [{}, {"FMNULL_THREAD_ENGINES": "1"}])
def test_a_build_without_the_kernels_answers_unsupported(built, tmp_path, env):
    a = subprocess.run([os.path.join(built, "drive_group_absent_asan")], capture_output=True, text=True, timeout=600, env=_env(tmp_path, env))
    assert a.returncode == 0 and "Sanitizer" not in a.stderr and "runtime error" not in a.stderr, a.stdout[-500:] + a.stderr[-6000:]
    assert a.stdout.count("group absent done") == 2


# ---------------------------------------------------------------- Merton's series term by term: the comparison, and where its seed was fixed
MERTON = dict(initial_value=100.0, risk_free_rate=0.03, volatility=0.2, jump_intensity=1.0, jump_size_mean=-0.1, jump_size_stddev=0.2, maturity=1.0, strike=100.0)
MERTON_PATHS, MERTON_STEPS, MERTON_SEED, MERTON_MAX_JUMPS = 1 << 18, 10, 20261, 15


def merton_term(k, initial_value, risk_free_rate, volatility, jump_intensity, jump_size_mean, jump_size_stddev, maturity, strike):
    """(the Poisson probability of k jumps, e^{-rT}·Black(F_k, K, σ²T + kδ²))"""
    lam_t = jump_intensity * maturity
    half = jump_size_mean + 0.5 * jump_size_stddev ** 2
    forward = initial_value * math.exp((risk_free_rate - jump_intensity * (math.exp(half) - 1.0)) * maturity + k * half)
    v = volatility ** 2 * maturity + k * jump_size_stddev ** 2
    d1 = (math.log(forward / strike) + 0.5 * v) / math.sqrt(v)
    cdf = lambda z: 0.5 * (1.0 + math.erf(z / math.sqrt(2.0)))
    black = forward * cdf(d1) - strike * cdf(d1 - math.sqrt(v))
    return math.exp(-lam_t) * lam_t ** k / math.factorial(k), math.exp(-risk_free_rate * maturity) * black


def check_merton_by_jump_count(result, paths, par=MERTON):
    """Groups 0 … 4 are all compared (expected counts above 4000), further groups where the count is at least 1000: the mean within 4
    standard errors of the series' term, the share within 4 binomial standard errors of the Poisson probability — 4 because about a
    dozen comparisons are made at once.  Prints every figure before it asserts; returns the number of groups compared."""
    compared = 0
    assert sum(result["count"]) + result["ungrouped"] == paths
    for k, (share, mean, se, count) in enumerate(zip(result["share"], result["mean"], result["standard_error"], result["count"])):
        p, term = merton_term(k, **par)
        if k > 4 and count < 1000: continue
        assert count > 0, (k, count)                                                  # (k <= 4 is never skipped: 2^18 paths expect 4018 at k = 4)
        share_se = math.sqrt(p * (1.0 - p) / paths)
        print(f"k = {k}: count {count:.0f}, share {share:.6f} vs {p:.6f} ({(share - p) / share_se:+.2f} se), mean {mean:.5f} vs {term:.5f} ({(mean - term) / se:+.2f} se)")
        assert abs(share - p) <= 4.0 * share_se, (k, share, p, share_se)
        assert abs(mean - term) <= 4.0 * se, (k, mean, term, se)
        compared += 1
    assert compared >= 5
    return compared


def test_the_merton_comparison_holds_for_the_definition_alone(fm):
    """The driver's arithmetic restated in numpy on the increments of fmhip_increments_host (narrowed to float32, as the device draws
    them) with the grouping by the twin: the seed of tests/test_gpu_group.py was fixed HERE, where no kernel is involved."""
    from test_increments_cpu import NORMAL, POISSON, call_host
    par = MERTON
    dt = par["maturity"] / MERTON_STEPS
    laws = [[(NORMAL, math.sqrt(dt), 0.0), (NORMAL, 1.0, 0.0), (POISSON, par["jump_intensity"] * dt, 0.0)] for _ in range(MERTON_STEPS)]
    rc, inc = call_host(fm, MERTON_SEED, laws, MERTON_PATHS)
    assert rc == 0
    inc = inc.astype(np.float32).reshape(MERTON_STEPS, 3, MERTON_PATHS)
    half = par["jump_size_mean"] + 0.5 * par["jump_size_stddev"] ** 2
    drift = par["risk_free_rate"] - 0.5 * par["volatility"] ** 2 - par["jump_intensity"] * (math.exp(half) - 1.0)
    x = np.full(MERTON_PATHS, math.log(par["initial_value"]), dtype=np.float64)
    jumps = np.zeros(MERTON_PATHS, dtype=np.float32)
    for i in range(MERTON_STEPS):
        dw, z, dn = (inc[i, f].astype(np.float64) for f in range(3))
        x += drift * dt + par["volatility"] * dw + par["jump_size_mean"] * dn + par["jump_size_stddev"] * np.sqrt(dn) * z
        jumps += inc[i, 2]
    value = (np.maximum(np.exp(x) - par["strike"], 0.0) * math.exp(-par["risk_free_rate"] * par["maturity"])).astype(np.float32)
    m = MERTON_MAX_JUMPS + 1
    ((mean, variance),), counts, ungrouped = fm.group_sums_host(jumps, [value], m, what=("mean", "variance"))
    count = [float(c) for c in counts]
    result = {"share": [c / MERTON_PATHS for c in count], "mean": [float(v) for v in mean], "count": count, "ungrouped": ungrouped,
              "standard_error": [math.sqrt(float(v) / c) if c > 0 else math.nan for v, c in zip(variance, count)]}
    assert check_merton_by_jump_count(result, MERTON_PATHS) >= 5
