"""Kernel regression without a GPU (include/fmhip.h: fmhip_kernel_moments_host; host/kernel_regression.hpp; kernel_regression.py; DESIGN.md
§4.19): the host DEFINITION against a plain numpy restatement (a mask and a sum per point) — within the derived bound on random data, for
EQUALITY on dyadic data whose terms and partial sums are shown to be exact —, membership on and one ulp beside every support end, every
argument refusal, kernel_local_fit, the host half of the kernel under the sanitizers (tests/cpp/test_kernel_regression_host.cpp), the
engine's side on the null device under ASan/UBSan and TSan (tests/nulldev/kreg.mk), the kernel's resource usage for gfx950 (0 bytes of
scratch), and the Python mirror on the oracle's float class."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "finmath-lib-cuda-extensions_amd", "csrc")
NULLDEV = os.path.join(ROOT, "tests", "nulldev")
PD = C.POINTER(C.c_double)
KERNELS = ["uniform", "triangular", "epanechnikov", "quartic", "triweight"]
BAD = -5                                                            # FMHIP_ERR_INVALID_ARGUMENT


def bits(a): return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def host(fm, key, points, h, ys=(), kernel=2, order=0, n_points=None, n_y=None, n=None):
    """fmhip_kernel_moments_host through ctypes: (status, sums[Q][entries])."""
    key = np.ascontiguousarray(key, dtype=np.float32)
    p = np.ascontiguousarray(points, dtype=np.float64); b = np.ascontiguousarray(np.broadcast_to(np.asarray(h, dtype=np.float64), p.shape))
    ys = [np.ascontiguousarray(y, dtype=np.float32) for y in ys]
    Q = p.size if n_points is None else n_points
    ny = len(ys) if n_y is None else n_y
    out = np.full((max(Q, 1), 1 + ny if order == 0 else 3 + 2 * max(ny, 0)), -7.0)
    cols = (C.c_void_p * max(len(ys), 1))(*[y.ctypes.data for y in ys])
    st = fm.lib().fmhip_kernel_moments_host(key.ctypes.data_as(C.c_void_p), key.size if n is None else n, p.ctypes.data_as(PD), b.ctypes.data_as(PD), Q, kernel, order,
                                            cols if ys else None, ny, out.ctypes.data_as(PD))
    return st, out


def weights(kernel, d, rh):
    """The definition's weight, operation by operation, in numpy's fp64 (which contracts nothing)."""
    u = d * rh
    t = 1.0 - u * u
    w = {"uniform": np.ones_like(u), "triangular": 1.0 - np.abs(u), "epanechnikov": t, "quartic": t * t, "triweight": (t * t) * t}[kernel]
    return np.where(w < 0.0, 0.0, w)


def terms_of(key, points, h, ys, kernel, order, q):
    """(member mask, [terms per entry]) of point q: the plain restatement — a mask and the definition's products."""
    xd = key.astype(np.float64)
    p, b = float(points[q]), float(np.broadcast_to(h, np.shape(points))[q])
    lower, upper, rh = p - b, p + b, 1.0 / b
    with np.errstate(invalid="ignore"):
        m = (lower < xd) & (xd < upper)
    d = xd[m] - p
    w = weights(kernel, d, rh)
    yd = [y.astype(np.float64)[m] for y in ys]
    if order == 0: return m, [w] + [w * y for y in yd]
    e1 = w * d
    return m, [w, e1, e1 * d] + [w * y for y in yd] + [e1 * y for y in yd]


def numpy_moments(key, points, h, ys, kernel, order):
    """sums, Σ|terms| and member counts per (point, entry)."""
    Q = len(points)
    qe = 1 + len(ys) if order == 0 else 3 + 2 * len(ys)
    sums, absolute, members = np.zeros((Q, qe)), np.zeros((Q, qe)), np.zeros(Q, dtype=np.int64)
    for q in range(Q):
        m, terms = terms_of(key, points, h, ys, kernel, order, q)
        members[q] = int(m.sum())
        for e, t in enumerate(terms): sums[q, e] = t.sum(); absolute[q, e] = np.abs(t).sum()
    return sums, absolute, members


def bound(absolute, members):
    """Two summation orders of the same exact fp64 terms: each within m·2⁻⁵³·Σ|terms| of the exact sum."""
    return 2.0 * members[:, None] * 2.0 ** -53 * absolute * (1 + 1e-6)


def dyadic_case(n, Q, h, seed, n_y=4, span=8.0):
    """Keys k/8, points multiples of 1/4 (each one twice), one dyadic bandwidth, integer |y| <= 16."""
    rng = np.random.default_rng(seed)
    key = (rng.integers(-int(span * 8), int(span * 8) + 1, n) / 8.0).astype(np.float32)
    points = np.sort(-span + 0.25 * (np.arange(Q) // 2 * 2 % int(8 * span)))
    ys = [rng.integers(-16, 17, n).astype(np.float32) for _ in range(n_y)]
    return key, points, float(h), ys


GRID = 2.0 ** -30      # d is a multiple of 1/8 and rh of 1/2: u of 1/16, t = 1 − u² of 2⁻⁸, (t·t)·t of 2⁻²⁴, ·d of 2⁻²⁷, ·d of 2⁻³⁰; y is an integer


def assert_exact(terms, what):
    """Every term is a multiple of GRID and Σ|terms| / GRID < 2⁵³: every partial sum, in ANY order, is exactly representable."""
    scaled = np.asarray(terms, dtype=np.float64) / GRID
    assert (scaled == np.rint(scaled)).all(), what
    assert math.fsum(np.abs(scaled)) < 2.0 ** 53, what


@pytest.mark.parametrize("kernel", KERNELS)
def test_definition_equals_numpy_on_dyadic_data(fm, kernel):
    """Keys k/8, points on multiples of 1/4, h in {0.5, 1, 2}, integer |y| <= 16: the terms and every partial sum are exact (shown with
    math.fsum and the power-of-two grid of the terms, not assumed), so the definition's path-order sums EQUAL numpy's pairwise sums."""
    n = 2 ** 16 if kernel == "triweight" else 2 ** 20
    for h, order, n_y in ((0.5, 1, 2), (1.0, 0, 4), (2.0, 1, 1)):
        key, points, h, ys = dyadic_case(n, 8, h, seed=int(h * 8) + order, n_y=n_y)
        st, got = host(fm, key, points, h, ys, KERNELS.index(kernel), order)
        assert st == 0
        for q in range(len(points)):
            m, terms = terms_of(key, points, h, ys, kernel, order, q)
            for e, t in enumerate(terms):
                assert_exact(t, (kernel, h, order, q, e))
                assert got[q, e] == t.sum() == math.fsum(t), (kernel, h, order, q, e)


@pytest.mark.parametrize("kernel", KERNELS)
def test_definition_against_numpy_on_random_data(fm, kernel):
    rng = np.random.default_rng(5)
    n = 50_001
    key = rng.standard_normal(n).astype(np.float32)
    ys = [rng.standard_normal(n).astype(np.float32), (2 + 3 * key).astype(np.float32)]
    points = np.linspace(-3, 3, 41); h = 0.25 + 0.004 * np.abs(np.arange(41) - 20)
    for order in (0, 1):
        st, got = host(fm, key, points, h, ys, KERNELS.index(kernel), order)
        want, absolute, members = numpy_moments(key, points, h, ys, kernel, order)
        assert st == 0 and members.min() > 10
        assert (np.abs(got - want) <= bound(absolute, members)).all(), (kernel, order)
    # the layout is one: W, Wd, Wdd are the same bits for both orders, a y's sums do not depend on its slot or on n_y
    s0 = host(fm, key, points, h, ys, KERNELS.index(kernel), 0)[1]; s1 = host(fm, key, points, h, ys, KERNELS.index(kernel), 1)[1]
    alone = host(fm, key, points, h, ys[1:], KERNELS.index(kernel), 1)[1]
    assert (bits(s0[:, 0]) == bits(s1[:, 0])).all() and (bits(s0[:, 1:]) == bits(s1[:, 3:5])).all()
    assert (bits(alone[:, 3]) == bits(s1[:, 4])).all() and (bits(alone[:, 4]) == bits(s1[:, 6])).all()


def edge_grid():
    """Duplicated points, bandwidths that differ per point (lower and upper stay non-decreasing), ends that are fp32 numbers and ends that are not."""
    points = np.array([-2.0, -2.0, -1.0, -0.5, 0.0, 0.0, 0.1, 0.75, 1.5, 1.5, 4.0])
    h = np.array([0.5, 0.5, 0.75, 0.5, 0.25, 0.25, 0.3, 0.5, 1.0, 1.0, 3.0])
    assert (np.diff(points - h) >= 0).all() and (np.diff(points + h) >= 0).all()
    return points, h


def edge_keys(points, h):
    """Exactly ON lower_q and upper_q (narrowed to fp32), one fp32 ulp to either side, the points, NaN, ±inf, ±0, denormals."""
    ends = np.concatenate([points - h, points + h, points]).astype(np.float32)
    keys = np.concatenate([ends, np.nextafter(ends, np.float32(np.inf)), np.nextafter(ends, np.float32(-np.inf)),
                           np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-45, -1e-45, 3.4e38, -3.4e38], dtype=np.float32)])
    return keys.astype(np.float32)


def test_membership_is_the_pair_predicate(fm):
    points, h = edge_grid()
    key = edge_keys(points, h)
    st, got = host(fm, key, points, h, [], 0, 0)                     # uniform kernel: W is the member count
    assert st == 0
    xd = key.astype(np.float64)
    with np.errstate(invalid="ignore"):
        member = ((points - h)[:, None] < xd[None, :]) & (xd[None, :] < (points + h)[:, None])
    assert (got[:, 0] == member.sum(axis=1)).all()
    assert not member[:, ~np.isfinite(xd)].any()                     # a NaN or infinite key is a member of no point
    assert (fm.kernel_counts(key, points, h) == member.sum(axis=1)).all()      # the counting identity, on the host
    # every single key: its members are a contiguous range [a, b)
    for i in range(key.size):
        st, one = host(fm, key[i:i + 1], points, h, [], 0, 0)
        assert st == 0 and (one[:, 0] == member[:, i]).all(), key[i]
        inside = np.flatnonzero(member[:, i])
        assert inside.size == 0 or (np.diff(inside) == 1).all()


def test_bad_arguments_are_refused(fm):
    key = np.zeros(8, dtype=np.float32)
    fine, h = np.array([0.0, 1.0, 2.0]), 1.0
    assert host(fm, key, fine, h, [key])[0] == 0
    assert host(fm, key, fine, np.array([1.0, 2.5, 2.5]))[0] == BAD                 # lower: -1, -1.5
    assert host(fm, key, fine, np.array([2.5, 1.0, 1.0]))[0] == BAD                 # upper: 2.5, 2
    assert host(fm, key, fine, np.array([1.0, 0.0, 1.0]))[0] == BAD
    assert host(fm, key, fine, np.array([1.0, -1.0, 1.0]))[0] == BAD
    assert host(fm, key, fine, np.array([1.0, np.nan, 1.0]))[0] == BAD
    assert host(fm, key, fine, np.array([1.0, np.inf, 1.0]))[0] == BAD
    assert host(fm, key, np.array([0.0, np.nan, 2.0]), h)[0] == BAD
    assert host(fm, key, np.array([0.0, np.inf, np.inf]), h)[0] == BAD
    assert host(fm, key, np.array([0.0, 2.0, 1.0]), h)[0] == BAD
    assert host(fm, key, fine, h, n_points=0)[0] == BAD
    assert host(fm, key, np.zeros(257), h)[0] == BAD and host(fm, key, np.zeros(256), h)[0] == 0
    assert host(fm, key, fine, h, [key] * 5)[0] == BAD and host(fm, key, fine, h, [key] * 4)[0] == 0
    assert host(fm, key, fine, h, [key], n_y=-1)[0] == BAD
    assert host(fm, key, fine, h, order=2)[0] == BAD and host(fm, key, fine, h, order=-1)[0] == BAD
    assert host(fm, key, fine, h, kernel=5)[0] == BAD and host(fm, key, fine, h, kernel=-1)[0] == BAD
    assert host(fm, key, fine, h, n=0)[0] == BAD
    lib = fm.lib()
    out = np.zeros(16); p = fine.ctypes.data_as(PD); b = np.ones(3).ctypes.data_as(PD)
    k = key.ctypes.data_as(C.c_void_p)
    assert lib.fmhip_kernel_moments_host(None, 8, p, b, 3, 0, 0, None, 0, out.ctypes.data_as(PD)) == BAD
    assert lib.fmhip_kernel_moments_host(k, 8, None, b, 3, 0, 0, None, 0, out.ctypes.data_as(PD)) == BAD
    assert lib.fmhip_kernel_moments_host(k, 8, p, None, 3, 0, 0, None, 0, out.ctypes.data_as(PD)) == BAD
    assert lib.fmhip_kernel_moments_host(k, 8, p, b, 3, 0, 0, None, 1, out.ctypes.data_as(PD)) == BAD
    assert lib.fmhip_kernel_moments_host(k, 8, p, b, 3, 0, 0, (C.c_void_p * 1)(None), 1, out.ctypes.data_as(PD)) == BAD
    assert lib.fmhip_kernel_moments_host(k, 8, p, b, 3, 0, 0, None, 0, None) == BAD
    for name in ("fmhip_kernel_moments", "fmhip_kernel_moments_host"):
        assert name in fm._native.SYMBOLS


def test_local_fit(fm):
    rng = np.random.default_rng(9)
    key = (rng.integers(-512, 513, 5000) / 256.0).astype(np.float32)
    line = (2.0 + 3.0 * key).astype(np.float32)
    assert (line.astype(np.float64) == 2.0 + 3.0 * key.astype(np.float64)).all()      # the data lie ON the line
    points = np.array([-1.5, -0.5, 0.0, 0.75, 1.5])
    for kernel in KERNELS:
        sums = fm.kernel_moments_host(key, points, 0.5, [line], kernel, 1)
        values, slopes = fm.kernel_local_fit(sums, 1, 1, points)
        # order 1 reproduces a straight line up to the rounding of the sums (members·2⁻⁵³ relative, each) through a 2×2 solve whose
        # determinant W·Wdd − Wd² keeps at least a tenth of W·Wdd for these symmetric windows
        assert np.abs(values[0] - (2.0 + 3.0 * points)).max() <= 1e-11 and np.abs(slopes[0] - 3.0).max() <= 1e-10, kernel
        v0, s0 = fm.kernel_local_fit(fm.kernel_moments_host(key, points, 0.5, [line], kernel, 0), 0, 1, points)
        assert (s0 == 0.0).all() and np.abs(v0[0] - (2.0 + 3.0 * points)).max() < 0.2                # local constant: biased by the design, not wrong
    # a singular point (every member at one key: W·Wdd = Wd²) falls back to Wy / W; empty points are filled from their neighbours
    pts = np.arange(5.0)
    s = np.zeros((5, 5))
    s[1] = [4.0, 1.0, 0.25, 28.0, 7.0]
    s[3] = [2.0, -1.0, 0.5, 22.0, -11.0]
    v, sl = fm.kernel_local_fit(s, 1, 1, pts)
    assert v[0].tolist() == [7.0, 7.0, 9.0, 11.0, 11.0] and (sl == 0.0).all()
    s0 = np.array([[0, 0], [2.0, 6.0], [0, 0], [0, 0], [4.0, 4.0]])
    v, _ = fm.kernel_local_fit(s0, 0, 1, pts)
    assert v[0].tolist() == [3.0, 3.0, 3.0 + (1.0 / 3.0) * (1.0 - 3.0), 3.0 + (2.0 / 3.0) * (1.0 - 3.0), 1.0]
    with pytest.raises(ValueError): fm.kernel_local_fit(np.zeros((5, 5)), 1, 1, pts)
    # a regular point between two empty ones, two dependents
    s2 = np.zeros((3, 7)); s2[1] = [2.0, 0.0, 2.0, 6.0, 10.0, 4.0, -2.0]          # members at d = ±1: y0 = 1, 5 -> 3 + 2d; y1 = 6, 4 -> 5 − d
    v, sl = fm.kernel_local_fit(s2, 1, 2, np.array([0.0, 1.0, 2.0]))
    assert v.tolist() == [[3.0] * 3, [5.0] * 3] and sl.tolist() == [[2.0] * 3, [-1.0] * 3]


# ---------------------------------------------------------------- the host half of the kernel under the sanitizers
def test_host_half_under_the_sanitizers(tmp_path):
    """tests/cpp/test_kernel_regression_host.cpp: the two branch-free searches against the pair predicate on and beside every support end,
    a model of the kernel's index arithmetic and slice loop over exactly-sized allocations against the definition (equal on dyadic data,
    within the bound on random data), kernel_local_fit, the refusals."""
    gxx = shutil.which("g++")
    if not gxx or not os.path.exists("/opt/rocm/include/hip/hip_runtime_api.h"):
        pytest.skip("needs g++ and the HIP headers (csrc/kreg_kernel.h declares the launcher)")
    exe = tmp_path / "kreg_host"
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-ffp-contract=off",
                        "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-Wno-deprecated-declarations",
                        os.path.join(ROOT, "tests", "cpp", "test_kernel_regression_host.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "kernel regression host ok" in r.stdout and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stdout[-1500:] + r.stderr[-3000:]


def test_the_kernel_is_in_the_library(fm):
    """A missing kernel is an error, never a fallback: the launcher is a weak reference, so the library must be shown to hold it."""
    out = subprocess.check_output(["nm", "-D", "--defined-only", fm._native.LIB_PATH], text=True) + subprocess.check_output(["nm", "--defined-only", fm._native.LIB_PATH], text=True, stderr=subprocess.DEVNULL)
    assert "launch_kernel_moments" in out
    assert b"fm_kernel_moments_kernel" in open(fm._native.LIB_PATH, "rb").read()


def test_kernel_compiles_for_gfx950_without_scratch():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc): pytest.skip("needs hipcc")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                        "-c", os.path.join(CSRC, "kreg_kernel.hip"), "-o", os.devnull], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    seen = {}
    for blk in re.split(r"remark: Function Name: ", r.stderr)[1:]:
        seen[blk.split()[0]] = (int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", blk).group(1)), int(re.search(r"LDS Size \[bytes/block\]: (\d+)", blk).group(1)))
    kernels = {k: v for k, v in seen.items() if "fm_kernel_moments_kernel" in k}
    assert len(kernels) == 1, seen
    for name, (scratch, lds) in kernels.items():
        assert scratch == 0, (name, scratch)
        assert lds <= 160 * 1024, (name, lds)                        # a CU's LDS (one workgroup may declare all of it)


# ---------------------------------------------------------------- the engine's side on the null device
@pytest.fixture(scope="module")
def built():
    if not shutil.which("g++") or not os.path.exists("/opt/rocm/include/hip/hip_runtime_api.h"):
        pytest.skip("needs g++ and the HIP headers")
    r = subprocess.run(["make", "-C", NULLDEV, "-f", "kreg.mk", "-j8", "kreg_asan", "kreg_tsan", "kreg_absent_asan", "kreg_absent_tsan"], capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return os.path.join(NULLDEV, "build")


def _env(tmp_path, env):
    return dict(os.environ, FMHIP_JIT_CACHE_DIR=str(tmp_path / "code_objects"), FMHIP_JIT_PACK_DIR="off", FMHIP_RING_BYTES="16384", FMHIP_ARENA_BYTES="4096",
                ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1", TSAN_OPTIONS="halt_on_error=1", **env)


@pytest.mark.parametrize("env", [{}, {"FMNULL_DEVICES": "2"}, {"FMNULL_DEVICES": "3"}, {"FMNULL_THREAD_ENGINES": "1"}])
def test_engine_pass_is_clean_under_the_sanitizers(built, tmp_path, env):
    """drive_kreg: fmhip_kernel_moments on dyadic data at 1 … 256 points, every kernel, both orders, 0 … 4 dependents, sliced and unsliced,
    bit for bit against fmhip_kernel_moments_host (the stand-in launcher runs the definition slice by slice from the tables the engine sent
    up); pending operands whose inputs another thread releases during the call; every refusal before a flush, with nothing allocated — on
    one engine, behind 2 and 3 shards (sums in shard order), with thread engines (a caller that does not own the vectors)."""
    full = _env(tmp_path, env)
    a = subprocess.run([os.path.join(built, "drive_kreg_asan")], capture_output=True, text=True, timeout=600, env=full)
    assert a.returncode == 0 and "Sanitizer" not in a.stderr and "runtime error" not in a.stderr, a.stdout[-500:] + a.stderr[-6000:]
    assert a.stdout.count("kreg done") == 2 and a.stderr == ""
    t = subprocess.run([os.path.join(built, "drive_kreg_tsan")], capture_output=True, text=True, timeout=600, env=full)
    assert t.returncode == 0 and "ThreadSanitizer" not in t.stderr, t.stdout[-500:] + t.stderr[-6000:]
    assert t.stdout.count("kreg done") == 2 and t.stderr == ""


@pytest.mark.parametrize("env", [{}, {"FMNULL_DEVICES": "2"}, {"FMNULL_THREAD_ENGINES": "1"}])
def test_a_build_without_the_kernel_answers_unsupported(built, tmp_path, env):
    for exe in ("drive_kreg_absent_asan", "drive_kreg_absent_tsan"):
        a = subprocess.run([os.path.join(built, exe)], capture_output=True, text=True, timeout=600, env=_env(tmp_path, env))
        assert a.returncode == 0 and "Sanitizer" not in a.stderr and "runtime error" not in a.stderr, a.stdout[-500:] + a.stderr[-6000:]
        assert a.stdout.count("kreg absent done") == 2


# ---------------------------------------------------------------- the Python mirror on the oracle's float class
def test_mirror_on_the_oracle_backed_factory(fm, oracle, monkeypatch):
    monkeypatch.setenv("FMHIP_DEVICE_KERNEL_MOMENTS", "0")
    rng = np.random.default_rng(3)
    n = 20_000
    x = rng.standard_normal(n).astype(np.float32)
    y = (2.0 + 3.0 * x).astype(np.float32)
    z = (x.astype(np.float64) ** 2).astype(np.float32)
    f = oracle.RandomVariableFloatFactory()
    X, Y, Z = (f.createRandomVariable(0.0, a.astype(np.float64)) for a in (x, y, z))
    points = np.linspace(-2.0, 2.0, 17)
    sums = fm.kernel_moments(X, points, 0.4, [Y, Z], "quartic", 1)
    st, want = host(fm, x, points, 0.4, [y, z], 3, 1)
    assert st == 0 and sums.shape == (17, 7) and (bits(sums) == bits(want)).all()
    counts = fm.kernel_counts(X, points, 0.4)
    assert (counts == fm.kernel_moments(X, points, 0.4, (), "uniform", 0)[:, 0]).all() and counts.sum() > n
    sigma = math.sqrt(X.getVariance())
    assert fm.silverman_bandwidth(X) == 1.06 * sigma * n ** -0.2 and fm.silverman_bandwidth(X, 2.0) == 2.0 * fm.silverman_bandwidth(X)
    # the density of a standard normal sample: within the kernel's bias h²/2·|φ''|·μ₂ <= 0.4²/2·0.4/5 and five standard errors sqrt(φ·R(K)/(n·h))
    density = fm.kernel_density(X, points, 0.4, "epanechnikov")
    phi = np.exp(-0.5 * points ** 2) / math.sqrt(2 * math.pi)
    assert np.abs(density - phi).max() <= 0.4 ** 2 / 2 * 0.4 / 5 + 5 * math.sqrt(0.4 * 0.6 / (n * 0.4))
    est = fm.MonteCarloConditionalExpectationKernelRegression(X, points, 0.4, "epanechnikov", order=1)
    fitted = est.getFittedValues(Y)
    assert np.abs(fitted - (2.0 + 3.0 * points)).max() <= 1e-5                     # y is the line narrowed to fp32: 2⁻²⁴·|y| per element
    both = est.getFittedValues([Y, Z])
    assert both.shape == (2, 17) and (bits(both[0]) == bits(fitted)).all() and np.abs(both[1] - points ** 2).max() < 0.1
    ce = est.getConditionalExpectation(Y)
    assert type(ce) is type(X) and ce.getFiltrationTime() == 0.0
    table = fm.TabulatedFunction(points, fitted, "linear", "constant")
    assert (np.asarray(ce.getRealizations(), dtype=np.float32).view(np.uint32) == fm.table_apply_host(x, [table])[0].view(np.uint32)).all()
    inside = np.abs(x) <= 2.0
    assert np.abs(np.asarray(ce.getRealizations())[inside] - y[inside]).max() <= 1e-4
    # defaults: 64 points between the 0.1 % and 99.9 % quantiles, bandwidth max(3·Silverman, 1.5·spacing)
    default = fm.MonteCarloConditionalExpectationKernelRegression(X)
    s = np.sort(x.astype(np.float64))
    assert default.points.size == 64 and default.points[0] == s[int(0.001 * (n - 1))] and default.points[-1] == s[math.ceil(0.999 * (n - 1))]
    spacing = np.diff(default.points).max()
    assert (default.bandwidths == max(3 * fm.silverman_bandwidth(X), 1.5 * spacing)).all() and default.order == 1
    assert np.abs(default.getFittedValues(Y) - (2.0 + 3.0 * default.points)).max() <= 1e-4
    with pytest.raises(ValueError): fm.MonteCarloConditionalExpectationKernelRegression(f.createRandomVariable(0.0, 1.0))
    with pytest.raises(ValueError): fm.MonteCarloConditionalExpectationKernelRegression(X, points, 0.4, "gaussian")
    with pytest.raises(ValueError): fm.kernel_moments(X, points, 0.4, [Y], "cosine")
