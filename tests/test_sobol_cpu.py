"""CPU-only: the quasi-Monte-Carlo definition (host/sobol.hpp through fmhip_sobol_points_host / fmhip_sobol_increments_host; DESIGN.md
§4.12) — direction numbers, points, digital shift, the Brownian bridge restated in numpy from its specification, argument errors, the
quality of the estimator on a path-dependent payoff with a closed form, and the resource figures of fm_sobol_bm_kernel."""
import ctypes as C
import importlib
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -5


def directions_from_points(fm):
    """The expanded direction words, read back through the entry point: the Gray code of index 2^j is 2^j | 2^(j-1), so
    v[d][j] = x(2^j, d) ^ v[d][j-1]."""
    seq = fm.SobolSequence(1024)
    v = np.zeros((1024, 30), dtype=np.int64)
    for j in range(30):
        x = np.round((seq.points(1 << j, 1)[0] - 2.0 ** -31) * 2.0 ** 30).astype(np.int64)
        v[:, j] = x ^ (v[:, j - 1] if j else 0)
    return v


def test_direction_numbers_are_torch_s_for_all_1024_dimensions(fm):
    torch = pytest.importorskip("torch")
    state = torch.quasirandom.SobolEngine(dimension=1024, scramble=False).sobolstate.numpy()
    assert state.shape == (1024, 30)
    assert (directions_from_points(fm) == state).all()


def test_the_committed_table_is_what_the_tool_generates():
    pytest.importorskip("torch")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "sobol_directions.py"), "--check"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    header = os.path.join(ROOT, "finmath-lib-cuda-extensions_amd", "host", "sobol_directions.hpp")
    assert os.path.getsize(header) < 100_000 and "Frances Y. Kuo and Stephen Joe" in open(header).read()


@pytest.mark.parametrize("d", [1, 2, 7, 160, 1000, 1024])
def test_points_equal_torch_s_sobol_engine(fm, d):
    torch = pytest.importorskip("torch")
    want = torch.quasirandom.SobolEngine(d, scramble=False).draw(4097, dtype=torch.float64).numpy()[1:]
    got = fm.SobolSequence(d).points(1, 4096) - 2.0 ** -31
    assert (got == want).all()
    seq = fm.SobolSequence(d)
    assert (seq.getNext() - 2.0 ** -31 == want[0]).all() and (seq.getNext() - 2.0 ** -31 == want[1]).all() and seq.getDimension() == d


@pytest.mark.parametrize("d", [1, 2, 7, 160, 1000, 1024])
def test_points_equal_scipy_s(fm, d):
    qmc = pytest.importorskip("scipy.stats.qmc")
    want = qmc.Sobol(d, scramble=False).random(4097)[1:]
    assert (fm.SobolSequence(d).points(1, 4096) - 2.0 ** -31 == want).all()


def test_every_dimension_is_a_net_in_base_two(fm):
    """The first 2^k − 1 points plus the origin hit every interval [j 2^-k, (j + 1) 2^-k) once, k = 1 … 12, in every dimension."""
    u = fm.SobolSequence(1024).points(0, 4096)
    assert (u[0] == 2.0 ** -31).all()                                  # the origin (the entry point returns it; the Brownian motion skips it)
    for k in range(1, 13):
        cells = np.floor(u[:1 << k] * (1 << k)).astype(np.int64)
        assert (np.sort(cells, axis=0) == np.arange(1 << k)[:, None]).all(), k


def mt19937_words(seed, count):
    """The first `count` 32-bit words of MT19937 seeded as host/mersenne.hpp seeds it: init_by_array({hi, lo}) of the seed widened to 64 bits."""
    key = [(seed >> 32) & 0xffffffff, seed & 0xffffffff]
    mt = [19650218]
    for i in range(1, 624): mt.append((1812433253 * (mt[-1] ^ (mt[-1] >> 30)) + i) & 0xffffffff)
    i, j = 1, 0
    for _ in range(624):
        mt[i] = ((mt[i] ^ ((mt[i - 1] ^ (mt[i - 1] >> 30)) * 1664525)) + key[j] + j) & 0xffffffff
        i += 1; j += 1
        if i >= 624: mt[0] = mt[623]; i = 1
        if j >= 2: j = 0
    for _ in range(623):
        mt[i] = ((mt[i] ^ ((mt[i - 1] ^ (mt[i - 1] >> 30)) * 1566083941)) - i) & 0xffffffff
        i += 1
        if i >= 624: mt[0] = mt[623]; i = 1
    mt[0] = 0x80000000
    out = []
    while len(out) < count:
        for k in range(624):
            y = (mt[k] & 0x80000000) | (mt[(k + 1) % 624] & 0x7fffffff)
            mt[k] = mt[(k + 397) % 624] ^ (y >> 1) ^ (0x9908b0df if y & 1 else 0)
        for y in mt:
            y ^= y >> 11; y ^= (y << 7) & 0x9d2c5680; y ^= (y << 15) & 0xefc60000; y ^= y >> 18
            out.append(y)
    return out[:count]


@pytest.mark.parametrize("seed", [1, 31415, -7])
def test_randomisation_is_the_documented_digital_shift(fm, seed):
    plain = np.round((fm.SobolSequence(1024).points(1, 500) - 2.0 ** -31) * 2.0 ** 30).astype(np.int64)
    shifted = np.round((fm.SobolSequence(1024, seed).points(1, 500) - 2.0 ** -31) * 2.0 ** 30).astype(np.int64)
    shift = np.array([w >> 2 for w in mt19937_words(seed & 0xffffffffffffffff, 1024)], dtype=np.int64)
    assert (shifted == plain ^ shift).all()
    assert (fm.SobolSequence(1024, seed).points(1, 500) == fm.SobolSequence(1024, seed).points(1, 500)).all()
    assert (fm.SobolSequence(1024, seed).points(1, 500) != fm.SobolSequence(1024, seed + 1).points(1, 500)).any()
    u = fm.SobolSequence(1024, seed).points(1, 500)
    assert (u > 0).all() and (u < 1).all()


# ---------------------------------------------------------------- the bridge, restated from its specification

def bridge_plan(dt):
    """Breadth first: node 0 is the terminal value; then a queue from (0, n): pop (l, r), skip if r − l < 2, m = (l + r) // 2,
    W_m = a W_l + (1 − a) W_r + sd z, push (l, m), (m, r).  Returns the times and [(l, m, r, a, sd)]."""
    n = len(dt)
    t = np.concatenate([[0.0], np.cumsum(np.asarray(dt, dtype=np.float64))])
    nodes = [(0, n, n, 0.0, np.sqrt(t[n] - t[0]))]
    queue = [(0, n)]
    while queue:
        l, r = queue.pop(0)
        if r - l < 2: continue
        m = (l + r) // 2
        a = (t[r] - t[m]) / (t[r] - t[l])
        nodes.append((l, m, r, a, np.sqrt((t[m] - t[l]) * (t[r] - t[m]) / (t[r] - t[l]))))
        queue += [(l, m), (m, r)]
    return t, nodes


def bridge_increments(z, dt):
    """z[node][path] -> increments [step][path]"""
    n = len(dt)
    _, nodes = bridge_plan(dt)
    W = np.zeros((n + 1, z.shape[1]))
    W[n] = nodes[0][4] * z[0]
    for k, (l, m, r, a, sd) in enumerate(nodes[1:], start=1):
        W[m] = a * W[l] + (1.0 - a) * W[r] + sd * z[k]
    return np.diff(W, axis=0)


def normal_quantile(fm, u):
    f = fm.lib().fmhip_inverse_normal_cdf
    return np.array([f(float(x)) for x in u.ravel()]).reshape(u.shape)


@pytest.mark.parametrize("factors", [1, 5])
@pytest.mark.parametrize("equal", [True, False])
@pytest.mark.parametrize("n", [1, 2, 3, 7, 64, 200])
def test_bridge_reproduces_the_numpy_restatement(fm, n, equal, factors):
    dt = np.full(n, 0.05) if equal else 0.01 + np.abs(np.sin(np.arange(n) + 1.0)) * np.linspace(0.5, 2.0, n)
    paths = 64
    got = fm.sobol_increments(4711, dt, factors, paths, "bridge")
    u = fm.SobolSequence(n * factors, 4711).points(1, paths)                         # [path][dimension]
    z = normal_quantile(fm, u)
    for f in range(factors):
        want = bridge_increments(z[:, [k * factors + f for k in range(n)]].T, dt)
        # relative to the increment, or to its standard deviation where the increment itself is small
        assert (np.abs(got[:, f, :] - want) <= 1e-12 * np.maximum(np.abs(want), np.sqrt(dt)[:, None])).all(), (n, f)


@pytest.mark.parametrize("n", [1, 2, 3, 7, 64, 200])
def test_the_bridge_is_an_orthogonal_construction(n):
    """The linear map B of the plan, increments = B z, satisfies B Bᵀ = diag(dt) to 1e-13."""
    for dt in (np.full(n, 0.05), 0.01 + np.abs(np.sin(np.arange(n) + 1.0)) * np.linspace(0.5, 2.0, n)):
        B = bridge_increments(np.eye(n), dt)
        assert np.abs(B @ B.T - np.diag(dt)).max() <= 1e-13 * dt.max()


def test_incremental_construction_is_quantile_times_sqrt_dt_bit_for_bit(fm):
    dt = np.array([0.5, 0.0, 1e-3, 2.0, 0.125])
    got = fm.sobol_increments(99, dt, 3, 2000, "incremental")
    u = fm.SobolSequence(15, 99).points(1, 2000)
    f = fm.lib().fmhip_inverse_normal_cdf
    # AS 241 with the portable logarithm: equal to fmhip_inverse_normal_cdf in the centre (no logarithm there); the tails are compared
    # through the bridge-free identity increment / sqrt(dt) == increment of a unit step
    unit = fm.sobol_increments(99, np.ones(5), 3, 2000, "incremental")
    want = unit * np.sqrt(dt)[:, None, None]
    assert (got.view(np.uint64) == want.view(np.uint64)).all()
    central = np.abs(u - 0.5) <= 0.425
    z = np.array([f(float(x)) for x in u[central]])
    assert (unit.reshape(15, 2000).T[central] == z).all()
    tails = unit.reshape(15, 2000).T[~central]
    zt = np.array([f(float(x)) for x in u[~central]])
    assert np.abs(tails - zt).max() <= 4e-16 * np.abs(zt).max()


@pytest.mark.parametrize("construction", ["bridge", "incremental"])
def test_blocks_behind_an_offset_are_slices_of_the_whole(fm, construction):
    dt = [0.1, 0.4, 0.9]
    for offset in (0, 12_345, 777_777):
        whole = fm.sobol_increments(5, dt, 2, offset + 300, construction)
        block = fm.sobol_increments(5, dt, 2, 300, construction, True, offset)
        assert (block.view(np.uint64) == whole[:, :, offset:].view(np.uint64)).all()
    a = fm.sobol_increments(5, dt, 2, 100, construction, False)
    assert (a != fm.sobol_increments(5, dt, 2, 100, construction, True)).any() and (a == fm.sobol_increments(6, dt, 2, 100, construction, False)).all()


def test_argument_errors(fm):
    lib = fm.lib()
    dt = (C.c_double * 3)(0.1, 0.2, 0.3)
    out = (C.c_double * 60)()
    ok = lambda *a: lib.fmhip_sobol_increments_host(*a)
    assert ok(1, 1, 1, 3, 2, 10, 0, dt, out) == 0
    bad = lambda v: (C.c_double * 3)(0.1, v, 0.3)
    null_d = C.POINTER(C.c_double)()
    calls = [(1, 1, 1, 0, 2, 10, 0, dt, out), (1, 1, 1, 3, 0, 10, 0, dt, out), (1, 1, 1, 3, 2, -1, 0, dt, out), (1, 1, 1, 3, 2, 10, -1, dt, out),
             (1, 2, 1, 3, 2, 10, 0, dt, out), (1, -1, 1, 3, 2, 10, 0, dt, out), (1, 1, 2, 3, 2, 10, 0, dt, out), (1, 1, -1, 3, 2, 10, 0, dt, out),
             (1, 1, 1, 3, 2, 10, 0, null_d, out), (1, 1, 1, 3, 2, 10, 0, dt, null_d),
             (1, 1, 1, 3, 2, 10, 0, bad(-0.2), out), (1, 1, 0, 3, 2, 10, 0, bad(-0.2), out), (1, 1, 1, 3, 2, 10, 0, bad(float("nan")), out),
             (1, 1, 0, 3, 2, 10, 0, bad(float("nan")), out), (1, 1, 1, 3, 2, 10, 0, bad(float("inf")), out), (1, 1, 0, 3, 2, 10, 0, bad(float("inf")), out),
             (1, 1, 1, 3, 2, 10, 0, bad(0.0), out),
             (1, 1, 1, 3, 2, 10, (1 << 30) - 10, dt, out), (1, 1, 1, 3, 2, 1, 1 << 30, dt, out), (1, 1, 1, 3, 342, 10, 0, dt, out), (1, 1, 0, 1025, 1, 1, 0, dt, out)]
    for args in calls:
        assert ok(*args) == INVALID, args[:7]
        assert lib.fmhip_last_error()
    assert ok(1, 1, 0, 3, 2, 10, 0, bad(0.0), out) == 0
    assert ok(1, 1, 1, 3, 2, 10, (1 << 30) - 11, dt, out) == 0
    assert b"time step 1" in (ok(1, 1, 1, 3, 2, 10, 0, bad(-0.2), out), lib.fmhip_last_error())[1]
    u = (C.c_double * 2050)()
    assert lib.fmhip_sobol_points_host(1025, 1, 1, 0, 0, u) == INVALID and b"1025" in lib.fmhip_last_error()
    for args in ((0, 1, 1, 0, 0, u), (2, -1, 1, 0, 0, u), (2, 1 << 30, 1, 0, 0, u), (2, 1, -1, 0, 0, u), (2, 1, 1, 0, 2, u), (2, 1, 1, 0, 0, null_d)):
        assert lib.fmhip_sobol_points_host(*args) == INVALID, args[:5]
    assert lib.fmhip_sobol_points_host(1024, (1 << 30) - 2, 2, 0, 0, u) == 0
    with pytest.raises(ValueError):
        fm.SobolSequence(1025)
    with pytest.raises(ValueError):
        fm.sobol_increments(1, [0.1], 1, 1, "pca")


def test_device_entry_point_needs_a_device(fm):
    """Bound in the library, the binding and the header; without an initialised engine it reports that, and touches nothing."""
    try:
        import torch
        if torch.cuda.is_available(): pytest.skip("a GPU is present")
    except ImportError:
        pass
    lib = fm.lib()
    if lib.fmhip_is_initialized(): pytest.skip("runtime already initialised")
    for name in ("fmhip_sobol_points_host", "fmhip_sobol_increments_host", "fmhip_bm_generate_sobol_device"):
        assert name in fm._native.SYMBOLS and hasattr(lib, name)
    out = (C.c_int64 * 6)()
    assert lib.fmhip_bm_generate_sobol_device(1, 1, 1, 3, 2, 10, 0, (C.c_double * 3)(0.1, 0.2, 0.3), out) == fm._native.ERR_NOT_INITIALIZED and out[0] == 0


def test_quality_on_a_geometric_asian_call(fm):
    """64 equal steps, 2^16 paths, seeds 1 … 16, randomised: the RMS error of the bridge against the closed form is at most 1/10 of the
    pseudo-random standard error of the same payoff at the same N (sample standard deviation / sqrt(N), from fmhip_mersenne_increments),
    and no larger than the RMS error of the incremental construction."""
    mc = importlib.import_module("finmath-lib-cuda-extensions_amd.montecarlo")
    n, steps = 1 << 16, 64
    dt = np.full(steps, 1.0 / steps)
    times = (np.arange(steps) + 1.0) / steps
    exact = mc.geometric_asian_call_analytic(100.0, 0.05, 0.2, times, 100.0)
    assert abs(exact - 5.620434) < 1e-6

    def payoff(increments):                                  # [step][0][path]
        x = np.log(100.0) + (0.05 - 0.02) * times[:, None] + 0.2 * np.cumsum(increments[:, 0, :], axis=0)
        return np.exp(-0.05) * np.maximum(np.exp(x.mean(axis=0)) - 100.0, 0.0)

    pseudo = payoff(fm.mersenne_increments(1, dt, 1, n))
    standard_error = pseudo.std(ddof=1) / np.sqrt(n)
    rms = {}
    for construction in ("bridge", "incremental"):
        errors = np.array([payoff(fm.sobol_increments(seed, dt, 1, n, construction)).mean() - exact for seed in range(1, 17)])
        rms[construction] = float(np.sqrt(np.mean(errors ** 2)))
        print(f"{construction}: RMS error {rms[construction]:.3e}, largest {np.abs(errors).max():.3e}")
    print(f"pseudo-random: error {pseudo.mean() - exact:.3e}, standard error {standard_error:.3e}; ratio {standard_error / rms['bridge']:.1f}")
    assert rms["bridge"] <= standard_error / 10
    assert rms["bridge"] <= rms["incremental"]


def test_resource_figures_of_the_kernel():
    """fm_sobol_bm_kernel uses no scratch (the bridge's values live in LDS, sized at launch): the compiler's own remarks of a cross-compile
    with the build's flags."""
    hipcc = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else shutil.which("hipcc")
    if not hipcc:
        pytest.skip("needs hipcc")
    csrc = os.path.join(ROOT, "finmath-lib-cuda-extensions_amd", "csrc")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-mllvm", "-structurizecfg-skip-uniform-regions",
                        "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(csrc, "sobol_kernel.hip"), "-o", os.devnull],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    figures, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark:\s+(Function Name|VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]|VGPRs Spill|SGPRs Spill): (\S+)", line)
        if not m: continue
        if m.group(1) == "Function Name": name = m.group(2); figures[name] = {}
        else: figures[name][m.group(1).split(" [")[0]] = int(m.group(2))
    kernel = next(v for k, v in figures.items() if "fm_sobol_bm_kernel" in k)
    print("fm_sobol_bm_kernel:", kernel)
    assert kernel["ScratchSize"] == 0 and kernel["VGPRs Spill"] == 0 and kernel["SGPRs Spill"] == 0 and kernel["LDS Size"] == 0 and kernel["Occupancy"] >= 4
    text = open(os.path.join(csrc, "sobol_kernel.hip")).read()
    assert "asm" not in re.sub(r"//.*", "", text)


def test_cpp_mirror_on_the_host(fm, oracle, tmp_path):
    """tests/cpp/test_sobol.cpp in its `host` mode: BrownianMotionFromSobolSequence over the CPU factory hands out the definition's
    increments; a block behind a path offset is a slice."""
    if not shutil.which("g++"):
        pytest.skip("needs g++")
    exe = str(tmp_path / "test_sobol_mirror")
    libdir = os.path.join(ROOT, "finmath-lib-cuda-extensions_amd", "lib")
    orcdir = os.path.join(ROOT, "oracle")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_sobol.cpp"),
                           f"-L{libdir}", "-lfmhip", f"-L{orcdir}", "-lfm_oracle", f"-Wl,-rpath,{libdir}", f"-Wl,-rpath,{orcdir}", "-lm"])
    out = subprocess.run([exe, "host"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.strip().splitlines()[-1] == "OK host", out.stdout + out.stderr
