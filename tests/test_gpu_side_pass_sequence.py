"""The reducing side passes back to back on ONE engine (csrc/side_pass_engine.hpp: they share the zeroed scratch, the other scratch, the pinned
block and the completion flag's sequence): binned cross moments with the most bins and products, a count, a refused call, a radix select, cross
moments with the constant 1, rank sums, binned cross moments with one bin — on one engine and behind a device list {0, 0}.  Every result is
held to the expectation of its pass's own GPU test (test_gpu_binned.py, test_gpu_order_statistics.py, test_gpu_cross_moments.py): the host
definition and the exact sums, never another run of the device code.

Sizes: one element (behind the device list the second shard holds no path), one tile of the widest pass plus one, three such tiles plus five."""
import json
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from test_binned_cpu import exact_and_bound, host_moments
from test_gpu_binned import packed
from test_gpu_cross_moments import bound, exact
from test_gpu_order_statistics import java_sorted, same_bits

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "finmath-lib-cuda-extensions_amd", "csrc")


def tile():
    """The largest of the three passes' tiles, from the headers the kernels are compiled with."""
    text = open(os.path.join(CSRC, "kernels.h")).read() + open(os.path.join(CSRC, "binned_kernel.h")).read()
    return max(int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1)) for name in ("FM_OS_TILE", "FM_XMOM_TILE", "FM_BINNED_TILE"))


SIZES = [1, tile() + 1, 3 * tile() + 5]
COUNT_BOUNDS = [-0.5, 0.0, 0.7, np.inf]


def case(n):
    """key (NaN and ±inf among the keys from 8 elements on), 63 bounds, two x and four y."""
    rng = np.random.default_rng(1000 + n)
    key = rng.standard_normal(n).astype(np.float32)
    if n >= 8: key[:4] = [np.nan, np.inf, -np.inf, -0.0]
    bounds = np.sort(rng.standard_normal(63))
    cols = [rng.standard_normal(n).astype(np.float32) for _ in range(6)]
    return key, bounds, cols[:2], cols[2:]


def ranks_of(n):
    return np.unique([0, n // 2, n - 1]).astype(np.int64), (n // 4, n - 1 - n // 4)


def run_sequence(fm, n):
    """The seven calls, on whatever `fm` was initialised with; what they returned, as plain lists."""
    import ctypes as C
    key, bounds, xs, ys = case(n)
    up = fm.DeviceVector.from_host
    K, X, Y = up(key), [up(a) for a in xs], [up(a) for a in ys]
    out = {}
    counts, S, T = fm.binned_cross_moments(K, bounds, [None] + X, Y)                  # 64 bins, 17 products and the count: the largest zeroed scratch
    out["binned64"] = [counts.tolist(), packed(S, T).tolist()]
    out["counts"] = X[0].count_not_above(COUNT_BOUNDS).tolist()
    try:
        fm.binned_cross_moments(K, bounds, [None, X[0]], [up(ys[0][:n - 1])])
        out["refused"] = 0
    except fm.FmhipError as e:
        out["refused"] = e.code
    ranks, (i0, i1) = ranks_of(n)
    out["select"] = fm.select_ranks_batch(X, ranks).tolist()
    S, T = fm.cross_moments([None] + X, Y[:1])
    out["xmom"] = [S.tolist(), T.tolist()]
    sums = (C.c_double * 2)()
    fm._native.check(fm.lib().fmhip_rank_sums_batch((C.c_int64 * 2)(X[0].handle, X[1].handle), 2, i0, i1, sums))
    out["rank_sums"] = list(sums)
    counts, S, T = fm.binned_cross_moments(K, [], [None] + X, Y)
    out["binned1"] = [counts.tolist(), packed(S, T).tolist()]
    return out


def check(fm, n, out):
    key, bounds, xs, ys = case(n)
    for name, b in (("binned64", bounds), ("binned1", [])):
        st, want_counts, _ = host_moments(fm, key, b, [None] + xs, ys)                # fmhip_binned_cross_moments_host
        exact_counts, want, tol = exact_and_bound(key, b, [None] + xs, ys)
        counts, sums = np.array(out[name][0]), np.array(out[name][1])
        assert st == 0 and (counts == want_counts).all() and (counts == exact_counts).all(), (n, name)
        err = np.abs(sums - want)
        print(f"n={n} {name}: max error / bound = {np.max(err / np.maximum(tol, 1e-300)):.3g}")
        assert (err <= tol).all(), (n, name)
    assert out["counts"] == np.searchsorted(np.sort(xs[0]).astype(np.float64), COUNT_BOUNDS, side="right").tolist(), n
    assert out["refused"] == fm._native.ERR_SIZE_MISMATCH, (n, out["refused"])
    ranks, (i0, i1) = ranks_of(n)
    for k in range(2):
        assert same_bits(out["select"][k], java_sorted(xs[k])[ranks]), (n, k)
        s = java_sorted(xs[k]).astype(np.float64)
        assert abs(out["rank_sums"][k] - math.fsum(s[i0:i1 + 1])) <= 1e-13 * np.abs(s).sum(), (n, k)
    S, T = np.array(out["xmom"][0]), np.array(out["xmom"][1])
    full = [np.ones(n)] + xs
    assert S[0, 0] == n
    for i in range(3):
        for j in range(3):
            assert abs(S[i, j] - exact(full[i], full[j])) <= bound(full[i], full[j]), (n, i, j)
        assert abs(T[i, 0] - exact(full[i], ys[0])) <= bound(full[i], ys[0]), (n, i)


@pytest.mark.parametrize("n", SIZES)
def test_on_one_engine(gpu, n):
    before = gpu.pool_stats().n_kernel_launches
    out = run_sequence(gpu, n)
    assert gpu.pool_stats().n_kernel_launches > before
    check(gpu, n, out)


_DEVICES = r'''
import importlib, json, sys
sys.path[:0] = [%(root)r, %(tests)r]
fm = importlib.import_module("finmath-lib-cuda-extensions_amd")
from test_gpu_side_pass_sequence import SIZES, run_sequence
fm.init_devices([0, 0])
out = {str(n): run_sequence(fm, n) for n in SIZES}
print("RESULT " + json.dumps(out))
fm.shutdown()
'''


def test_behind_a_device_list(gpu, tmp_path):
    """The same sequences behind a device list {0, 0}, in a process of its own as test_gpu_binned.py's: counts add, sums add in shard order."""
    script = tmp_path / "devices.py"
    script.write_text(_DEVICES % {"root": ROOT, "tests": os.path.join(ROOT, "tests")})
    r = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = json.loads([line for line in r.stdout.splitlines() if line.startswith("RESULT ")][-1][7:])
    for n in SIZES:
        check(gpu, n, out[str(n)])
