"""bench.py's contract, checked on the GPU box: ONE JSON line with the keys the driver reads; with --full the roofline and
cpu_baseline objects and the in-run parity of the timed kernel's expectations against the CPU twin (stream half only; short);
without it a lean run: both halves of the metric, the same dump, and little time outside the steps."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_stream_half_of_the_full_bench_line(tmp_path):
    dump = tmp_path / "outputs"
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--workload", "stream", "--gpus", "1", "--steps", "6", "--warmup", "2",
                          "--sustained-seconds", "0.3", "--dump-outputs", str(dump)], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1                                               # ONE JSON line
    d = json.loads(lines[0])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config",
                "roofline", "cpu_baseline"):
        assert key in d, key
    assert d["n_gpus"] == 1 and d["steps"] == 6 and d["warmup"] == 2 and d["higher_is_better"] is True and d["vs_baseline"] is None and d["full"] is True
    assert d["unit"] == "path-ops/s" and d["dtype"] == "f32" and d["scaling"] == "weak" and "workload" in d["config"]
    r = d["roofline"]
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and r["peak"] == 8000.0 and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-12
    assert 0.3 < r["frac"] < 0.78                                        # below the streaming ceiling of this data, above a broken kernel
    assert r["tier"] == ("interpreter" if os.environ.get("FMHIP_JIT") == "off" else "specialised")
    # value = path-ops of the whole job / step time; consistent with ms_per_step
    assert abs(d["value"] - 12 * 1_000_000 * 64 / (d["ms_per_step"] * 1e-3)) / d["value"] < 1e-9
    c = d["cpu_baseline"]
    assert c["kind"] == "port" and c["cores"] == 1 and c["value"] > 1e8 and "sample" in c
    assert d["parity_triple0"]["ok"] and d["parity_triple0"]["min_max_identical"]
    assert d["value"] > 1000 * c["value"]
    # --dump-outputs: the output vectors of the last timed step (the same sample of paths for every triple) and its moments
    assert sorted(os.listdir(dump)) == ["moments.npy", "w.npy"] and sum(os.path.getsize(dump / f) for f in os.listdir(dump)) <= 64 << 20
    w, m = np.load(dump / "w.npy"), np.load(dump / "moments.npy")
    assert w.dtype == np.float32 and w.shape[0] == 64 and w.shape[1] >= 100_000 and m.dtype == np.float64 and m.shape == (64, 4)
    g = d["parity_triple0"]["gpu"]
    assert m[0, 0] / 1_000_000 == g["average"] and m[0, 2] == g["min"] and m[0, 3] == g["max"]
    assert np.isfinite(w).all() and (w.min(axis=1) >= m[:, 2]).all() and (w.max(axis=1) <= m[:, 3]).all()


def test_a_plain_run_is_lean(tmp_path):
    """`bench.py --gpus 1 --steps K --warmup W` as it is typed for the headline: the contract keys, both halves of the metric, the whole
    dump - and nothing that takes a run of its own, so that little of the process's life is spent outside its steps."""
    dump = tmp_path / "outputs"
    steps, warmup = 20, 5
    t0 = time.perf_counter()
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
                          "--dump-outputs", str(dump)], capture_output=True, text=True, timeout=600, cwd=ROOT)
    wall = time.perf_counter() - t0
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["metric"] == "Monte-Carlo path-ops/sec (fused RandomVariable stream)" and d["unit"] == "path-ops/s" and d["higher_is_better"] is True
    assert d["dtype"] == "f32" and d["n_gpus"] == 1 and d["steps"] == steps and d["warmup"] == warmup and d["full"] is False
    assert abs(d["value"] - 12 * 1_000_000 * 64 / (d["ms_per_step"] * 1e-3)) / d["value"] < 1e-9
    r = d["roofline"]
    assert r["tier"] == ("interpreter" if os.environ.get("FMHIP_JIT") == "off" else "specialised")
    assert 0.3 < r["frac"] < 0.78 and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-12           # the timed region's own device time
    assert d["sustained"]["launches"] >= 200                                                         # the steady state in front of the timed region
    # what takes a run or a pass of its own is behind --full
    for key in ("cpu_baseline", "parity_triple0", "brownian"):
        assert key not in d, key
    assert d["fast_math"] is None and d["interpreter_tier"] is None and r["avg_kernel_us_one_event_pair_per_launch"] is None
    lmm = d["lmm"]
    assert lmm["unit"] == "s" and lmm["higher_is_better"] is False and lmm["paths"] == 1_000_000 and lmm["accepted"] is True and lmm["value"] > 0
    for key in ("roofline", "cpu_baseline", "box_speed", "smile_calibration", "finmath_like", "finmath_like_threads", "finmath_like_gc", "device_list_rehearsal"):
        assert key not in lmm, key
    # the dump is the whole dump
    assert sorted(os.listdir(dump)) == ["lmm_parameters.npy", "moments.npy", "w.npy"] and sum(os.path.getsize(dump / f) for f in os.listdir(dump)) <= 64 << 20
    w, m, p = np.load(dump / "w.npy"), np.load(dump / "moments.npy"), np.load(dump / "lmm_parameters.npy")
    assert w.dtype == np.float32 and w.shape[0] == 64 and w.shape[1] >= 100_000 and m.dtype == np.float64 and m.shape == (64, 4)
    assert np.isfinite(w).all() and (w.min(axis=1) >= m[:, 2]).all() and (w.max(axis=1) <= m[:, 3]).all()
    assert p.dtype == np.float64 and p.ndim == 1 and p.size >= 50 and np.isfinite(p).all()
    # the process from start to exit, less its W + K steps
    assert wall - (steps + warmup) * d["ms_per_step"] * 1e-3 <= 30.0, wall
