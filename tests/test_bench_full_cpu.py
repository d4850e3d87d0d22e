"""bench.py without a GPU: which child processes the LMM half starts in a plain run and which only with --full, and that the
option is there and off by default."""
import importlib.util
import json
import os
import subprocess
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_bench():
    spec = importlib.util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


# every key bench.py reads from a line of lmm_hip / lmm_smile_hip / lmm_cpu / box_speed, in one answer
CHILD_LINE = {"seconds": 1.25, "iterations": 12, "evaluations": 621, "parameters": [0.1 * k for k in range(60)], "mean_deviation": 5e-7, "rms_deviation": 5e-5,
              "initial_rms": 1e-3, "kernel_launches": 2117, "path_ops": 1.5e13, "kernel_ms_total": 800.0, "achieved_GBps": 4400.0, "profiled_launches": 2117,
              "specialised_launches": 2100, "algorithmic_bytes": 3.5e12, "engine": {}, "seconds_simulation_per_evaluation": 9.0, "seconds_valuation_per_evaluation": 3.0}


def record_children(bench, monkeypatch, tmp_path):
    """bench.py's module with the native drivers 'built' and every child process replaced by its recorded command line."""
    driver = tmp_path / "driver"
    driver.write_text("")
    monkeypatch.setattr(bench, "LMM_HIP", str(driver))
    monkeypatch.setattr(bench, "LMM_CPU", str(tmp_path / "cpu_driver"))
    (tmp_path / "cpu_driver").write_text("")
    commands = []

    def fake_run(cmd, **kwargs):
        commands.append((list(cmd), {k: v for k, v in (kwargs.get("env") or {}).items() if k.startswith("FMHIP_")}))
        return types.SimpleNamespace(returncode=0, stdout=json.dumps(CHILD_LINE) + "\n", stderr="")

    monkeypatch.setattr(subprocess, "run", fake_run)
    monkeypatch.setattr(bench.time, "sleep", lambda seconds: None)
    for name in [k for k in os.environ if k.startswith("FMHIP_")]:
        monkeypatch.delenv(name)
    return commands


def bench_args(bench, monkeypatch, *argv):
    """main() as far as the LMM half goes (no GPU is touched before it): what it is called with."""
    seen = {}
    monkeypatch.setattr(bench, "lmm_leg", lambda args, *a, **k: seen.update(full=k.get("full")) or {"lm_iterations": 1, "value": 1.0, "workload": "w"})
    monkeypatch.setattr(sys, "argv", ["bench.py", "--workload", "lmm", *argv])
    bench.main()
    return seen


def test_a_plain_run_starts_the_calibration_once_and_nothing_else(monkeypatch, tmp_path):
    bench = load_bench()
    commands = record_children(bench, monkeypatch, tmp_path)
    args = types.SimpleNamespace(paths=1_000_000, lmm_iterations=12, dump_outputs=str(tmp_path / "dump"))
    lmm = bench.lmm_leg(args, 1, 0, None)
    assert commands == [([bench.LMM_HIP, "--paths", "1000000", "--mode", "calibrate", "--max-iterations", "12"], {})]
    assert lmm["metric"] == "LMM calib wall-time, 1M paths" and lmm["value"] == 1.25 and lmm["unit"] == "s" and lmm["higher_is_better"] is False
    assert lmm["lm_iterations"] == 12 and lmm["objective_evaluations"] == 621 and lmm["accepted"] is True and lmm["paths"] == 1_000_000
    for key in ("roofline", "cpu_baseline", "box_speed", "smile_calibration", "finmath_like", "finmath_like_threads", "finmath_like_gc", "device_list_rehearsal"):
        assert key not in lmm, key
    # the dump of the LMM half comes from that one calibration
    assert os.listdir(tmp_path / "dump") == ["lmm_parameters.npy"]
    assert (np.load(tmp_path / "dump" / "lmm_parameters.npy") == np.asarray(CHILD_LINE["parameters"])).all()


def test_full_adds_the_other_runs_behind_the_same_first_one(monkeypatch, tmp_path):
    bench = load_bench()
    commands = record_children(bench, monkeypatch, tmp_path)
    args = types.SimpleNamespace(paths=1_000_000, lmm_iterations=12, dump_outputs=None)
    plain = bench.lmm_leg(args, 1, 0, None)
    first = list(commands)
    del commands[:]
    lmm = bench.lmm_leg(args, 1, 0, None, full=True)
    calibration = [c for c in commands if c[0][0] == bench.LMM_HIP]
    assert calibration[0] == first[0] and len(first) == 1                       # the figure of the metric is the same run in both
    assert [bench.LMM_HIP, "--paths", "1000000", "--mode", "calibrate", "--max-iterations", "12", "--profile"] in [c[0] for c in commands]
    assert any(c[0][0].endswith("box_speed") for c in commands) and any(c[0][0].endswith("lmm_smile_hip") for c in commands)
    assert any("--finmath-like" in c[0] for c in commands) and any("--release-lag" in c[0] for c in commands) and any("--devices" in c[0] for c in commands)
    assert any(c[1].get("FMHIP_MERGE_CHAINS") == "0" for c in commands) and any(c[0][0] == bench.LMM_CPU for c in commands)
    for key, value in plain.items():                                             # every plain key with its plain value, and the rest beside them
        assert lmm[key] == value or key == "process_wall_s", key
    for key in ("roofline", "cpu_baseline", "box_speed", "smile_calibration", "finmath_like", "finmath_like_threads", "finmath_like_gc", "device_list_rehearsal",
                "seconds_second_run_warm_code_object_cache_profiled"):
        assert key in lmm and "error" not in (lmm[key] if isinstance(lmm[key], dict) else {}), key
    assert lmm["roofline"]["frac"] == 4400.0 / 8000.0 and "error" not in lmm["roofline"]["one_launch_per_shape"]
    assert lmm["cpu_baseline"]["value"] == 12.0 * 621
    assert bench.lmm_leg(args, 1, 0, None, cpu_base=False, full=True).get("cpu_baseline") is None


def test_full_is_an_option_and_off_by_default(monkeypatch, capsys):
    bench = load_bench()
    assert bench_args(bench, monkeypatch, "--gpus", "1", "--steps", "20", "--warmup", "5")["full"] is False
    assert bench_args(bench, monkeypatch, "--gpus", "1", "--steps", "20", "--warmup", "5", "--full")["full"] is True
    assert len([ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]) == 2          # ONE line per run
