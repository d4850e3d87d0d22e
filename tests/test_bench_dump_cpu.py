"""bench.py --dump-outputs without a GPU: which paths of the output vectors are written, and how many bytes."""
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class HostVector:
    def __init__(self, values):
        self.values, self.n = values, values.size

    def to_float32(self):
        return self.values


def load_bench():
    spec = importlib.util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def test_a_dump_is_a_fixed_sample_within_the_budget(tmp_path):
    bench = load_bench()
    n, batch = 1_000_000, 64
    paths = np.arange(n, dtype=np.float32)                  # exact in fp32: a dumped value names the path it came from
    rows = [[HostVector(paths)] for _ in range(batch)]
    moments = np.arange(batch * 4, dtype=np.float64).reshape(batch, 4)
    for d in ("first", "second"):
        bench.dump_stream_outputs(str(tmp_path / d), rows, moments)
    first = {f: np.load(tmp_path / "first" / f) for f in sorted(os.listdir(tmp_path / "first"))}
    assert list(first) == ["moments.npy", "w.npy"]
    assert sum(os.path.getsize(tmp_path / "first" / f) for f in first) <= 64 << 20
    w = first["w.npy"]
    assert w.dtype == np.float32 and w.shape == (batch, bench.DUMP_BUDGET_BYTES // (4 * batch))
    assert (np.diff(w[0]) > 0).all() and (w == w[0]).all()                       # distinct paths, the same ones for every triple
    assert first["moments.npy"].dtype == np.float64 and (first["moments.npy"] == moments).all()
    for f, a in first.items():                                                    # and the same ones in every run
        assert a.tobytes() == np.load(tmp_path / "second" / f).tobytes()
    small = [[HostVector(paths[:1000] + b)] for b in range(batch)]                # an output that fits is written whole
    bench.dump_stream_outputs(str(tmp_path / "small"), small, moments)
    assert (np.load(tmp_path / "small" / "w.npy") == np.stack([r[0].values for r in small])).all()
