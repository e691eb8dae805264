"""bench.py's host-side pieces that need no GPU: the --dump-outputs writer and the option checks that run before anything touches HIP."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _records(n, seed=3):
    rs = np.random.RandomState(seed)
    return rs.uniform(0, 416, (n, 6)).astype(np.float32)


def test_dump_outputs_writes_float_arrays(tmp_path):
    import bench
    rec, off = _records(50), np.array([0, 20, 20, 50], dtype=np.int32)
    bench.dump_outputs(str(tmp_path / "d"), rec, off)
    assert sorted(os.listdir(tmp_path / "d")) == ["detections.npy", "offsets.npy"]
    got, goff = np.load(tmp_path / "d" / "detections.npy"), np.load(tmp_path / "d" / "offsets.npy")
    assert got.dtype == np.float32 and np.array_equal(got, rec)
    assert goff.dtype == np.float64 and np.array_equal(goff, off)


def test_dump_outputs_samples_a_fixed_subset_above_the_limit(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, "DUMP_LIMIT", 4096)
    rec, off = _records(1000), np.array([0, 400, 1000], dtype=np.int32)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), rec, off)
    total = sum(os.path.getsize(tmp_path / "a" / f) - 128 for f in os.listdir(tmp_path / "a"))      # minus the .npy headers
    assert total <= 4096
    rows = np.load(tmp_path / "a" / "detections_rows.npy")
    got = np.load(tmp_path / "a" / "detections.npy")
    assert rows.dtype == np.float64 and len(rows) == len(got) > 0 and np.all(np.diff(rows) > 0)
    assert np.array_equal(got, rec[rows.astype(np.int64)])
    for f in os.listdir(tmp_path / "a"):                                                         # seeded: the same rows every time
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f))


def test_per_kernel_options_need_full():
    for opt in (["--layers"], ["--dump-layers", "x.json"]):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + opt, cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert r.returncode == 2 and "--full" in r.stderr, r.stderr[-2000:]
