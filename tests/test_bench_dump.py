"""CPU: bench.py --dump-outputs (bench.dump_outputs): the valid region of the iteration buffer, float32 while every count is exact
in it and float64 above 2^24; a frame over the size limit as a seeded sample of its pixels beside their indices -- the same
pixels on every run."""
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench_module():
    spec = importlib.util.spec_from_file_location("fs_bench_dump", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)  # top level of bench.py imports the standard library only
    return m


def test_whole_frame(tmp_path):
    b = _bench_module()
    frame = np.arange(40 * 72, dtype=np.uint32).reshape(40, 72)  # padded rows and rounded width, as the host buffers are
    b.dump_outputs(str(tmp_path / "f32"), frame, 37, 70, 4718592)
    it = np.load(tmp_path / "f32" / "iterations.npy")
    assert it.dtype == np.float32 and it.shape == (37, 70) and np.array_equal(it, frame[:37, :70])
    assert not (tmp_path / "f32" / "pixel_index.npy").exists()
    b.dump_outputs(str(tmp_path / "f64"), frame, 37, 70, 1 << 24)
    it = np.load(tmp_path / "f64" / "iterations.npy")
    assert it.dtype == np.float64 and np.array_equal(it, frame[:37, :70])


def test_frame_over_the_limit_is_a_fixed_sample(tmp_path, monkeypatch):
    b = _bench_module()
    monkeypatch.setattr(b, "DUMP_LIMIT_BYTES", 1000)
    monkeypatch.setattr(b, "DUMP_SAMPLE_DRAWS", 500)
    frame = (np.arange(64 * 128, dtype=np.uint64) * 7919 % 100003).astype(np.uint32).reshape(64, 128)
    for d in ("a", "b"):
        b.dump_outputs(str(tmp_path / d), frame, 60, 100, 1 << 31)
    it, idx = np.load(tmp_path / "a" / "iterations.npy"), np.load(tmp_path / "a" / "pixel_index.npy")
    assert it.dtype == idx.dtype == np.float64 and it.shape == idx.shape and 0 < idx.size <= 500
    assert np.all(np.diff(idx) > 0) and idx[0] >= 0 and idx[-1] < 60 * 100
    k = idx.astype(np.int64)
    assert np.array_equal(it, frame[k // 100, k % 100])
    assert np.array_equal(np.load(tmp_path / "b" / "iterations.npy"), it)
    assert np.array_equal(np.load(tmp_path / "b" / "pixel_index.npy"), idx)
