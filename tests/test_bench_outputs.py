"""bench.py --dump-outputs without a GPU: the files it writes, their dtypes, and the fixed sample it takes of outputs past its size limit."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_dump_outputs_writes_each_array_as_computed(tmp_path):
    import bench
    W = np.asfortranarray(np.arange(12, dtype=np.float32).reshape(4, 3))
    bench.dump_outputs(str(tmp_path / "out"), {"W": W, "frobenius": np.array([1.5])})
    got = np.load(tmp_path / "out" / "W.npy")
    assert got.dtype == np.float32 and np.array_equal(got, W)
    f = np.load(tmp_path / "out" / "frobenius.npy")
    assert f.dtype == np.float64 and f.tolist() == [1.5]
    with pytest.raises(TypeError):
        bench.dump_outputs(str(tmp_path / "bad"), {"idx": np.arange(4)})


def test_dump_outputs_past_the_limit_keeps_the_same_seeded_sample(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 2 * 4096 + 8000)
    rng = np.random.default_rng(1)
    arrays = {"X": np.asfortranarray(rng.random((100, 50))), "Y": rng.random((50, 40)).astype(np.float32)}
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), arrays)
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total <= bench.DUMP_LIMIT_BYTES
    for name, a in arrays.items():
        x, y = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")
        assert x.dtype == a.dtype and 0 < x.size < a.size and np.array_equal(x, y)
        assert np.isin(x, a).all()
