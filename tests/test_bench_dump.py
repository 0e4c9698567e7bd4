"""CPU tests (no GPU) of bench.py's --dump-outputs writer: whole arrays in float32 / float64 while the set fits the
budget, and past it the same seeded sample of every array's flattened positions, never more bytes than the budget."""
import glob
import os

import numpy as np
import torch

import bench


def _data_bytes(d):
    return sum(np.load(f).nbytes for f in glob.glob(os.path.join(d, "*.npy")))


def test_whole_arrays_keep_their_values(tmp_path):
    arrays = {"dist": torch.linspace(0, 1, 12).reshape(3, 4), "dist64": torch.arange(5, dtype=torch.float64) / 3,
              "idx": torch.arange(-6, 6, dtype=torch.int32).reshape(2, 6),
              "big_idx": torch.tensor([0, 2 ** 24 + 1, -(2 ** 40)], dtype=torch.int64)}
    info = bench.dump_outputs(str(tmp_path), arrays)
    for name, t in arrays.items():
        a = np.load(tmp_path / (name + ".npy"))
        assert a.shape == tuple(t.shape) and info[name] == {"shape": list(t.shape), "written": t.numel()}
        assert np.array_equal(a, t.numpy())      # integers exactly, in float32 or float64
    assert np.load(tmp_path / "dist.npy").dtype == np.float32 and np.load(tmp_path / "idx.npy").dtype == np.float32
    assert np.load(tmp_path / "dist64.npy").dtype == np.float64 and np.load(tmp_path / "big_idx.npy").dtype == np.float64


def test_over_budget_every_array_is_the_same_seeded_sample(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BYTES", 20000)
    n_a, n_b = 10000, 3000
    arrays = {"a": torch.arange(n_a, dtype=torch.float32), "b": torch.arange(n_b, dtype=torch.int32).reshape(100, 30)}
    info = bench.dump_outputs(str(tmp_path / "1"), arrays)
    bench.dump_outputs(str(tmp_path / "2"), arrays)
    assert _data_bytes(str(tmp_path / "1")) <= 20000
    for name, n in (("a", n_a), ("b", n_b)):
        pos = np.load(tmp_path / "1" / (name + ".npy"))     # the values are the flat positions sampled
        k = info[name]["written"]
        assert pos.dtype == np.float32 and pos.shape == (k,) and 0 < k < n
        assert np.array_equal(pos, np.load(tmp_path / "2" / (name + ".npy")))
        # one position in each of k equal strata of the flattened array
        edges = np.arange(k + 1) * n // k
        assert np.all(pos >= edges[:-1]) and np.all(pos < edges[1:])
    assert info["b"]["shape"] == [100, 30]
