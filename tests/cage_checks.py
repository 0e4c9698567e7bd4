"""Checks that the cage-coordinate GPU tests share (test_gpu_mvc.py, test_gpu_green.py, test_gpu_mvc2d.py)."""
import numpy as np


def rel_close(got, ref, rtol):
    scale = max(1.0, float(np.abs(ref).max(initial=0.0)))
    err = np.abs(got - ref).max(initial=0.0)
    assert err <= rtol * scale, (err, scale)


def same_bits(x, y):
    it = {4: np.int32, 8: np.int64}[x.dtype.itemsize]
    return x.shape == y.shape and np.array_equal(np.ascontiguousarray(x).view(it), np.ascontiguousarray(y).view(it))
