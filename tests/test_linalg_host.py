"""CPU tests (no GPU) of the batched SVD: the drop-in names import, the C ABI declares and exports pp_batch_svd_f32,
and batch_svd_backward equals torch's own SVD gradient in fp64."""
import ctypes
import os
import re

import pytest
import torch

from pytorch_points_amd import _build, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_drop_in_names_import():
    import pytorch_points_amd
    pytorch_points_amd.install_as_pytorch_points()
    from pytorch_points._ext import linalg
    from pytorch_points.network.operations import batch_svd, BatchSVDFunction  # noqa: F401
    from pytorch_points.network.geo_operations import batch_normals  # noqa: F401
    assert callable(linalg.batch_svd_forward) and callable(linalg.batch_svd_backward)
    assert callable(batch_svd) and callable(batch_normals)


def test_header_declares_and_library_exports_batch_svd():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pp_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+pp_batch_svd_f32\s*\(", text)
    assert "pp_batch_svd_f32" in _lib.SIGNATURES
    _build.build()
    assert hasattr(ctypes.CDLL(_build.LIB), "pp_batch_svd_f32")


def test_batch_svd_rejects_bad_sizes_on_the_host():
    L = _lib.lib()
    args = (None, None, None, None, None)
    assert L.pp_batch_svd_f32(*args, 0, 3, 3, 0, 1, 1e-7, 100, None) == 0            # nothing to do
    for b, m, n, sweeps, tol in [(1, 33, 3, 100, 1e-7), (1, 3, 0, 100, 1e-7), (-1, 3, 3, 100, 1e-7),
                                 (1, 3, 3, 0, 1e-7), (1, 3, 3, 100, -1.0), (1, 3, 3, 100, 1e-7)]:
        assert L.pp_batch_svd_f32(*args, b, m, n, 0, 1, tol, sweeps, None) != 0     # (last: null pointers)


def test_forward_preconditions_raise_before_any_launch():
    from pytorch_points_amd._ext import linalg
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        linalg.batch_svd_forward(torch.zeros(2, 3, 3), True)


SHAPES = [(5, 5), (7, 3), (3, 7), (20, 3), (32, 32)]
COMBOS = [(True, False, False), (False, True, False), (False, False, True), (True, True, True)]


@pytest.mark.parametrize("m,n", SHAPES)
@pytest.mark.parametrize("use", COMBOS, ids=["gU", "gS", "gV", "all"])
def test_backward_equals_torch_autograd_fp64(m, n, use):
    from pytorch_points_amd._ext import linalg
    gen = torch.Generator().manual_seed(m * 100 + n)
    a = torch.randn(6, m, n, dtype=torch.float64, generator=gen, requires_grad=True)
    u, s, vh = torch.linalg.svd(a, full_matrices=False)
    v = vh.transpose(-2, -1)
    grads = [torch.randn(t.shape, dtype=torch.float64, generator=gen) if on else None
             for t, on in zip((u, s, v), use)]
    outs = [t for t, g in zip((u, s, v), grads) if g is not None]
    (expected,) = torch.autograd.grad(outs, [a], [g for g in grads if g is not None])
    got = linalg.batch_svd_backward(grads, a.detach(), True, True, u.detach(), s.detach(), v.detach())
    assert got.shape == a.shape and got.dtype == torch.float64
    assert (got - expected).abs().max().item() <= 1e-10


def test_backward_with_full_factors_uses_the_first_k_columns():
    from pytorch_points_amd._ext import linalg
    gen = torch.Generator().manual_seed(3)
    a = torch.randn(4, 9, 4, dtype=torch.float64, generator=gen)
    u, s, vh = torch.linalg.svd(a, full_matrices=True)
    gs = torch.randn(s.shape, dtype=torch.float64, generator=gen)
    thin = linalg.batch_svd_backward([None, gs, None], a, True, True, u[..., :4], s, vh.transpose(-2, -1))
    full = linalg.batch_svd_backward([None, gs, None], a, True, True, u, s, vh.transpose(-2, -1))
    assert torch.equal(thin, full)
    zero = linalg.batch_svd_backward([None, None, None], a, True, True, u, s, vh.transpose(-2, -1))
    assert torch.equal(zero, torch.zeros_like(a))
