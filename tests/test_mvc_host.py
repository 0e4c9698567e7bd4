"""CPU tests (no GPU) of mean_value_coordinates_3D: the drop-in name imports, the C ABI declares and exports the
pp_mvc3d_* entry points, and the in-tree torch composition (the path of CPU tensors and of dtypes the kernels do not
serve) matches the reference's own fp64 results recorded in tests/golden/mvc_*.npz (tools/gen_mvc_golden.py)."""
import ctypes
import glob
import os
import re

import numpy as np
import pytest
import torch

from pytorch_points_amd import _build, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "mvc_*.npz")))
SYMBOLS = ["pp_mvc3d_workspace_bytes", "pp_mvc3d_forward_f32", "pp_mvc3d_forward_f64", "pp_mvc3d_backward_f32",
           "pp_mvc3d_backward_f64"]
VERTEX = 2


def load(path):
    z = dict(np.load(path))
    faces = torch.from_numpy(z["faces"])
    if z["expand"]:
        faces = faces[:1].expand(z["query"].shape[0], -1, -1)
    return z, faces


def test_drop_in_name_imports():
    import pytorch_points_amd
    pytorch_points_amd.install_as_pytorch_points()
    from pytorch_points.network.geo_operations import mean_value_coordinates_3D
    assert callable(mean_value_coordinates_3D)


def test_header_declares_and_library_exports_mvc():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pp_hip.h")).read(), flags=re.S)
    _build.build()
    handle = ctypes.CDLL(_build.LIB)
    for s in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, text), s
        assert s in _lib.SIGNATURES, s
        assert hasattr(handle, s), s


def test_workspace_query_and_argument_checks_are_host_only():
    L = _lib.lib()
    assert L.pp_mvc3d_workspace_bytes(8, 16384, 162, 4) == 8 * 256 * 162 * 3 * 4
    assert L.pp_mvc3d_workspace_bytes(2, 65, 10, 8) == 2 * 2 * 10 * 3 * 8
    assert L.pp_mvc3d_workspace_bytes(0, 10, 10, 4) == 0
    assert L.pp_mvc3d_workspace_bytes(1, 10, 10, 2) == 0
    assert L.pp_mvc3d_forward_f32(None, None, None, 0, None, None, None, None, -1, 4, 4, 4, None) != 0
    assert L.pp_mvc3d_forward_f32(None, None, None, 0, None, None, None, None, 2, 0, 4, 4, None) == 0
    assert L.pp_mvc3d_forward_f64(None, None, None, -1, None, None, None, None, 1, 1, 4, 4, None) != 0
    assert L.pp_mvc3d_backward_f32(None, None, None, 0, None, None, None, None, None, None, None, 1, 4, 4, 4, None, 0,
                                   None) != 0
    # a P whose tile count would overflow an int: refused before any arithmetic on it
    big = 2 ** 31 - 1
    assert L.pp_mvc3d_workspace_bytes(1, big, 10, 4) == 0
    for fwd in (L.pp_mvc3d_forward_f32, L.pp_mvc3d_forward_f64):
        assert fwd(None, None, None, 0, None, None, None, None, 1, big, 4, 4, None) != 0
    for bwd in (L.pp_mvc3d_backward_f32, L.pp_mvc3d_backward_f64):
        assert bwd(None, None, None, 0, None, None, None, None, None, None, None, 1, big, 4, 4, None, 0, None) != 0


def row_error(got, ref, shape):
    """max |got - ref| per query row, NaN where both are NaN counted as equal"""
    err = np.abs(got - ref)
    err[np.isnan(got) & np.isnan(ref)] = 0.0
    return np.nan_to_num(err, nan=np.inf).reshape(shape + (-1,)).max(-1)


def check_rows(wj, wi, z):
    """wj / wi against the reference's fp64 rows to 1e-12; returns the rows that agree.  The composition is the
    reference's chain of torch operations, but LAPACK's LU behind torch.linalg.det rounds differently on different
    CPUs (MKL picks its code path by CPU), and a row the reference decides by rounding (``stable`` False: it moves
    under a 1e-9 translation of the scene) can take the other branch there: such a row is held only to be finite
    wherever the reference's is.  Every stable row agrees."""
    st = z["stable"]
    same = (row_error(wj, z["wj64"], st.shape) <= 1e-12) & (row_error(wi, z["wi64"], st.shape) <= 1e-12)
    assert same[st].all(), np.argwhere(st & ~same)
    assert np.isfinite(wj[~same][np.isfinite(z["wj64"][~same])]).all()
    assert np.isfinite(wi[~same][np.isfinite(z["wi64"][~same])]).all()
    return same


@pytest.mark.parametrize("path", GOLDEN, ids=lambda p: os.path.basename(p)[4:-4])
def test_composition_matches_reference_fp64(path):
    from pytorch_points_amd import mvc
    z, faces = load(path)
    q = torch.tensor(z["query"], dtype=torch.float64, requires_grad=True)
    v = torch.tensor(z["vertices"], dtype=torch.float64, requires_grad=True)
    wj, wi = mvc.composition(q, v, faces, verbose=True)
    same = check_rows(wj.detach().numpy(), wi.detach().numpy(), z)
    gq, gv = torch.autograd.grad((wj * torch.from_numpy(z["G"])).sum(), (q, v))
    gq, gv = gq.numpy(), gv.numpy()
    assert np.isfinite(gq).all() and np.isfinite(gv).all()
    # the gradients of the rows that agree: the query gradient of such a row, the vertex gradient of a batch element
    # whose rows all agree (on the CPU the fixtures were recorded on: every row, every batch element)
    whole = same.all(1)
    for got, ref in ((gq[same], z["gq64"][same]), (gv[whole], z["gv64"][whole])):
        fin = np.isfinite(ref)
        np.testing.assert_allclose(got[fin], ref[fin], rtol=1e-9, atol=1e-9 * np.abs(ref[fin]).max(initial=1.0))
    assert (gq[z["kind"] == VERTEX] == 0).all()


def test_golden_fixtures_cover_the_issue():
    names = {os.path.basename(p)[4:-4] for p in GOLDEN}
    assert {"octahedron", "ico1", "ico2", "star", "cube", "b2_two_cages", "b2_expanded"} <= names
    total = sum(os.path.getsize(p) for p in GOLDEN)
    assert total < 1 << 20
    kinds = np.concatenate([np.load(p)["kind"].ravel() for p in GOLDEN])
    assert set(range(7)) <= set(kinds.tolist())
    # the reference's gradient is NaN somewhere (on vertices, on edges): the composition's is finite there
    assert any(np.isnan(np.load(p)["gq64"]).any() for p in GOLDEN)


def test_composition_fp32_and_other_dtypes_run():
    from pytorch_points_amd.network.geo_operations import mean_value_coordinates_3D
    z, faces = load(GOLDEN[0])
    for dt, tol in ((torch.float32, 1e-4), (torch.bfloat16, None)):
        q = torch.from_numpy(z["query"]).to(dt)
        v = torch.from_numpy(z["vertices"]).to(dt)
        wj = mean_value_coordinates_3D(q, v, faces)
        assert wj.dtype == dt and wj.shape == z["wj64"].shape
        if tol:
            stable = z["stable"]
            np.testing.assert_allclose(wj.numpy()[stable], z["wj32"][stable], rtol=0, atol=tol)
    # int32 faces are accepted too, and give the int64 faces' result
    from pytorch_points_amd import mvc
    q, v = torch.from_numpy(z["query"]).double(), torch.from_numpy(z["vertices"]).double()
    wj = mean_value_coordinates_3D(q, v, faces.int())
    wj64, wi64 = mvc.composition(q, v, faces, verbose=True)
    assert torch.equal(wj, wj64)
    check_rows(wj.numpy(), wi64.numpy(), z)


def test_composition_edge_sizes_and_bad_indices():
    from pytorch_points_amd import mvc
    v = torch.randn(2, 5, 3, dtype=torch.float64)
    f = torch.tensor([[[0, 1, 2], [2, 3, 4]], [[0, 1, 2], [2, 3, 5]]])
    q = torch.randn(2, 4, 3, dtype=torch.float64)
    wj, wi = mvc.composition(q, v, f, verbose=True)
    assert torch.isnan(wj[1]).all() and torch.isnan(wi[1]).all()
    assert not torch.isnan(wj[0]).any()
    assert mvc.composition(q[:, :0], v, f).shape == (2, 0, 5)
    wj = mvc.composition(q, v, f[:, :0])
    assert wj.shape == (2, 4, 5) and (wj == 0).all()


def test_shape_and_dtype_errors():
    from pytorch_points_amd.network.geo_operations import mean_value_coordinates_3D as mvc3d
    q = torch.zeros(2, 4, 3)
    v = torch.zeros(2, 6, 3)
    f = torch.zeros(2, 8, 3, dtype=torch.long)
    with pytest.raises(RuntimeError, match="query must have shape"):
        mvc3d(torch.zeros(2, 4, 2), v, f)
    with pytest.raises(RuntimeError, match="vertices must have shape"):
        mvc3d(q, torch.zeros(2, 6), f)
    with pytest.raises(RuntimeError, match="faces must have shape"):
        mvc3d(q, v, torch.zeros(2, 8, 4, dtype=torch.long))
    with pytest.raises(RuntimeError, match="same batch size"):
        mvc3d(q, torch.zeros(3, 6, 3), f)
    with pytest.raises(RuntimeError, match="one dtype"):
        mvc3d(q, v.double(), f)
    with pytest.raises(RuntimeError, match="floating"):
        mvc3d(q.long(), v.long(), f)
    with pytest.raises(RuntimeError, match="integer"):
        mvc3d(q, v, f.float())
