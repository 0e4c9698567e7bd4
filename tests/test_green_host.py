"""CPU tests (no GPU) of green_coordinates_3D: the drop-in names import, the C ABI declares and exports the pp_gc3d_*
entry points, and the in-tree torch composition (the path of CPU tensors and of dtypes the kernels do not serve)
matches the reference's own fp64 results recorded in tests/golden/gc_*.npz (tools/gen_gc_golden.py)."""
import ctypes
import glob
import os
import re

import numpy as np
import pytest
import torch

from pytorch_points_amd import _build, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "gc_*.npz")))
SYMBOLS = ["pp_gc3d_workspace_bytes", "pp_gc3d_forward_f32", "pp_gc3d_forward_f64", "pp_gc3d_backward_f32",
           "pp_gc3d_backward_f64"]
INTERIOR = 0


def load(path):
    z = dict(np.load(path))
    faces = torch.from_numpy(z["faces"])
    if z["expand"]:
        faces = faces[:1].expand(z["query"].shape[0], -1, -1)
    return z, faces


def test_drop_in_names_import():
    import pytorch_points_amd
    pytorch_points_amd.install_as_pytorch_points()
    from pytorch_points.network.geo_operations import compute_face_normals_and_areas, green_coordinates_3D
    assert callable(green_coordinates_3D) and callable(compute_face_normals_and_areas)


def test_header_declares_and_library_exports_gc():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pp_hip.h")).read(), flags=re.S)
    _build.build()
    handle = ctypes.CDLL(_build.LIB)
    for s in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, text), s
        assert s in _lib.SIGNATURES, s
        assert hasattr(handle, s), s


def test_workspace_query_and_argument_checks_are_host_only():
    L = _lib.lib()
    assert L.pp_gc3d_workspace_bytes(8, 16384, 320, 4) == 8 * 256 * 320 * 3 * 4
    assert L.pp_gc3d_workspace_bytes(2, 65, 10, 8) == 2 * 2 * 10 * 3 * 8
    assert L.pp_gc3d_workspace_bytes(0, 10, 10, 4) == 0
    assert L.pp_gc3d_workspace_bytes(1, 10, 10, 2) == 0
    assert L.pp_gc3d_forward_f32(None, None, None, 0, None, None, None, None, None, -1, 4, 4, 4, None) != 0
    assert L.pp_gc3d_forward_f32(None, None, None, 0, None, None, None, None, None, 2, 0, 4, 4, None) == 0
    assert L.pp_gc3d_forward_f64(None, None, None, -1, None, None, None, None, None, 1, 1, 4, 4, None) != 0
    assert L.pp_gc3d_backward_f32(None, None, None, 0, None, None, None, None, None, None, None, None, 1, 4, 4, 4,
                                  None, 0, None) != 0
    # a P whose tile count would overflow an int: refused before any arithmetic on it
    big = 2 ** 31 - 1
    assert L.pp_gc3d_workspace_bytes(1, big, 10, 4) == 0
    for fwd in (L.pp_gc3d_forward_f32, L.pp_gc3d_forward_f64):
        assert fwd(None, None, None, 0, None, None, None, None, None, 1, big, 4, 4, None) != 0
    for bwd in (L.pp_gc3d_backward_f32, L.pp_gc3d_backward_f64):
        assert bwd(None, None, None, 0, *[None] * 8, 1, big, 4, 4, None, 0, None) != 0


def row_error(got, ref, shape):
    err = np.abs(got - ref)
    err[np.isnan(got) & np.isnan(ref)] = 0.0
    return np.nan_to_num(err, nan=np.inf).reshape(shape + (-1,)).max(-1, initial=0.0)


@pytest.mark.parametrize("path", GOLDEN, ids=lambda p: os.path.basename(p)[3:-4])
def test_composition_matches_reference_fp64(path):
    from pytorch_points_amd import green
    z, faces = load(path)
    st = z["stable"]
    q = torch.tensor(z["query"], dtype=torch.float64, requires_grad=True)
    v = torch.tensor(z["vertices"], dtype=torch.float64, requires_grad=True)
    gcv, gcf, ext = green.composition(q, v, faces)
    assert ext.dtype == torch.bool and ext.shape == z["ext64"].shape
    np.testing.assert_array_equal(ext.numpy(), z["ext64"])
    assert (row_error(gcv.detach().numpy(), z["gcv64"], st.shape)[st] <= 1e-10).all()
    assert (row_error(gcf.detach().numpy(), z["gcf64"], st.shape)[st] <= 1e-10).all()
    Gv, Gf = torch.from_numpy(z["Gv"]).double(), torch.from_numpy(z["Gf"]).double()
    gq, gv = torch.autograd.grad((gcv * Gv).sum() + (gcf * Gf).sum(), (q, v))
    gq = gq.numpy()
    assert np.isfinite(gq).all() and np.isfinite(gv.numpy()).all()
    fin = np.isfinite(z["gq64"]) & st[..., None]
    np.testing.assert_allclose(gq[fin], z["gq64"][fin], rtol=1e-9, atol=1e-9 * np.abs(z["gq64"][fin]).max(initial=1))
    # the normals passed in: their own gradient
    n = torch.tensor(z["normals"], requires_grad=True)
    q2 = q.detach().clone().requires_grad_(True)
    gcv, gcf, _ = green.composition(q2, v.detach(), faces, face_normals=n)
    gq2, gn = torch.autograd.grad((gcv * Gv).sum() + (gcf * Gf).sum(), (q2, n))
    fin = np.isfinite(z["gqn64"]) & st[..., None]
    np.testing.assert_allclose(gq2.numpy()[fin], z["gqn64"][fin], rtol=1e-9,
                               atol=1e-9 * np.abs(z["gqn64"][fin]).max(initial=1))
    if np.isfinite(z["gn64"]).all():
        np.testing.assert_allclose(gn.numpy(), z["gn64"], rtol=1e-9, atol=1e-9 * np.abs(z["gn64"]).max())


def test_golden_fixtures_cover_the_issue():
    names = {os.path.basename(p)[3:-4] for p in GOLDEN}
    assert {"octahedron", "ico1", "ico2", "star", "cube", "b2_two_cages", "b2_expanded"} <= names
    assert all(os.path.getsize(p) < 400 << 10 for p in GOLDEN)
    kinds = np.concatenate([np.load(p)["kind"].ravel() for p in GOLDEN])
    assert set(range(7)) <= set(kinds.tolist())
    assert any(np.isnan(np.load(p)["gq64"]).any() for p in GOLDEN)
    for p in GOLDEN:                       # interior queries: stable, inside, rows summing to S / (S + 1e-10)
        z = np.load(p)
        inner = z["kind"] == INTERIOR
        assert z["stable"][inner].all() and not z["ext64"][..., 0][inner].any()
        assert np.abs(z["gcv64"].sum(-1) - 1)[inner].max() <= 2e-10


def test_face_normals_and_areas():
    from pytorch_points_amd.network.geo_operations import compute_face_normals_and_areas
    v = torch.tensor([[0.0, 0, 0], [2, 0, 0], [0, 3, 0], [0, 0, 1]])
    f = torch.tensor([[0, 1, 2], [0, 3, 1]])
    n, a = compute_face_normals_and_areas(v, f)
    assert n.shape == (2, 3) and a.shape == (2,)
    torch.testing.assert_close(n, torch.tensor([[0.0, 0, 1], [0, 1, 0]]))
    torch.testing.assert_close(a, torch.tensor([3.0, 1.0]))
    nb, ab = compute_face_normals_and_areas(v[None].expand(3, -1, -1), f[None].expand(3, -1, -1))
    assert nb.shape == (3, 2, 3) and torch.equal(nb[2], n) and torch.equal(ab[1], a)
    assert v.shape == (4, 3) and f.shape == (2, 3)          # the inputs are not reshaped in place


def test_composition_fp32_and_other_dtypes_run():
    from pytorch_points_amd.network.geo_operations import green_coordinates_3D
    z, faces = load(GOLDEN[0])
    st = z["stable"]
    for dt in (torch.float32, torch.bfloat16):
        gcv, gcf, ext = green_coordinates_3D(torch.from_numpy(z["query"]).to(dt),
                                             torch.from_numpy(z["vertices"]).to(dt), faces)
        assert gcv.dtype == dt and gcf.dtype == dt and gcv.shape == z["gcv64"].shape and ext.dtype == torch.bool
        if dt == torch.float32:
            np.testing.assert_allclose(gcv.numpy()[st], z["gcv32"][st], rtol=0, atol=1e-5)
            np.testing.assert_allclose(gcf.numpy()[st], z["gcf32"][st], rtol=0, atol=1e-5)
    from pytorch_points_amd import green
    q, v = torch.from_numpy(z["query"]).double(), torch.from_numpy(z["vertices"]).double()
    a = green_coordinates_3D(q, v, faces.int(), verbose=True)
    b = green.composition(q, v, faces)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_composition_edge_sizes_and_bad_indices():
    from pytorch_points_amd import green
    v = torch.randn(2, 5, 3, dtype=torch.float64)
    f = torch.tensor([[[0, 1, 2], [2, 3, 4]], [[0, 1, 2], [2, 3, 5]]])
    q = torch.randn(2, 4, 3, dtype=torch.float64)
    gcv, gcf, ext = green.composition(q, v, f)
    assert torch.isnan(gcv[1]).all() and torch.isnan(gcf[1]).all() and not ext[1].any()
    assert not torch.isnan(gcv[0]).any()
    assert [t.shape for t in green.composition(q[:, :0], v, f)] == [(2, 0, 5), (2, 0, 2), (2, 0, 1)]
    gcv, gcf, ext = green.composition(q, v, f[:, :0])
    assert gcv.shape == (2, 4, 5) and (gcv == 0).all() and gcf.shape == (2, 4, 0) and ext.all()


def test_shape_and_dtype_errors():
    from pytorch_points_amd.network.geo_operations import green_coordinates_3D as gc3d
    q = torch.zeros(2, 4, 3)
    v = torch.zeros(2, 6, 3)
    f = torch.zeros(2, 8, 3, dtype=torch.long)
    with pytest.raises(RuntimeError, match="query must have shape"):
        gc3d(torch.zeros(2, 4, 2), v, f)
    with pytest.raises(RuntimeError, match="vertices must have shape"):
        gc3d(q, torch.zeros(2, 6), f)
    with pytest.raises(RuntimeError, match="faces must have shape"):
        gc3d(q, v, torch.zeros(2, 8, 4, dtype=torch.long))
    with pytest.raises(RuntimeError, match="same batch size"):
        gc3d(q, torch.zeros(3, 6, 3), f)
    with pytest.raises(RuntimeError, match="one dtype"):
        gc3d(q, v.double(), f)
    with pytest.raises(RuntimeError, match="floating"):
        gc3d(q.long(), v.long(), f)
    with pytest.raises(RuntimeError, match="integer"):
        gc3d(q, v, f.float())
    with pytest.raises(RuntimeError, match="face_normals must have shape"):
        gc3d(q, v, f, face_normals=torch.zeros(2, 7, 3))
    with pytest.raises(RuntimeError, match="face_normals must have the dtype"):
        gc3d(q, v, f, face_normals=torch.zeros(2, 8, 3, dtype=torch.float64))
