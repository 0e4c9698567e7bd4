"""CPU tests (no GPU) of the mesh normals (pytorch_points_amd/mesh_normals.py, network/geo_operations.py
mesh_face_normals / mesh_vertex_normals / normalize_to_same_area, network/model_loss.py MeshNormalLoss) through their
torch compositions, against a numpy loop over the faces, by gradcheck and on inputs with known answers.  The numpy
references here also serve tests/test_gpu_mesh_normals.py."""
import ctypes

import numpy as np
import pytest
import torch

from pytorch_points_amd import _build, _lib, mesh_normals, synthetic
from pytorch_points_amd.mesh_laplacian import MeshCorners
from pytorch_points_amd.network import geo_operations, model_loss
from test_abi_and_host import declared_symbols
from test_mesh_dihedral_host import jittered_cage, torus_mesh, two_topologies
from test_mesh_edges_host import grid_mesh, jittered_grid, soup_mesh, tetrahedron

EPS32 = 2.0 ** -23
EPS64 = 2.0 ** -52
ENTRIES = ["pp_mesh_face_normals_forward_f32", "pp_mesh_face_normals_backward_f32",
           "pp_mesh_vertex_normals_forward_f32", "pp_mesh_vertex_normals_backward_f32"]
WEIGHTINGS = ["area", "uniform"]


# --------------------------------------------------------------------------------------------- numpy references
def np_face_normals(v, faces):
    """one mesh, float64, face by face: (normals (F,3), areas (F,), cross products (F,3))"""
    v = np.asarray(v, np.float64)
    cross = np.zeros((faces.shape[0], 3))
    for f, (i0, i1, i2) in enumerate(faces.tolist()):
        cross[f] = np.cross(v[i1] - v[i0], v[i2] - v[i1])
    length = np.sqrt((cross * cross).sum(-1))
    return cross / np.maximum(length, 1e-12)[:, None], length / 2, cross


def np_vertex_normals(v, faces, weighting):
    """one mesh, float64: (normals (N,3), |S| (N,), the sum over a vertex's corners of |c| (N,)); every face's weighted
    cross product goes to its three vertices with np.add.at"""
    v = np.asarray(v, np.float64)
    unit, _, cross = np_face_normals(v, faces)
    sums, sizes = np.zeros_like(v), np.zeros(v.shape[0])
    for f, face in enumerate(faces.tolist()):
        np.add.at(sums, face, unit[f] if weighting == "uniform" else cross[f])
        np.add.at(sizes, face, 1.0 if weighting == "uniform" else np.sqrt((cross[f] ** 2).sum()))
    length = np.sqrt((sums * sums).sum(-1))
    return sums / np.maximum(length, 1e-12)[:, None], length, sizes


def face_shape_quality(v, faces):
    """2A / (sum of the squared edge lengths) of every face of one mesh: 1 / (2 sqrt 3) = 0.289 for an equilateral
    triangle, 0 for one without area"""
    v = np.asarray(v, np.float64)
    p = v[faces]
    edges = ((p - p[:, [1, 2, 0]]) ** 2).sum((1, 2))
    return 2 * np_face_normals(v, faces)[1] / edges


def host_meshes(name):
    """(vertices (B,N,3) float64, faces (F,3) or (B,F,3))"""
    if name == "tetrahedron":
        return synthetic.unit_sphere(4, 1, 4).astype(np.float64), tetrahedron()[0]
    if name == "grid_3x3":
        v, faces = jittered_grid(3, 3, 5)
        v = v.astype(np.float64)
        v[..., 2] = 0.2 * (2 * synthetic.uniform01(6, (1, 9)).reshape(1, 9) - 1)
        return v, faces
    if name == "cage":
        faces, v = jittered_cage(7, batch=2)
        return v, faces
    assert name == "two_topologies"
    return two_topologies()


def corners_of(faces, n):
    return MeshCorners.from_faces(torch.from_numpy(faces), n)


# ------------------------------------------------------------------------------------------- symbols and names
def test_symbols_are_declared_exported_and_bound():
    declared = declared_symbols()
    _build.build()
    handle = ctypes.CDLL(_build.LIB)
    for name in ENTRIES:
        assert name in declared and hasattr(handle, name) and name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["pp_mesh_vertex_normals_backward_f32"]) == 12


def test_entries_check_their_sizes_before_any_launch():
    """PP_OK (0) for an empty problem and PP_EINVAL (1) for sizes or pointers that cannot be served: both are decided
    on the host, so neither needs a device"""
    lib = _lib.lib()
    face_fwd, face_bwd = lib.pp_mesh_face_normals_forward_f32, lib.pp_mesh_face_normals_backward_f32
    vert_fwd, vert_bwd = lib.pp_mesh_vertex_normals_forward_f32, lib.pp_mesh_vertex_normals_backward_f32
    for b, n, f in ((0, 5, 5), (2, 0, 5), (2, 5, 0)):
        assert face_fwd(None, None, None, None, b, n, f, 0, None) == 0
        assert face_bwd(None, None, None, None, None, None, None, b, n, f, 0, None) == 0
        assert vert_fwd(None, None, None, None, b, n, f, 1, 0, None) == 0
        assert vert_bwd(None, None, None, None, None, None, b, n, f, 1, 0, None) == 0
    for b, n, f in ((-1, 5, 5), (2, -1, 5), (2, 5, -1), (65536, 65536, 5), (65536, 5, 65536), (1, 5, 2 ** 30),
                    (2, 5, 5)):                                              # the last: sizes fine, pointers NULL
        assert face_fwd(None, None, None, None, b, n, f, 0, None) == 1
        assert face_bwd(None, None, None, None, None, None, None, b, n, f, 0, None) == 1
        assert vert_fwd(None, None, None, None, b, n, f, 0, 0, None) == 1
        assert vert_bwd(None, None, None, None, None, None, b, n, f, 0, 0, None) == 1
    for weighting in (-1, 2):
        assert vert_fwd(None, None, None, None, 0, 5, 5, weighting, 0, None) == 1
        assert vert_bwd(None, None, None, None, None, None, 0, 5, 5, weighting, 0, None) == 1


def test_drop_in_names_resolve():
    import pytorch_points_amd
    pytorch_points_amd.install_as_pytorch_points()
    from pytorch_points.network.geo_operations import (mesh_face_normals, mesh_vertex_normals,  # noqa: F401
                                                       normalize_to_same_area)
    from pytorch_points.network.model_loss import MeshNormalLoss
    assert issubclass(MeshNormalLoss, torch.nn.Module) and MeshNormalLoss is model_loss.MeshNormalLoss
    for name in ("mesh_face_normals", "mesh_vertex_normals", "face_normals_composition", "vertex_normals_composition",
                 "MeshFaceNormals", "MeshVertexNormals"):
        assert hasattr(mesh_normals, name)


# -------------------------------------------------------------------------------- the compositions against numpy
@pytest.mark.parametrize("name", ["tetrahedron", "grid_3x3", "cage", "two_topologies"])
def test_fp64_compositions_against_the_numpy_loop(name):
    v, faces = host_meshes(name)
    corners = corners_of(faces, v.shape[1])
    assert corners.batch == (1 if faces.ndim == 2 else v.shape[0])
    x = torch.from_numpy(v)
    normals, areas = mesh_normals.mesh_face_normals(x, corners)            # CPU tensors take the composition
    assert normals.dtype == torch.float64 and normals.shape == (v.shape[0], faces.shape[-2], 3)
    assert areas.shape == normals.shape[:2]
    per_vertex = {w: mesh_normals.mesh_vertex_normals(x, corners, w) for w in WEIGHTINGS}
    for b in range(v.shape[0]):
        fb = faces if faces.ndim == 2 else faces[b]
        want_n, want_a, _ = np_face_normals(v[b], fb)
        np.testing.assert_allclose(normals[b].numpy(), want_n, rtol=0, atol=1e-13)
        np.testing.assert_allclose(areas[b].numpy(), want_a, rtol=1e-13, atol=0)
        for w in WEIGHTINGS:
            want, length, _ = np_vertex_normals(v[b], fb, w)
            assert per_vertex[w].shape == v.shape
            np.testing.assert_allclose(per_vertex[w][b].numpy(), want, rtol=0, atol=1e-12)
            used = length > 0
            np.testing.assert_allclose(np.linalg.norm(per_vertex[w][b].numpy()[used], axis=-1), 1, rtol=0, atol=1e-14)
    # the same values as the function the cage deformation uses
    old_n, old_a = geo_operations.compute_face_normals_and_areas(
        x, torch.from_numpy(faces if faces.ndim == 3 else np.broadcast_to(faces, (v.shape[0],) + faces.shape).copy()))
    np.testing.assert_allclose(normals.numpy(), old_n.numpy(), rtol=0, atol=1e-14)
    np.testing.assert_allclose(areas.numpy(), old_a.numpy(), rtol=1e-14, atol=0)


@pytest.mark.parametrize("name", ["tetrahedron", "grid_3x3"])
def test_gradcheck_of_both_compositions(name):
    v, faces = host_meshes(name)
    corners = corners_of(faces, v.shape[1])
    x = torch.from_numpy(v).requires_grad_(True)
    for part in (0, 1):                                                     # g_n alone, g_a alone
        assert torch.autograd.gradcheck(lambda t: mesh_normals.face_normals_composition(t, corners)[part], (x,),
                                        eps=1e-6, atol=1e-7, rtol=1e-6)
    for w in WEIGHTINGS:
        assert torch.autograd.gradcheck(lambda t: mesh_normals.vertex_normals_composition(t, corners, w), (x,),
                                        eps=1e-6, atol=1e-7, rtol=1e-6)


# ------------------------------------------------------------------------------------------------ fixed values
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_a_flat_grid_has_the_normal_z_and_the_area_one(dtype):
    v, faces = grid_mesh(7, 9)
    corners = corners_of(faces, 63)
    x = torch.from_numpy(v)[None].to(dtype)
    normals, areas = mesh_normals.mesh_face_normals(x, corners)
    up = torch.tensor([0.0, 0.0, 1.0], dtype=dtype)
    assert bool((normals == up).all())
    assert abs(float(areas.double().sum()) - 1) <= faces.shape[0] * EPS32
    for w in WEIGHTINGS:
        assert bool((mesh_normals.mesh_vertex_normals(x, corners, w) == up).all())


def test_the_cross_products_of_a_closed_mesh_sum_to_zero():
    v, faces = torus_mesh(8, 10)
    normals, areas = mesh_normals.mesh_face_normals(torch.from_numpy(v)[None], corners_of(faces, 80))
    cross = (2 * areas[..., None] * normals)[0].numpy()
    size = np.abs(cross).sum()
    assert size > 1 and np.abs(cross.sum(0)).max() <= faces.shape[0] * EPS64 * size


def test_unused_vertices_get_plus_zero_and_no_gradient():
    v, faces = two_topologies()
    used = np.zeros(99, bool)
    used[faces[1].reshape(-1)] = True
    assert (~used).sum() == 19
    corners = corners_of(faces, 99)
    for w in WEIGHTINGS:
        x = torch.from_numpy(v).requires_grad_(True)
        out = mesh_normals.mesh_vertex_normals(x, corners, w)
        idle = out[1].detach().numpy()[~used]
        assert (idle == 0).all() and not np.signbit(idle).any()
        grad, = torch.autograd.grad(out.sum() + (out * out).sum(), x)
        assert bool((grad[1][torch.from_numpy(~used)] == 0).all()) and bool((grad[1] != 0).any())
        assert bool(torch.isfinite(grad).all())
    x = torch.from_numpy(v).requires_grad_(True)
    normals, areas = mesh_normals.mesh_face_normals(x, corners)
    grad, = torch.autograd.grad(normals.sum() + areas.sum(), x)
    assert bool((grad[1][torch.from_numpy(~used)] == 0).all())


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_a_face_with_a_repeated_vertex(dtype):
    faces, n = soup_mesh(50, 200, 1)
    flat = (faces[:, 0] == faces[:, 1]) | (faces[:, 1] == faces[:, 2]) | (faces[:, 0] == faces[:, 2])
    assert 20 < flat.sum() < 100
    corners = corners_of(faces, n)
    x = torch.from_numpy(synthetic.unit_sphere(2, 1, n)).to(dtype).requires_grad_(True)
    normals, areas = mesh_normals.mesh_face_normals(x, corners)
    mask = torch.from_numpy(flat)
    assert bool((areas[0][mask] == 0).all()) and bool((normals[0][mask] == 0).all())
    assert bool((areas[0][~mask] > 0).all())
    grad, = torch.autograd.grad(normals.sum() + areas.sum(), x)          # (sqrt's own backward gives NaN here)
    assert bool(torch.isfinite(grad).all()) and bool((grad != 0).any())
    for w in WEIGHTINGS:
        y = torch.from_numpy(synthetic.unit_sphere(2, 1, n)).to(dtype).requires_grad_(True)
        out = mesh_normals.mesh_vertex_normals(y, corners, w)
        grad, = torch.autograd.grad(out.sum(), y)
        assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(grad).all())


# ------------------------------------------------------------------------------------------------ the API paths
def test_normalize_to_same_area():
    v, faces = two_topologies()
    faces_ref, v_ref = jittered_cage(8, batch=2)
    x = torch.from_numpy(v).requires_grad_(True)
    tf, tr = torch.from_numpy(faces), torch.from_numpy(faces_ref)
    out = geo_operations.normalize_to_same_area(torch.from_numpy(v_ref), tr, x, tf)
    want = geo_operations.mesh_face_normals(torch.from_numpy(v_ref), tr)[1].sum(-1)
    got = geo_operations.mesh_face_normals(out, tf)[1].sum(-1)
    assert out.shape == v.shape and not torch.allclose(out.detach(), x.detach())
    np.testing.assert_allclose(got.detach().numpy(), want.numpy(), rtol=1e-13, atol=0)
    grad, = torch.autograd.grad(out.sum(), x)
    assert bool(torch.isfinite(grad).all()) and bool((grad != 0).any())
    kept = corners_of(faces, 99), corners_of(faces_ref, 162)                 # kept topologies: the same bits
    assert torch.equal(geo_operations.normalize_to_same_area(torch.from_numpy(v_ref), kept[1], x, kept[0]), out)


def test_geo_operations_names_build_or_keep_the_topology():
    v, faces = two_topologies()
    x = torch.from_numpy(v)
    corners = corners_of(faces, 99)
    for a, b in zip(geo_operations.mesh_face_normals(x, torch.from_numpy(faces)),
                    mesh_normals.mesh_face_normals(x, corners)):
        assert torch.equal(a, b)
    for w in WEIGHTINGS:
        want = mesh_normals.mesh_vertex_normals(x, corners, w)
        assert torch.equal(geo_operations.mesh_vertex_normals(x, torch.from_numpy(faces), w), want)
        assert torch.equal(geo_operations.mesh_vertex_normals(x, corners, weighting=w), want)
    shared = geo_operations.mesh_vertex_normals(x, torch.from_numpy(faces[0]))      # (F,3): one topology for the batch
    assert torch.equal(shared[0], mesh_normals.mesh_vertex_normals(x, corners)[0])
    with pytest.raises(TypeError):
        geo_operations.mesh_face_normals(x, faces)


@pytest.mark.parametrize("use_face", [False, True])
@pytest.mark.parametrize("weighting", WEIGHTINGS)
def test_mesh_normal_loss(use_face, weighting):
    v, faces = two_topologies()
    other = v + 0.02 * (2 * synthetic.uniform01(40, v.shape).reshape(v.shape) - 1)
    x1, x2 = (torch.from_numpy(a).requires_grad_(True) for a in (v, other))
    mod = model_loss.MeshNormalLoss(torch.nn.MSELoss(), use_face, weighting)
    got = mod(x1, x2, torch.from_numpy(faces))
    want = []
    for a in (v, other):
        want.append(np.stack([np_face_normals(a[b], faces[b])[0] if use_face
                              else np_vertex_normals(a[b], faces[b], weighting)[0] for b in range(2)]))
    np.testing.assert_allclose(float(got.detach()), ((want[0] - want[1]) ** 2).mean(), rtol=1e-11, atol=0)
    grads = torch.autograd.grad(got, (x1, x2))
    assert all(bool(torch.isfinite(g).all()) and bool((g != 0).any()) for g in grads)


def test_mesh_normal_loss_keeps_its_topology():
    v, faces = two_topologies()
    x = torch.from_numpy(v)
    mod = model_loss.MeshNormalLoss(torch.nn.L1Loss(), consistent_topology=True)
    first = mod(x, x.flip(0), torch.from_numpy(faces))
    kept = mod.E
    assert isinstance(kept, MeshCorners) and float(first) > 0
    assert torch.equal(mod(x, x.flip(0)), first) and mod.E is kept
    fresh = model_loss.MeshNormalLoss(torch.nn.L1Loss())
    with pytest.raises(AssertionError):
        fresh(x, x)
    fresh(x, x, torch.from_numpy(faces))
    assert fresh.E is not None and fresh.E is not kept
    with pytest.raises(AssertionError):                                      # rebuilt on every call: faces again
        fresh(x, x)


# ------------------------------------------------------------------------------------------------------ errors
def test_errors():
    faces, n = tetrahedron()
    corners = corners_of(faces, n)
    quads = MeshCorners.from_faces(torch.tensor([[0, 1, 2, 3]]), 4)
    two = corners_of(np.stack([faces, faces]), n)
    for fn in (mesh_normals.mesh_face_normals, mesh_normals.mesh_vertex_normals,
               mesh_normals.face_normals_composition, mesh_normals.vertex_normals_composition):
        with pytest.raises(ValueError):
            fn(torch.zeros(1, 4, 2), corners)                                # D
        with pytest.raises(ValueError):
            fn(torch.zeros(4, 3), corners)
        with pytest.raises(ValueError):
            fn(torch.zeros(1, 5, 3), corners)                                # another vertex count
        with pytest.raises(NotImplementedError, match="triangles only"):
            fn(torch.zeros(1, 4, 3), quads)
        with pytest.raises(ValueError, match="2 batch elements"):
            fn(torch.zeros(3, 4, 3), two)
        with pytest.raises(RuntimeError, match="the topology is on cpu"):
            fn(torch.zeros(1, 4, 3, device="meta"), corners)
        with pytest.raises(RuntimeError):
            fn(torch.zeros(1, 4, 3, dtype=torch.int64), corners)
        with pytest.raises(TypeError):
            fn(torch.zeros(1, 4, 3), torch.from_numpy(faces))
    for fn in (mesh_normals.mesh_vertex_normals, mesh_normals.vertex_normals_composition,
               geo_operations.mesh_vertex_normals):
        with pytest.raises(ValueError, match="weighting"):
            fn(torch.zeros(1, 4, 3), corners, "angle")
    with pytest.raises(IndexError):
        geo_operations.mesh_face_normals(torch.zeros(1, 3, 3), torch.from_numpy(faces))
    # and the sizes of an empty problem
    none = MeshCorners.from_faces(torch.zeros(0, 3, dtype=torch.int64), 4)
    normals, areas = mesh_normals.mesh_face_normals(torch.ones(2, 4, 3), none)
    assert normals.shape == (2, 0, 3) and areas.shape == (2, 0)
    assert bool((mesh_normals.mesh_vertex_normals(torch.ones(2, 4, 3), none) == 0).all())
    assert mesh_normals.mesh_vertex_normals(torch.ones(0, 4, 3), corners).shape == (0, 4, 3)
