"""CPU tests (no GPU) of the mesh surface sampling (pytorch_points_amd/mesh_sample.py and its names in
network/geo_operations.py and network/model_loss.py) through ``sample_composition``: against a numpy fp64 restatement,
by the statistics of the draw, on inputs with known answers and on argument errors.  The meshes, the random numbers and
the numpy references here also serve tests/test_gpu_mesh_sample.py."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from pytorch_points_amd import _build, _lib, mesh_sample, synthetic
from pytorch_points_amd.mesh_laplacian import MeshCorners
from pytorch_points_amd.network import geo_operations, model_loss
from test_abi_and_host import declared_symbols
from test_mesh_dihedral_host import folded_grid, jittered_cage, two_topologies, zigzag_fan
from test_mesh_edges_host import soup_mesh

F32 = np.float32
EPS32 = 2.0 ** -23
MESHES = ["cage", "grid_40x130", "fan_300", "two_topologies", "soup"]
SIZES = [1, 63, 65, 1000, 5000]
ENTRIES = ["pp_mesh_sample_cdf_f32", "pp_mesh_sample_forward_f32", "pp_mesh_sample_backward_f32"]


@functools.lru_cache(maxsize=None)
def mesh(name):
    """(vertices (B,N,3) float64 that are exact in fp32, faces (F,3) or (B,F,3))"""
    if name == "cage":
        faces, v = jittered_cage(12, batch=3)
    elif name == "grid_40x130":
        v, faces = folded_grid(40, 130, 13, batch=3)
    elif name == "fan_300":
        v, faces = zigzag_fan(300, 14, batch=3)
    elif name == "two_topologies":
        v, faces = two_topologies()
    else:
        faces, n = soup_mesh(50, 200, 1)                   # 25 faces with a repeated vertex: no area
        v = synthetic.unit_sphere(2, 1, n)
    return v.astype(F32).astype(np.float64), faces


def uniforms(seed, batch, samples):
    """(B,S,3) fp32 in [0,1)"""
    return np.random.default_rng(seed).random((batch, samples, 3), dtype=F32)


def corners_of(faces, n, device="cpu"):
    return MeshCorners.from_faces(torch.from_numpy(faces).to(device), n)


def faces_of(faces, b):
    return faces if faces.ndim == 2 else faces[b]


# --------------------------------------------------------------------------------------------- numpy references
def np_faces(areas, u1):
    """The face choice of the contract for fp32 ``areas`` (B,F) and ``u1`` (B,S) with numpy's sequential fp64 prefix
    sum: ``(face (B,S), clear)``.  ``clear`` says that no target lies within ``2 F 2^-53 cdf[F-1]`` of the CDF values
    on either side of it -- two summation orders of F non-negative fp64 terms differ by no more than that -- so that
    every fixed association gives the same faces."""
    cdf = np.cumsum(areas.astype(np.float64), axis=1)
    f = cdf.shape[1]
    face = np.empty(u1.shape, np.int64)
    clear = True
    for b in range(cdf.shape[0]):
        total = cdf[b, -1]
        assert total > 0 and np.isfinite(total)
        target = u1[b].astype(np.float64) * total
        face[b] = np.searchsorted(cdf[b], target, side="right")
        assert (face[b] < f).all()
        above = cdf[b][face[b]] - target
        below = np.where(face[b] > 0, target - cdf[b][np.maximum(face[b] - 1, 0)], np.inf)
        clear = clear and bool((np.minimum(above, below) > 2 * f * 2.0 ** -53 * total).all())
    return face, clear


def np_points(v, faces, face, u):
    """fp64: ``(points (B,S,3), bary (B,S,3))`` of the contract, given the faces chosen"""
    u = u.astype(np.float64)
    su = np.sqrt(u[..., 1])
    bary = np.stack([1 - su, su * (1 - u[..., 2]), su * u[..., 2]], -1)
    points = np.empty(face.shape + (3,))
    for b in range(v.shape[0]):
        p = v[b][faces_of(faces, b)[face[b]]]                          # (S, 3 corners, 3)
        points[b] = (bary[b][:, :, None] * p).sum(1)
    return points, bary


def brute_nndistance(a, b):
    """``nndistance`` on any device and dtype, every pair"""
    d = ((a[:, :, None, :] - b[:, None, :, :]) ** 2).sum(-1)
    d1, i1 = d.min(2)
    d2, i2 = d.min(1)
    return d1, d2, i1.int(), i2.int()


# ------------------------------------------------------------------------------------------- symbols and names
def test_symbols_are_declared_exported_and_bound():
    declared = declared_symbols()
    _build.build()
    handle = ctypes.CDLL(_build.LIB)
    for name in ENTRIES:
        assert name in declared and hasattr(handle, name) and name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["pp_mesh_sample_forward_f32"]) == 18
    assert len(_lib.SIGNATURES["pp_mesh_sample_backward_f32"]) == 19


def test_entries_check_their_sizes_before_any_launch():
    """PP_OK (0) for an empty problem and PP_EINVAL (1) for sizes that cannot be served: decided on the host"""
    lib = _lib.lib()
    assert lib.pp_mesh_sample_cdf_f32(None, None, 0, 5, None) == 0
    assert lib.pp_mesh_sample_cdf_f32(None, None, 2, 0, None) == 0
    assert lib.pp_mesh_sample_cdf_f32(None, None, -1, 5, None) == 1
    assert lib.pp_mesh_sample_cdf_f32(None, None, 2, 5, None) == 1
    for b, n, f, s in ((0, 5, 5, 5), (2, 5, 0, 5), (2, 5, 5, 0)):
        assert lib.pp_mesh_sample_forward_f32(*(None,) * 4, 3, *(None,) * 7, b, n, f, s, 0, None) == 0
        assert lib.pp_mesh_sample_backward_f32(*(None,) * 11, b, n, f, s, 0, None, 0, None) == 0
    assert lib.pp_mesh_sample_backward_f32(*(None,) * 11, 2, 0, 5, 5, 0, None, 0, None) == 0
    for b, n, f, s in ((-1, 5, 5, 5), (2, -1, 5, 5), (2, 5, -1, 5), (2, 5, 5, -1), (2, 5, 5, 2 ** 30), (2, 5, 5, 5)):
        assert lib.pp_mesh_sample_forward_f32(*(None,) * 4, 3, *(None,) * 7, b, n, f, s, 0, None) == 1
        assert lib.pp_mesh_sample_backward_f32(*(None,) * 11, b, n, f, s, 0, None, 0, None) == 1


def test_names_are_reexported():
    from pytorch_points.network.geo_operations import sample_points_from_meshes  # noqa: F401
    from pytorch_points.network.model_loss import SampledMeshChamferLoss
    assert issubclass(SampledMeshChamferLoss, torch.nn.Module)
    assert SampledMeshChamferLoss is model_loss.SampledMeshChamferLoss is mesh_sample.SampledMeshChamferLoss
    for name in ("mesh_sample_faces", "mesh_interpolate", "sample_points_from_meshes"):
        assert getattr(geo_operations, name) is getattr(mesh_sample, name)
    assert hasattr(mesh_sample, "sample_composition")


# ------------------------------------------------------------------------------------- against the restatement
@pytest.mark.parametrize("name", MESHES)
def test_composition_against_the_numpy_restatement(name):
    v, faces = mesh(name)
    b, n = v.shape[0], v.shape[1]
    corners = corners_of(faces, n)
    x = torch.from_numpy(v.astype(F32))
    _, areas = geo_operations.mesh_face_normals(x, corners)
    scale = np.abs(v).max()
    for k, s in enumerate(SIZES):
        u = uniforms(100 + k, b, s)
        out = mesh_sample.sample_points_from_meshes(x, corners, u=torch.from_numpy(u), return_normals=True)
        assert out._fields == ("points", "face", "bary", "normals")
        assert out.face.dtype == torch.int64 and out.points.dtype == torch.float32 and out.points.shape == (b, s, 3)
        face, clear = np_faces(areas.numpy(), u[..., 0])
        assert clear
        assert np.array_equal(out.face.numpy(), face)
        assert torch.equal(out.face, mesh_sample.mesh_sample_faces(areas, torch.from_numpy(u[..., 0])))
        points, bary = np_points(v, faces, face, u)
        assert np.abs(out.bary.double().numpy() - bary).max() <= 4 * EPS32
        assert np.abs(out.points.double().numpy() - points).max() <= 8 * EPS32 * scale
        assert torch.equal(mesh_sample.mesh_interpolate(x, corners, out.face, out.bary), out.points)
        normals = geo_operations.mesh_face_normals(x, corners)[0]
        for i in range(b):
            assert torch.equal(out.normals[i], normals[i][out.face[i]])


def test_gradient_of_the_composition():
    v, faces = mesh("two_topologies")
    corners = corners_of(faces, 99)
    u = torch.from_numpy(uniforms(7, 2, 40))
    x = torch.from_numpy(v).requires_grad_(True)
    fixed = mesh_sample.sample_points_from_meshes(x, corners, u=u)
    assert not fixed.face.requires_grad and not fixed.bary.requires_grad

    def both(t):
        out = mesh_sample.sample_composition(t, corners, face=fixed.face, bary=fixed.bary, return_normals=True)
        return out[0], out[3]

    assert torch.autograd.gradcheck(both, (x,), eps=1e-6, atol=1e-6)


# ------------------------------------------------------------------------------------------------ the statistics
def test_face_counts_follow_the_areas_and_the_weights_are_uniform():
    v, faces = mesh("cage")
    s = 5000
    x = torch.from_numpy(v.astype(F32))
    corners = corners_of(faces, x.shape[1])
    out = mesh_sample.sample_points_from_meshes(x, corners, u=torch.from_numpy(uniforms(3, 3, s)))
    areas = geo_operations.mesh_face_normals(x, corners)[1].double().numpy()
    for b in range(3):
        p = areas[b] / areas[b].sum()
        count = np.bincount(out.face[b].numpy(), minlength=p.shape[0])
        assert (np.abs(count - s * p) <= 6 * np.sqrt(s * p * (1 - p)) + 1).all()
        mean = out.bary[b].double().numpy().mean(0)
        assert (np.abs(mean - 1 / 3) <= 6 * np.sqrt(1 / 18) / np.sqrt(s)).all()
    assert float((out.bary.sum(-1) - 1).abs().max()) <= 4 * EPS32 and bool((out.bary >= 0).all())


def test_faces_without_area_are_never_drawn():
    v, faces = mesh("soup")
    flat = (faces[:, 0] == faces[:, 1]) | (faces[:, 1] == faces[:, 2]) | (faces[:, 0] == faces[:, 2])
    assert flat.sum() >= 20
    x = torch.from_numpy(v.astype(F32)).requires_grad_(True)
    u = uniforms(4, 1, 5000)
    u[0, :3, 0] = (0.0, 1 - 2.0 ** -24, 0.5)
    out = mesh_sample.sample_points_from_meshes(x, torch.from_numpy(faces), u=torch.from_numpy(u))
    drawn = np.bincount(out.face[0].numpy(), minlength=faces.shape[0])
    assert (drawn[flat] == 0).all() and drawn.sum() == 5000 and (drawn > 0).sum() > 100
    grad, = torch.autograd.grad(out.points.sum(), x)
    assert bool(torch.isfinite(grad).all())
    only_flat = np.ones(50, bool)
    only_flat[faces[~flat].reshape(-1)] = False
    assert bool((grad[0][torch.from_numpy(only_flat)] == 0).all())


def test_a_mesh_without_area_gives_minus_one_and_nan():
    v, faces = mesh("two_topologies")
    x = torch.from_numpy(v.astype(F32)).clone()
    x[1] = 0.25                                                          # every face of element 1 is a point
    x.requires_grad_(True)
    u = torch.from_numpy(uniforms(5, 2, 65))
    out = mesh_sample.sample_points_from_meshes(x, torch.from_numpy(faces), u=u, return_normals=True)
    assert bool((out.face[1] == -1).all()) and bool((out.face[0] >= 0).all())
    for t in (out.points, out.bary, out.normals):
        assert bool(torch.isnan(t[1]).all()) and bool(torch.isfinite(t[0]).all())
    grad, = torch.autograd.grad(out.points[0].sum() + out.normals[0].sum(), x)
    assert bool(torch.isfinite(grad).all()) and bool((grad[1] == 0).all()) and bool((grad[0] != 0).any())
    none = MeshCorners.from_faces(torch.zeros(0, 3, dtype=torch.int64), 99)
    out = mesh_sample.sample_points_from_meshes(x, none, u=u)
    assert out.face.shape == (2, 65) and bool((out.face == -1).all()) and bool(torch.isnan(out.points).all())
    assert bool((mesh_sample.mesh_sample_faces(torch.zeros(2, 0), u[..., 0]) == -1).all())
    assert bool((mesh_sample.mesh_sample_faces(torch.tensor([[1.0, float("inf")], [0.0, 0.0]]), u[..., 0]) == -1).all())
    empty = mesh_sample.sample_points_from_meshes(x, torch.from_numpy(faces), 0)
    assert empty.points.shape == (2, 0, 3) and empty.face.shape == (2, 0) and empty.bary.shape == (2, 0, 3)


# ------------------------------------------------------------------------------------------- the API and errors
def test_u_and_a_generator_give_the_same_samples():
    v, faces = mesh("cage")
    x = torch.from_numpy(v.astype(F32))
    tf = torch.from_numpy(faces)
    first = geo_operations.sample_points_from_meshes(x, tf, 100, generator=torch.Generator().manual_seed(5))
    u = torch.rand((3, 100, 3), generator=torch.Generator().manual_seed(5))
    second = geo_operations.sample_points_from_meshes(x, corners_of(faces, x.shape[1]), u=u)
    third = geo_operations.sample_points_from_meshes(x, tf, 100, u=u, return_normals=True)
    assert first._fields == ("points", "face", "bary")
    for a, b, c in zip(first, second, third):
        assert torch.equal(a, b) and torch.equal(a, c)
    other = geo_operations.sample_points_from_meshes(x, tf, 100, generator=torch.Generator().manual_seed(6))
    assert not torch.equal(other.face, first.face)


def test_argument_errors():
    v, faces = mesh("cage")
    x = torch.from_numpy(v.astype(F32))
    corners = corners_of(faces, x.shape[1])
    u = torch.from_numpy(uniforms(1, 3, 10))
    sample, interpolate = mesh_sample.sample_points_from_meshes, mesh_sample.mesh_interpolate
    with pytest.raises(NotImplementedError, match="triangles only, got faces of 4 corners"):
        sample(x, corners_of(np.zeros((5, 4), np.int64), x.shape[1]), 10)
    with pytest.raises(TypeError, match="faces_or_corners"):
        sample(x, [1, 2, 3], 10)
    with pytest.raises(ValueError, match="num_samples"):
        sample(x, corners)
    with pytest.raises(ValueError, match="num_samples is 11"):
        sample(x, corners, 11, u=u)
    with pytest.raises(ValueError, match="u must have shape"):
        sample(x, corners, u=u[:2])
    with pytest.raises(ValueError, match="u must have shape"):
        sample(x, corners, u=u[..., :2])
    with pytest.raises(TypeError, match="float32"):
        sample(x, corners, u=u.double())
    with pytest.raises(ValueError, match="built for 162 vertices"):
        sample(x[:, :100], corners, u=u)
    with pytest.raises(ValueError, match="vertices must have shape"):
        sample(x[..., :2], corners, u=u)
    with pytest.raises(IndexError, match="batch element 0"):
        sample(x, torch.tensor([[0, 1, 162]]), u=u)
    with pytest.raises(TypeError, match="MeshCorners"):
        interpolate(x, torch.from_numpy(faces), torch.zeros(3, 10, dtype=torch.int64), torch.rand(3, 10, 3))
    with pytest.raises(TypeError, match="face must be an integer"):
        interpolate(x, corners, torch.zeros(3, 10), torch.rand(3, 10, 3))
    with pytest.raises(ValueError, match="face must have shape"):
        interpolate(x, corners, torch.zeros(2, 10, dtype=torch.int64), torch.rand(2, 10, 3))
    with pytest.raises(ValueError, match="bary must have shape"):
        interpolate(x, corners, torch.zeros(3, 10, dtype=torch.int64), torch.rand(3, 10, 2))
    with pytest.raises(ValueError, match="areas must have shape"):
        mesh_sample.mesh_sample_faces(torch.rand(5), u[..., 0])
    with pytest.raises(ValueError, match="u must have shape"):
        mesh_sample.mesh_sample_faces(torch.rand(3, 5), u)
    bad = interpolate(x, corners, torch.tensor([[0, -1, 320]] * 3), torch.full((3, 3, 3), 1 / 3))
    assert bool(torch.isfinite(bad[:, 0]).all()) and bool(torch.isnan(bad[:, 1:]).all())


def test_the_loss_with_the_kept_topology_equals_the_loss_with_the_topology_rebuilt(monkeypatch):
    monkeypatch.setattr(model_loss, "nndistance", brute_nndistance)
    v, faces = mesh("two_topologies")
    x = torch.from_numpy(v).requires_grad_(True)
    tf = torch.from_numpy(faces)
    target = torch.from_numpy(synthetic.unit_sphere(9, 2, 70).astype(np.float64))
    u = torch.from_numpy(uniforms(8, 2, 63))
    kept = model_loss.SampledMeshChamferLoss(63, consistent_topology=True)
    fresh = model_loss.SampledMeshChamferLoss(63)
    first = kept(x, tf, target, u=u)
    topology = kept.E
    again = kept(x, None, target, u=u)
    assert kept.E is topology and torch.equal(first, again) and torch.equal(first, fresh(x, tf, target, u=u))
    assert fresh.E is not topology
    points = mesh_sample.sample_points_from_meshes(x, tf, u=u).points
    d1, d2, _, _ = brute_nndistance(points, target)
    assert torch.equal(first, d1.mean() + d2.mean())
    grad, = torch.autograd.grad(first, x)
    assert bool(torch.isfinite(grad).all()) and bool((grad != 0).any())
    drawn = fresh(x, tf, target)                                          # its own random numbers
    assert drawn.shape == () and bool(torch.isfinite(drawn))
    with pytest.raises(AssertionError, match="Face is required"):
        model_loss.SampledMeshChamferLoss(63)(x, None, target)
