"""CPU tests (no GPU) of the mesh winding number, the signed point-to-mesh distance and MeshEnclosureLoss
(pytorch_points_amd/mesh_winding.py and its names in network/geo_operations.py and network/model_loss.py) through
``winding_composition`` and ``signed_distance_composition``: against a numpy fp64 brute force written independently of
the formula, on closed meshes where every point has a side, on inputs with known answers, fp32 against fp64, by
``gradcheck`` and on argument errors.  The clouds and the references here also serve tests/test_gpu_mesh_winding.py."""
import ctypes
import functools
import math
import os

import numpy as np
import pytest
import torch

from pytorch_points_amd import _build, _lib, mesh_distance, mesh_winding
from pytorch_points_amd.mesh_laplacian import MeshCorners
from pytorch_points_amd.network import geo_operations, model_loss
from test_abi_and_host import declared_symbols
from test_mesh_distance_host import SIZES, extent, has_area, np_all_pairs, unusable_cases
from test_mesh_sample_host import MESHES, corners_of, faces_of, mesh

F32 = np.float32
EPS32 = 2.0 ** -23
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CAGES = ["gc_star", "gc_cube"]                   # closed, oriented outwards, one batch element
CLOSED = ["cage"] + CAGES                        # every point off their surface is inside (1) or outside (0)
NAMES = MESHES + CAGES
TILE = ["grid_255", "grid_256", "grid_257"]      # the first faces of the grid: one LDS tile of the walk less one, full, plus one
ENTRIES = ["pp_mesh_winding_forward_f32", "pp_mesh_signed_distance_forward_f32"]
PUSH = np.array([1e-3, -1e-3, 0.3, -0.3, 0.0])   # of the extent along the face normal; the last kind is a far point


# --------------------------------------------------------------------------------------------------- the inputs
@functools.lru_cache(maxsize=None)
def winding_mesh(name):
    """(vertices (B,N,3) float64 that are exact in fp32, faces (F,3) or (B,F,3)): ``mesh(name)`` or a committed cage"""
    if name in MESHES:
        return mesh(name)
    if name in TILE:
        v, faces = mesh("grid_40x130")
        return v, faces[:int(name[5:])]
    data = np.load(os.path.join(GOLDEN, name + ".npz"))
    return data["vertices"].astype(np.float64), data["faces"]


@functools.lru_cache(maxsize=None)
def sided_cloud(name, k):
    """``((B,P,3) float64 that is exact in fp32, kind (B,P))``, P = SIZES[k]: built as ``cloud(name, k)`` builds its
    points, without the kinds that lie on the surface: surface samples pushed along the face normal by PUSH[kind] of
    the mesh's extent (kinds 0 to 3), and points at 10 x the extent (kind 4)"""
    v, faces = winding_mesh(name)
    size = extent(v)
    rng = np.random.default_rng(300 + k)
    p = SIZES[k]
    out, kinds = np.empty((v.shape[0], p, 3)), np.empty((v.shape[0], p), np.int64)
    for b in range(v.shape[0]):
        tri = v[b][faces_of(faces, b)]                                         # (F, 3, 3)
        kind = rng.integers(0, 5, size=p)
        f = rng.choice(np.nonzero(has_area(v[b], faces_of(faces, b)))[0], size=p)   # (a face without area has no side)
        w = rng.dirichlet((1.0, 1.0, 1.0), size=p)
        normal = np.cross(tri[f, 1] - tri[f, 0], tri[f, 2] - tri[f, 0])
        normal /= np.maximum(np.linalg.norm(normal, axis=1, keepdims=True), 1e-30)
        pts = (w[:, :, None] * tri[f]).sum(1) + (PUSH[kind] * size)[:, None] * normal
        far = rng.normal(size=(p, 3))
        far *= 10 * size / np.linalg.norm(far, axis=1, keepdims=True)
        pts[kind == 4] = far[kind == 4]
        out[b], kinds[b] = pts, kind
    return out.astype(F32).astype(np.float64), kinds


@functools.lru_cache(maxsize=None)
def surface_cloud(name):
    """(B,96,3) on the surface itself: surface samples, copies of vertices and edge midpoints"""
    v, faces = winding_mesh(name)
    rng = np.random.default_rng(310)
    p = 96
    out = np.empty((v.shape[0], p, 3))
    for b in range(v.shape[0]):
        tri = v[b][faces_of(faces, b)]
        kind = rng.integers(0, 3, size=p)
        f, j = rng.integers(0, tri.shape[0], size=p), rng.integers(0, 3, size=p)
        pts = (rng.dirichlet((1.0, 1.0, 1.0), size=p)[:, :, None] * tri[f]).sum(1)
        pts[kind == 1] = tri[f, j][kind == 1]
        pts[kind == 2] = (0.5 * (tri[f, j] + tri[f, (j + 1) % 3]))[kind == 2]
        out[b] = pts
    return out.astype(F32).astype(np.float64)


def host_corners(name):
    v, faces = winding_mesh(name)
    return corners_of(faces, v.shape[1])


@functools.lru_cache(maxsize=None)
def winding64(name, k):
    """the fp64 CPU composition on ``sided_cloud(name, k)``, computed once: the reference of both test files"""
    v, _ = winding_mesh(name)
    return mesh_winding.winding_composition(torch.from_numpy(sided_cloud(name, k)[0]), torch.from_numpy(v),
                                            host_corners(name))


@functools.lru_cache(maxsize=None)
def winding32(name, k):
    v, _ = winding_mesh(name)
    return mesh_winding.winding_composition(torch.from_numpy(sided_cloud(name, k)[0].astype(F32)),
                                            torch.from_numpy(v.astype(F32)), host_corners(name))


@functools.lru_cache(maxsize=None)
def signed32(name, k):
    """the fp32 CPU ``signed_distance_composition`` on ``sided_cloud(name, k)``"""
    v, _ = winding_mesh(name)
    return mesh_winding.signed_distance_composition(torch.from_numpy(sided_cloud(name, k)[0].astype(F32)),
                                                    torch.from_numpy(v.astype(F32)), host_corners(name))


# --------------------------------------------------------------------------------------------- the brute force
def np_cross(m, n):
    """the cross product of two triples of component arrays"""
    return m[1] * n[2] - m[2] * n[1], m[2] * n[0] - m[0] * n[2], m[0] * n[1] - m[1] * n[0]


def np_dot(m, n):
    return m[0] * n[0] + m[1] * n[1] + m[2] * n[2]


def np_angle(m, n):
    """the angle between the vectors m and n, triples of component arrays"""
    x = np_cross(m, n)
    return np.arctan2(np.sqrt(np_dot(x, x)), np_dot(m, n))


def np_winding(points, tri):
    """fp64 (P,): every triangle is projected on the unit sphere about the point, its solid angle is the spherical
    excess A + B + C - pi of the projected triangle's three angles (Girard), each the angle between the planes of the
    two great circles that meet at the corner, and its sign is that of det(a - p, b - p, c - p); a triangle without
    area takes no part, one seen edge on (a determinant of 0) adds nothing."""
    tri = tri[(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]) ** 2).sum(-1) > 0]
    unit = []
    for corner in range(3):
        rel = [tri[None, :, corner, d] - points[:, None, d] for d in range(3)]    # components (P, F)
        length = np.sqrt(np_dot(rel, rel))
        unit.append([x / length for x in rel])
    a, b, c = unit
    ab, bc, ca = np_cross(a, b), np_cross(b, c), np_cross(c, a)                     # the planes' normals
    flip = lambda n: [-x for x in n]   # noqa: E731
    total = np_angle(ab, flip(ca)) + np_angle(bc, flip(ab)) + np_angle(ca, flip(bc))
    sign = np.sign(np_dot(a, bc))
    return (np.where(sign != 0, sign * (total - np.pi), 0.0)).sum(1) / (4 * np.pi)


# ------------------------------------------------------------------------------------------- symbols and names
def test_symbols_are_declared_exported_and_bound():
    declared = declared_symbols()
    _build.build()
    handle = ctypes.CDLL(_build.LIB)
    for name in ENTRIES:
        assert name in declared and hasattr(handle, name) and name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["pp_mesh_winding_forward_f32"]) == 7
    assert len(_lib.SIGNATURES["pp_mesh_signed_distance_forward_f32"]) == 10


def test_entries_check_their_sizes_before_any_launch():
    """PP_OK (0) for an empty problem and PP_EINVAL (1) for sizes that cannot be served: decided on the host"""
    lib = _lib.lib()
    for entry, pointers in ((lib.pp_mesh_winding_forward_f32, 3), (lib.pp_mesh_signed_distance_forward_f32, 6)):
        for b, p, f in ((0, 5, 5), (2, 0, 5), (2, 5, 0)):
            assert entry(*(None,) * pointers, b, p, f, None) == 0
        for b, p, f in ((-1, 5, 5), (2, -1, 5), (2, 5, -1), (2, 2 ** 30, 5), (2, 5, 2 ** 30), (1, 5, 2 ** 30), (2, 5, 5)):
            assert entry(*(None,) * pointers, b, p, f, None) == 1


def test_names_are_reexported():
    from pytorch_points.network.geo_operations import point_mesh_signed_distance  # noqa: F401
    from pytorch_points.network.model_loss import MeshEnclosureLoss
    assert issubclass(MeshEnclosureLoss, torch.nn.Module)
    assert MeshEnclosureLoss is model_loss.MeshEnclosureLoss is mesh_winding.MeshEnclosureLoss
    for name in ("mesh_winding_number", "points_inside_mesh", "point_mesh_signed_distance", "PointMeshSignedDistance"):
        assert getattr(geo_operations, name) is getattr(mesh_winding, name)
    assert hasattr(mesh_winding, "winding_composition") and hasattr(mesh_winding, "signed_distance_composition")
    assert mesh_winding.PointMeshSignedDistance._fields == ("signed", "dist", "face", "bary", "winding")


# ----------------------------------------------------------------------------------------- against brute force
# The largest |fp64 composition - fp64 brute force| over every point of the four clouds, as measured here (printed again by the
# test below).  The two differ in everything but the input: an atan2 of a triple product against a sum of three angles
# between planes, so the difference is both roundings', and the bound is 4 x the figure, never below 1e-12 (a few
# thousand fp64 roundings of terms of size 1).
BRUTE_MEASURED = {
    "cage": 4.45e-15, "grid_40x130": 1.04e-13, "fan_300": 1.87e-14, "two_topologies": 4.77e-15, "soup": 4.66e-14,
    "gc_star": 9.88e-15, "gc_cube": 6.33e-15,
}


@pytest.mark.parametrize("name", NAMES)
def test_fp64_composition_against_the_fp64_brute_force(name):
    v, faces = winding_mesh(name)
    worst = 0.0
    for k, p in enumerate(SIZES):
        got = winding64(name, k)
        assert got.shape == (v.shape[0], p) and got.dtype == torch.float64
        pts = sided_cloud(name, k)[0]
        for b in range(v.shape[0]):
            tri = v[b][faces_of(faces, b)]
            want = np.concatenate([np_winding(pts[b][i:i + 64], tri) for i in range(0, p, 64)])   # (blocks: memory)
            worst = max(worst, float(np.abs(got[b].numpy() - want).max()))
    print("%s: |fp64 composition - fp64 brute force| %.3g (pinned %.3g)" % (name, worst, BRUTE_MEASURED[name]))
    assert worst <= 4 * max(BRUTE_MEASURED[name], 1e-12), worst


# --------------------------------------------------------------------------------------------- every point's side
# The largest |winding - round(winding)| on the closed meshes over the four sided clouds: (fp64, fp32) compositions, as
# measured here.  The fp64 bound is 4 x the figure, never below 1e-12; the fp32 bound 4 x the figure, never below 16
# eps32: the bound that the GPU test sets on HIP against fp64.
SIDE_MEASURED = {"cage": (2e-15, 1.31e-06), "gc_star": (9.44e-15, 5.48e-06), "gc_cube": (6.4e-15, 4.65e-06)}


@pytest.mark.parametrize("name", CLOSED)
def test_every_point_of_a_closed_mesh_has_a_side(name):
    worst = [0.0, 0.0]
    for k in range(len(SIZES)):
        kind = sided_cloud(name, k)[1]
        for slot, w in enumerate((winding64(name, k), winding32(name, k).double())):
            side = torch.round(w)
            assert bool(((side == 0) | (side == 1)).all()), name                # no point is left out
            worst[slot] = max(worst[slot], float((w - side).abs().max()))
            inside = (w > 0.5).numpy()
            assert (inside == (side.numpy() == 1)).all()
            assert not inside[kind == 4].any()                                   # the far points
            if name != "gc_star":                                                # convex: the push's sign is the side
                assert inside[kind == 1].all() and not inside[kind == 0].any()
                assert inside[kind == 3].all() and not inside[kind == 2].any()
    print("%s: |winding - round(winding)|: fp64 %.3g, fp32 %.3g (pinned %s)" % (name, worst[0], worst[1],
                                                                               SIDE_MEASURED[name]))
    assert worst[0] <= 4 * max(SIDE_MEASURED[name][0], 1e-12) and worst[1] <= 4 * max(SIDE_MEASURED[name][1], 16 * EPS32)


# ------------------------------------------------------------------------------------------------ known answers
def test_known_answers():
    v, faces = winding_mesh("gc_cube")
    x, tf = torch.from_numpy(v), torch.from_numpy(faces)
    centre = torch.zeros(1, 1, 3, dtype=torch.float64)
    assert abs(float(mesh_winding.mesh_winding_number(centre, x, tf)) - 1.0) <= 1e-15
    for f in range(12):                                                        # by symmetry, 1/12 per triangle
        assert abs(float(mesh_winding.mesh_winding_number(centre, x, tf[:, f:f + 1])) - 1 / 12) <= 1e-15
    # one equilateral triangle from above its centroid: the apex of a regular pyramid, whose solid angle is 3 theta - pi
    # with theta the dihedral angle between two neighbouring side planes
    r, h = 2.0, 0.75
    corners = np.array([[r * math.cos(t), r * math.sin(t), 0.0] for t in (0.0, 2 * math.pi / 3, 4 * math.pi / 3)])
    apex = np.array([0.0, 0.0, h])
    n1, n2 = np.cross(corners[0] - apex, corners[1] - apex), np.cross(corners[1] - apex, corners[2] - apex)
    theta = math.pi - math.acos(float(n1 @ n2) / float(np.linalg.norm(n1) * np.linalg.norm(n2)))
    omega = 3 * theta - math.pi
    tri = torch.from_numpy(corners)[None]
    one = torch.tensor([[0, 1, 2]])
    above = mesh_winding.mesh_winding_number(torch.from_numpy(apex)[None, None], tri, one)
    below = mesh_winding.mesh_winding_number(torch.from_numpy(-apex)[None, None], tri, one)
    assert abs(float(above) + omega / (4 * math.pi)) <= 1e-15                  # counter-clockwise from above: outside
    assert abs(float(below) - omega / (4 * math.pi)) <= 1e-15
    for dtype in (torch.float64, torch.float32):
        name, k = "cage", 2
        v, faces = winding_mesh(name)
        x, pts = torch.from_numpy(v).to(dtype), torch.from_numpy(sided_cloud(name, k)[0]).to(dtype)
        plain = mesh_winding.mesh_winding_number(pts, x, torch.from_numpy(faces))
        assert plain.dtype == dtype
        assert torch.equal(plain, (winding64 if dtype == torch.float64 else winding32)(name, k))
        flipped = mesh_winding.mesh_winding_number(pts, x, torch.from_numpy(faces[:, ::-1].copy()))
        assert float((flipped + plain).abs().max()) <= (1e-14 if dtype == torch.float64 else 4 * fp32_bound(name, k))
        twice = mesh_winding.mesh_winding_number(pts, x, torch.from_numpy(np.concatenate([faces, faces])))
        assert float((twice - 2 * plain).abs().max()) <= (1e-14 if dtype == torch.float64 else 16 * EPS32)
        host = corners_of(faces, v.shape[1])
        bad = np.concatenate([faces, [[0, 1, v.shape[1]], [-1, 2, 3]]])
        beyond = MeshCorners(torch.from_numpy(bad)[None], host.start, host.codes, host.nbr, v.shape[1])
        assert torch.equal(mesh_winding.winding_composition(pts, x, beyond), plain)   # an invalid face adds nothing
    inside = mesh_winding.points_inside_mesh(pts, x, torch.from_numpy(faces))
    assert inside.dtype == torch.bool and torch.equal(inside, plain > 0.5) and bool(inside.any()) and not bool(inside.all())


def test_nan_points_and_empty_meshes():
    v, faces = winding_mesh("gc_cube")
    x, tf = torch.from_numpy(v.astype(F32)), torch.from_numpy(faces)
    pts = torch.tensor([[[0.0, 0.0, 0.0], [float("nan"), 0.0, 0.0]]])
    w = mesh_winding.mesh_winding_number(pts, x, tf)
    assert float(w[0, 0]) == 1.0 and bool(torch.isnan(w[0, 1]))
    assert mesh_winding.points_inside_mesh(pts, x, tf).tolist() == [[True, False]]
    none = corners_of(np.zeros((0, 3), np.int64), 8)
    assert mesh_winding.mesh_winding_number(pts, x, none).tolist() == [[0.0, 0.0]]
    out = mesh_winding.point_mesh_signed_distance(pts, x, none)
    assert out.winding.tolist() == [[0.0, 0.0]] and bool((out.face == -1).all()) and bool(torch.isnan(out.signed).all())
    assert mesh_winding.mesh_winding_number(torch.zeros(1, 0, 3), x, tf).shape == (1, 0)
    assert not w.requires_grad
    w = mesh_winding.mesh_winding_number(pts.clone().requires_grad_(True), x.clone().requires_grad_(True), tf)
    assert not w.requires_grad


@pytest.mark.parametrize("name", NAMES)
def test_the_surface_itself_is_finite(name):
    v, _ = winding_mesh(name)
    for dtype in (torch.float32, torch.float64):
        w = mesh_winding.winding_composition(torch.from_numpy(surface_cloud(name)).to(dtype),
                                             torch.from_numpy(v).to(dtype), host_corners(name))
        assert bool(torch.isfinite(w).all())


# ------------------------------------------------------------------------------------------------ fp32 and fp64
# The largest |w32 - w64| of the fp32 CPU composition against the fp64 one, per mesh and for each of the four sided
# clouds (P = 1, 63, 65, 1000), as measured here (printed again by the test below).  tests/test_gpu_mesh_winding.py
# bounds HIP against fp64 by 4 x max(figure, 16 eps32); here the fp32 CPU composition itself is held to 2 x that
# maximum: another CPU's vectorised atan2 and sqrt may differ from this one's in their last bits.
CPU_MEASURED = {
    "cage": (9.71e-09, 7.15e-07, 1.31e-06, 1.05e-06),
    "grid_40x130": (2.65e-07, 5.38e-07, 5.98e-07, 1.02e-06),
    "fan_300": (5.42e-07, 2.76e-06, 2.12e-06, 1.33e-05),
    "two_topologies": (5.06e-08, 4.77e-07, 8.94e-07, 1.8e-06),
    "soup": (6.7e-08, 9.13e-07, 9.09e-06, 1.06e-05),
    "gc_star": (1.26e-07, 1.7e-07, 5.25e-06, 5.48e-06),
    "gc_cube": (5.05e-08, 1.19e-07, 1.73e-06, 4.65e-06),
    "grid_255": (1.51e-08, 5.44e-07, 4.87e-07, 6.71e-07),
    "grid_256": (2.38e-08, 6.97e-07, 5.49e-07, 6.45e-07),
    "grid_257": (1.37e-08, 7.07e-07, 5.53e-07, 6.58e-07),
}


def fp32_bound(name, k):
    return max(CPU_MEASURED[name][k], 16 * EPS32)


@pytest.mark.parametrize("name", NAMES + TILE)
def test_fp32_composition_against_the_fp64_composition(name):
    got = [float((winding32(name, k).double() - winding64(name, k)).abs().max()) for k in range(len(SIZES))]
    print("%s: |w32 - w64| %s (pinned %s)" % (name, ", ".join("%.3g" % e for e in got), CPU_MEASURED[name]))
    assert winding32(name, 3).dtype == torch.float32
    assert all(e <= 2 * fp32_bound(name, k) for k, e in enumerate(got)), got


def test_blocks_of_the_pair_matrix_change_nothing(monkeypatch):
    v, faces = winding_mesh("two_topologies")
    want = winding32("two_topologies", 3)
    monkeypatch.setattr(mesh_winding, "CHUNK_PAIRS", 7 * 2 * faces.shape[1])     # blocks of seven points
    again = mesh_winding.winding_composition(torch.from_numpy(sided_cloud("two_topologies", 3)[0].astype(F32)),
                                             torch.from_numpy(v.astype(F32)), host_corners("two_topologies"))
    assert again.numpy().tobytes() == want.numpy().tobytes()


# -------------------------------------------------------------------------------------------- the signed distance
@pytest.mark.parametrize("name", NAMES)
def test_signed_distance_is_the_distance_with_the_winding_numbers_sign(name):
    v, _ = winding_mesh(name)
    x, corners = torch.from_numpy(v.astype(F32)), host_corners(name)
    for k in (1, 3):
        pts = torch.from_numpy(sided_cloud(name, k)[0].astype(F32))
        out = signed32(name, k)
        assert out._fields == ("signed", "dist", "face", "bary", "winding")
        want = mesh_distance.distance_composition(pts, x, corners, face_point=False)[0]
        for a, b in zip((out.dist, out.face, out.bary), want):
            assert a.dtype == b.dtype and a.numpy().tobytes() == b.numpy().tobytes()
        assert out.winding.numpy().tobytes() == winding32(name, k).numpy().tobytes()
        assert bool((out.face >= 0).all())
        inside = out.winding > 0.5
        assert torch.equal(out.signed, torch.where(inside, -out.dist.sqrt(), out.dist.sqrt()))
        if name in CLOSED:
            assert bool((out.signed[inside] < 0).all()) and bool((out.signed[~inside] > 0).all())
            assert bool(inside.any()) or k == 1
    public = mesh_winding.point_mesh_signed_distance(pts, x, corners)
    assert all(a.numpy().tobytes() == b.numpy().tobytes() for a, b in zip(public, out))


def test_signed_is_zero_with_a_zero_gradient_on_the_surface():
    v, faces = winding_mesh("gc_cube")
    x = torch.from_numpy(v.astype(F32)).requires_grad_(True)
    pts = torch.cat([torch.from_numpy(v.astype(F32))[:, :4], torch.tensor([[[0.25, 0.5, 0.0], [3.0, 0.5, 0.0]]])], 1)
    pts.requires_grad_(True)
    out = mesh_winding.point_mesh_signed_distance(pts, x, torch.from_numpy(faces))
    assert out.dist[0, :4].tolist() == [0.0] * 4 and out.signed[0, :4].tolist() == [0.0] * 4
    assert out.signed[0, 4:].tolist() == [-0.5, 2.0]
    assert not out.winding.requires_grad and not out.face.requires_grad and not out.bary.requires_grad
    for k in range(6):
        g_p, g_x = torch.autograd.grad(out.signed[0, k], (pts, x), retain_graph=True)
        assert bool(torch.isfinite(g_p).all()) and bool(torch.isfinite(g_x).all())
        assert bool((g_p != 0).any()) == (k >= 4) and bool((g_x != 0).any()) == (k >= 4)
    g_p, = torch.autograd.grad(out.signed.sum(), pts)
    assert g_p[0, 4:].tolist() == [[0.0, 1.0, 0.0], [1.0, 0.0, 0.0]]       # inside under the face y = 1; outside x = 1


def test_gradients_of_the_signed_distance_by_gradcheck():
    """fp64, the jittered octahedron of the distances' gradcheck with a point over the inside of every face, outside
    by 0.1 and inside by 0.1: the runner-up of every choice is farther than the winner by a margin that the finite
    differences (1e-6) cannot bridge, and no point is near the surface, where the sign switches."""
    rng = np.random.default_rng(41)
    v = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float64)
    v = v + rng.uniform(-0.05, 0.05, size=v.shape)
    faces = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]])
    tri = v[faces]
    w = rng.dirichlet((4.0, 4.0, 4.0), size=8)
    centre = (w[:, :, None] * tri).sum(1)
    normal = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    normal /= np.linalg.norm(normal, axis=1, keepdims=True)
    assert ((normal * centre).sum(1) > 0).all()                                # outwards
    pts = np.concatenate([centre + 0.1 * normal, centre - 0.1 * normal])
    ranked = np.sort(np_all_pairs(pts, tri), axis=1)
    assert (ranked[:, 1] - ranked[:, 0] > 1e-3).all()
    corners = corners_of(faces, 6)
    p, x = torch.from_numpy(pts)[None].requires_grad_(True), torch.from_numpy(v)[None].requires_grad_(True)
    out = mesh_winding.point_mesh_signed_distance(p, x, corners)
    assert bool((out.signed[0, :8] > 0).all()) and bool((out.signed[0, 8:] < 0).all())
    assert float((out.signed.detach().abs() - 0.1).abs().max()) <= 1e-12
    assert torch.autograd.gradcheck(lambda a, b: mesh_winding.point_mesh_signed_distance(a, b, corners).signed, (p, x),
                                    eps=1e-6, atol=1e-6)


@pytest.mark.parametrize("case", ["no faces", "a collapsed edge", "NaN points", "a vertex index out of range"])
def test_an_item_without_a_face_is_nan_and_passes_no_gradient(case):
    pts, x, corners = unusable_cases()[case]
    pts, x = pts.clone().requires_grad_(True), x.clone().requires_grad_(True)
    out = mesh_winding.point_mesh_signed_distance(pts, x, corners)
    assert bool((out.face == -1).all()) and bool(torch.isnan(out.signed).all()) and bool(torch.isnan(out.dist).all())
    g_p, g_x = torch.autograd.grad(out.signed.sum() + out.dist.sum(), (pts, x))
    assert bool((g_p == 0).all()) and bool((g_x == 0).all())
    loss = model_loss.MeshEnclosureLoss("outside", margin=0.5)
    loss.E, loss.consistent_topology = corners, True
    value = loss(pts, x)
    assert float(value.detach()) == 0.0                                                 # left out of the numerator
    g_p, g_x = torch.autograd.grad(value, (pts, x))
    assert bool((g_p == 0).all()) and bool((g_x == 0).all())


# ------------------------------------------------------------------------------------------------------- the loss
def test_the_loss_on_both_sides_and_its_kept_topology():
    v, faces = winding_mesh("cage")
    x = torch.from_numpy(v).requires_grad_(True)
    pts = torch.from_numpy(sided_cloud("cage", 3)[0]).requires_grad_(True)
    tf = torch.from_numpy(faces)
    out = mesh_winding.point_mesh_signed_distance(pts, x, tf)
    inside = out.winding > 0.5
    assert bool(inside.any()) and bool((~inside).any())
    zero = torch.zeros_like(out.dist)
    for side, wrong in (("inside", ~inside), ("outside", inside)):
        kept = model_loss.MeshEnclosureLoss(side, consistent_topology=True)
        fresh = model_loss.MeshEnclosureLoss(side)
        first = kept(pts, x, tf)
        topology = kept.E
        assert isinstance(topology, MeshCorners)
        again = kept(pts, x)
        assert kept.E is topology and torch.equal(first, again) and torch.equal(first, fresh(pts, x, tf))
        assert fresh.E is not topology
        want = torch.where(wrong, out.dist, zero).mean()                       # margin = 0: the masked dist mean
        assert float(first) > 0 and abs(float(first - want)) <= 4 * 2.0 ** -52 * float(want)
        g_p, g_x = torch.autograd.grad(first, (pts, x))
        assert bool(torch.isfinite(g_p).all()) and bool(torch.isfinite(g_x).all()) and bool((g_x != 0).any())
        assert bool((g_p[wrong] != 0).any()) and bool((g_p[~wrong] == 0).all())
        margin = model_loss.MeshEnclosureLoss(side, margin=0.05)(pts, x, tf)
        s = out.signed if side == "inside" else -out.signed
        assert abs(float(margin - (torch.relu(s + 0.05) ** 2).mean())) <= 1e-15 and float(margin) > float(first)
    with pytest.raises(AssertionError, match="Face is required"):
        model_loss.MeshEnclosureLoss()(pts, x)
    with pytest.raises(ValueError, match="side must be"):
        model_loss.MeshEnclosureLoss("above")


# ------------------------------------------------------------------------------------------- the API and errors
def test_argument_errors():
    v, faces = winding_mesh("cage")
    x = torch.from_numpy(v.astype(F32))
    corners = corners_of(faces, x.shape[1])
    pts = torch.from_numpy(sided_cloud("cage", 1)[0].astype(F32))
    for function in (mesh_winding.mesh_winding_number, mesh_winding.points_inside_mesh,
                     mesh_winding.point_mesh_signed_distance):
        with pytest.raises(NotImplementedError, match="triangles only, got faces of 4 corners"):
            function(pts, x, corners_of(np.zeros((5, 4), np.int64), x.shape[1]))
        with pytest.raises(TypeError, match="faces_or_corners"):
            function(pts, x, [1, 2, 3])
        with pytest.raises(TypeError, match="points must be a floating tensor"):
            function(pts.long(), x, corners)
        with pytest.raises(TypeError, match="points are torch.float64 but vertices are torch.float32"):
            function(pts.double(), x, corners)
        with pytest.raises(ValueError, match="points must have shape"):
            function(pts[:2], x, corners)
        with pytest.raises(ValueError, match="built for 162 vertices"):
            function(pts, x[:, :100], corners)
        with pytest.raises(IndexError, match="batch element 0"):
            function(pts, x, torch.tensor([[0, 1, 162]]))
