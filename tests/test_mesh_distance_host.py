"""CPU tests (no GPU) of the point-to-mesh distances (pytorch_points_amd/mesh_distance.py and its names in
network/geo_operations.py and network/model_loss.py) through ``distance_composition``: against a numpy fp64 brute
force written independently of the region walk, on ties, on inputs with known answers, on items left without a
partner, by ``gradcheck`` and on argument errors.  The clouds and the references here also serve
tests/test_gpu_mesh_distance.py."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from pytorch_points_amd import _build, _lib, mesh_distance
from pytorch_points_amd.mesh_laplacian import MeshCorners
from pytorch_points_amd.network import geo_operations, model_loss
from test_abi_and_host import declared_symbols
from test_mesh_sample_host import MESHES, corners_of, faces_of, mesh

F32 = np.float32
EPS32 = 2.0 ** -23
SIZES = [1, 63, 65, 1000]
ENTRIES = ["pp_mesh_distance_records_f32", "pp_mesh_point_face_forward_f32", "pp_mesh_face_point_forward_f32",
           "pp_mesh_distance_backward_f32"]


# --------------------------------------------------------------------------------------------------- the inputs
def extent(v):
    return float((v.reshape(-1, 3).max(0) - v.reshape(-1, 3).min(0)).max())


@functools.lru_cache(maxsize=None)
def cloud(name, k):
    """(B,P,3) float64 that is exact in fp32, P = SIZES[k]: surface samples pushed along +- the face normal by 0, 1e-3
    and 0.3 of the mesh's extent, copies of vertices, edge midpoints, and points at 10 x the extent"""
    v, faces = mesh(name)
    size = extent(v)
    rng = np.random.default_rng(200 + k)
    p = SIZES[k]
    out = np.empty((v.shape[0], p, 3))
    for b in range(v.shape[0]):
        tri = v[b][faces_of(faces, b)]                                         # (F, 3, 3)
        kind = rng.integers(0, 6, size=p)
        f = rng.integers(0, tri.shape[0], size=p)
        w = rng.dirichlet((1.0, 1.0, 1.0), size=p)
        normal = np.cross(tri[f, 1] - tri[f, 0], tri[f, 2] - tri[f, 0])
        normal /= np.maximum(np.linalg.norm(normal, axis=1, keepdims=True), 1e-30)
        push = np.array([0.0, 1e-3, 0.3, 0.0, 0.0, 0.0])[kind] * size * rng.choice([-1.0, 1.0], size=p)
        pts = (w[:, :, None] * tri[f]).sum(1) + push[:, None] * normal
        j = rng.integers(0, 3, size=p)
        pts[kind == 3] = tri[f, j][kind == 3]
        pts[kind == 4] = (0.5 * (tri[f, j] + tri[f, (j + 1) % 3]))[kind == 4]
        far = rng.normal(size=(p, 3))
        far *= 10 * size / np.linalg.norm(far, axis=1, keepdims=True)
        pts[kind == 5] = far[kind == 5]
        out[b] = pts
    return out.astype(F32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def repeated_cloud(name):
    """the cloud of 1000 points with its first 32 repeated at the end: ties between points"""
    pts = cloud(name, 3)
    return np.concatenate([pts, pts[:, :32]], axis=1)


@functools.lru_cache(maxsize=None)
def tie_mesh():
    """the grid with every face row listed twice: the copies fall in different tiles"""
    v, faces = mesh("grid_40x130")
    assert faces.ndim == 2
    return v, np.concatenate([faces, faces], axis=0)


@functools.lru_cache(maxsize=None)
def composed(name, k):
    """the fp32 CPU composition on ``cloud(name, k)`` (k = "repeated": on ``repeated_cloud``), computed once"""
    v, faces = mesh(name)
    pts = repeated_cloud(name) if k == "repeated" else cloud(name, k)
    return mesh_distance.distance_composition(torch.from_numpy(pts.astype(F32)), torch.from_numpy(v.astype(F32)),
                                              corners_of(faces, v.shape[1]))


@functools.lru_cache(maxsize=None)
def composed_ties():
    v, faces = tie_mesh()
    return mesh_distance.distance_composition(torch.from_numpy(cloud("grid_40x130", 2).astype(F32)),
                                              torch.from_numpy(v.astype(F32)), corners_of(faces, v.shape[1]))


# --------------------------------------------------------------------------------------------- the brute force
def np_segment(p, u, w):
    """fp64 squared distance of the points p to the segments u-w (broadcast): the projection's parameter clamped"""
    e = w - u
    t = ((p - u) * e).sum(-1) / np.maximum((e * e).sum(-1), 1e-300)
    r = p - (u + np.clip(t, 0.0, 1.0)[..., None] * e)
    return (r * r).sum(-1)


def np_pair(p, a, b, c):
    """fp64 squared distances of the points p (...,3) to the triangles a, b, c (...,3), broadcast: the distance to
    the plane where the foot of the perpendicular lies inside the triangle, and the three segments (their ends are
    the vertices), minimum of all.  A triangle without area has its segments only."""
    d = np.minimum(np.minimum(np_segment(p, a, b), np_segment(p, b, c)), np_segment(p, c, a))
    n = np.cross(b - a, c - a)
    nn = (n * n).sum(-1)
    has = nn > 0
    height = ((p - a) * n).sum(-1) / np.where(has, nn, 1.0)
    foot = p - height[..., None] * n
    inside = has
    for u, w in ((a, b), (b, c), (c, a)):
        inside = inside & ((np.cross(w - u, foot - u) * n).sum(-1) >= 0)
    return np.where(inside, np.minimum(d, height * height * nn), d)


def np_all_pairs(points, tri):
    """(P,F): every pair"""
    return np_pair(points[:, None, :], tri[None, :, 0], tri[None, :, 1], tri[None, :, 2])


def np_minima(points, tri):
    """fp64: ``(the minimum over the triangles for every point (P), the minimum over the points for every triangle
    (F))`` of ``np_pair``.  A pair is evaluated unless it cannot be either minimum: its distance is at least (|p -
    centroid| - the triangle's radius about its centroid)^2 and at most |p - centroid|^2, the centroid being a point
    of the triangle, so a pair whose lower bound is beyond the smallest upper bound of both its row and its column
    is left out."""
    centre = tri.mean(1)
    radius = np.linalg.norm(tri - centre[:, None], axis=2).max(1)
    gap = np.concatenate([np.linalg.norm(points[i:i + 128, None] - centre[None], axis=2)
                          for i in range(0, points.shape[0], 128)], axis=0)
    lower, upper = np.maximum(gap - radius, 0.0) ** 2 * (1 - 1e-9), gap ** 2
    i, j = np.nonzero((lower <= upper.min(1, keepdims=True)) | (lower <= upper.min(0, keepdims=True)))
    d = np_pair(points[i], tri[j, 0], tri[j, 1], tri[j, 2])
    per_point, per_face = np.full(points.shape[0], np.inf), np.full(tri.shape[0], np.inf)
    np.minimum.at(per_point, i, d)
    np.minimum.at(per_face, j, d)
    return per_point, per_face


def has_area(v, faces):
    tri = v[faces]
    return (np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]) ** 2).sum(-1) > 0


def np_at(points, tri, bary):
    """fp64 squared distance of points (S,3) to the points ``bary`` (S,3) of triangles (S,3,3)"""
    r = points - (bary[:, :, None] * tri).sum(1)
    return (r * r).sum(-1)


def excess(name, k, pf, fp):
    """The largest amount by which the fp64 distance at the chosen ``(index, bary)`` exceeds the fp64 minimum over
    all partners, in units of ``(largest |coordinate difference|)^2 eps32``: ``(point -> face, face -> point)``.
    Faces without area take no part on the triangles' side: the walk does not promise its answer on them."""
    v, faces = mesh(name)
    pts = cloud(name, k)
    worst = [0.0, 0.0]
    for b in range(v.shape[0]):
        fb = faces_of(faces, b)
        keep = has_area(v[b], fb)
        tri = v[b][fb]
        unit = np.abs(pts[b][:, None, :] - v[b][None, :, :]).max() ** 2 * EPS32
        per_point, per_face = np_minima(pts[b], tri[keep])
        face, bary = pf.face[b].numpy(), pf.bary[b].double().numpy()
        assert (face >= 0).all() and (face < fb.shape[0]).all()
        got = np_at(pts[b], tri[face], bary)
        worst[0] = max(worst[0], float((got - per_point).max() / unit))
        point, bary = fp.point[b].numpy()[keep], fp.bary[b].double().numpy()[keep]
        assert (point >= 0).all() and (point < pts.shape[1]).all()
        got = np_at(pts[b][point], tri[keep], bary)
        worst[1] = max(worst[1], float((got - per_face).max() / unit))
    return worst


# ------------------------------------------------------------------------------------------- symbols and names
def test_symbols_are_declared_exported_and_bound():
    declared = declared_symbols()
    _build.build()
    handle = ctypes.CDLL(_build.LIB)
    for name in ENTRIES:
        assert name in declared and hasattr(handle, name) and name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["pp_mesh_distance_records_f32"]) == 8
    assert len(_lib.SIGNATURES["pp_mesh_point_face_forward_f32"]) == 9
    assert len(_lib.SIGNATURES["pp_mesh_face_point_forward_f32"]) == 9
    assert len(_lib.SIGNATURES["pp_mesh_distance_backward_f32"]) == 19


def test_entries_check_their_sizes_before_any_launch():
    """PP_OK (0) for an empty problem and PP_EINVAL (1) for sizes that cannot be served: decided on the host"""
    lib = _lib.lib()
    for b, n, f in ((0, 5, 5), (2, 0, 5), (2, 5, 0)):
        assert lib.pp_mesh_distance_records_f32(None, None, None, b, n, f, 0, None) == 0
    for b, n, f in ((-1, 5, 5), (2, -1, 5), (2, 5, -1), (2, 2 ** 30, 5), (2, 5, 2 ** 30), (2, 5, 5)):
        assert lib.pp_mesh_distance_records_f32(None, None, None, b, n, f, 0, None) == 1
    for entry in (lib.pp_mesh_point_face_forward_f32, lib.pp_mesh_face_point_forward_f32):
        for b, p, f in ((0, 5, 5), (2, 0, 5), (2, 5, 0)):
            assert entry(*(None,) * 5, b, p, f, None) == 0
        for b, p, f in ((-1, 5, 5), (2, -1, 5), (2, 5, -1), (2, 2 ** 30, 5), (2, 5, 2 ** 30), (1, 5, 2 ** 30), (2, 5, 5)):
            assert entry(*(None,) * 5, b, p, f, None) == 1
    for b, n, f, p in ((0, 5, 5, 5), (2, 0, 5, 5), (2, 5, 0, 5), (2, 5, 5, 0)):
        assert lib.pp_mesh_distance_backward_f32(*(None,) * 11, b, n, f, p, 0, None, 0, None) == 0
    for b, n, f, p in ((-1, 5, 5, 5), (2, -1, 5, 5), (2, 5, -1, 5), (2, 5, 5, -1), (2, 5, 5, 2 ** 30), (2, 5, 5, 5)):
        assert lib.pp_mesh_distance_backward_f32(*(None,) * 11, b, n, f, p, 0, None, 0, None) == 1


def test_names_are_reexported():
    from pytorch_points.network.geo_operations import point_face_distance  # noqa: F401
    from pytorch_points.network.model_loss import PointMeshDistanceLoss
    assert issubclass(PointMeshDistanceLoss, torch.nn.Module)
    assert PointMeshDistanceLoss is model_loss.PointMeshDistanceLoss is mesh_distance.PointMeshDistanceLoss
    for name in ("point_face_distance", "face_point_distance"):
        assert getattr(geo_operations, name) is getattr(mesh_distance, name)
    assert hasattr(mesh_distance, "distance_composition")


# ----------------------------------------------------------------------------------------- against brute force
# The largest excess of the fp32 CPU composition over the fp64 brute-force minimum, in units of (largest |coordinate
# difference|)^2 eps32, over the four cloud sizes: (point -> face, face -> point), as measured (printed again by the
# test below).  A figure below 4 stands as 4: the residual's three subtractions, squares and two sums alone may err by
# that much of the unit, and another CPU's torch build may measure less.
CPU_MEASURED = {
    "cage": (0.0245, 0.29),
    "grid_40x130": (0.0001, 0.661),
    "fan_300": (0.0158, 0.000126),
    "two_topologies": (0.0104, 0.462),
    "soup": (0.0104, 0.196),
}
EXCESS_BOUND = {name: tuple(max(figure, 4.0) for figure in row) for name, row in CPU_MEASURED.items()}


@pytest.mark.parametrize("name", MESHES)
def test_composition_against_the_fp64_brute_force(name):
    v, _ = mesh(name)
    worst = [0.0, 0.0]
    for k, p in enumerate(SIZES):
        pf, fp = composed(name, k)
        assert pf._fields == ("dist", "face", "bary") and fp._fields == ("dist", "point", "bary")
        assert pf.dist.shape == (v.shape[0], p) and pf.face.dtype == torch.int64 and pf.bary.shape == (v.shape[0], p, 3)
        assert fp.point.dtype == torch.int64 and fp.dist.dtype == torch.float32
        got = excess(name, k, pf, fp)
        worst = [max(a, b) for a, b in zip(worst, got)]
    print("%s: excess over the fp64 minimum: point -> face %.3g, face -> point %.3g units (pinned %s)"
          % (name, worst[0], worst[1], CPU_MEASURED[name]))
    assert worst[0] <= EXCESS_BOUND[name][0] and worst[1] <= EXCESS_BOUND[name][1], worst


@pytest.mark.parametrize("name", MESHES)
def test_dist_is_the_residual_of_the_interpolated_point(name):
    """the identity of the contract, to the bit, and the public functions are the composition's two halves"""
    v, faces = mesh(name)
    x, corners = torch.from_numpy(v.astype(F32)), corners_of(faces, v.shape[1])
    pf, fp = composed(name, 2)
    pts = torch.from_numpy(cloud(name, 2).astype(F32))
    r = pts - geo_operations.mesh_interpolate(x, corners, pf.face, pf.bary)
    assert torch.equal(pf.dist, (r[..., 0] * r[..., 0] + r[..., 1] * r[..., 1]) + r[..., 2] * r[..., 2])
    own = torch.arange(corners.n_faces).expand(v.shape[0], -1)
    chosen = torch.gather(pts, 1, fp.point.clamp(min=0)[..., None].expand(-1, -1, 3))
    r = chosen - geo_operations.mesh_interpolate(x, corners, own, fp.bary)
    want = (r[..., 0] * r[..., 0] + r[..., 1] * r[..., 1]) + r[..., 2] * r[..., 2]
    taken = fp.point >= 0
    assert torch.equal(fp.dist[taken], want[taken]) and bool(torch.isnan(fp.dist[~taken]).all())
    one = mesh_distance.point_face_distance(pts, x, torch.from_numpy(faces))
    other = mesh_distance.face_point_distance(pts, x, corners)
    assert all(torch.equal(a, b) for a, b in zip(one, pf))
    assert all(torch.equal(a[taken], b[taken]) for a, b in zip(other, fp))


def test_blocks_of_the_pair_matrix_change_nothing(monkeypatch):
    pf, fp = composed("two_topologies", 3)
    v, faces = mesh("two_topologies")
    monkeypatch.setattr(mesh_distance, "CHUNK_PAIRS", 7 * 2 * faces.shape[1])     # blocks of seven points
    again = mesh_distance.distance_composition(torch.from_numpy(cloud("two_topologies", 3).astype(F32)),
                                               torch.from_numpy(v.astype(F32)), corners_of(faces, v.shape[1]))
    for a, b in zip(pf + fp, again[0] + again[1]):
        assert a.numpy().tobytes() == b.numpy().tobytes()


# --------------------------------------------------------------------------------------------------------- ties
def test_the_lowest_index_wins_among_equal_distances():
    v, faces = tie_mesh()
    f = faces.shape[0] // 2
    pf, fp = composed_ties()
    assert bool((pf.face >= 0).all()) and bool((pf.face < f).all())
    single = composed("grid_40x130", 2)
    assert torch.equal(pf.face, single[0].face) and torch.equal(pf.dist, single[0].dist)
    assert torch.equal(fp.point[:, :f], fp.point[:, f:]) and torch.equal(fp.dist[:, :f], single[1].dist)
    for name in ("cage", "two_topologies"):
        pf, fp = composed(name, "repeated")
        plain = composed(name, 3)
        assert bool((fp.point < 1000).all()) and torch.equal(fp.point, plain[1].point)
        assert torch.equal(pf.face[:, 1000:], pf.face[:, :32]) and torch.equal(pf.dist[:, 1000:], pf.dist[:, :32])
        assert bool((fp.point < 32).any())                                    # some tie was there to be decided


# ------------------------------------------------------------------------------------------------ known answers
TRIANGLE = np.array([[0, 0, 0], [4, 0, 0], [0, 4, 0]], np.float64)
KNOWN = [  # region, point, weights, squared distance
    (1, (-1, -1, 0), (1, 0, 0), 2),
    (2, (5, -1, 0), (0, 1, 0), 2),
    (3, (1, -2, 0), (0.75, 0.25, 0), 4),
    (4, (-1, 5, 0), (0, 0, 1), 2),
    (5, (-2, 1, 0), (0.75, 0, 0.25), 4),
    (6, (3, 3, 0), (0, 0.5, 0.5), 2),
    (7, (1, 1, 2), (0.5, 0.25, 0.25), 4),
    (7, (1, 1, -2), (0.5, 0.25, 0.25), 4),
    (3, (1, -2, 1), (0.75, 0.25, 0), 5),
]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_known_answers_in_every_region(dtype):
    pts = torch.tensor([row[1] for row in KNOWN], dtype=dtype)[None]
    x = torch.from_numpy(TRIANGLE).to(dtype)[None]
    out = mesh_distance.point_face_distance(pts, x, torch.tensor([[0, 1, 2]]))
    assert out.dist.dtype == dtype and bool((out.face == 0).all())
    assert out.bary[0].tolist() == [list(map(float, row[2])) for row in KNOWN]
    assert out.dist[0].tolist() == [float(row[3]) for row in KNOWN]
    for region, point, weights, d in KNOWN:                                   # one face and one point at a time
        back = mesh_distance.face_point_distance(torch.tensor([[point]], dtype=dtype), x, torch.tensor([[0, 1, 2]]))
        assert back.point.tolist() == [[0]] and back.bary[0, 0].tolist() == list(map(float, weights)), region
        assert back.dist.tolist() == [[float(d)]]


# ------------------------------------------------------------------------------------------ nothing to choose
def unusable_cases():
    x = torch.from_numpy(TRIANGLE.astype(F32))[None]
    pts = torch.tensor([[[1.0, 1.0, 0.0], [3.0, 0.5, 1.0]]])
    one = corners_of(np.array([[0, 1, 2]]), 3)
    collapsed = x.clone()
    collapsed[0, 1] = collapsed[0, 0]                                         # a == b: 0/0 in region 3 for these points
    beyond = MeshCorners(torch.tensor([[[0, 1, 3]]]), one.start, one.codes, one.nbr, 3)
    return {"no faces": (pts, x, corners_of(np.zeros((0, 3), np.int64), 3)),
            "a collapsed edge": (pts, collapsed, one),
            "NaN points": (torch.full_like(pts, float("nan")), x, one),
            "a vertex index out of range": (pts, x, beyond)}


@pytest.mark.parametrize("case", ["no faces", "a collapsed edge", "NaN points", "a vertex index out of range"])
def test_an_item_without_a_partner_is_nan_and_passes_no_gradient(case):
    pts, x, corners = unusable_cases()[case]
    pts, x = pts.clone().requires_grad_(True), x.clone().requires_grad_(True)
    pf = mesh_distance.point_face_distance(pts, x, corners)
    assert bool((pf.face == -1).all()) and bool(torch.isnan(pf.dist).all()) and bool(torch.isnan(pf.bary).all())
    g_p, g_x = torch.autograd.grad(pf.dist.sum(), (pts, x))
    assert bool((g_p == 0).all()) and bool((g_x == 0).all())
    fp = mesh_distance.face_point_distance(pts, x, corners)
    assert fp.dist.shape == (1, corners.n_faces)
    assert bool((fp.point == -1).all()) and bool(torch.isnan(fp.dist).all()) and bool(torch.isnan(fp.bary).all())
    g_p, g_x = torch.autograd.grad(fp.dist.sum(), (pts, x), allow_unused=True)
    assert bool((g_p == 0).all()) and bool((g_x == 0).all())


def test_a_cloud_without_points():
    v, faces = mesh("cage")
    x = torch.from_numpy(v.astype(F32)).requires_grad_(True)
    none = torch.zeros(3, 0, 3, requires_grad=True)
    pf = mesh_distance.point_face_distance(none, x, torch.from_numpy(faces))
    fp = mesh_distance.face_point_distance(none, x, torch.from_numpy(faces))
    assert pf.dist.shape == (3, 0) and pf.face.shape == (3, 0) and pf.bary.shape == (3, 0, 3)
    assert fp.dist.shape == (3, 320) and bool((fp.point == -1).all()) and bool(torch.isnan(fp.dist).all())
    assert bool((torch.autograd.grad(fp.dist.sum(), x)[0] == 0).all())


# ---------------------------------------------------------------------------------------------------- gradients
def test_gradients_of_the_composition_by_gradcheck():
    """fp64, a jittered octahedron with a point over the inside of every face, outside by 0.1: away from the medial
    set (a point whose closest point is on an edge or a vertex is on it: the faces around are equally far).  The
    runner-up of every choice is farther than the winner by a margin that the finite differences (1e-6) cannot
    bridge, so nothing is differentiated across a switch."""
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
    pts = centre + 0.1 * normal
    every = np_all_pairs(pts, tri)
    for axis in (0, 1):
        ranked = np.sort(every, axis=axis)
        first, second = (ranked[0], ranked[1]) if axis == 0 else (ranked[:, 0], ranked[:, 1])
        assert (second - first > 1e-3).all()
    face, point = torch.from_numpy(every.argmin(1)), torch.from_numpy(every.argmin(0))
    corners = corners_of(faces, 6)
    p, x = torch.from_numpy(pts)[None].requires_grad_(True), torch.from_numpy(v)[None].requires_grad_(True)

    def both(a, b):
        pf, fp = mesh_distance.distance_composition(a, b, corners)
        assert torch.equal(pf.face[0], face) and torch.equal(fp.point[0], point)
        return pf.dist, fp.dist


    assert torch.autograd.gradcheck(both, (p, x), eps=1e-6, atol=1e-6)


# ------------------------------------------------------------------------------------------- the API and errors
def test_the_loss_keeps_its_topology_and_is_the_mean_of_the_two_operators():
    v, faces = mesh("two_topologies")
    x = torch.from_numpy(v).requires_grad_(True)
    pts = torch.from_numpy(cloud("two_topologies", 1)).requires_grad_(True)
    tf = torch.from_numpy(faces)
    kept = model_loss.PointMeshDistanceLoss(consistent_topology=True)
    fresh = model_loss.PointMeshDistanceLoss()
    first = kept(pts, x, tf)
    topology = kept.E
    assert isinstance(topology, MeshCorners)
    again = kept(pts, x)
    assert kept.E is topology and torch.equal(first, again) and torch.equal(first, fresh(pts, x, tf))
    assert fresh.E is not topology
    pf, fp = mesh_distance.distance_composition(pts, x, topology)
    assert torch.equal(first, pf.dist.mean() + fp.dist.mean())
    g_p, g_x = torch.autograd.grad(first, (pts, x))
    assert bool(torch.isfinite(g_p).all()) and bool((g_p != 0).any())
    assert bool(torch.isfinite(g_x).all()) and bool((g_x != 0).any())
    with pytest.raises(AssertionError, match="Face is required"):
        model_loss.PointMeshDistanceLoss()(pts, x)


def test_argument_errors():
    v, faces = mesh("cage")
    x = torch.from_numpy(v.astype(F32))
    corners = corners_of(faces, x.shape[1])
    pts = torch.from_numpy(cloud("cage", 1).astype(F32))
    for function in (mesh_distance.point_face_distance, mesh_distance.face_point_distance):
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
        with pytest.raises(ValueError, match="points must have shape"):
            function(pts[..., :2], x, corners)
        with pytest.raises(ValueError, match="built for 162 vertices"):
            function(pts, x[:, :100], corners)
        with pytest.raises(ValueError, match="vertices must have shape"):
            function(pts, x[..., :2], corners)
        with pytest.raises(IndexError, match="batch element 0"):
            function(pts, x, torch.tensor([[0, 1, 162]]))
    with pytest.raises(TypeError, match="face must be an integer"):
        mesh_distance.point_face_at(pts, x, corners, torch.zeros(3, 63), torch.rand(3, 63, 3))
    with pytest.raises(ValueError, match="bary must have shape"):
        mesh_distance.point_face_at(pts, x, corners, torch.zeros(3, 63, dtype=torch.int64), torch.rand(3, 63, 2))
    with pytest.raises(ValueError, match="point must have shape"):
        mesh_distance.face_point_at(pts, x, corners, torch.zeros(2, 320, dtype=torch.int64), torch.rand(2, 320, 3))
