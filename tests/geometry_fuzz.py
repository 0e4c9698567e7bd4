"""Seeded ill-shaped geometry for the operators that do arithmetic per triangle: the exact point-to-mesh distances, the
winding number and the signed distance, the surface sampling, the face and vertex normals, the dihedral angles and the
cotangent weights.  A helper module, not a test file: tests/test_geometry_fuzz_host.py pins the generators and the fp32
CPU compositions against fp64 on the CPU, and tests/test_gpu_geometry_fuzz.py runs the HIP kernels on the same cases.
tests/topology_fuzz.py randomises connectivity; this one randomises coordinates.

Every case comes from ``(family, seed)`` alone: ``case`` gives vertices (2,N,3) float64 that are exact in fp32, faces
(F,3) (one shared topology) or (2,F,3) (one per batch element) and a cloud (2,P,3).  The two batch elements are drawn
from different seeds.  Every family stays inside ``1e-5 <= |edge|`` (of the edges that are not collapsed on purpose)
and ``|coordinate| <= 2e3``.  The fp32 CPU composition and the fp64 reference of a case are computed once
(``lru_cache``) and serve both test files."""
import collections
import functools

import numpy as np
import torch

import topology_fuzz as T
from pytorch_points_amd import mesh_distance, mesh_winding
from test_mesh_dihedral_host import folded_grid, jittered_cage, torus_mesh
from test_mesh_distance_host import extent, has_area, np_all_pairs, np_at
from test_mesh_sample_host import corners_of, faces_of

F32 = np.float32
EPS32 = 2.0 ** -23
SOUP_FACES = [1, 255, 256, 257, 600]     # the walk's LDS tile of 256 less one, full and plus one
CLOUD_SIZES = [1, 257, 1000]
SOUPS = ["well", "sliver_2", "sliver_4", "sliver_6", "needle", "collinear", "coincident", "lattice", "offset",
         "mixed_scale", "mixed", "dyadic"]
MANIFOLDS = ["thin", "rows", "collapsed", "far"]
FAMILIES = SOUPS + MANIFOLDS
ORDER = SOUPS[:-1] + MANIFOLDS + SOUPS[-1:]   # as the families were added: a family's sizes hang on its place here
CLOSED = ["thin", "far"]                 # oriented outwards: every point off the surface is inside or outside
FLAT = ["collinear", "coincident", "lattice", "collapsed"]   # a face without fp64 area has none in fp32 either
NEAR = 1e-4                              # of the extent: a point closer to some face is "near", on the surface

Case = collections.namedtuple("Case", ["family", "seed", "vertices", "faces", "points"])


def seed_count():
    """topology_fuzz's PP_FUZZ_SEEDS convention divided so that the default run has 8 seeds a family"""
    return max(1, T.seed_count() // 5)


def seeds():
    return range(seed_count())


def describe(c):
    """what a failure message names: the family, the seed and the sizes"""
    return "%s, seed %d: N = %d, F = %d (%s topology), P = %d" % (
        c.family, c.seed, c.vertices.shape[1], c.faces.shape[-2], "shared" if c.faces.ndim == 2 else "per-element",
        c.points.shape[1])


def exact32(a):
    return np.asarray(a, np.float64).astype(F32).astype(np.float64)


# ----------------------------------------------------------------------------------------------- soup triangles
def _unit(rng, size):
    d = rng.normal(size=size + (3,))
    return d / np.linalg.norm(d, axis=-1, keepdims=True)


def _orthogonal(rng, e):
    """unit vectors orthogonal to the vectors e (F,3), in a random direction about them"""
    d = np.cross(e, _unit(rng, e.shape[:1]))
    return d / np.linalg.norm(d, axis=-1, keepdims=True)


def _roll(rng, tri):
    """every triangle's corners rotated by a random amount: the ill-shaped corner is not always the same one"""
    k = rng.integers(0, 3, size=tri.shape[0])
    return tri[np.arange(tri.shape[0])[:, None], (np.arange(3)[None] + k[:, None]) % 3]


def well(rng, f, size=None):
    """(f,3,3): jittered equilateral triangles of circumradius ``size`` (0.1 to 0.4) in random planes, centres in
    [-1,1]^3; the smallest angle stays above some 25 degrees"""
    size = rng.uniform(0.1, 0.4, size=f) if size is None else size
    u = _unit(rng, (f,))
    w = _orthogonal(rng, u)
    angle = 2 * np.pi * (np.arange(3) / 3)[None] + rng.uniform(-0.25, 0.25, size=(f, 3))
    corner = np.cos(angle)[..., None] * u[:, None] + np.sin(angle)[..., None] * w[:, None]
    return rng.uniform(-1, 1, size=(f, 1, 3)) + size[:, None, None] * corner


def sliver(rng, f, height):
    """the third vertex is a random interior point of the opposite edge plus ``height`` of that edge's length"""
    tri = well(rng, f)
    a, b = tri[:, 0], tri[:, 1]
    t = rng.uniform(0.2, 0.8, size=(f, 1))
    length = np.linalg.norm(b - a, axis=1, keepdims=True)
    tri[:, 2] = a + t * (b - a) + height * length * _orthogonal(rng, b - a)
    return _roll(rng, tri)


def needle(rng, f):
    """one edge is 1e-5 of the other two, which are 1.1 to 2 long"""
    a = rng.uniform(-1, 1, size=(f, 3))
    length = rng.uniform(1.1, 2, size=(f, 1))
    along = _unit(rng, (f,))
    return _roll(rng, np.stack([a, a + 1e-5 * length * _orthogonal(rng, along), a + length * along], 1))


def collinear(rng, f):
    """three distinct vertices a, a + d, a + 3 d on the integer lattice: every product of the cross product is an
    integer below 2^24, so it is exactly zero in fp32"""
    a = rng.integers(-8, 9, size=(f, 3)).astype(np.float64)
    d = rng.integers(-3, 4, size=(f, 3)).astype(np.float64)
    d[(d == 0).all(1)] = (1.0, -2.0, 3.0)
    return _roll(rng, np.stack([a, a + d, a + 3 * d], 1))


def coincident(rng, f):
    """equal coordinates under distinct indices: face k is (a,a,c), (a,c,a), (a,c,c), (a,a,a) for k mod 4 = 0, 1, 2,
    3"""
    tri = well(rng, f)
    a, c = tri[:, 0].copy(), tri[:, 2].copy()
    k = np.arange(f) % 4
    tri[:, 1] = np.where((k == 0)[:, None] | (k == 3)[:, None], a, c)
    tri[:, 2] = np.where((k == 1)[:, None] | (k == 3)[:, None], a, c)
    return tri


def lattice(rng, f):
    return rng.integers(0, 5, size=(f, 3, 3)) / 2.0


GRID = 2.0 ** -16


def dyadic(rng, f):
    """slivers on the grid 2^-16 Z^3 in [-1.4,1.4]^3: the third vertex is the grid point next to a random interior point
    of the opposite edge, moved by 1 to 3 grid steps along the axis the edge runs along least.  Coordinates of 18 bits:
    every edge vector is exact in fp32, every product of two of their components has up to 32 bits and is not, and
    the cross product, a multiple of 2^-32 of size 1e-5, is.  So a difference of products that recovers the products'
    rounding (csrc/mesh_common.h v3_dop, within 1.5 ulp of the exact value) gives such a face's area to a few eps32
    of itself, and the plain ``a*b - c*d`` of two rounded products to some 1e3 eps32."""
    tri = np.round(well(rng, f) / GRID)
    a, b = tri[:, 0], tri[:, 1]
    c = np.round(a + rng.uniform(0.2, 0.8, size=(f, 1)) * (b - a))
    c[np.arange(f), np.abs(b - a).argmin(1)] += rng.integers(1, 4, size=f) * rng.choice([-1, 1], size=f)
    tri[:, 2] = c
    return _roll(rng, tri * GRID)


def offset(rng, f):
    """``well`` at an extent of 0.05 to 1, whatever ``f``, moved to |x| about 1000"""
    tri = well(rng, f)
    tri = (tri - tri.reshape(-1, 3).min(0)) * (10.0 ** rng.uniform(np.log10(0.05), 0.0) / extent(tri))
    return tri + rng.choice([-1.0, 1.0], size=3) * rng.uniform(900, 1100, size=3)


def mixed_scale(rng, f):
    return well(rng, f, size=10.0 ** rng.integers(-4, 2, size=f))


SOUP_TRIANGLES = {"well": well, "sliver_2": lambda r, f: sliver(r, f, 1e-2),
                  "sliver_4": lambda r, f: sliver(r, f, 1e-4), "sliver_6": lambda r, f: sliver(r, f, 1e-6),
                  "needle": needle, "collinear": collinear,
                  "coincident": coincident, "lattice": lattice, "offset": offset, "mixed_scale": mixed_scale,
                  "dyadic": dyadic}
MIXED = ["well", "sliver_4", "collinear", "coincident", "repeated index"]


def _soup(family, seed):
    pick = np.random.default_rng([seed, 77, ORDER.index(family)])
    f, p = int(pick.choice(SOUP_FACES)), int(pick.choice(CLOUD_SIZES))
    faces = np.arange(3 * f, dtype=np.int64).reshape(f, 3)
    kind = np.arange(f) % 5
    if family == "mixed":                                    # a fifth each, interleaved: every tile holds all of them
        again = kind == 4
        faces[again, 1 + (np.arange(f)[again] // 5) % 2] = faces[again, 0]     # (i, i, k) and (i, j, i)
    vertices = np.empty((2, 3 * f, 3))
    for b in range(2):
        rng = np.random.default_rng([seed, b])
        if family == "mixed":
            tri = well(rng, f)
            for k, name in enumerate(MIXED[:4]):
                tri[kind == k] = SOUP_TRIANGLES[name](rng, int((kind == k).sum()))
            tri[kind == 2] /= 8.0                             # the lattice of ``collinear`` at the scale of the rest
        else:
            tri = SOUP_TRIANGLES[family](rng, f)
        vertices[b] = tri.reshape(-1, 3)
    if seed % 2:                                             # one topology per element: the second lists the faces
        faces = np.stack([faces, np.roll(faces[::-1], 1, axis=1)])      # backwards with their corners rotated
    return exact32(vertices), faces, p, None


# ------------------------------------------------------------------------------------------------ manifold meshes
def outwards(v, faces):
    """the signed volume of a closed mesh: positive where its faces are oriented outwards"""
    tri = v[faces]
    return float((tri[:, 0] * np.cross(tri[:, 1], tri[:, 2])).sum() / 6)


def _closed(seed):
    """a closed mesh oriented outwards, extent about 1, centred: the torus (640 or 960 faces) or the cage (320)"""
    if seed % 3 == 2:
        faces, v = jittered_cage(100 + seed)
        v = v[0]
    else:
        v, faces = torus_mesh(16, 20 + 10 * (seed % 3))
    if outwards(v, faces) < 0:
        faces = faces[:, ::-1].copy()
    v = v - 0.5 * (v.max(0) + v.min(0))
    return v / extent(v), faces


def _manifold(family, seed):
    """``(vertices, faces, P, before)``; ``before`` is None, or for ``thin`` per batch element the mesh before the
    squash and the squash's matrix A (a point x goes to A x): its cloud is drawn there and mapped with the mesh"""
    pick = np.random.default_rng([seed, 78, ORDER.index(family)])
    p = int(pick.choice(CLOUD_SIZES))
    out, before = [], []
    for b in range(2):
        rng = np.random.default_rng([seed, b])
        if family == "thin":
            v0, faces = _closed(seed)
            axis = seed % 3

            def squash(x, axis=axis, k=rng.uniform(0.3, 0.7, size=2)):
                x = x.copy()
                x[:, axis] *= 1e-3                            # squashed, then sheared: a linear map of determinant
                x[:, (axis + 1) % 3] += k[0] * x[:, axis]     # 1e-3 > 0 keeps the mesh closed and oriented outwards
                x[:, (axis + 2) % 3] += k[1] * x[:, (axis + 1) % 3]
                return x

            v = squash(v0)
            before.append((v0, squash(np.eye(3)).T))
        elif family == "far":
            v, faces = torus_mesh(16, 20)
            if outwards(v, faces) < 0:
                faces = faces[:, ::-1].copy()
            v = v / extent(v) + 0.002 * rng.uniform(-1, 1, size=v.shape) + rng.choice([-1.0, 1.0], size=3) * 1000.0
        else:
            rows, cols = 15 + seed % 3, 21 + seed % 5
            v, faces = folded_grid(rows, cols, int(rng.integers(1 << 30)))
            grid = v[0].reshape(rows, cols, 3)
            if family == "rows":                              # the row widths run geometrically from 1e-5 to 1; the
                width = 10.0 ** np.linspace(-5, 0, rows - 1)  # fold's heights shrink with them, so its slopes stay
                grid[:, :, 1] = np.concatenate([[0.0], np.cumsum(width)])[:, None]
                grid[:, :, 2] *= np.minimum(np.append(width, 1.0) * (rows - 1), 1.0)[:, None]
            else:                                             # every seventh row lies on the row before it
                grid[6::7] = grid[5::7][:grid[6::7].shape[0]]
            v = grid.reshape(-1, 3)
        out.append((v, faces))
    vertices = exact32(np.stack([v for v, _ in out]))
    faces = out[0][1]
    if seed % 2:
        faces = np.stack([faces, np.roll(faces, 1, axis=1)])  # per element: the same surface, corners rotated
    return vertices, faces, p, before or None


# ----------------------------------------------------------------------------------------------------- the clouds
KINDS = [5, 0, 1, 2, 3, 2, 4, 1, 5]      # point i is of kind KINDS[i % 9]: a third on the surface, half of no prefix
PUSH = np.array([0.0, 1e-3, 0.3, 0.0, 0.0, 0.0])
THIN_PUSH = np.array([0.0, 0.12, 0.1, 0.0, 0.0, 0.0])   # before the squash, where the tube is 0.28 across


def face_normals(tri):
    """fp64 unit normals of (F,3,3); for a face without area any unit vector orthogonal to its longest edge (any unit
    vector at all where the three vertices coincide)"""
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    length = np.linalg.norm(n, axis=1)
    edges = tri[:, [1, 2, 0]] - tri
    longest = edges[np.arange(tri.shape[0]), (edges ** 2).sum(-1).argmax(1)]
    axis = np.eye(3)[np.abs(longest).argmin(1)]               # never parallel to a non-zero ``longest``
    other = np.cross(longest, axis)
    size = np.linalg.norm(other, axis=1)
    other = np.where((size > 0)[:, None], other / np.maximum(size, 1e-300)[:, None], np.array([0.0, 0.0, 1.0]))
    return np.where((length > 0)[:, None], n / np.maximum(length, 1e-300)[:, None], other)


def cloud_of(tri, p, rng, size, push=PUSH):
    """test_mesh_distance_host.cloud's recipe for any triangle list (F,3,3): surface samples pushed along +- the face
    normal by 0, 1e-3 and 0.3 of ``size``, copies of vertices, edge midpoints and points at 10 x ``size`` about the
    centre; the kinds follow KINDS, not a draw, so that the share of points on the surface is a third"""
    kind = np.array(KINDS)[np.arange(p) % len(KINDS)]
    f = rng.integers(0, tri.shape[0], size=p)
    w = rng.dirichlet((1.0, 1.0, 1.0), size=p)
    push = push[kind] * size * rng.choice([-1.0, 1.0], size=p)
    pts = (w[:, :, None] * tri[f]).sum(1) + push[:, None] * face_normals(tri)[f]
    j = rng.integers(0, 3, size=p)
    pts[kind == 3] = tri[f, j][kind == 3]
    pts[kind == 4] = (0.5 * (tri[f, j] + tri[f, (j + 1) % 3]))[kind == 4]
    centre = 0.5 * (tri.reshape(-1, 3).max(0) + tri.reshape(-1, 3).min(0))
    far = centre + 10 * size * _unit(rng, (p,))
    pts[kind == 5] = far[kind == 5]
    return pts


@functools.lru_cache(maxsize=None)
def case(family, seed):
    vertices, faces, p, before = (_soup if family in SOUPS else _manifold)(family, seed)
    points = np.empty((2, p, 3))
    for b in range(2):
        rng = np.random.default_rng([seed, b, 79])
        if family == "lattice":                               # points on {0,...,11}^3 / 4; every other one has x > 2,
            pts = rng.integers(0, 12, size=(p, 3))            # off the vertices' box: at most half are on a face
            pts[::2, 0] = rng.integers(9, 12, size=pts[::2].shape[0])
            points[b] = pts / 4.0
        elif before:                                          # (a push of 1e-3 would end 1e-6 from the squashed face,
            v0, matrix = before[b]                            # and one of 0.3 beyond the other side of the tube)
            points[b] = cloud_of(v0[faces_of(faces, b)], p, rng, extent(v0), THIN_PUSH) @ matrix.T
        else:
            points[b] = cloud_of(vertices[b][faces_of(faces, b)], p, rng, max(extent(vertices[b]), 1e-3))
    return Case(family, seed, vertices, faces, exact32(points))


def triangles(c, b):
    return c.vertices[b][faces_of(c.faces, b)]


def host_corners(c):
    return corners_of(c.faces, c.vertices.shape[1])


def tensors(c, dtype=torch.float32):
    """(points, vertices) of the case as CPU tensors of ``dtype``"""
    return torch.from_numpy(c.points).to(dtype), torch.from_numpy(c.vertices).to(dtype)


# ------------------------------------------------------------------------------------------ the fp64 references
def np_usable(p, a, b, c):
    """The contract's rule for one pair in fp64, (...,3) broadcast: False where the first region of the walk that holds
    divides 0 by 0 -- the pair's distance is NaN and the face is never taken for this point -- and True elsewhere.  On
    the coincident faces the deciding quantities are exact zeros in fp32 as in fp64."""
    dot = lambda u, v: (u * v).sum(-1)   # noqa: E731
    ab, ac, ap, bp, cp = b - a, c - a, p - a, p - b, p - c
    d1, d2, d3, d4, d5, d6 = dot(ab, ap), dot(ac, ap), dot(ab, bp), dot(ac, bp), dot(ab, cp), dot(ac, cp)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    e43, e56 = d4 - d3, d5 - d6
    regions = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
               (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & (e43 >= 0) & (e56 >= 0), np.ones_like(d1, bool)]
    zero_over_zero = [False, False, (d1 == 0) & (d1 - d3 == 0), False, (d2 == 0) & (d2 - d6 == 0),
                      (e43 == 0) & (e43 + e56 == 0), (va + vb) + vc == 0]
    usable, open_ = np.ones_like(d1, bool), np.ones_like(d1, bool)
    for region, bad in zip(regions, zero_over_zero):
        usable = np.where(open_ & region, ~np.asarray(bad), usable)
        open_ = open_ & ~region
    return usable


@functools.lru_cache(maxsize=None)
def reference(family, seed):
    """Per batch element, from fp64 alone: ``every`` (P,F) the ``np_pair`` distances of all pairs, ``area`` (F,) which
    faces have area, ``served`` (P,) whether some face is usable for the point by the contract's rule, ``near`` (P,)
    whether the point is within NEAR of the extent of some face, ``unit`` the excess measure's unit."""
    c = case(family, seed)
    out = []
    for b in range(2):
        tri, pts = triangles(c, b), c.points[b]
        every = np_all_pairs(pts, tri)
        usable = np_usable(pts[:, None], tri[None, :, 0], tri[None, :, 1], tri[None, :, 2])
        out.append(dict(every=every, area=has_area(c.vertices[b], faces_of(c.faces, b)), served=usable.any(1),
                        near=every.min(1) < (NEAR * extent(c.vertices[b])) ** 2,
                        unit=np.abs(pts[:, None, :] - c.vertices[b][None, :, :]).max() ** 2 * EPS32))
    return out


# ---------------------------------------------------------------------------------------------- the distances
@functools.lru_cache(maxsize=None)
def composed(family, seed):
    """the fp32 CPU ``distance_composition`` of the case: ``(PointFaceDistance, FacePointDistance)``"""
    c = case(family, seed)
    pts, x = tensors(c)
    return mesh_distance.distance_composition(pts, x, host_corners(c))


def excess(c, pf, fp, flat_too=False):
    """test_mesh_distance_host.excess for a case: the largest amount by which the fp64 distance at the chosen ``(index,
    bary)`` exceeds the fp64 minimum over the partners (``reference``'s matrix of every pair serves as ``np_minima``),
    in units of ``(largest |coordinate difference|)^2 eps32``, ``[point -> face, face -> point]``.  Faces without area
    take no part on the triangles' side, as the contract says, unless ``flat_too``; an item left without a partner
    takes none."""
    worst = [0.0, 0.0]
    ref = reference(c.family, c.seed)
    for b in range(2):
        tri, pts, keep = triangles(c, b), c.points[b], ref[b]["area"] | flat_too
        if not keep.any():
            continue
        per_point, per_face = ref[b]["every"][:, keep].min(1), ref[b]["every"][:, keep].min(0)
        face, bary = pf.face[b].cpu().numpy(), pf.bary[b].double().cpu().numpy()
        took = face >= 0
        got = np_at(pts[took], tri[face[took]], bary[took])
        worst[0] = max(worst[0], float((got - per_point[took]).max(initial=0.0) / ref[b]["unit"]))
        point, bary = fp.point[b].cpu().numpy()[keep], fp.bary[b].double().cpu().numpy()[keep]
        took = point >= 0
        got = np_at(pts[point[took]], tri[keep][took], bary[took])
        worst[1] = max(worst[1], float((got - per_face[took]).max(initial=0.0) / ref[b]["unit"]))
    return worst


@functools.lru_cache(maxsize=None)
def incoming(family, seed):
    """g for dist (2,P) and for dist (2,F), exact in fp32"""
    c = case(family, seed)
    rng = np.random.default_rng([seed, 80])
    return tuple(exact32(rng.uniform(-1, 1, size=(2, s))) for s in (c.points.shape[1], c.faces.shape[-2]))


def composition_gradients(c, pf, fp, dtype):
    """test_gpu_mesh_distance.composition_gradients for a case: the gradients of point -> face and face -> point
    to (points, vertices) from the CPU composition in ``dtype`` at the choices given, four float64 arrays"""
    pts, x = tensors(c, dtype)
    pts.requires_grad_(True), x.requires_grad_(True)
    corners = host_corners(c)
    g1, g2 = (torch.from_numpy(g).to(dtype) for g in incoming(c.family, c.seed))
    d1 = mesh_distance.point_face_at(pts, x, corners, pf.face.cpu(), pf.bary.cpu().to(dtype))
    d2 = mesh_distance.face_point_at(pts, x, corners, fp.point.cpu(), fp.bary.cpu().to(dtype))
    one, two = pf.face.cpu() >= 0, fp.point.cpu() >= 0                     # (an item without a partner is NaN)
    zero = torch.zeros((), dtype=dtype)
    out = (torch.autograd.grad(torch.where(one, d1, zero), (pts, x), g1)
           + torch.autograd.grad(torch.where(two, d2, zero), (pts, x), g2))
    return [t.double().numpy() for t in out]


def gradient_error(got, ref):
    """test_gpu_mesh_distance.gradient_error: the largest absolute error over the largest |gradient| of the reference
    (where the reference is all zero, the largest absolute error itself)"""
    assert got.shape == ref.shape and np.isfinite(got).all()
    return float(np.abs(got - ref).max(initial=0.0) / max(np.abs(ref).max(initial=0.0), 1e-300)) if np.any(ref) \
        else float(np.abs(got).max(initial=0.0))


def gradient_figures(c, got, ref):
    """``gradient_error`` in eps32 of the four gradients of ``composition_gradients``.  The face -> point pair is left
    at 0 for a soup of one face with more than one point: some point of the cloud lies on that face, its distance is 0
    and its gradient rounding alone (1e-7 in fp64, exactly 0 in fp32), so the measure is 100 % and says nothing -- as
    on the fan of test_gpu_mesh_distance.py.  The gradients must be finite all the same."""
    out = [gradient_error(g, r) / EPS32 for g, r in zip(got, ref)]
    return out[:2] + [0.0, 0.0] if c.faces.shape[-2] == 1 and c.points.shape[1] > 1 else out


# -------------------------------------------------------------------------------------------------- the winding
@functools.lru_cache(maxsize=None)
def winding(family, seed):
    """``(the fp64 composition, the fp32 CPU composition)`` of the winding number, (2,P) each"""
    c = case(family, seed)
    corners = host_corners(c)
    return tuple(mesh_winding.winding_composition(*tensors(c, dtype), corners)
                 for dtype in (torch.float64, torch.float32))


def not_near(family, seed):
    """(2,P) bool: the points that are held to the fp64 winding number"""
    return np.stack([~r["near"] for r in reference(family, seed)])


def pair_matrix32(c):
    """(2,P,F) float64 numpy: the composition's own fp32 pair matrix, +inf where the pair is NaN or the face has an
    index out of range: its first minimum along either axis is the sequential rule of the contract"""
    pts, x = tensors(c)
    corners = host_corners(c)
    a, c1, c2, valid = mesh_distance._face_corners(x, corners)
    tri = [tuple(t[:, None] for t in mesh_distance._xyz(s)) for s in (a, c1, c2, c1 - a, c2 - a)]
    d = mesh_distance.pair_composition(tuple(t[:, :, None] for t in mesh_distance._xyz(pts)), *tri)[0]
    return torch.where((d == d) & valid[:, None, :], d, torch.full_like(d, float("inf"))).double().numpy()


def check_choice(c, pf, fp, interpolate):
    """What the contract promises of ``(PointFaceDistance, FacePointDistance)`` on its own, whoever computed them (CPU
    tensors); ``interpolate(face (2,S), bary (2,S,3))`` is ``mesh_interpolate`` on the computing side, returned as a
    CPU tensor.  Index in range or -1; a partner wherever the fp64 rule says one is usable; NaN exactly beside -1;
    weights in [-2 eps32, 1 + 2 eps32] that sum to 1 within 4 eps32; ``dist`` the residual of the interpolated point to
    the bit; the fp64 distance at the choice never below the fp64 minimum over all partners by more than rounding: the
    chosen point is a combination of the corners whose weights are off a convex one by at most 2 eps32 each and 4
    eps32 in their sum, so it lies within 8 eps32 max|coordinate| of the triangle, and the root of its distance is short
    of the root of the minimum by no more than that."""
    what = describe(c)
    ref = reference(c.family, c.seed)
    pts32 = torch.from_numpy(c.points.astype(F32))
    p, f = c.points.shape[1], c.faces.shape[-2]
    for out, index, size in ((pf, pf.face, f), (fp, fp.point, p)):
        assert index.dtype == torch.int64 and bool(((index >= -1) & (index < size)).all()), what
        took = index >= 0
        assert bool(torch.isfinite(out.dist[took]).all()) and bool(torch.isfinite(out.bary[took]).all()), what
        assert bool(torch.isnan(out.dist[~took]).all()) and bool(torch.isnan(out.bary[~took]).all()), what
        w = out.bary[took].double()
        assert bool((w >= -2 * EPS32).all()) and bool((w <= 1 + 2 * EPS32).all()), (what, float(w.min()),
                                                                                    float(w.max()))
        assert bool(((w.sum(-1) - 1).abs() <= 4 * EPS32).all()), (what, float((w.sum(-1) - 1).abs().max()))
    own = torch.arange(f).expand(2, -1)
    chosen = torch.gather(pts32, 1, fp.point.clamp(min=0)[..., None].expand(-1, -1, 3))
    for out, index, p_of, face_of in ((pf, pf.face, pts32, pf.face), (fp, fp.point, chosen, own)):
        took = index >= 0
        r = p_of - interpolate(torch.where(took, face_of, torch.full_like(face_of, -1)), out.bary)
        want = (r[..., 0] * r[..., 0] + r[..., 1] * r[..., 1]) + r[..., 2] * r[..., 2]
        assert torch.equal(out.dist[took], want[took]), (what, "dist is not the residual of the interpolated point")
    for b in range(2):
        tri, pts = triangles(c, b), c.points[b]
        face, point = pf.face[b].numpy(), fp.point[b].numpy()
        slack = 8 * EPS32 * max(np.abs(c.vertices[b]).max(), np.abs(pts).max())
        assert (face[ref[b]["served"]] >= 0).all(), (what, "face = -1 beside a usable face")
        took = face >= 0
        got = np_at(pts[took], tri[face[took]], pf.bary[b].double().numpy()[took])
        assert (np.sqrt(got) >= np.sqrt(ref[b]["every"].min(1)[took]) - slack).all(), what
        took = point >= 0
        got = np_at(pts[point[took]], tri[took], fp.bary[b].double().numpy()[took])
        assert (np.sqrt(got) >= np.sqrt(ref[b]["every"].min(0)[took]) - slack).all(), what


# ------------------------------------------------------------------------- the operators, on either device
def _x(c, device, dtype, grad=True):
    return torch.from_numpy(c.vertices).to(device=device, dtype=dtype).requires_grad_(grad)


def _corners(c, device):
    from pytorch_points_amd.mesh_laplacian import MeshCorners
    return MeshCorners.from_faces(torch.from_numpy(c.faces).to(device), c.vertices.shape[1])


@functools.lru_cache(maxsize=None)
def incoming_mesh(family, seed):
    """g_n (2,F,3), g_a (2,F), g_v (2,N,3), g_e (2,3F), exact in fp32"""
    c = case(family, seed)
    n, f = c.vertices.shape[1], c.faces.shape[-2]
    rng = np.random.default_rng([seed, 81])
    return [exact32(rng.uniform(-1, 1, size=shape)) for shape in ((2, f, 3), (2, f), (2, n, 3), (2, 3 * f))]


NORMALS_METRICS = ["face normals", "areas", "face gradient", "vertex normals, area", "vertex gradient, area",
                   "vertex normals, uniform", "vertex gradient, uniform"]


def normals_run(c, device, dtype):
    """test_gpu_mesh_normals.run for a case: every output and gradient of both operators, in the order of
    NORMALS_METRICS, as float64 numpy"""
    from pytorch_points_amd import mesh_normals
    corners = _corners(c, device)
    g_n, g_a, g_v, _ = (torch.from_numpy(a).to(device=device, dtype=dtype) for a in incoming_mesh(c.family, c.seed))
    x = _x(c, device, dtype)
    normals, areas = mesh_normals.mesh_face_normals(x, corners)
    out = [normals, areas, torch.autograd.grad((normals, areas), x, (g_n, g_a))[0]]
    for w in ("area", "uniform"):
        per_vertex = mesh_normals.mesh_vertex_normals(x, corners, w)
        out += [per_vertex, torch.autograd.grad(per_vertex, x, g_v)[0]]
    return [t.detach().double().cpu().numpy() for t in out]


def normals_errors(c, got, ref):
    """test_gpu_mesh_normals.errors with the areas in the unit that ill-shaped faces need: per metric the largest
    absolute error of the unit normals, the largest area error over |ab| |ac| (a face with a zero edge product must
    have the area 0 exactly), the largest gradient error over the largest |gradient| of the reference"""
    out = []
    for what, a, r in zip(NORMALS_METRICS, got, ref):
        assert a.shape == r.shape and np.isfinite(a).all(), (describe(c), what)
        if what == "areas":
            tri = np.stack([triangles(c, b) for b in range(2)])
            ab, ac = tri[:, :, 1] - tri[:, :, 0], tri[:, :, 2] - tri[:, :, 0]
            unit = np.linalg.norm(ab, axis=-1) * np.linalg.norm(ac, axis=-1)
            assert (a[unit == 0] == 0).all(), (describe(c), what)
            out.append(float(np.max(np.abs(a - r)[unit > 0] / unit[unit > 0], initial=0.0)))
        elif "gradient" in what:
            out.append(gradient_error(a, r))
        else:
            out.append(float(np.abs(a - r).max()))
    return out


def np_dop(a, b, c, d):
    """csrc/mesh_common.h v3_dop on fp32 numpy arrays: ``a*b - c*d`` with the rounding of ``c*d`` recovered by one fma
    and added back (Kahan), within 1.5 ulp of the exact value"""
    w = c * d
    return T.fma32(a, b, -w) + T.fma32(-c, d, w)


def np_area32(tri, dop):
    """(F,) fp32 areas of (F,3,3) by the kernels' formula, ``c = cross(p1 - p0, p2 - p1)`` through the difference of
    products ``dop(a, b, c, d)``, ``len = sqrt((cx cx + cy cy) + cz cz)``, ``area = len / 2``"""
    tri = tri.astype(F32)
    u, v = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 1]
    c = [dop(u[:, 1], v[:, 2], u[:, 2], v[:, 1]), dop(u[:, 2], v[:, 0], u[:, 0], v[:, 2]),
         dop(u[:, 0], v[:, 1], u[:, 1], v[:, 0])]
    return np.sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]) * F32(0.5)


def dyadic_errors(c, normals, areas):
    """``dyadic``: the largest relative error of the areas and the largest absolute error of the unit normals (2,F,.)
    against the exact values -- fp64 is exact on this family up to its own last bit"""
    tri = np.stack([triangles(c, b) for b in range(2)])
    cross = np.cross(tri[:, :, 1] - tri[:, :, 0], tri[:, :, 2] - tri[:, :, 1])
    length = np.linalg.norm(cross, axis=-1)
    assert (length > 0).all(), describe(c)
    return float(np.abs(areas / (length / 2) - 1).max()), float(np.abs(normals - cross / length[..., None]).max())


def flat_faces(c):
    """(2,F) bool: the faces without fp64 area"""
    return np.stack([~has_area(c.vertices[b], faces_of(c.faces, b)) for b in range(2)])


def check_flat_normals(c, got):
    """DESIGN.md "Mesh normals", the degenerate rule on a family of FLAT: a face of |c| <= 1e-12 has the normal
    c / 1e-12 -- exactly 0 here, where c is exactly 0 -- and the area 0, and passes no gradient; a vertex whose faces
    are all flat has the normal 0 and, in a soup, where no other face reaches it, no gradient at all"""
    flat = flat_faces(c)
    normals, areas, face_grad = got[:3]
    assert (normals[flat] == 0).all() and (areas[flat] == 0).all(), describe(c)
    for b in range(2):
        faces = faces_of(c.faces, b)
        only_flat = np.ones(c.vertices.shape[1], bool)
        only_flat[faces[~flat[b]].reshape(-1)] = False
        assert (face_grad[b][only_flat] == 0).all(), describe(c)
        for values in got[3:]:
            assert (values[b][only_flat] == 0).all(), describe(c)


def dihedral_run(c, device, dtype):
    """(angles (2,Ecap), gradient (2,N,3)) as float64 numpy, and the edge table (2,Ecap,4) with its counts"""
    from pytorch_points_amd import mesh_dihedral
    topo = mesh_dihedral.MeshEdgePoints.from_faces(torch.from_numpy(c.faces).to(device), c.vertices.shape[1])
    x = _x(c, device, dtype)
    out = mesh_dihedral.mesh_dihedral_angle(x, topo)
    g = torch.from_numpy(incoming_mesh(c.family, c.seed)[3][:, :out.shape[1]]).to(device=device, dtype=dtype)
    grad, = torch.autograd.grad(out, x, g)
    table = topo.edge_points.expand(2, -1, -1).cpu().numpy()
    counts = [int(k) for k in topo.counts_host]
    counts = counts if len(counts) == 2 else counts * 2       # (a shared topology has one count)
    return [out.detach().double().cpu().numpy(), grad.double().cpu().numpy()], table, counts


def cot_run(c, device, dtype):
    """[cotangent weights (2,F,3), the cot-Laplacian of the vertices with them (2,N,3), its gradient (2,N,3)]"""
    from pytorch_points_amd import mesh_laplacian
    corners = _corners(c, device)
    x = _x(c, device, dtype)
    weights = mesh_laplacian.cotangent(x.detach(), torch.from_numpy(c.faces).to(device))
    out = mesh_laplacian.mesh_cot_laplacian(x, corners, weights)
    g = torch.from_numpy(incoming_mesh(c.family, c.seed)[2]).to(device=device, dtype=dtype)
    grad, = torch.autograd.grad(out, x, g)
    return [t.detach().double().cpu().numpy() for t in (weights, out, grad)]


@functools.lru_cache(maxsize=None)
def mesh_references(family, seed, op):
    """``(the fp64 CPU composition, the fp32 CPU composition)`` of ``op`` ("normals", "dihedral", "cot"), once"""
    c = case(family, seed)
    run = {"normals": normals_run, "dihedral": lambda *a: dihedral_run(*a)[0], "cot": cot_run}[op]
    return run(c, "cpu", torch.float64), run(c, "cpu", torch.float32)


# -------------------------------------------------------------------------------------------------- the sampling
def sample_uniforms(c):
    """(2,S,3) fp32 in [0,1) from test_mesh_sample_host.uniforms, S the case's cloud size"""
    from test_mesh_sample_host import uniforms
    return uniforms(1000 + c.seed, 2, c.points.shape[1])


def sample_run(c, device):
    """``(sample_points_from_meshes' (points, face, bary, normals), the operator's own areas (2,F))`` in fp32"""
    from pytorch_points_amd import mesh_normals, mesh_sample
    corners, x = _corners(c, device), _x(c, device, torch.float32, grad=False)
    u = torch.from_numpy(sample_uniforms(c)).to(device)
    return (mesh_sample.sample_points_from_meshes(x, corners, u=u, return_normals=True),
            mesh_normals.mesh_face_normals(x, corners)[1])


def check_samples(c, out, areas):
    """What holds of a draw whoever computed it (any device): the faces are the numpy fp64 restatement's on the
    operator's own areas (``np_faces``, whose ``clear`` must hold); a drawn face never has exactly zero fp64 area; a
    batch element whose areas are all zero gives -1 and NaN; the weights and points are ``np_points``' within
    test_mesh_sample_host's bounds (4 eps32, 8 eps32 of the largest |coordinate|); every sample lies on its face: its
    ``np_pair`` distance to the chosen triangle is within 4 units, the unit being the case's own, the one its distances
    are measured in: ``(largest |coordinate difference| between the case's cloud and its vertices)^2 eps32``.  (A unit
    taken from the samples alone cannot be met by any fp32 output on ``offset``: a coordinate of 1000 is stored to
    3e-5, and the squares of three of those are 14 units of a single triangle of extent 0.05.)  Returns the largest
    such distance in units."""
    from test_mesh_distance_host import np_pair
    from test_mesh_sample_host import np_faces, np_points
    what = describe(c)
    u = sample_uniforms(c)
    areas = areas.cpu().numpy()
    face, points, bary = out.face.cpu().numpy(), out.points.double().cpu().numpy(), out.bary.double().cpu().numpy()
    flat = flat_faces(c)
    worst = 0.0
    assert np.isfinite(areas).all() and (areas >= 0).all(), what
    for b in range(2):
        if not (areas[b] > 0).any():
            assert flat[b].all() and (face[b] == -1).all(), what
            assert np.isnan(points[b]).all() and np.isnan(bary[b]).all(), what
            assert bool(torch.isnan(out.normals[b]).all()), what
            continue
        want, clear = np_faces(areas[b:b + 1], u[b:b + 1, :, 0])
        assert clear, what
        assert np.array_equal(face[b], want[0]), what
        assert not flat[b][face[b]].any(), (what, "a face without area was drawn")
        ref_points, ref_bary = np_points(c.vertices[b:b + 1], faces_of(c.faces, b), want, u[b:b + 1])
        assert np.abs(bary[b] - ref_bary[0]).max() <= 4 * EPS32, what
        assert np.abs(points[b] - ref_points[0]).max() <= 8 * EPS32 * np.abs(c.vertices[b]).max(), what
        tri = triangles(c, b)[face[b]]
        on_face = np_pair(points[b], tri[:, 0], tri[:, 1], tri[:, 2]).max()
        worst = max(worst, float(on_face / reference(c.family, c.seed)[b]["unit"]))
    assert worst <= 4, (what, worst)
    return worst
