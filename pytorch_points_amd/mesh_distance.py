"""The exact squared distance between a point cloud and a triangle mesh, over the kept corner lists of
``mesh_laplacian``:

    point_face_distance(points (B,P,3), vertices (B,N,3), faces_or_corners)
                                    ->   PointFaceDistance(dist (B,P), face (B,P) int64, bary (B,P,3))
    face_point_distance(points, vertices, faces_or_corners)
                                    ->   FacePointDistance(dist (B,F), point (B,F) int64, bary (B,F,3))
    PointMeshDistanceLoss(consistent_topology)       mean(point -> face dist) + mean(face -> point dist)

Every (point, triangle) pair is walked; nothing is culled.  **The pair function** of point ``p`` and triangle
``(a, b, c)`` is the region walk of Ericson's closest point on a triangle, in fp32 with every operation rounded on its
own and ``dot(u, v) = (ux vx + uy vy) + uz vz``: with ``ab = b-a, ac = c-a, ap = p-a, bp = p-b, cp = p-c``, ``d1 =
ab.ap, d2 = ac.ap, d3 = ab.bp, d4 = ac.bp, d5 = ab.cp, d6 = ac.cp``, ``vc = d1 d4 - d3 d2``, ``vb = d5 d2 - d1 d6``,
``va = d3 d6 - d5 d4``, the first of these that holds gives the weights:

    1. d1 <= 0 and d2 <= 0                         (1, 0, 0)
    2. d3 >= 0 and d4 <= d3                        (0, 1, 0)
    3. vc <= 0, d1 >= 0, d3 <= 0                   t = d1 / (d1 - d3),                          (1 - t, t, 0)
    4. d6 >= 0 and d5 <= d6                        (0, 0, 1)
    5. vb <= 0, d2 >= 0, d6 <= 0                   t = d2 / (d2 - d6),                          (1 - t, 0, t)
    6. va <= 0, d4 - d3 >= 0, d5 - d6 >= 0         t = (d4 - d3) / ((d4 - d3) + (d5 - d6)),     (0, 1 - t, t)
    7. otherwise                                   t = 1 / ((va + vb) + vc), v = vb t, w = vc t, ((1 - v) - w, v, w)

The closest point is ``q = (w0 a + w1 b) + w2 c``, ``mesh_interpolate``'s formula, and the pair's value ``d = (rx rx +
ry ry) + rz rz`` with ``r = p - q``; so ``dist`` equals ``sqrNorm(points - mesh_interpolate(vertices, corners, face,
bary))`` to the bit.  **The choice**: from ``best = +inf`` and index -1 the pairs are visited in ascending index and
one is taken where ``d < best``: the lowest index wins among equal distances, a NaN ``d`` (a triangle without area can
give one in region 7) is never taken, and a face with a vertex index outside [0,N) is skipped.  An item left with
index -1 (nothing on the other side, a NaN point, only unusable faces) has NaN ``dist`` and ``bary`` and passes no
gradient.  The gradient treats the chosen ``(index, bary)`` as constants, which is exact wherever the choice is locally
unique (the envelope theorem).

CUDA fp32 runs the HIP kernels of csrc/mesh_distance.hip (``pp_mesh_distance_*``, ``pp_mesh_point_face_*``,
``pp_mesh_face_point_*``): one launch for the faces' records and one for a direction; the backward is one elementwise
launch, ``pp_mesh_sample_backward_f32`` for the vertices and, for the points of face -> point, a sum over sorted
point -> face lists -- no floating-point atomics, the same bits on every run, one form only, and nothing synchronises
with the host.  CPU tensors and other dtypes go through ``distance_composition``, the same contract written as torch
operations, which the kernels equal to the bit.  DESIGN.md "Point-to-mesh distances" states the contract.
"""
import collections

import torch

from . import _lib
from . import _mesh_topology as _topology
from . import mesh_sample as _mesh_sample
from .mesh_laplacian import MeshCorners

PointFaceDistance = collections.namedtuple("PointFaceDistance", ["dist", "face", "bary"])
FacePointDistance = collections.namedtuple("FacePointDistance", ["dist", "point", "bary"])

CHUNK_PAIRS = 1 << 22   # pairs of one evaluated block of the composition's (B, P, F) matrix: some 60 temporaries of it
RECORD = 16             # floats of a face record of csrc/mesh_distance.hip


def _check(what, points, vertices, corners):
    _mesh_sample._check(what, vertices, corners)
    if not isinstance(points, torch.Tensor) or not points.is_floating_point():
        raise TypeError("%s: points must be a floating tensor, got %s"
                        % (what, points.dtype if isinstance(points, torch.Tensor) else type(points).__name__))
    if points.dim() != 3 or points.shape[2] != 3 or points.shape[0] != vertices.shape[0]:
        raise ValueError("%s: points must have shape (B, P, 3) with B = %d, got %s"
                         % (what, vertices.shape[0], tuple(points.shape)))
    if points.dtype != vertices.dtype:
        raise TypeError("%s: points are %s but vertices are %s" % (what, points.dtype, vertices.dtype))
    if points.device != vertices.device:
        raise RuntimeError("%s: points are on %s, expected %s" % (what, points.device, vertices.device))


def _check_items(what, name, index, bary, batch):
    if not isinstance(index, torch.Tensor) or not _topology.is_index(index):
        raise TypeError("%s: %s must be an integer tensor, got %s"
                        % (what, name, index.dtype if isinstance(index, torch.Tensor) else type(index).__name__))
    if index.dim() != 2 or index.shape[0] != batch:
        raise ValueError("%s: %s must have shape (B, S) with B = %d, got %s" % (what, name, batch, tuple(index.shape)))
    if not isinstance(bary, torch.Tensor) or not bary.is_floating_point():
        raise TypeError("%s: bary must be a floating tensor" % what)
    if bary.shape != index.shape + (3,):
        raise ValueError("%s: bary must have shape (B, S, 3) = %s, got %s"
                         % (what, tuple(index.shape) + (3,), tuple(bary.shape)))


# ------------------------------------------------------------------------------------------- the composition
def _xyz(t):
    return t[..., 0], t[..., 1], t[..., 2]


def _sub(u, v):
    return u[0] - v[0], u[1] - v[1], u[2] - v[2]


def _dot(u, v):
    return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]


def pair_composition(p, a, b, c, ab, ac):
    """The pair function on triples of broadcastable component tensors: ``(d, w0, w1, w2)``.  All seven regions are
    computed and selected with ``torch.where`` in the contract's order.  A region divides at most once, so the one
    division is of the operands of the first region that holds among those that divide."""
    ap, bp, cp = _sub(p, a), _sub(p, b), _sub(p, c)
    d1, d2 = _dot(ab, ap), _dot(ac, ap)
    d3, d4 = _dot(ab, bp), _dot(ac, bp)
    d5, d6 = _dot(ab, cp), _dot(ac, cp)
    vc = d1 * d4 - d3 * d2
    vb = d5 * d2 - d1 * d6
    va = d3 * d6 - d5 * d4
    e43, e56 = d4 - d3, d5 - d6
    regions = [(d1 <= 0) & (d2 <= 0),
               (d3 >= 0) & (d4 <= d3),
               (vc <= 0) & (d1 >= 0) & (d3 <= 0),
               (d6 >= 0) & (d5 <= d6),
               (vb <= 0) & (d2 >= 0) & (d6 <= 0),
               (va <= 0) & (e43 >= 0) & (e56 >= 0)]
    r3, r5, r6 = regions[2], regions[4], regions[5]
    one, zero = torch.ones_like(d1), torch.zeros_like(d1)
    num = torch.where(r3, d1, torch.where(r5, d2, torch.where(r6, e43, one)))
    den = torch.where(r3, d1 - d3, torch.where(r5, d2 - d6, torch.where(r6, e43 + e56, (va + vb) + vc)))
    t = num / den
    omt = 1 - t
    v7, w7 = vb * t, vc * t
    u7 = (1 - v7) - w7
    weights = []
    for last, row in ((u7, (one, zero, omt, zero, omt, zero)), (v7, (zero, one, t, zero, zero, omt)),
                      (w7, (zero, zero, zero, one, t, t))):
        w = last
        for region, value in zip(reversed(regions), reversed(row)):
            w = torch.where(region, value, w)
        weights.append(w)
    w0, w1, w2 = weights
    r = tuple(p[k] - ((w0 * a[k] + w1 * b[k]) + w2 * c[k]) for k in range(3))
    return _dot(r, r), w0, w1, w2


def _face_corners(vertices, corners):
    """``(a, b, c (B,F,3), valid (B,F))``: the faces' corners, and whether all three indices are in [0,N)"""
    b, n, _ = vertices.shape
    faces = corners.faces.expand(b, -1, -1)
    valid = ((faces >= 0) & (faces < n)).all(-1)
    rows = (faces.clamp(0, n - 1) + torch.arange(b, device=faces.device)[:, None, None] * n).reshape(-1, 3)
    flat = vertices.reshape(b * n, 3)
    return tuple(flat[rows[:, k]].reshape(b, -1, 3) for k in range(3)) + (valid,)


def _first(clean, low, size, dim):
    """the first index along ``dim`` at which ``clean`` equals its minimum ``low``, -1 where that is +inf.
    (``torch.min(dim)`` and ``argmin`` do not promise the first index among ties.)"""
    shape = [1, 1, 1]
    shape[dim] = size
    order = torch.arange(size, device=clean.device).reshape(shape)
    index = torch.where(clean == low.unsqueeze(dim), order, size).amin(dim)
    return torch.where(low < float("inf"), index, torch.full_like(index, -1))


def choice_composition(points, vertices, corners, point_face=True, face_point=True):
    """The choice of the contract as torch operations, not differentiable: ``((face (B,P), bary (B,P,3)) or None,
    (point (B,F), bary (B,F,3)) or None)``.  The (B,P,F) pair matrix is evaluated in blocks of at most ``CHUNK_PAIRS``
    pairs over P (one point where B F alone is beyond that), so the peak memory does not grow with P F."""
    b, p, _ = points.shape
    f = corners.n_faces
    dev, dtype = points.device, points.dtype
    nan = float("nan")
    def nothing(items):
        return (torch.full((b, items), -1, dtype=torch.int64, device=dev),
                torch.full((b, items, 3), nan, dtype=dtype, device=dev))

    pf = nothing(p) if point_face else None
    fp = nothing(f) if face_point else None
    if b == 0 or p == 0 or f == 0 or vertices.shape[1] == 0:
        return pf, fp
    with torch.no_grad():
        a, c1, c2, valid = _face_corners(vertices.detach(), corners)
        ab, ac = c1 - a, c2 - a
        tri = [tuple(x[:, None] for x in _xyz(t)) for t in (a, c1, c2, ab, ac)]   # components (B,1,F)
        inf = torch.full((), float("inf"), dtype=dtype, device=dev)
        best = torch.full((b, f), float("inf"), dtype=dtype, device=dev)
        step = max(1, CHUNK_PAIRS // (b * f))
        for p0 in range(0, p, step):
            block = points.detach()[:, p0:p0 + step]
            pc = block.shape[1]
            d, w0, w1, w2 = pair_composition(tuple(x[:, :, None] for x in _xyz(block)), *tri)
            clean = torch.where((d == d) & valid[:, None, :], d, inf)     # a NaN or an unusable face is never taken
            w = torch.stack([w0, w1, w2], dim=-1)                         # (B,pc,F,3)
            if point_face:
                face = _first(clean, clean.amin(2), f, 2)
                pf[0][:, p0:p0 + pc] = face
                took = w.gather(2, face.clamp(min=0)[:, :, None, None].expand(-1, -1, 1, 3))[:, :, 0]
                pf[1][:, p0:p0 + pc] = torch.where((face >= 0)[..., None], took, torch.full_like(took, nan))
            if face_point:
                low = clean.amin(1)
                index = _first(clean, low, pc, 1)
                better = low < best                                       # ascending blocks: the lowest point stays
                took = w.gather(1, index.clamp(min=0)[:, None, :, None].expand(-1, 1, -1, 3))[:, 0]
                best = torch.where(better, low, best)
                fp[0].copy_(torch.where(better, index + p0, fp[0]))
                fp[1].copy_(torch.where(better[..., None], took, fp[1]))
    return pf, fp


def _anchored_nan(points, vertices, shape):
    """NaN of ``shape`` that hangs on both inputs and passes them a zero gradient"""
    anchor = points.reshape(-1)[:0].sum() + vertices.reshape(-1)[:0].sum()
    never = torch.zeros(shape, dtype=torch.bool, device=points.device)
    return torch.where(never, anchor, torch.full_like(anchor, float("nan")))


def _valid_faces(vertices, corners):
    n = vertices.shape[1]
    return ((corners.faces >= 0) & (corners.faces < n)).all(-1).expand(vertices.shape[0], -1)


def _residual(p, q, ok):
    zero = torch.zeros_like(q)
    r = torch.where(ok[..., None], p, zero) - torch.where(ok[..., None], q, zero)   # (no NaN reaches the backward)
    d = (r[..., 0] * r[..., 0] + r[..., 1] * r[..., 1]) + r[..., 2] * r[..., 2]
    return torch.where(ok, d, torch.full_like(d, float("nan")))


def point_face_at(points, vertices, corners, face, bary):
    """``dist`` (B,P) of the points to the closest points ``(face (B,P), bary (B,P,3))`` given, as differentiable
    torch operations: ``sqrNorm(points - sample_composition(vertices, corners, face, bary))``; NaN and no gradient
    where ``face`` is outside [0,F) or holds a vertex index outside [0,N)."""
    _check("point_face_distance", points, vertices, corners)
    _check_items("point_face_distance", "face", face, bary, points.shape[0])
    b, p, _ = points.shape
    f = corners.n_faces
    if b == 0 or p == 0 or f == 0 or vertices.shape[1] == 0:
        return _anchored_nan(points, vertices, (b, p))
    face = face.long()
    ok = (face >= 0) & (face < f)
    ok = ok & _valid_faces(vertices, corners).gather(1, face.clamp(0, f - 1))
    q = _mesh_sample.sample_composition(vertices, corners, face=torch.where(ok, face, torch.full_like(face, -1)),
                                        bary=bary)[0]
    return _residual(points, q, ok)


def face_point_at(points, vertices, corners, point, bary):
    """``dist`` (B,F) of the faces' closest points ``bary (B,F,3)`` to the points ``point (B,F)`` given, as
    differentiable torch operations; NaN and no gradient where ``point`` is outside [0,P) or the face holds a vertex
    index outside [0,N)."""
    _check("face_point_distance", points, vertices, corners)
    _check_items("face_point_distance", "point", point, bary, points.shape[0])
    b, p, _ = points.shape
    f = corners.n_faces
    if b == 0 or p == 0 or f == 0 or vertices.shape[1] == 0:
        return _anchored_nan(points, vertices, (b, f))
    point = point.long()
    ok = (point >= 0) & (point < p) & _valid_faces(vertices, corners)
    own = torch.arange(f, device=points.device).expand(b, -1)
    q = _mesh_sample.sample_composition(vertices, corners, face=torch.where(ok, own, torch.full_like(own, -1)),
                                        bary=bary)[0]
    rows = point.clamp(0, p - 1) + torch.arange(b, device=points.device)[:, None] * p
    chosen = torch.index_select(points.reshape(b * p, 3), 0, rows.reshape(-1)).reshape(b, f, 3)
    return _residual(chosen, q, ok)


def distance_composition(points, vertices, corners, point_face=True, face_point=True):
    """The contract as torch operations, for any device and floating dtype: ``(PointFaceDistance or None,
    FacePointDistance or None)``.  The choice is ``choice_composition``'s; the distances are ``point_face_at`` and
    ``face_point_at`` on it, whose backward is autograd through ``sample_composition(face=, bary=)`` and a
    subtraction."""
    _check("distance_composition", points, vertices, corners)
    pf, fp = choice_composition(points, vertices, corners, point_face, face_point)
    if pf is not None:
        pf = PointFaceDistance(point_face_at(points, vertices, corners, *pf), *pf)
    if fp is not None:
        fp = FacePointDistance(face_point_at(points, vertices, corners, *fp), *fp)
    return pf, fp


# ------------------------------------------------------------------------------------------------- the kernels
class MeshDistance(torch.autograd.Function):
    """HIP forward and backward (CUDA fp32): ``(points, vertices, corners, per_face)`` -> ``(dist, index, bary)``, per
    point with the faces as ``index`` or, with ``per_face``, per face with the points as ``index``."""

    @staticmethod
    def forward(ctx, points, vertices, corners, per_face):
        dev = _lib.require_cuda(("points", points), ("vertices", vertices), ("faces", corners.faces))
        points, vertices = points.contiguous(), vertices.contiguous()
        b, n, _ = vertices.shape
        p, f = points.shape[1], corners.n_faces
        s = f if per_face else p
        dist = torch.empty(b, s, dtype=torch.float32, device=dev)
        index = torch.empty(b, s, dtype=torch.int64, device=dev)
        bary = torch.empty(b, s, 3, dtype=torch.float32, device=dev)
        if b == 0 or s == 0:
            pass
        elif p == 0 or f == 0 or n == 0:
            dist.fill_(float("nan"))
            index.fill_(-1)
            bary.fill_(float("nan"))
        else:
            records = torch.empty(b, f, RECORD, dtype=torch.float32, device=dev)   # (a capture takes it from its pool)
            lib = _lib.lib()
            entry = lib.pp_mesh_face_point_forward_f32 if per_face else lib.pp_mesh_point_face_forward_f32
            with _lib.on_device(dev) as stream:
                _lib.check(lib.pp_mesh_distance_records_f32(
                    _lib.ptr(vertices), _lib.ptr(corners.faces), _lib.ptr(records), b, n, f, int(corners.batch == 1),
                    stream), "mesh_distance records")
                _lib.check(entry(_lib.ptr(points), _lib.ptr(records), _lib.ptr(dist), _lib.ptr(index), _lib.ptr(bary),
                                 b, p, f, stream), "mesh_distance forward")
        ctx.save_for_backward(points, vertices, index, bary)
        ctx.corners = corners
        ctx.per_face = per_face
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(index, bary)
        return dist, index, bary

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_dist, *_):
        return _distance_backward(ctx, grad_dist) + (None, None)


def _distance_backward(ctx, grad_dist):
    """``(grad_points, grad_vertices)`` of ``dist`` at the chosen ``(index, bary)``, for a context that saved ``(points,
    vertices, index, bary)`` and holds ``corners`` and ``per_face``: ``MeshDistance``'s backward, and that of
    ``mesh_winding.MeshSignedDistance``, whose fused forward makes the same choice."""
    want_points, want_vertices = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
    if grad_dist is None or not (want_points or want_vertices):
        return None, None
    points, vertices, index, bary = ctx.saved_tensors
    corners, per_face = ctx.corners, ctx.per_face
    b, n, _ = vertices.shape
    p, f = points.shape[1], corners.n_faces
    if b == 0 or n == 0 or f == 0 or p == 0:
        return (torch.zeros_like(points) if want_points else None,
                torch.zeros_like(vertices) if want_vertices else None)
    dev = vertices.device
    s = f if per_face else p
    shared = int(corners.batch == 1)
    grad_dist = grad_dist.contiguous()
    grad_points = torch.empty_like(points) if want_points else None
    grad_vertices = torch.empty_like(vertices) if want_vertices else None
    vec = torch.empty(b, f, 3, dtype=torch.float32, device=dev) if per_face and want_points else None
    neg = torch.empty(b, s, 3, dtype=torch.float32, device=dev) if want_vertices else None
    face = torch.empty(b, f, dtype=torch.int64, device=dev) if per_face and want_vertices else None
    opt = lambda t: None if t is None else _lib.ptr(t)   # noqa: E731
    lib = _lib.lib()
    with _lib.on_device(dev) as stream:
        if per_face:
            wsp, nbytes, ws = _topology.workspace(dev, b, p, f) if want_points else (None, 0, None)
            _lib.check(lib.pp_mesh_distance_backward_f32(
                _lib.ptr(points), _lib.ptr(vertices), _lib.ptr(corners.faces), None, _lib.ptr(index),
                _lib.ptr(bary), _lib.ptr(grad_dist), opt(vec), opt(neg), opt(face), opt(grad_points), b, n, f, p,
                shared, wsp, nbytes, stream), "mesh_distance backward")
        else:
            face = index
            _lib.check(lib.pp_mesh_distance_backward_f32(
                _lib.ptr(points), _lib.ptr(vertices), _lib.ptr(corners.faces), _lib.ptr(index), None,
                _lib.ptr(bary), _lib.ptr(grad_dist), opt(grad_points), opt(neg), None, None, b, n, f, p, shared,
                None, 0, stream), "mesh_distance backward")
        if want_vertices:
            scratch = torch.empty(9 * b * f, dtype=torch.float32, device=dev)
            wsp, nbytes, ws = _topology.workspace(dev, b, f, s)
            _lib.check(lib.pp_mesh_sample_backward_f32(
                _lib.ptr(vertices), _lib.ptr(corners.faces), _lib.ptr(corners.start), _lib.ptr(corners.nbr),
                _lib.ptr(corners.codes), _lib.ptr(face), _lib.ptr(bary), _lib.ptr(neg), None, _lib.ptr(scratch),
                _lib.ptr(grad_vertices), b, n, f, s, shared, wsp, nbytes, stream), "mesh_distance vertex gather")
    return grad_points, grad_vertices


def _hip_serves(points, vertices, corners):
    b, n, _ = vertices.shape
    return (vertices.is_cuda and vertices.dtype == torch.float32 and points.dtype == torch.float32
            and b * max(n, corners.n_faces, points.shape[1]) <= _topology.LIMIT
            and 3 * corners.n_faces <= _topology.LIMIT)


# ----------------------------------------------------------------------------------------- the public interface
def point_face_distance(points, vertices, faces_or_corners):
    """For every point of ``points`` (B,P,3) the squared distance to the nearest triangle of the mesh ``vertices``
    (B,N,3), that triangle and the barycentric weights of the closest point on it: the named tuple ``(dist (B,P), face
    (B,P) int64, bary (B,P,3))``.  ``faces_or_corners``: the faces (F,3) or (B,F,3), whose corner lists are then built
    for this call (one host read), or a kept ``MeshCorners``; a topology of one batch element serves every ``b``
    without a copy.  Triangles only.  The module's docstring states the pair function and the choice.  ``dist`` is
    differentiable in ``points`` and ``vertices`` at the chosen ``(face, bary)``; ``face`` and ``bary`` are not.  A
    point left with ``face = -1`` (no faces, a NaN point, only unusable faces) has NaN ``dist`` and ``bary`` and
    passes no gradient.

    CUDA fp32: the HIP kernels, two launches forward; the backward has no floating-point atomics and gives the same
    bits on every run; anything else: ``distance_composition``.  Nothing synchronises with the host."""
    what = "point_face_distance"
    corners = _mesh_sample._corners_of(what, vertices, faces_or_corners)
    _check(what, points, vertices, corners)
    if _hip_serves(points, vertices, corners):
        return PointFaceDistance(*MeshDistance.apply(points, vertices, corners, False))
    return distance_composition(points, vertices, corners, face_point=False)[0]


def face_point_distance(points, vertices, faces_or_corners):
    """For every face of the mesh the squared distance to the nearest point of ``points`` (B,P,3), measured to the
    triangle and not to its plane, that point and the barycentric weights of the triangle's point closest to it: the
    named tuple ``(dist (B,F), point (B,F) int64, bary (B,F,3))``.  The lowest point index wins among equal distances.
    Arguments, gradients, ``point = -1`` and the two paths are ``point_face_distance``'s."""
    what = "face_point_distance"
    corners = _mesh_sample._corners_of(what, vertices, faces_or_corners)
    _check(what, points, vertices, corners)
    if _hip_serves(points, vertices, corners):
        return FacePointDistance(*MeshDistance.apply(points, vertices, corners, True))
    return distance_composition(points, vertices, corners, point_face=False)[1]


class PointMeshDistanceLoss(torch.nn.Module):
    """``mean(point -> face dist) + mean(face -> point dist)`` between the cloud ``points`` (B,P,3) and the mesh
    ``vertices`` (B,N,3) over ``faces`` (B,F,3) or a shared (F,3): the exact counterpart of
    ``SampledMeshChamferLoss``.  ``self.E`` is the ``MeshCorners`` of the last build; it is kept, and never checked
    against later faces, while ``consistent_topology`` is set."""

    def __init__(self, consistent_topology=False):
        super().__init__()
        self.consistent_topology = consistent_topology
        self.E = None

    def forward(self, points, vertices, faces=None):
        if (not self.consistent_topology) or (self.E is None):
            assert(faces is not None), "Face is required"
            self.E = MeshCorners.from_faces(faces.to(vertices.device), vertices.shape[1])
        return (point_face_distance(points, vertices, self.E).dist.mean()
                + face_point_distance(points, vertices, self.E).dist.mean())
