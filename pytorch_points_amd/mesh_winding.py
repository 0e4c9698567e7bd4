"""The winding number of a triangle mesh about the points of a cloud, and with it the side that
``mesh_distance.point_face_distance`` lacks: a signed point-to-mesh distance and an enclosure loss.

    mesh_winding_number(points (B,P,3), vertices (B,N,3), faces_or_corners)      ->   winding (B,P)
    points_inside_mesh(points, vertices, faces_or_corners)                       ->   inside (B,P) bool
    point_mesh_signed_distance(points, vertices, faces_or_corners)
                    ->   PointMeshSignedDistance(signed (B,P), dist (B,P), face (B,P) int64, bary (B,P,3), winding (B,P))
    MeshEnclosureLoss(side, margin, consistent_topology)      mean(relu(margin +- signed)^2)

Every (point, triangle) pair is walked; nothing is culled or approximated.  **The pair's half solid angle** of point
``p`` and a face ``(a, b, c)`` is Van Oosterom and Strackee's, in fp32 with every operation rounded on its own and
``dot(x, y) = (x0 y0 + x1 y1) + x2 y2``: with ``u = a - p, v = b - p, w = c - p``, ``lu = sqrt(dot(u, u))`` and ``lv``,
``lw`` likewise, ``x = cross(v, w)`` (each component two products and their difference), ``det = dot(u, x)`` and

    den = (((lu lv) lw + dot(u, v) lw) + dot(v, w) lu) + dot(w, u) lv,              h = atan2(det, den).

**Per point** the halves are added in fp64 in ascending face order from +0, and ``winding = (float)(sum / (2 pi))``,
rounded once.  A face with a vertex index outside [0,N) adds nothing.  A closed mesh whose faces are oriented outwards
gives +1 inside and 0 outside; flipping the orientation negates the value; an open mesh gives a fraction; ``inside =
winding > 0.5``.  A NaN point gives a NaN ``winding`` (where a usable face is there to be seen) and ``inside =
False``; no faces or no vertices give ``winding = 0``.  On the surface itself the value is finite and means nothing
(about a half on a face).  ``winding`` and ``inside`` are **not differentiable** (``mark_non_differentiable``): the
winding number is piecewise constant away from the surface, and its derivative is not built.

**The signed distance**: ``dist``, ``face`` and ``bary`` are ``point_face_distance``'s, to the bit, and ``signed`` is
``-sqrt(dist)`` where ``winding > 0.5`` and ``+sqrt(dist)`` elsewhere, as torch elementwise operations on (B,P).  Its
gradient is finite: where ``dist == 0``, ``signed = 0`` and passes no gradient; where ``face = -1`` (no faces, a NaN
point, only unusable faces), ``signed`` and ``dist`` are NaN and pass none.  The gradient of ``dist`` is
``point_face_distance``'s own.

CUDA fp32 runs the HIP kernels of csrc/mesh_winding.hip on the face records of csrc/mesh_distance.hip: one launch for
the records and one walk, ``pp_mesh_winding_forward_f32`` for the winding number alone and
``pp_mesh_signed_distance_forward_f32`` for the winding number and the distance's choice in the same walk; the backward
is ``point_face_distance``'s (``mesh_distance._distance_backward``).  No atomics, the same bits on every run, nothing
synchronises with the host.  CPU tensors and other dtypes go through ``winding_composition`` and
``signed_distance_composition``, the same contract as torch operations (torch's fp64 sum is not promised to run in
ascending order, and a host's ``atan2`` may differ from the device's in its last bits).  DESIGN.md "Mesh winding numbers
and signed distance" states the contract.
"""
import collections
import math

import torch

from . import _lib
from . import mesh_distance as _mesh_distance
from . import mesh_sample as _mesh_sample
from .mesh_laplacian import MeshCorners

PointMeshSignedDistance = collections.namedtuple("PointMeshSignedDistance",
                                                 ["signed", "dist", "face", "bary", "winding"])

CHUNK_PAIRS = 1 << 22   # pairs of one evaluated block of the composition's (B, P, F) matrix: some 40 temporaries of it


# ------------------------------------------------------------------------------------------- the composition
def half_angle_composition(p, a, b, c):
    """The pair's half solid angle on triples of broadcastable component tensors, in their dtype"""
    sub, dot = _mesh_distance._sub, _mesh_distance._dot
    u, v, w = sub(a, p), sub(b, p), sub(c, p)
    lu, lv, lw = torch.sqrt(dot(u, u)), torch.sqrt(dot(v, v)), torch.sqrt(dot(w, w))
    x = (v[1] * w[2] - v[2] * w[1], v[2] * w[0] - v[0] * w[2], v[0] * w[1] - v[1] * w[0])
    det = dot(u, x)
    den = (((lu * lv) * lw + dot(u, v) * lw) + dot(v, w) * lu) + dot(w, u) * lv
    return torch.atan2(det, den)


def winding_composition(points, vertices, corners):
    """The winding number of the contract as torch operations, for any device and floating dtype, not differentiable:
    ``winding`` (B,P) in the points' dtype.  The halves are computed in that dtype and summed with ``.double()``.  The
    (B,P,F) pair matrix is evaluated in blocks of at most ``CHUNK_PAIRS`` pairs over P (one point where B F alone is
    beyond that), so the peak memory does not grow with P F."""
    _mesh_distance._check("winding_composition", points, vertices, corners)
    b, p, _ = points.shape
    f = corners.n_faces
    out = torch.zeros(b, p, dtype=points.dtype, device=points.device)
    if b == 0 or p == 0 or f == 0 or vertices.shape[1] == 0:
        return out
    xyz = _mesh_distance._xyz
    with torch.no_grad():
        a, c1, c2, valid = _mesh_distance._face_corners(vertices.detach(), corners)
        tri = [tuple(x[:, None] for x in xyz(t)) for t in (a, c1, c2)]           # components (B,1,F)
        step = max(1, CHUNK_PAIRS // (b * f))
        for p0 in range(0, p, step):
            block = points.detach()[:, p0:p0 + step]
            h = half_angle_composition(tuple(x[:, :, None] for x in xyz(block)), *tri)
            h = torch.where(valid[:, None, :], h, torch.zeros_like(h))            # an unusable face adds nothing
            out[:, p0:p0 + step] = (h.double().sum(-1) / (2 * math.pi)).to(points.dtype)
    return out


def _signed(dist, face, winding):
    """``signed`` (B,P) from ``dist``: elementwise, with a finite gradient (module docstring)"""
    ok = dist > 0                                                                  # (false for NaN too)
    root = torch.sqrt(torch.where(ok, dist, torch.ones_like(dist)))
    size = torch.where(ok, root, torch.zeros_like(dist))
    size = torch.where(face < 0, torch.full_like(size, float("nan")), size)
    return torch.where(winding > 0.5, -size, size)


def signed_distance_composition(points, vertices, corners):
    """``point_mesh_signed_distance``'s contract as torch operations, for any device and floating dtype:
    ``distance_composition``'s point -> face half, ``winding_composition`` and the sign."""
    _mesh_distance._check("signed_distance_composition", points, vertices, corners)
    pf = _mesh_distance.distance_composition(points, vertices, corners, face_point=False)[0]
    winding = winding_composition(points, vertices, corners)
    return PointMeshSignedDistance(_signed(pf.dist, pf.face, winding), pf.dist, pf.face, pf.bary, winding)


# ------------------------------------------------------------------------------------------------- the kernels
def _records(lib, vertices, corners, stream):
    b, n, _ = vertices.shape
    f = corners.n_faces
    records = torch.empty(b, f, _mesh_distance.RECORD, dtype=torch.float32, device=vertices.device)
    _lib.check(lib.pp_mesh_distance_records_f32(
        _lib.ptr(vertices), _lib.ptr(corners.faces), _lib.ptr(records), b, n, f, int(corners.batch == 1), stream),
        "mesh_winding records")
    return records


class MeshWinding(torch.autograd.Function):
    """HIP forward (CUDA fp32): ``(points, vertices, corners)`` -> ``winding`` (B,P); no backward"""

    @staticmethod
    def forward(ctx, points, vertices, corners):
        dev = _lib.require_cuda(("points", points), ("vertices", vertices), ("faces", corners.faces))
        points, vertices = points.contiguous(), vertices.contiguous()
        b, n, _ = vertices.shape
        p, f = points.shape[1], corners.n_faces
        winding = torch.empty(b, p, dtype=torch.float32, device=dev)
        if b == 0 or p == 0:
            pass
        elif f == 0 or n == 0:
            winding.zero_()
        else:
            lib = _lib.lib()
            with _lib.on_device(dev) as stream:
                records = _records(lib, vertices, corners, stream)
                _lib.check(lib.pp_mesh_winding_forward_f32(_lib.ptr(points), _lib.ptr(records), _lib.ptr(winding),
                                                           b, p, f, stream), "mesh_winding forward")
        ctx.mark_non_differentiable(winding)
        return winding

    @staticmethod
    def backward(ctx, *_):
        return None, None, None


class MeshSignedDistance(torch.autograd.Function):
    """HIP forward and backward (CUDA fp32): ``(points, vertices, corners)`` -> ``(dist, face, bary, winding)`` from
    one walk; the backward is ``mesh_distance.MeshDistance``'s for the points' direction."""

    @staticmethod
    def forward(ctx, points, vertices, corners):
        dev = _lib.require_cuda(("points", points), ("vertices", vertices), ("faces", corners.faces))
        points, vertices = points.contiguous(), vertices.contiguous()
        b, n, _ = vertices.shape
        p, f = points.shape[1], corners.n_faces
        dist = torch.empty(b, p, dtype=torch.float32, device=dev)
        face = torch.empty(b, p, dtype=torch.int64, device=dev)
        bary = torch.empty(b, p, 3, dtype=torch.float32, device=dev)
        winding = torch.empty(b, p, dtype=torch.float32, device=dev)
        if b == 0 or p == 0:
            pass
        elif f == 0 or n == 0:
            dist.fill_(float("nan"))
            face.fill_(-1)
            bary.fill_(float("nan"))
            winding.zero_()
        else:
            lib = _lib.lib()
            with _lib.on_device(dev) as stream:
                records = _records(lib, vertices, corners, stream)
                _lib.check(lib.pp_mesh_signed_distance_forward_f32(
                    _lib.ptr(points), _lib.ptr(records), _lib.ptr(dist), _lib.ptr(face), _lib.ptr(bary),
                    _lib.ptr(winding), b, p, f, stream), "mesh_signed_distance forward")
        ctx.save_for_backward(points, vertices, face, bary)
        ctx.corners = corners
        ctx.per_face = False
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(face, bary, winding)
        return dist, face, bary, winding

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_dist, *_):
        return _mesh_distance._distance_backward(ctx, grad_dist) + (None,)


# ----------------------------------------------------------------------------------------- the public interface
def _resolve(what, points, vertices, faces_or_corners):
    corners = _mesh_sample._corners_of(what, vertices, faces_or_corners)
    _mesh_distance._check(what, points, vertices, corners)
    return corners


def mesh_winding_number(points, vertices, faces_or_corners):
    """The winding number of the mesh ``vertices`` (B,N,3) about every point of ``points`` (B,P,3): (B,P), +1 inside a
    closed mesh whose faces are oriented outwards and 0 outside it.  ``faces_or_corners``: the faces (F,3) or (B,F,3),
    whose corner lists are then built for this call (one host read), or a kept ``MeshCorners`` (none); a topology of
    one batch element serves every ``b`` without a copy.  Triangles only.  The module's docstring states the pair's
    solid angle and the sum.  Not differentiable.

    CUDA fp32: the HIP kernels, two launches; anything else: ``winding_composition``.  Nothing synchronises with the
    host."""
    corners = _resolve("mesh_winding_number", points, vertices, faces_or_corners)
    if _mesh_distance._hip_serves(points, vertices, corners):
        return MeshWinding.apply(points, vertices, corners)
    return winding_composition(points, vertices, corners)


def points_inside_mesh(points, vertices, faces_or_corners):
    """``mesh_winding_number(...) > 0.5``: (B,P) bool; False for a NaN point.  Arguments and paths are
    ``mesh_winding_number``'s."""
    corners = _resolve("points_inside_mesh", points, vertices, faces_or_corners)
    return mesh_winding_number(points, vertices, corners) > 0.5


def point_mesh_signed_distance(points, vertices, faces_or_corners):
    """The signed distance of every point of ``points`` (B,P,3) to the mesh ``vertices`` (B,N,3), negative inside: the
    named tuple ``(signed (B,P), dist (B,P), face (B,P) int64, bary (B,P,3), winding (B,P))``.  ``dist``, ``face`` and
    ``bary`` are ``point_face_distance``'s, to the bit, ``winding`` is ``mesh_winding_number``'s, and ``signed`` is
    ``-sqrt(dist)`` where ``winding > 0.5`` and ``sqrt(dist)`` elsewhere.  ``signed`` and ``dist`` are differentiable
    in ``points`` and ``vertices`` at the chosen ``(face, bary)``; the others are not.  Where ``dist == 0``, ``signed =
    0`` and passes no gradient; where ``face = -1``, ``signed`` and ``dist`` are NaN and pass none.  Arguments are
    ``mesh_winding_number``'s.

    CUDA fp32: the HIP kernels, two launches forward, the winding number and the distance from one walk; the backward
    is ``point_face_distance``'s; anything else: ``signed_distance_composition``."""
    corners = _resolve("point_mesh_signed_distance", points, vertices, faces_or_corners)
    if not _mesh_distance._hip_serves(points, vertices, corners):
        return signed_distance_composition(points, vertices, corners)
    dist, face, bary, winding = MeshSignedDistance.apply(points, vertices, corners)
    return PointMeshSignedDistance(_signed(dist, face, winding), dist, face, bary, winding)


class MeshEnclosureLoss(torch.nn.Module):
    """How far the points ``points`` (B,P,3) are on the wrong side of the mesh ``vertices`` (B,N,3) over ``faces``
    (B,F,3) or a shared (F,3), whose faces are oriented outwards: with ``side="inside"`` the points are to lie inside
    by ``margin``, ``mean(relu(signed + margin)^2)``; with ``side="outside"``, outside by it, ``mean(relu(margin -
    signed)^2)``, ``signed`` being ``point_mesh_signed_distance``'s.  At ``margin = 0`` that is ``dist`` over the points
    on the wrong side and 0 over the others.  An item whose ``signed`` is NaN is left out of the mean's numerator and
    counted in its denominator.  ``self.E`` is the ``MeshCorners`` of the last build; it is kept, and never checked
    against later faces, while ``consistent_topology`` is set."""

    def __init__(self, side="inside", margin=0.0, consistent_topology=False):
        super().__init__()
        if side not in ("inside", "outside"):
            raise ValueError("MeshEnclosureLoss: side must be 'inside' or 'outside', got %r" % (side,))
        self.side = side
        self.margin = margin
        self.consistent_topology = consistent_topology
        self.E = None

    def forward(self, points, vertices, faces=None):
        if (not self.consistent_topology) or (self.E is None):
            assert(faces is not None), "Face is required"
            self.E = MeshCorners.from_faces(faces.to(vertices.device), vertices.shape[1])
        signed = point_mesh_signed_distance(points, vertices, self.E).signed
        missing = torch.isnan(signed)
        signed = torch.where(missing, torch.zeros_like(signed), signed)           # (no NaN reaches the backward)
        over = torch.relu(signed + self.margin if self.side == "inside" else self.margin - signed)
        return torch.where(missing, torch.zeros_like(over), over * over).mean()
