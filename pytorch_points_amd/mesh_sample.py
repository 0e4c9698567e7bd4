"""The step from a triangle mesh to a cloud of points on its surface, over the kept corner lists of ``mesh_laplacian``:

    mesh_sample_faces(areas (B,F), u (B,S))                       ->   face (B,S) int64, drawn in proportion to area
    mesh_interpolate(vertices (B,N,3), corners, face, bary)       ->   points (B,S,3): a sample set on a deformed mesh
    sample_points_from_meshes(vertices, faces_or_corners, num_samples, return_normals, generator, u)
                                                                  ->   (points, face, bary[, normals])
    SampledMeshChamferLoss(num_samples, consistent_topology)      the Chamfer distance of a sampled mesh to a cloud

With ``u`` (B,S,3) fp32 in [0,1): ``cdf`` is the fp64 inclusive prefix sum of the fp32 face areas, ``face`` the first
``f`` with ``cdf[f] > double(u1) * cdf[F-1]`` (a face without area is never chosen; a mesh whose total area is not a
positive finite number gives ``face = -1`` and NaN), and with ``su = sqrt(u2)`` the weights are ``bary = (1 - su,
su (1 - u3), su u3)`` and ``points = (w0 p0 + w1 p1) + w2 p2``, all in fp32 with every operation rounded on its own.
``normals`` are the chosen faces' rows of ``mesh_face_normals``.

CUDA fp32 runs the HIP kernels of csrc/mesh_sample.hip (``pp_mesh_sample_*``): the CDF is one launch and a sample set
one more; the backward builds the face -> sample lists of the call, sums per face in sample order and gathers per
vertex over the sorted corner slice -- no floating-point atomics, the same bits on every run, one form only, and
nothing synchronises with the host.  CPU tensors and other dtypes go through ``sample_composition``, the same contract
written as torch operations.  DESIGN.md "Mesh surface sampling" states the contract.
"""
import collections

import torch

from . import _lib
from . import _mesh_topology as _topology
from . import mesh_normals as _mesh_normals
from .mesh_laplacian import MeshCorners

MeshSamples = collections.namedtuple("MeshSamples", ["points", "face", "bary"])
MeshSamplesWithNormals = collections.namedtuple("MeshSamplesWithNormals", ["points", "face", "bary", "normals"])


def _check(what, vertices, corners):
    _topology.check_vertices(what, vertices, corners, MeshCorners, "corners", "faces", d3=True)
    if corners.degree != 3:
        raise NotImplementedError("%s: triangles only, got faces of %d corners" % (what, corners.degree))


def _check_u(what, u, batch, cols, device):
    shape = "(B, S, 3)" if cols else "(B, S)"
    if not isinstance(u, torch.Tensor) or u.dtype != torch.float32:
        raise TypeError("%s: u must be a float32 tensor, got %s"
                        % (what, u.dtype if isinstance(u, torch.Tensor) else type(u).__name__))
    if u.dim() != (3 if cols else 2) or u.shape[0] != batch or (cols and u.shape[2] != 3):
        raise ValueError("%s: u must have shape %s with B = %d, got %s" % (what, shape, batch, tuple(u.shape)))
    if u.device != device:
        raise RuntimeError("%s: u is on %s, expected %s" % (what, u.device, device))


def _check_samples(what, vertices, face, bary):
    if not isinstance(face, torch.Tensor) or not _topology.is_index(face):
        raise TypeError("%s: face must be an integer tensor, got %s"
                        % (what, face.dtype if isinstance(face, torch.Tensor) else type(face).__name__))
    if face.dim() != 2 or face.shape[0] != vertices.shape[0]:
        raise ValueError("%s: face must have shape (B, S) with B = %d, got %s"
                         % (what, vertices.shape[0], tuple(face.shape)))
    if not isinstance(bary, torch.Tensor) or not bary.is_floating_point():
        raise TypeError("%s: bary must be a floating tensor" % what)
    if bary.shape != face.shape + (3,):
        raise ValueError("%s: bary must have shape (B, S, 3) = %s, got %s"
                         % (what, tuple(face.shape) + (3,), tuple(bary.shape)))
    for name, t in (("face", face), ("bary", bary)):
        if t.device != vertices.device:
            raise RuntimeError("%s: %s is on %s, expected %s" % (what, name, t.device, vertices.device))


# ------------------------------------------------------------------------------------------- the composition
def faces_composition(areas, u1):
    """``mesh_sample_faces`` as torch operations: ``cumsum`` in fp64 and ``searchsorted(right=True)``"""
    b, f = areas.shape
    if f == 0 or u1.shape[1] == 0:
        return torch.full(u1.shape, -1, dtype=torch.int64, device=areas.device)
    cdf = torch.cumsum(areas.double(), dim=1)
    total = cdf[:, -1:]
    face = torch.searchsorted(cdf, (u1.double() * total).contiguous(), right=True)
    ok = (total > 0) & torch.isfinite(total) & (face < f)
    return torch.where(ok, face, torch.full_like(face, -1))


def bary_composition(u):
    """``(1 - su, su (1 - u3), su u3)`` with ``su = sqrt(u2)`` of fp32 ``u`` (B,S,3), every operation on its own.
    The root is taken in fp64 and rounded to fp32, which is the correctly rounded fp32 root (53 >= 2 * 24 + 2 bits):
    ``torch.sqrt`` of an fp32 CPU tensor is not correctly rounded in every torch build."""
    su = torch.sqrt(u[..., 1].double()).float()
    return torch.stack([1 - su, su * (1 - u[..., 2]), su * u[..., 2]], dim=-1)


def sample_composition(vertices, corners, u=None, face=None, bary=None, return_normals=False):
    """The contract as torch operations, for any device and floating dtype: ``(points, face, bary[, normals])`` from
    ``u`` (B,S,3) fp32, or from a given ``face`` (B,S) and ``bary`` (B,S,3).  The weights are computed in fp32 and
    cast to the vertices' dtype; the corners are gathered with ``index_select``, whose backward is ``index_add_`` in
    sample order.  A sample whose face is outside [0,F), or whose face holds a vertex index outside [0,N), is NaN and
    passes no gradient."""
    _check("sample_points_from_meshes", vertices, corners)
    b, n, _ = vertices.shape
    f = corners.n_faces
    s = (u if u is not None else face).shape[1]
    nan = vertices.new_full((b, s, 3), float("nan"))
    if f == 0 or n == 0 or b == 0 or s == 0:
        if u is not None:
            face, bary = torch.full((b, s), -1, dtype=torch.int64, device=vertices.device), nan.clone()
        out = (nan, face.long(), bary.to(vertices.dtype))
        return out + (nan.clone(),) if return_normals else out
    if u is not None or return_normals:
        normals_of, areas = _mesh_normals.face_normals_composition(vertices, corners)
    if u is not None:
        face = faces_composition(areas.detach(), u[..., 0])
        bary = bary_composition(u)
        bary = torch.where((face >= 0)[..., None], bary, torch.full_like(bary, float("nan")))
    face = face.long()
    bary = bary.to(vertices.dtype)
    ok = (face >= 0) & (face < f)
    rows = face.clamp(0, f - 1) + (0 if corners.batch == 1 else torch.arange(b, device=face.device)[:, None] * f)
    tri = corners.faces.reshape(-1, 3)[rows.reshape(-1)].reshape(b, s, 3)
    ok = ok & ((tri >= 0) & (tri < n)).all(-1)
    tri = tri.clamp(0, n - 1) + torch.arange(b, device=face.device)[:, None, None] * n
    flat = vertices.reshape(b * n, 3)
    p0, p1, p2 = (torch.index_select(flat, 0, tri[..., k].reshape(-1)).reshape(b, s, 3) for k in range(3))
    w = torch.where(ok[..., None], bary, torch.zeros_like(bary))       # (a NaN weight times a zero gradient is NaN)
    points = (w[..., 0:1] * p0 + w[..., 1:2] * p1) + w[..., 2:3] * p2
    points = torch.where(ok[..., None], points, nan)
    if not return_normals:
        return points, face, bary
    per_batch = face.clamp(0, f - 1) + torch.arange(b, device=face.device)[:, None] * f
    normals = torch.index_select(normals_of.reshape(b * f, 3), 0, per_batch.reshape(-1)).reshape(b, s, 3)
    return points, face, bary, torch.where(ok[..., None], normals, nan)


# ------------------------------------------------------------------------------------------------- the kernels
def _cdf(areas):
    """contiguous CUDA fp32 ``areas`` (B,F), B and F > 0 -> fp64 (B,F), one launch"""
    b, f = areas.shape
    cdf = torch.empty(b, f, dtype=torch.float64, device=areas.device)
    with _lib.on_device(areas.device) as stream:
        _lib.check(_lib.lib().pp_mesh_sample_cdf_f32(_lib.ptr(areas), _lib.ptr(cdf), b, f, stream), "mesh_sample cdf")
    return cdf


class MeshSamplePoints(torch.autograd.Function):
    """HIP forward and backward (CUDA fp32): ``(vertices, corners, u, face, bary, want_normals)`` ->
    ``(points, face, bary[, normals])``; either ``u`` is given, or ``face`` and ``bary`` are."""

    @staticmethod
    def forward(ctx, vertices, corners, u, face, bary, want_normals):
        dev = _lib.require_cuda(("vertices", vertices), ("faces", corners.faces))
        vertices = vertices.contiguous()
        b, n, _ = vertices.shape
        f = corners.n_faces
        choose = u is not None
        if choose:
            u = u.contiguous()
            s = u.shape[1]
            face = torch.empty(b, s, dtype=torch.int64, device=dev)
            bary = torch.empty(b, s, 3, dtype=torch.float32, device=dev)
        else:
            face, bary = face.contiguous(), bary.contiguous()
            s = face.shape[1]
        points = torch.empty(b, s, 3, dtype=torch.float32, device=dev)
        normals = torch.empty(b, s, 3, dtype=torch.float32, device=dev) if want_normals else None
        if b == 0 or s == 0:
            pass
        elif f == 0 or n == 0:
            points.fill_(float("nan"))
            if want_normals:
                normals.fill_(float("nan"))
            if choose:
                face.fill_(-1)
                bary.fill_(float("nan"))
        else:
            shared = int(corners.batch == 1)
            lib = _lib.lib()
            with _lib.on_device(dev) as stream:
                cdf = face_normals = None
                if choose or want_normals:
                    face_normals = torch.empty(b, f, 3, dtype=torch.float32, device=dev)
                    areas = torch.empty(b, f, dtype=torch.float32, device=dev)
                    _lib.check(lib.pp_mesh_face_normals_forward_f32(
                        _lib.ptr(vertices), _lib.ptr(corners.faces), _lib.ptr(face_normals), _lib.ptr(areas), b, n, f,
                        shared, stream), "mesh_sample face areas")
                if choose:
                    cdf = _cdf(areas)
                _lib.check(lib.pp_mesh_sample_forward_f32(
                    _lib.ptr(vertices), _lib.ptr(corners.faces), None if cdf is None else _lib.ptr(cdf),
                    _lib.ptr(u) if choose else None, 3 if choose else 0, None if choose else _lib.ptr(face),
                    None if choose else _lib.ptr(bary), _lib.ptr(face_normals) if want_normals else None,
                    _lib.ptr(face) if choose else None, _lib.ptr(bary) if choose else None, _lib.ptr(points),
                    _lib.ptr(normals) if want_normals else None, b, n, f, s, shared, stream), "mesh_sample forward")
        ctx.save_for_backward(vertices, face, bary)
        ctx.corners = corners
        ctx.set_materialize_grads(False)
        if choose:
            ctx.mark_non_differentiable(face, bary)
            out = (points, face, bary)
        else:
            out = (points,)
        return out + (normals,) if want_normals else out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_points, *rest):
        grad_normals = rest[-1] if len(rest) in (1, 3) else None
        if not ctx.needs_input_grad[0] or (grad_points is None and grad_normals is None):
            return (None,) * 6
        vertices, face, bary = ctx.saved_tensors
        corners = ctx.corners
        b, n, _ = vertices.shape
        f, s = corners.n_faces, face.shape[1]
        if b == 0 or n == 0 or f == 0 or s == 0:
            return (torch.zeros_like(vertices),) + (None,) * 5
        dev = vertices.device
        grad_points = None if grad_points is None else grad_points.contiguous()
        grad_normals = None if grad_normals is None else grad_normals.contiguous()
        floats = 9 * b * f + (0 if grad_normals is None else 3 * b * f + 3 * b * n)
        scratch = torch.empty(floats, dtype=torch.float32, device=dev)   # (torch.empty: a capture takes it from its pool)
        grad = torch.empty_like(vertices)
        with _lib.on_device(dev) as stream:
            wsp, nbytes, ws = _topology.workspace(dev, b, f, s)
            _lib.check(_lib.lib().pp_mesh_sample_backward_f32(
                _lib.ptr(vertices), _lib.ptr(corners.faces), _lib.ptr(corners.start), _lib.ptr(corners.nbr),
                _lib.ptr(corners.codes), _lib.ptr(face), _lib.ptr(bary),
                None if grad_points is None else _lib.ptr(grad_points),
                None if grad_normals is None else _lib.ptr(grad_normals), _lib.ptr(scratch), _lib.ptr(grad), b, n, f, s,
                int(corners.batch == 1), wsp, nbytes, stream), "mesh_sample backward")
        return (grad,) + (None,) * 5


def _hip_serves(vertices, corners, samples, *others):
    b, n, _ = vertices.shape
    return (vertices.is_cuda and vertices.dtype == torch.float32
            and all(t.dtype == torch.float32 for t in others)
            and b * max(n, corners.n_faces, samples) <= _topology.LIMIT and 3 * corners.n_faces <= _topology.LIMIT)


# ----------------------------------------------------------------------------------------- the public interface
def mesh_sample_faces(areas, u):
    """``face`` (B,S) int64 for ``areas`` (B,F) and ``u`` (B,S) fp32 in [0,1): the first ``f`` with ``cdf[b,f] >
    double(u[b,s]) * cdf[b,F-1]``, ``cdf`` the fp64 inclusive prefix sum of ``areas[b,:]``; -1 for every sample of a
    ``b`` whose total is not a positive finite number (``F == 0`` among it).  A face without area is never chosen.
    Not differentiable.

    CUDA fp32: two HIP launches (the CDF with a fixed association, then one lane per sample); anything else:
    ``faces_composition``.  Nothing synchronises with the host."""
    what = "mesh_sample_faces"
    if not isinstance(areas, torch.Tensor) or not areas.is_floating_point():
        raise TypeError("%s: areas must be a floating tensor" % what)
    if areas.dim() != 2:
        raise ValueError("%s: areas must have shape (B, F), got %s" % (what, tuple(areas.shape)))
    _check_u(what, u, areas.shape[0], False, areas.device)
    b, f = areas.shape
    s = u.shape[1]
    areas = areas.detach()
    if not (areas.is_cuda and areas.dtype == torch.float32 and b * max(f, s) <= _topology.LIMIT):
        return faces_composition(areas, u)
    face = torch.full((b, s), -1, dtype=torch.int64, device=areas.device)
    if b == 0 or f == 0 or s == 0:
        return face
    cdf = _cdf(areas.contiguous())
    u = u.contiguous()
    with _lib.on_device(areas.device) as stream:
        _lib.check(_lib.lib().pp_mesh_sample_forward_f32(
            None, None, _lib.ptr(cdf), _lib.ptr(u), 1, None, None, None, _lib.ptr(face), None, None, None, b, 0, f, s,
            0, stream), "mesh_sample faces")
    return face


def mesh_interpolate(vertices, corners, face, bary):
    """``points`` (B,S,3) of the samples ``(face (B,S), bary (B,S,3))`` on the triangle mesh ``corners`` (a
    ``MeshCorners``) over ``vertices`` (B,N,3): ``(w0 p0 + w1 p1) + w2 p2`` with ``p_k = vertices[b, faces[face,k]]``.
    Handing the ``face`` and ``bary`` of ``sample_points_from_meshes`` to a deformed mesh of the same connectivity
    re-evaluates the same sample set there, in correspondence.  Differentiable in ``vertices`` only.  A ``face``
    outside [0,F) gives NaN and passes no gradient.  A topology of one batch element serves every ``b`` without a
    copy.

    CUDA fp32: one HIP launch forward, and the gather backward of ``sample_points_from_meshes``; anything else:
    ``sample_composition``.  Nothing synchronises with the host."""
    _check("mesh_interpolate", vertices, corners)
    _check_samples("mesh_interpolate", vertices, face, bary)
    if _hip_serves(vertices, corners, face.shape[1], bary):
        return MeshSamplePoints.apply(vertices, corners, None, face.long(), bary, False)[0]
    return sample_composition(vertices, corners, face=face, bary=bary)[0]


def _corners_of(what, vertices, faces_or_corners):
    from .network.geo_operations import _corners_of as resolve   # (that module re-exports this one's names)
    return resolve(what, vertices, faces_or_corners)


def sample_points_from_meshes(vertices, faces_or_corners, num_samples=None, return_normals=False, generator=None,
                              u=None):
    """``num_samples`` points on the surface of every triangle mesh of the batch, drawn uniformly by area: the named
    tuple ``(points (B,S,3), face (B,S) int64, bary (B,S,3)[, normals (B,S,3)])``.  ``faces_or_corners``: the faces
    (F,3) or (B,F,3), whose corner lists are then built for this call (one host read), or a kept ``MeshCorners``.
    ``u`` (B,S,3) fp32 in [0,1) are the random numbers; without it they are ``torch.rand((B,S,3), device=...,
    generator=generator)``, and with it ``num_samples`` may be None.  The module's docstring states how a sample
    follows from its three numbers.  ``points`` and ``normals`` (the chosen faces' rows of ``mesh_face_normals``) are
    differentiable in ``vertices``; ``face`` and ``bary`` are not.  A batch element whose total area is not a positive
    finite number (a mesh without faces among it) gets ``face = -1`` and NaN, and no gradient.

    CUDA fp32: the HIP kernels, three launches forward; the backward has no floating-point atomics and gives the same
    bits on every run (``torch.use_deterministic_algorithms`` changes nothing); anything else:
    ``sample_composition``.  Nothing synchronises with the host."""
    what = "sample_points_from_meshes"
    corners = _corners_of(what, vertices, faces_or_corners)
    _check(what, vertices, corners)
    if u is None:
        if num_samples is None or int(num_samples) < 0:
            raise ValueError("%s: num_samples must be a non-negative integer where u is not given, got %r"
                             % (what, num_samples))
        u = torch.rand((vertices.shape[0], int(num_samples), 3), device=vertices.device, generator=generator)
    else:
        _check_u(what, u, vertices.shape[0], True, vertices.device)
        if num_samples is not None and int(num_samples) != u.shape[1]:
            raise ValueError("%s: num_samples is %d but u holds %d samples" % (what, int(num_samples), u.shape[1]))
    if _hip_serves(vertices, corners, u.shape[1]):
        out = MeshSamplePoints.apply(vertices, corners, u, None, None, bool(return_normals))
    else:
        out = sample_composition(vertices, corners, u=u, return_normals=return_normals)
    return MeshSamplesWithNormals(*out) if return_normals else MeshSamples(*out)


class SampledMeshChamferLoss(torch.nn.Module):
    """The Chamfer distance between ``num_samples`` points sampled on the mesh ``vertices`` (B,N,3) over ``faces``
    (B,F,3) or a shared (F,3) and the cloud ``target`` (B,M,3): ``mean(dist1) + mean(dist2)`` of ``nndistance(points,
    target)``.  ``u`` (B,S,3) fixes the random numbers.  ``self.E`` is the ``MeshCorners`` of the last build; it is
    kept, and never checked against later faces, while ``consistent_topology`` is set."""

    def __init__(self, num_samples, consistent_topology=False):
        super().__init__()
        self.num_samples = num_samples
        self.consistent_topology = consistent_topology
        self.E = None

    def forward(self, vertices, faces=None, target=None, u=None):
        from .network.model_loss import nndistance   # (that module re-exports this class)
        assert(target is not None), "target is required"
        if (not self.consistent_topology) or (self.E is None):
            assert(faces is not None), "Face is required"
            self.E = MeshCorners.from_faces(faces.to(vertices.device), vertices.shape[1])
        points = sample_points_from_meshes(vertices, self.E, None if u is not None else self.num_samples, u=u).points
        dist1, dist2, _, _ = nndistance(points, target)
        return dist1.mean() + dist2.mean()
