"""The normals of a triangle mesh, per face and per vertex, over the kept corner lists of ``mesh_laplacian``:

    mesh_face_normals(vertices (B,N,3), corners)                     ->   (normals (B,F,3), areas (B,F))
    mesh_vertex_normals(vertices (B,N,3), corners, weighting="area") ->   (B,N,3)

``corners`` is a ``MeshCorners`` of triangles: nothing else is built.  The face operator is the reference's
``compute_face_normals_and_areas`` (network/geo_operations.py:529-559): ``c = (p1-p0) x (p2-p1)``, ``areas = |c| / 2``,
``normals = c / max(|c|, 1e-12)``.  The vertex operator normalises the sum over a vertex's corners of ``c`` ("area":
every incident face weighs in with twice its area) or of ``c / max(|c|, 1e-12)`` ("uniform"), again with
``max(|S|, 1e-12)``; a vertex without corners gets ``+0``.  The reference has no vertex normals.

CUDA fp32 runs the HIP kernels of csrc/mesh_normals.hip (``pp_mesh_face_normals_*``, ``pp_mesh_vertex_normals_*``): one
launch forward, a backward that is a gather over each vertex's sorted corner slice -- no floating-point atomics, the
same bits on every run, one form only, and nothing synchronises with the host.  CPU tensors and other dtypes go through
``face_normals_composition`` / ``vertex_normals_composition``, the same contracts written as torch operations.  A face
(or a vertex sum) of length <= 1e-12 keeps its forward value and passes NO gradient, where ``sqrt``'s and
``F.normalize``'s backward give NaN or 1e12: the rule of ``mesh_dihedral``.  DESIGN.md "Mesh normals" states the
contract.
"""
import torch

from . import _lib
from . import _mesh_topology as _topology
from .mesh_laplacian import MeshCorners, _corner_rows

_EPS = 1e-12                      # F.normalize's eps
WEIGHTINGS = {"area": 0, "uniform": 1}


def _check(what, vertices, corners):
    _topology.check_vertices(what, vertices, corners, MeshCorners, "corners", "faces", d3=True)
    if corners.degree != 3:
        raise NotImplementedError("%s: triangles only, got faces of %d corners" % (what, corners.degree))


def _weighting(weighting):
    if weighting not in WEIGHTINGS:
        raise ValueError("mesh_vertex_normals: weighting must be one of %s, got %r" % (sorted(WEIGHTINGS), weighting))
    return WEIGHTINGS[weighting]


def _cross(a, b):
    """``a x b`` with every product rounded on its own: a face with a repeated vertex then has the cross product 0
    exactly, as in the kernels (``torch.cross`` may contract ``a*b - c*d`` and leave the products' rounding error)"""
    ax, ay, az = a.unbind(-1)
    bx, by, bz = b.unbind(-1)
    return torch.stack([ay * bz - az * by, az * bx - ax * bz, ax * by - ay * bx], dim=-1)


def _unit(c):
    """``(c / max(|c|, 1e-12), |c|, |c| > 1e-12)``; a vector of length <= 1e-12 keeps both values and passes no
    gradient"""
    sq = (c[..., 0] * c[..., 0] + c[..., 1] * c[..., 1]) + c[..., 2] * c[..., 2]
    short = torch.sqrt(sq.detach())
    ok = short > _EPS
    length = torch.sqrt(torch.where(ok, sq, torch.ones_like(sq)))
    unit = torch.where(ok[..., None], c / length[..., None], c.detach() / _EPS)
    return unit, torch.where(ok, length, short), ok


def face_normals_composition(vertices, corners):
    """``mesh_face_normals`` as torch operations, for any device and floating dtype: the gather of the three corners,
    ``c = cross(p1 - p0, p2 - p1)``, ``areas = |c| / 2``, ``normals = c / max(|c|, 1e-12)``; a face with
    ``|c| <= 1e-12`` contributes a zero gradient."""
    _check("mesh_face_normals", vertices, corners)
    b, n, _ = vertices.shape
    flat = vertices.reshape(b * n, 3)
    i, nxt, prv = (rows.reshape(b, -1, 3)[:, :, 0] for rows in _corner_rows(vertices, corners))   # corner 0's
    p0, p1, p2 = flat[i], flat[nxt], flat[prv]
    normals, length, _ = _unit(_cross(p1 - p0, p2 - p1))
    return normals, length * 0.5


def vertex_normals_composition(vertices, corners, weighting="area"):
    """``mesh_vertex_normals`` as torch operations, for any device and floating dtype: per corner
    ``c = cross(v_next - v_i, v_prev - v_i)``, one ``index_add_`` of ``c`` ("area") or ``c / max(|c|, 1e-12)``
    ("uniform") over the corner rows, then ``S / max(|S|, 1e-12)``; a face or a sum of length <= 1e-12 contributes a
    zero gradient."""
    _check("mesh_vertex_normals", vertices, corners)
    uniform = _weighting(weighting) == 1
    b, n, _ = vertices.shape
    flat = vertices.reshape(b * n, 3)
    i, nxt, prv = _corner_rows(vertices, corners)
    vi = flat[i]
    c = _cross(flat[nxt] - vi, flat[prv] - vi)
    if uniform:
        c = _unit(c)[0]
    return _unit(torch.zeros_like(flat).index_add_(0, i, c))[0].reshape(b, n, 3)


def _empty(vertices, corners):
    return vertices.shape[0] == 0 or vertices.shape[1] == 0 or corners.n_faces == 0


class MeshFaceNormals(torch.autograd.Function):
    """HIP forward and backward (CUDA fp32)."""

    @staticmethod
    def forward(ctx, vertices, corners):
        dev = _lib.require_cuda(("vertices", vertices), ("faces", corners.faces))
        vertices = vertices.contiguous()
        b, n, _ = vertices.shape
        f = corners.n_faces
        if _empty(vertices, corners):
            normals, areas = vertices.new_zeros(b, f, 3), vertices.new_zeros(b, f)
        else:
            normals = torch.empty(b, f, 3, dtype=torch.float32, device=dev)
            areas = torch.empty(b, f, dtype=torch.float32, device=dev)
            with _lib.on_device(dev) as stream:
                _lib.check(_lib.lib().pp_mesh_face_normals_forward_f32(
                    _lib.ptr(vertices), _lib.ptr(corners.faces), _lib.ptr(normals), _lib.ptr(areas), b, n, f,
                    int(corners.batch == 1), stream), "mesh_face_normals forward")
        ctx.save_for_backward(vertices)
        ctx.corners = corners
        ctx.set_materialize_grads(False)
        return normals, areas

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_normals, grad_areas):
        if not ctx.needs_input_grad[0] or (grad_normals is None and grad_areas is None):
            return None, None
        (vertices,) = ctx.saved_tensors
        corners = ctx.corners
        b, n, _ = vertices.shape
        if _empty(vertices, corners):
            return torch.zeros_like(vertices), None
        grad_normals = None if grad_normals is None else grad_normals.contiguous()
        grad_areas = None if grad_areas is None else grad_areas.contiguous()
        grad = torch.empty_like(vertices)
        with _lib.on_device(vertices.device) as stream:
            _lib.check(_lib.lib().pp_mesh_face_normals_backward_f32(
                _lib.ptr(vertices), _lib.ptr(corners.start), _lib.ptr(corners.nbr), _lib.ptr(corners.codes),
                None if grad_normals is None else _lib.ptr(grad_normals),
                None if grad_areas is None else _lib.ptr(grad_areas), _lib.ptr(grad), b, n, corners.n_faces,
                int(corners.batch == 1), stream), "mesh_face_normals backward")
        return grad, None


class MeshVertexNormals(torch.autograd.Function):
    """HIP forward and backward (CUDA fp32); ``weighting`` 0 "area", 1 "uniform"."""

    @staticmethod
    def forward(ctx, vertices, corners, weighting):
        dev = _lib.require_cuda(("vertices", vertices), ("faces", corners.faces))
        vertices = vertices.contiguous()
        b, n, _ = vertices.shape
        if _empty(vertices, corners):
            out = torch.zeros_like(vertices)
        else:
            out = torch.empty_like(vertices)
            with _lib.on_device(dev) as stream:
                _lib.check(_lib.lib().pp_mesh_vertex_normals_forward_f32(
                    _lib.ptr(vertices), _lib.ptr(corners.start), _lib.ptr(corners.nbr), _lib.ptr(out), b, n,
                    corners.n_faces, weighting, int(corners.batch == 1), stream), "mesh_vertex_normals forward")
        ctx.save_for_backward(vertices)
        ctx.corners = corners
        ctx.weighting = weighting
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        if not ctx.needs_input_grad[0]:
            return None, None, None
        (vertices,) = ctx.saved_tensors
        corners = ctx.corners
        b, n, _ = vertices.shape
        if _empty(vertices, corners):
            return torch.zeros_like(vertices), None, None
        grad_out = grad_out.contiguous()
        scratch = torch.empty_like(vertices)     # (torch.empty: a capture takes it from the graph's own pool)
        grad = torch.empty_like(vertices)
        with _lib.on_device(vertices.device) as stream:
            _lib.check(_lib.lib().pp_mesh_vertex_normals_backward_f32(
                _lib.ptr(vertices), _lib.ptr(corners.start), _lib.ptr(corners.nbr), _lib.ptr(grad_out),
                _lib.ptr(scratch), _lib.ptr(grad), b, n, corners.n_faces, ctx.weighting, int(corners.batch == 1),
                stream), "mesh_vertex_normals backward")
        return grad, None, None


def _hip_serves(vertices, corners):
    return (vertices.is_cuda and vertices.dtype == torch.float32
            and vertices.shape[0] * max(vertices.shape[1], corners.n_faces) <= _topology.LIMIT
            and 3 * corners.n_faces <= _topology.LIMIT)


def mesh_face_normals(vertices, corners):
    """``(normals (B,F,3), areas (B,F))`` of the triangles of ``corners`` (a ``MeshCorners``) over ``vertices``
    (B,N,3): with ``c = (p1-p0) x (p2-p1)``, ``areas = |c| / 2`` and ``normals = c / max(|c|, 1e-12)``
    (``compute_face_normals_and_areas``' values).  A topology of one batch element serves every ``b`` without a copy.
    Differentiable in ``vertices``; a face with ``|c| <= 1e-12`` (one without area) has the normal ``c / 1e-12`` and
    passes no gradient.

    CUDA fp32: the HIP kernels (the backward gives the same bits on every run, so
    ``torch.use_deterministic_algorithms`` changes nothing); anything else: ``face_normals_composition``.  Nothing
    synchronises with the host."""
    _check("mesh_face_normals", vertices, corners)
    if _hip_serves(vertices, corners):
        return MeshFaceNormals.apply(vertices, corners)
    return face_normals_composition(vertices, corners)


def mesh_vertex_normals(vertices, corners, weighting="area"):
    """Unit vertex normals ``(B,N,3)`` of the triangle mesh ``corners`` (a ``MeshCorners``) over ``vertices`` (B,N,3):
    ``S_i / max(|S_i|, 1e-12)`` with ``S_i`` the sum over the corners at ``i`` of ``c = (v_next - v_i) x (v_prev -
    v_i)`` (``weighting="area"``) or of ``c / max(|c|, 1e-12)`` (``"uniform"``).  A vertex without corners gets ``+0``
    and no gradient.  A topology of one batch element serves every ``b`` without a copy.  Differentiable in
    ``vertices``.

    CUDA fp32: the HIP kernels, forward one launch and backward two, bit for bit the same on every run; anything
    else: ``vertex_normals_composition``.  Nothing synchronises with the host."""
    _check("mesh_vertex_normals", vertices, corners)
    code = _weighting(weighting)
    if _hip_serves(vertices, corners):
        return MeshVertexNormals.apply(vertices, corners, code)
    return vertex_normals_composition(vertices, corners, weighting)
