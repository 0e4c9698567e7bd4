"""The operators under the reference's mesh Laplacians (network/geo_operations.py:155-346):

    MeshCorners.from_faces(faces (B,F,L), n_vertices)       every vertex's sorted list of face corners
    cotangent(vertices (B,N,3), faces (B,F,3))         ->   (B,F,3) cotangent weights of the triangles' angles
    mesh_uniform_laplacian(vertices (B,N,D), corners)  ->   (B,N,D), UniformLaplacian's L v / (Lii + 1e-12)
    mesh_cot_laplacian(vertices, corners, weights)     ->   (B,N,D), CotLaplacian's L v for constant weights

A *corner* is ``(f, c)`` with vertex ``i = faces[f,c]``, ``next = faces[f,(c+1) % L]`` and ``prev = faces[f,(c-1) % L]``.
Both of the reference's matrices are sums over corners:

    uniform    (L v)_i = sum over the corners at i of (v_i - v_next) + (v_i - v_prev),  Lii_i = 2 * #corners at i
    cotangent  (L v)_i = sum over the corners at i of C[f,(c+2)%3] (v_next - v_i) + C[f,(c+1)%3] (v_prev - v_i)

so the vertex -> corner list is the only topology either needs, and an apply is a gather over it.  The list is built
once (one device-to-host copy) and kept; an apply is one launch, forward or backward, and never synchronises with the
host.  CUDA fp32 with D = 3 runs the HIP kernels of csrc/mesh_edges.hip (``pp_mesh_corner_incidence``,
``pp_mesh_cotangent_f32``, ``pp_mesh_laplacian_apply_f32``): no floating-point atomics, the same bits on every run, one
form only.  CPU tensors, other dtypes and D go through the ``*_composition`` twins, the same contracts written with
``index_add_`` over the corner list.  ``MeshCorners`` is an object of its own (no counts); its input normalising,
range check, errors and the applies' argument checks are ``_mesh_topology``'s.  DESIGN.md "Mesh Laplacians" states the
contract.
"""
import torch

from . import _lib
from . import _mesh_topology as _topology


class MeshCorners(object):
    """The corner incidence of a batch of meshes of ``L``-gons over ``n_vertices`` vertices each.

    ``faces`` (Bt,F,L) int64 contiguous; ``start`` (Bt,N+1) int32; ``codes`` (Bt,L*F) (uint32 values in int32
    storage): vertex v's slice ``[start[v], start[v+1])`` holds ``L*f + c`` for every corner with ``faces[f,c] == v``,
    ascending; ``nbr`` (Bt,L*F,2) int32: ``(next, prev)`` of every slot, in slice order.  ``Bt`` is 1 for a topology
    that a whole batch shares: 2-D faces, a batch of one, or a view with batch stride 0.

    ``from_faces`` makes EXACTLY ONE device-to-host copy -- the out-of-range flags -- and nothing that uses the
    object afterwards synchronises with the host.  An index outside ``[0, n_vertices)`` raises IndexError naming the
    batch element; on the GPU it is only ever compared, never used as an address.  The slices are sorted, so the
    bytes of the object do not depend on the order in which the build's integer atomics were served."""

    def __init__(self, faces, start, codes, nbr, n_vertices):
        self.faces = faces
        self.start = start
        self.codes = codes
        self.nbr = nbr
        self.n_vertices = int(n_vertices)

    @property
    def batch(self):
        return self.faces.shape[0]

    @property
    def n_faces(self):
        return self.faces.shape[1]

    @property
    def degree(self):
        return self.faces.shape[2]

    @property
    def device(self):
        return self.faces.device

    def counts(self):
        """(Bt,N) int32: the number of corners at every vertex"""
        return self.start[:, 1:] - self.start[:, :-1]

    def lii(self, dtype=torch.float32):
        """the reference's ``UniformLaplacian.Lii``: (Bt*N,) ``2 * #corners``"""
        return (2 * self.counts()).reshape(-1).to(dtype)

    @classmethod
    def from_faces(cls, faces, n_vertices):
        """``faces`` (F,L), (1,F,L) or (B,F,L), an integer tensor with L >= 3.  A face with a repeated vertex keeps
        all its corners, as the reference's sparse sum does."""
        what = "MeshCorners.from_faces"
        faces = _topology.index_table(what, "faces", faces, "(B, F, L) with L >= 3", lambda cols: cols >= 3)
        n_vertices = int(n_vertices)
        bt, f, deg = faces.shape
        _topology.fits("corner incidence", bt, n_vertices, deg * f)
        if not faces.is_cuda:
            _topology.raise_flagged(what, _topology.out_of_range(faces, n_vertices))
            keys = faces.reshape(bt, deg * f)
            codes = torch.argsort(keys, dim=1, stable=True)              # position L*f + c of every corner, by vertex
            count = torch.zeros(bt, n_vertices + 1, dtype=torch.int64)
            count[:, 1:].scatter_add_(1, keys, torch.ones_like(keys))
            nbr = torch.stack([torch.roll(faces, -1, 2).reshape(bt, -1).gather(1, codes),
                               torch.roll(faces, 1, 2).reshape(bt, -1).gather(1, codes)], dim=-1)
            return cls(faces, torch.cumsum(count, 1).int(), codes.int(), nbr.int(), n_vertices)
        dev = faces.device
        start = torch.empty(bt, n_vertices + 1, dtype=torch.int32, device=dev)
        codes = torch.empty(bt, deg * f, dtype=torch.int32, device=dev)
        nbr = torch.empty(bt, deg * f, 2, dtype=torch.int32, device=dev)
        flags = torch.empty(bt, dtype=torch.int32, device=dev)
        with _lib.on_device(dev) as stream:
            wsp, nbytes, ws = _topology.workspace(dev, bt, n_vertices, deg * f)
            _lib.check(_lib.lib().pp_mesh_corner_incidence(
                _lib.ptr(faces), _lib.ptr(start), _lib.ptr(codes), _lib.ptr(nbr), _lib.ptr(flags), bt, f, deg,
                n_vertices, wsp, nbytes, stream), "mesh corner incidence")
        _topology.raise_flagged(what, flags.tolist())                    # the one copy
        return cls(faces, start, codes, nbr, n_vertices)


def _check_weights(what, vertices, corners, weights):
    if corners.degree != 3:
        raise NotImplementedError("%s: triangles only, got faces of %d corners" % (what, corners.degree))
    if weights.shape != (vertices.shape[0], corners.n_faces, 3):
        raise ValueError("%s: weights must have shape (B, F, 3) = %s, got %s"
                         % (what, (vertices.shape[0], corners.n_faces, 3), tuple(weights.shape)))
    if weights.device != vertices.device:
        raise RuntimeError("%s: the weights are on %s, expected %s" % (what, weights.device, vertices.device))


def _corner_rows(vertices, corners):
    """the corners of every batch element as rows of the flattened (B*N, D) vertices: ``(i, next, prev)``, each
    (B*F*L,) int64 in (b, f, c) order"""
    b, n = vertices.shape[0], vertices.shape[1]
    faces = corners.faces.expand(b, -1, -1) + (torch.arange(b, device=vertices.device) * n)[:, None, None]
    return faces.reshape(-1), torch.roll(faces, -1, 2).reshape(-1), torch.roll(faces, 1, 2).reshape(-1)


def uniform_laplacian_composition(vertices, corners):
    """``mesh_uniform_laplacian`` as torch operations, for any device, floating dtype and D: one ``index_add_`` over
    the corner list, then the division by ``Lii + 1e-12``."""
    _topology.check_vertices("mesh_uniform_laplacian", vertices, corners, MeshCorners, "corners", "faces")
    b, n, d = vertices.shape
    flat = vertices.reshape(b * n, d)
    i, nxt, prv = _corner_rows(vertices, corners)
    vi = flat[i]
    acc = torch.zeros_like(flat).index_add_(0, i, (vi - flat[nxt]) + (vi - flat[prv]))
    lii = corners.lii(vertices.dtype).reshape(corners.batch, n, 1)
    return acc.reshape(b, n, d) / (lii + 1e-12)


def cot_laplacian_composition(vertices, corners, weights):
    """``mesh_cot_laplacian`` as torch operations, for any device, floating dtype and D (differentiable in the
    weights too, which the kernels are not)."""
    _topology.check_vertices("mesh_cot_laplacian", vertices, corners, MeshCorners, "corners", "faces")
    _check_weights("mesh_cot_laplacian", vertices, corners, weights)
    b, n, d = vertices.shape
    flat = vertices.reshape(b * n, d)
    i, nxt, prv = _corner_rows(vertices, corners)
    weights = weights.to(vertices.dtype)
    wa = weights[:, :, [2, 0, 1]].reshape(-1, 1)      # corner c: C[f, (c+2) % 3] on the edge to next
    wb = weights[:, :, [1, 2, 0]].reshape(-1, 1)      # and C[f, (c+1) % 3] on the edge to prev
    vi = flat[i]
    acc = torch.zeros_like(flat).index_add_(0, i, wa * (flat[nxt] - vi) + wb * (flat[prv] - vi))
    return acc.reshape(b, n, d)


def cotangent_composition(vertices, faces):
    """The reference's ``cotangent`` (geo_operations.py:306-346) operation for operation, as torch operations on any
    device and floating dtype: ``vertices`` (B,N,3), triangles ``faces`` (B,F,3) or a shared (1,F,3) / (F,3) ->
    (B,F,3), columns for the edges 23, 31, 12; exactly 0 for a face without area.  Differentiable."""
    if faces.dim() == 2:
        faces = faces.unsqueeze(0)
    if faces.shape[-1] != 3:
        raise NotImplementedError("cotangent: triangles only, got faces of %d corners" % faces.shape[-1])
    b = vertices.shape[0]
    faces = faces.to(device=vertices.device).long().expand(b, -1, -1)
    v1, v2, v3 = (torch.gather(vertices, 1, faces[:, :, c:c + 1].expand(-1, -1, 3)) for c in range(3))
    l1 = torch.sqrt(((v2 - v3) ** 2).sum(2))
    l2 = torch.sqrt(((v3 - v1) ** 2).sum(2))
    l3 = torch.sqrt(((v1 - v2) ** 2).sum(2))
    sp = (l1 + l2 + l3) * 0.5
    inside = sp * (sp - l1) * (sp - l2) * (sp - l3)
    inside = inside.masked_fill(inside < 0, 0)
    area = 2 * torch.sqrt(inside)
    cot23 = (l2 ** 2 + l3 ** 2 - l1 ** 2)
    cot31 = (l1 ** 2 + l3 ** 2 - l2 ** 2)
    cot12 = (l1 ** 2 + l2 ** 2 - l3 ** 2)
    c = torch.stack([cot23, cot31, cot12], 2) / (torch.unsqueeze(area, 2) + 1e-10) / 4
    return c.masked_fill(area.unsqueeze(2) == 0, 0.0)


def cotangent(vertices, faces):
    """Cotangent weights (B,F,3) of the triangles ``faces`` over ``vertices`` (B,N,3).  CUDA fp32 without a gradient
    to ``vertices`` (none is asked for, or under ``no_grad``): the HIP kernel, one thread per face, the composition's
    operation order; a face with an index outside [0, N) gives NaN there and nothing synchronises.  Anything else:
    ``cotangent_composition``."""
    if (vertices.is_cuda and vertices.dtype == torch.float32 and vertices.dim() == 3 and vertices.shape[2] == 3
            and not (vertices.requires_grad and torch.is_grad_enabled()) and isinstance(faces, torch.Tensor)
            and _topology.is_index(faces) and faces.dim() in (2, 3) and faces.shape[-1] == 3):
        if faces.dim() == 2:
            faces = faces.unsqueeze(0)
        b, n, f = vertices.shape[0], vertices.shape[1], faces.shape[1]
        if faces.shape[0] > 1 and faces.stride(0) == 0:
            faces = faces[:1]
        if faces.shape[0] in (1, b) and b * max(f, n) <= _topology.LIMIT:
            dev = vertices.device
            faces = faces.to(device=dev, dtype=torch.int64).contiguous()
            vertices = vertices.detach().contiguous()
            out = torch.empty(b, f, 3, dtype=torch.float32, device=dev)
            with _lib.on_device(dev) as stream:
                _lib.check(_lib.lib().pp_mesh_cotangent_f32(_lib.ptr(vertices), _lib.ptr(faces), _lib.ptr(out), b, n, f,
                                                            int(faces.shape[0] == 1), stream), "mesh cotangent")
            return out
    return cotangent_composition(vertices, faces)


def _apply(x, corners, weights, mode, what):
    """one launch of pp_mesh_laplacian_apply_f32 on contiguous CUDA fp32 ``x`` (B,N,3)"""
    dev = x.device
    b, n, _ = x.shape
    out = torch.empty_like(x)
    with _lib.on_device(dev) as stream:
        _lib.check(_lib.lib().pp_mesh_laplacian_apply_f32(
            _lib.ptr(x), _lib.ptr(corners.start), _lib.ptr(corners.nbr), _lib.ptr(corners.codes),
            None if weights is None else _lib.ptr(weights), _lib.ptr(out), b, n, corners.n_faces, corners.degree, mode,
            int(corners.batch == 1), stream), what)
    return out


class MeshUniformLaplacian(torch.autograd.Function):
    """HIP forward and backward (CUDA fp32, D = 3): modes 0 and 1 of one gather kernel."""

    @staticmethod
    def forward(ctx, vertices, corners):
        _lib.require_cuda(("vertices", vertices), ("faces", corners.faces))
        ctx.corners = corners
        return _apply(vertices.contiguous(), corners, None, 0, "mesh_uniform_laplacian forward")

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        if not ctx.needs_input_grad[0]:
            return None, None
        return _apply(grad_out.contiguous(), ctx.corners, None, 1, "mesh_uniform_laplacian backward"), None


class MeshCotLaplacian(torch.autograd.Function):
    """HIP forward and backward (CUDA fp32, D = 3): the operator is symmetric and constant, so the backward is the
    forward's launch on the incoming gradient (reference :288-302).  No gradient reaches the weights."""

    @staticmethod
    def forward(ctx, vertices, corners, weights):
        _lib.require_cuda(("vertices", vertices), ("faces", corners.faces), ("weights", weights))
        ctx.corners = corners
        weights = weights.contiguous()
        ctx.save_for_backward(weights)
        return _apply(vertices.contiguous(), corners, weights, 2, "mesh_cot_laplacian forward")

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        if not ctx.needs_input_grad[0]:
            return None, None, None
        (weights,) = ctx.saved_tensors
        return _apply(grad_out.contiguous(), ctx.corners, weights, 2, "mesh_cot_laplacian backward"), None, None


def _hip_serves(vertices):
    return (vertices.is_cuda and vertices.dtype == torch.float32 and vertices.shape[2] == 3
            and vertices.shape[0] * vertices.shape[1] <= _topology.LIMIT)


def mesh_uniform_laplacian(vertices, corners):
    """``UniformLaplacian``'s output (B,N,D) for ``vertices`` (B,N,D) over ``corners`` (a ``MeshCorners`` of any face
    degree): ``out_i = (sum over the corners at i of (v_i - v_next) + (v_i - v_prev)) / (2 * #corners + 1e-12)``.  The
    weights are half-edge multiplicities: an interior edge counts 2, a boundary edge 1, a face with a repeated vertex
    adds a zero term and still counts in the divisor; a vertex without corners gives exactly 0.  A topology of one
    batch element serves every ``b`` without a copy.  Differentiable in ``vertices``.

    CUDA fp32 with D = 3: the HIP gather, forward and backward, bit for bit the sequential fp32 loop over the sorted
    slices on every run (``torch.use_deterministic_algorithms`` selects nothing); anything else:
    ``uniform_laplacian_composition``.  Nothing synchronises with the host."""
    _topology.check_vertices("mesh_uniform_laplacian", vertices, corners, MeshCorners, "corners", "faces")
    if _hip_serves(vertices):
        return MeshUniformLaplacian.apply(vertices, corners)
    return uniform_laplacian_composition(vertices, corners)


def mesh_cot_laplacian(vertices, corners, weights):
    """``CotLaplacian``'s output (B,N,D) for ``vertices`` (B,N,D) over the triangle topology ``corners`` with the
    constant cotangent ``weights`` (B,F,3) of ``cotangent``: ``out_i = sum over the corners (f,c) at i of
    W[f,(c+2)%3] (v_next - v_i) + W[f,(c+1)%3] (v_prev - v_i)`` (the opposite sign convention to the uniform operator;
    it is the reference's).  Differentiable in ``vertices``; the weights are per batch element even where the
    topology is shared.

    CUDA fp32 with D = 3 and weights that need no gradient: the HIP gather, forward and backward; anything else:
    ``cot_laplacian_composition``.  Nothing synchronises with the host."""
    _topology.check_vertices("mesh_cot_laplacian", vertices, corners, MeshCorners, "corners", "faces")
    _check_weights("mesh_cot_laplacian", vertices, corners, weights)
    if (_hip_serves(vertices) and weights.dtype == torch.float32
            and not (weights.requires_grad and torch.is_grad_enabled())):
        return MeshCotLaplacian.apply(vertices, corners, weights)
    return cot_laplacian_composition(vertices, corners, weights)
