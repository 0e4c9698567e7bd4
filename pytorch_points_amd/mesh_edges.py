"""The edge operators under the reference's mesh losses (network/model_loss.py:166-308, geo_operations.py:562-600):

    MeshEdges.from_faces(faces (B,F,3), n_vertices)   the unique edges of a triangle mesh and their vertex incidence
    MeshEdges.from_edges(edges (E,2), n_vertices)     the same object over a user's edge list
    mesh_edge_sqrlen(vertices (B,N,3), topo)     ->   (B,Ecap) squared edge lengths, 0 in the padding

A mesh's connectivity does not change between training steps, so the topology is an object that is built once (with one
device-to-host copy) and kept; a step on it is two launches and never synchronises with the host.  CUDA runs the HIP
kernels of csrc/mesh_edges.hip (``pp_mesh_*``): the unique edges in ``torch.unique``'s row order bit for bit, and a
backward that is a gather over each vertex's sorted incidence list -- no floating-point atomics, the same bits on every
run, one form only.  CPU tensors, other dtypes and D != 3 go through ``sqrlen_composition``, the same contract written
as torch operations.  DESIGN.md "Mesh edge operators" states the contract.
"""
import ctypes

import torch

from . import _lib

_LIMIT = 2 ** 31 - 1   # csrc/mesh_edges.hip: the index words in use


def _is_index(t):
    return not (t.is_floating_point() or t.is_complex() or t.dtype == torch.bool)


def _workspace(dev, bt, n, items):
    nbytes = int(_lib.lib().pp_mesh_edges_workspace_bytes(bt, n, items))
    ws = _lib.workspace(dev, "mesh_edges", nbytes)
    return (_lib.ptr(ws) if ws is not None else None), ctypes.c_size_t(nbytes), ws


def _fits(what, bt, n, items):
    if bt * items > _LIMIT or bt * (n + 1) > _LIMIT:
        raise NotImplementedError("%s: %d batch elements of %d entries over %d vertices do not fit the kernels' 32-bit "
                                  "index words" % (what, bt, items, n))


def _unique_edges_hip(faces, n_vertices, status):
    """kernel (a): contiguous int64 CUDA ``faces`` (Bt,F,3) -> ``edges`` (Bt,3F,2); counts into ``status[0]``, flags
    into ``status[1]`` (int32 (2,Bt)).  No host synchronisation."""
    dev = faces.device
    bt, f = faces.shape[0], faces.shape[1]
    _fits("unique edges", bt, n_vertices, 3 * f)
    edges = torch.empty(bt, 3 * f, 2, dtype=torch.int64, device=dev)
    with _lib.on_device(dev) as stream:
        wsp, nbytes, ws = _workspace(dev, bt, n_vertices, 3 * f)
        _lib.check(_lib.lib().pp_mesh_unique_edges(_lib.ptr(faces), _lib.ptr(edges), _lib.ptr(status[0]),
                                                   _lib.ptr(status[1]), bt, f, n_vertices, wsp, nbytes, stream),
                   "mesh unique edges")
    return edges


def _incidence_hip(edges, counts, n_vertices, flags):
    """kernel (b): contiguous int64 CUDA ``edges`` (Bt,Ecap,2), int32 ``counts`` (Bt) -> ``(inc_start (Bt,N+1) int32,
    inc_entries (Bt,2*Ecap) as int32 storage)``; an out-of-range end is ORed into ``flags`` (Bt, initialised)."""
    dev = edges.device
    bt, ecap = edges.shape[0], edges.shape[1]
    _fits("edge incidence", bt, n_vertices, 2 * ecap)
    inc_start = torch.empty(bt, n_vertices + 1, dtype=torch.int32, device=dev)
    inc_entries = torch.empty(bt, 2 * ecap, dtype=torch.int32, device=dev)
    with _lib.on_device(dev) as stream:
        wsp, nbytes, ws = _workspace(dev, bt, n_vertices, 2 * ecap)
        _lib.check(_lib.lib().pp_mesh_edge_incidence(_lib.ptr(edges), _lib.ptr(counts), _lib.ptr(inc_start),
                                                     _lib.ptr(inc_entries), _lib.ptr(flags), bt, ecap, n_vertices, wsp,
                                                     nbytes, stream), "mesh edge incidence")
    return inc_start, inc_entries


def unique_edges_composition(faces):
    """The unique edges of ONE triangle list ``faces`` (F,3), an integer tensor on any device, as torch operations:
    every face's three corner pairs as (min,max), the distinct rows in ascending lexicographic order ``(E,2)``."""
    pairs = torch.stack([faces, faces[:, [1, 2, 0]]], dim=-1)
    return torch.unique(torch.sort(pairs, dim=-1)[0].reshape(-1, 2), dim=0)


class MeshEdges(object):
    """The edge topology of a batch of meshes over ``n_vertices`` vertices each.

    ``edges`` (Bt,Ecap,2) int64: rows ``[0, count[b])`` are the edges, later rows ``(-1,-1)``; ``counts`` (Bt,) int32 on
    the device; ``counts_host`` the same numbers as a tuple of Python ints; ``incidence()`` the ``(inc_start (Bt,N+1),
    inc_entries (Bt,2*Ecap))`` lists the backward gathers over (CUDA only).  ``Bt`` is 1 for a topology that a whole
    batch shares: a ``faces`` view with batch stride 0, or an un-batched edge list.

    Building with ``from_faces`` / ``from_edges`` makes EXACTLY ONE device-to-host copy -- the counts and the
    out-of-range flags together -- and nothing that uses the object afterwards synchronises with the host.  An index
    outside ``[0, n_vertices)`` raises IndexError naming the batch element (the reference would fault on the device);
    on the GPU it is only ever compared, never used as an address."""

    def __init__(self, edges, counts, counts_host, n_vertices, incidence=None):
        self.edges = edges
        self.counts = counts
        self.counts_host = counts_host
        self.n_vertices = int(n_vertices)
        self._incidence = incidence

    @property
    def batch(self):
        return self.edges.shape[0]

    @property
    def capacity(self):
        return self.edges.shape[1]

    def count(self, b):
        """the number of edges of batch element ``b`` of the vertices (a Python int)"""
        return self.counts_host[0 if self.batch == 1 else b]

    def edge_list(self, b):
        """``(E_b,2)`` int64 view of the edges of batch element ``b``"""
        return self.edges[0 if self.batch == 1 else b, :self.count(b)]

    def incidence(self):
        """``(inc_start, inc_entries)``; built here, without a host read, for an object made by ``_unchecked``"""
        if self._incidence is None:
            flags = torch.zeros(self.batch, dtype=torch.int32, device=self.edges.device)
            self._incidence = _incidence_hip(self.edges, self.counts, self.n_vertices, flags)
        return self._incidence

    @classmethod
    def _unchecked(cls, edges, n_vertices):
        """CUDA int64 ``edges`` (Bt,E,2), every row an edge, nothing read back: the incidence is built on first use
        and an out-of-range index is not reported (the step kernels give NaN for it)."""
        bt, e = edges.shape[0], edges.shape[1]
        counts = torch.full((bt,), e, dtype=torch.int32, device=edges.device)
        return cls(edges, counts, (e,) * bt, n_vertices)

    @staticmethod
    def _raise_flagged(what, flags):
        for b, flag in enumerate(flags):
            if flag:
                raise IndexError("%s: batch element %d holds a vertex index outside [0, n_vertices)" % (what, b))

    @classmethod
    def from_faces(cls, faces, n_vertices):
        """The unique edges of the triangles ``faces`` (B,F,3) or (F,3), an integer tensor.  A face with a repeated
        vertex keeps its ``(a,a)`` edge, as the reference's ``torch.unique`` does."""
        if not isinstance(faces, torch.Tensor) or not _is_index(faces):
            raise TypeError("MeshEdges.from_faces: faces must be an integer tensor, got %s"
                            % (faces.dtype if isinstance(faces, torch.Tensor) else type(faces).__name__))
        if faces.dim() == 2:
            faces = faces.unsqueeze(0)
        if faces.dim() != 3:
            raise ValueError("MeshEdges.from_faces: faces must have shape (B, F, 3), got %s" % (tuple(faces.shape),))
        if faces.shape[-1] != 3:
            raise NotImplementedError("MeshEdges.from_faces: triangles only (the reference pairs the corners through "
                                      "F[:, [1, 2, 0]]), got faces of %d corners" % faces.shape[-1])
        n_vertices = int(n_vertices)
        if faces.shape[0] > 1 and faces.stride(0) == 0:
            faces = faces[:1]
        faces = (faces if faces.dtype == torch.int64 else faces.long()).contiguous()
        bt, f = faces.shape[0], faces.shape[1]
        if not faces.is_cuda:
            bad = ((faces < 0) | (faces >= n_vertices)).reshape(bt, -1).any(1).tolist()
            cls._raise_flagged("MeshEdges.from_faces", bad)
            lists = [unique_edges_composition(faces[b]) for b in range(bt)]
            edges = faces.new_full((bt, 3 * f, 2), -1)
            for b, rows in enumerate(lists):
                edges[b, :rows.shape[0]] = rows
            host = tuple(int(rows.shape[0]) for rows in lists)
            return cls(edges, torch.tensor(host, dtype=torch.int32), host, n_vertices)
        status = torch.empty(2, bt, dtype=torch.int32, device=faces.device)
        edges = _unique_edges_hip(faces, n_vertices, status)
        incidence = _incidence_hip(edges, status[0], n_vertices, status[1])
        host = status.tolist()                       # the one copy: counts and flags
        cls._raise_flagged("MeshEdges.from_faces", host[1])
        return cls(edges, status[0], tuple(host[0]), n_vertices, incidence)

    @classmethod
    def from_edges(cls, edges, n_vertices):
        """Any edge list ``edges`` (E,2) -- shared by the batch -- or (B,E,2), an integer tensor: pairs may repeat, need
        no order and may join a vertex to itself.  Columns beyond the first two are ignored."""
        if not isinstance(edges, torch.Tensor) or not _is_index(edges):
            raise TypeError("MeshEdges.from_edges: edges must be an integer tensor, got %s"
                            % (edges.dtype if isinstance(edges, torch.Tensor) else type(edges).__name__))
        if edges.dim() == 2:
            edges = edges.unsqueeze(0)
        if edges.dim() != 3 or edges.shape[-1] < 2:
            raise ValueError("MeshEdges.from_edges: edges must have shape (E, 2) or (B, E, 2), got %s"
                             % (tuple(edges.shape),))
        n_vertices = int(n_vertices)
        if edges.shape[0] > 1 and edges.stride(0) == 0:
            edges = edges[:1]
        edges = edges[..., :2]
        edges = (edges if edges.dtype == torch.int64 else edges.long()).contiguous()
        bt, e = edges.shape[0], edges.shape[1]
        if not edges.is_cuda:
            bad = ((edges < 0) | (edges >= n_vertices)).reshape(bt, -1).any(1).tolist()
            cls._raise_flagged("MeshEdges.from_edges", bad)
            return cls(edges, torch.full((bt,), e, dtype=torch.int32), (e,) * bt, n_vertices)
        status = torch.empty(2, bt, dtype=torch.int32, device=edges.device)
        status[0] = e
        status[1] = 0
        incidence = _incidence_hip(edges, status[0], n_vertices, status[1])
        host = status.tolist()                       # the one copy: counts and flags
        cls._raise_flagged("MeshEdges.from_edges", host[1])
        return cls(edges, status[0], tuple(host[0]), n_vertices, incidence)


def _check(vertices, topo):
    if not isinstance(topo, MeshEdges):
        raise TypeError("mesh_edge_sqrlen: topo must be a MeshEdges, got %s" % type(topo).__name__)
    if vertices.dim() != 3:
        raise ValueError("mesh_edge_sqrlen: vertices must have shape (B, N, D), got %s" % (tuple(vertices.shape),))
    if not vertices.is_floating_point():
        raise RuntimeError("mesh_edge_sqrlen: vertices must be a floating tensor, got %s" % vertices.dtype)
    if vertices.shape[1] != topo.n_vertices:
        raise ValueError("mesh_edge_sqrlen: the topology was built for %d vertices, got %d"
                         % (topo.n_vertices, vertices.shape[1]))
    if topo.batch not in (1, vertices.shape[0]):
        raise ValueError("mesh_edge_sqrlen: a topology of %d batch elements does not serve %d vertex sets"
                         % (topo.batch, vertices.shape[0]))
    if topo.edges.device != vertices.device:
        raise RuntimeError("mesh_edge_sqrlen: the topology is on %s, expected %s" % (topo.edges.device, vertices.device))


def sqrlen_composition(vertices, topo):
    """``mesh_edge_sqrlen`` as torch operations, for any device, floating dtype and D: gather, subtract, square-sum in
    ascending dimension, padding masked to 0."""
    _check(vertices, topo)
    b, n, d = vertices.shape
    ecap = topo.capacity
    valid = torch.arange(ecap, device=vertices.device)[None, :] < topo.counts[:, None].long()      # (Bt,Ecap)
    ends = topo.edges.clamp(0, max(n - 1, 0)).expand(b, -1, -1)
    if n == 0:
        return vertices.new_zeros(b, ecap) + vertices.sum() * 0
    va = torch.gather(vertices, 1, ends[:, :, 0:1].expand(-1, -1, d))
    vb = torch.gather(vertices, 1, ends[:, :, 1:2].expand(-1, -1, d))
    t = va - vb
    d2 = t[..., 0] * t[..., 0]
    for c in range(1, d):
        d2 = torch.addcmul(d2, t[..., c], t[..., c])
    return torch.where(valid.expand(b, -1), d2, torch.zeros_like(d2))


class MeshEdgeSqrLen(torch.autograd.Function):
    """HIP forward and backward (CUDA fp32, D = 3)."""

    @staticmethod
    def forward(ctx, vertices, topo):
        dev = _lib.require_cuda(("vertices", vertices), ("edges", topo.edges))
        vertices = vertices.contiguous()
        b, n, _ = vertices.shape
        ecap = topo.capacity
        out = torch.empty(b, ecap, dtype=torch.float32, device=dev)
        with _lib.on_device(dev) as stream:
            _lib.check(_lib.lib().pp_mesh_edge_sqrlen_forward_f32(
                _lib.ptr(vertices), _lib.ptr(topo.edges), _lib.ptr(topo.counts), _lib.ptr(out), b, n, ecap,
                int(topo.batch == 1), stream), "mesh_edge_sqrlen forward")
        ctx.save_for_backward(vertices)
        ctx.topo = topo
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        if not ctx.needs_input_grad[0]:
            return None, None
        (vertices,) = ctx.saved_tensors
        topo = ctx.topo
        dev = vertices.device
        b, n, _ = vertices.shape
        grad_out = grad_out.contiguous()
        grad = torch.empty_like(vertices)
        with _lib.on_device(dev):
            inc_start, inc_entries = topo.incidence()
        with _lib.on_device(dev) as stream:
            _lib.check(_lib.lib().pp_mesh_edge_sqrlen_backward_f32(
                _lib.ptr(vertices), _lib.ptr(topo.edges), _lib.ptr(inc_start), _lib.ptr(inc_entries),
                _lib.ptr(grad_out), _lib.ptr(grad), b, n, topo.capacity, int(topo.batch == 1), stream),
                "mesh_edge_sqrlen backward")
        return grad, None


def mesh_edge_sqrlen(vertices, topo):
    """Squared lengths ``(B,Ecap)`` of the edges of ``topo`` (a ``MeshEdges``) over ``vertices`` (B,N,D):
    ``|v[b,edges[e,0]] - v[b,edges[e,1]]|^2`` for ``e < count[b]``, 0 in the padding rows.  A topology of one batch
    element serves every ``b`` without a copy.  Differentiable in ``vertices``.

    CUDA fp32 with D = 3: the HIP kernels (the value is bit-identical to ``knn_edge_lengths(..., squared=True)`` for
    the same vertex pair; the backward gives the same bits on every run, so ``torch.use_deterministic_algorithms``
    changes nothing); anything else: ``sqrlen_composition``.  Nothing synchronises with the host."""
    _check(vertices, topo)
    if (vertices.is_cuda and vertices.dtype == torch.float32 and vertices.shape[2] == 3
            and vertices.shape[0] * max(topo.capacity, vertices.shape[1]) <= _LIMIT):
        return MeshEdgeSqrLen.apply(vertices, topo)
    return sqrlen_composition(vertices, topo)
