"""The edge operators under the reference's mesh losses (network/model_loss.py:166-308, geo_operations.py:562-600):

    MeshEdges.from_faces(faces (B,F,3), n_vertices)   the unique edges of a triangle mesh and their vertex incidence
    MeshEdges.from_edges(edges (E,2), n_vertices)     the same object over a user's edge list
    mesh_edge_sqrlen(vertices (B,N,3), topo)     ->   (B,Ecap) squared edge lengths, 0 in the padding

A mesh's connectivity does not change between training steps, so the topology is an object that is built once (with one
device-to-host copy) and kept; a step on it is two launches and never synchronises with the host.  CUDA runs the HIP
kernels of csrc/mesh_edges.hip (``pp_mesh_*``): the unique edges in ``torch.unique``'s row order bit for bit, and a
backward that is a gather over each vertex's sorted incidence list -- no floating-point atomics, the same bits on every
run, one form only.  CPU tensors, other dtypes and D != 3 go through ``sqrlen_composition``, the same contract written
as torch operations.  What the topology object shares with the other mesh operators -- normalising the index tensor,
one topology for a batch, the single host read, the errors, the step's autograd Function -- is ``_mesh_topology``;
here are the build chain and the composition.  DESIGN.md "Mesh edge operators" states the contract.
"""
import torch

from . import _lib
from . import _mesh_topology as _topology


def _unique_edges_hip(faces, n_vertices, status):
    """kernel (a): contiguous int64 CUDA ``faces`` (Bt,F,3) -> ``edges`` (Bt,3F,2); counts into ``status[0]``, flags
    into ``status[1]`` (int32 (2,Bt)).  No host synchronisation."""
    dev = faces.device
    bt, f = faces.shape[0], faces.shape[1]
    _topology.fits("unique edges", bt, n_vertices, 3 * f)
    edges = torch.empty(bt, 3 * f, 2, dtype=torch.int64, device=dev)
    with _lib.on_device(dev) as stream:
        wsp, nbytes, ws = _topology.workspace(dev, bt, n_vertices, 3 * f)
        _lib.check(_lib.lib().pp_mesh_unique_edges(_lib.ptr(faces), _lib.ptr(edges), _lib.ptr(status[0]),
                                                   _lib.ptr(status[1]), bt, f, n_vertices, wsp, nbytes, stream),
                   "mesh unique edges")
    return edges


def unique_edges_composition(faces):
    """The unique edges of ONE triangle list ``faces`` (F,3), an integer tensor on any device, as torch operations:
    every face's three corner pairs as (min,max), the distinct rows in ascending lexicographic order ``(E,2)``."""
    pairs = torch.stack([faces, faces[:, [1, 2, 0]]], dim=-1)
    return torch.unique(torch.sort(pairs, dim=-1)[0].reshape(-1, 2), dim=0)


class MeshEdges(_topology.VertexTable):
    """The edge topology of a batch of meshes over ``n_vertices`` vertices each.

    ``edges`` (Bt,Ecap,2) int64: rows ``[0, count[b])`` are the edges, later rows ``(-1,-1)``; ``counts`` (Bt,) int32 on
    the device; ``counts_host`` the same numbers as a tuple of Python ints; ``incidence()`` the ``(inc_start (Bt,N+1),
    inc_entries (Bt,2*Ecap))`` lists the backward gathers over (CUDA only).  ``Bt`` is 1 for a topology that a whole
    batch shares: a ``faces`` view with batch stride 0, or an un-batched edge list.

    Building with ``from_faces`` / ``from_edges`` makes EXACTLY ONE device-to-host copy -- the counts and the
    out-of-range flags together -- and nothing that uses the object afterwards synchronises with the host.  An index
    outside ``[0, n_vertices)`` raises IndexError naming the batch element (the reference would fault on the device);
    on the GPU it is only ever compared, never used as an address.  (The shared layer, ``_mesh_topology``, keeps
    this.)"""

    COLS, NAME = 2, "edges"
    edges = property(lambda self: self._rows)

    def edge_list(self, b):
        """``(E_b,2)`` int64 view of the edges of batch element ``b``"""
        return self._view(b)

    @classmethod
    def from_faces(cls, faces, n_vertices):
        """The unique edges of the triangles ``faces`` (B,F,3) or (F,3), an integer tensor.  A face with a repeated
        vertex keeps its ``(a,a)`` edge, as the reference's ``torch.unique`` does."""
        what = "MeshEdges.from_faces"
        faces = _topology.index_table(what, "faces", faces, "(B, F, 3)", None,
                                      triangles=" (the reference pairs the corners through F[:, [1, 2, 0]])")
        n_vertices = int(n_vertices)
        bt, f = faces.shape[0], faces.shape[1]
        if not faces.is_cuda:
            _topology.raise_flagged(what, _topology.out_of_range(faces, n_vertices))
            return cls._padded([unique_edges_composition(faces[b]) for b in range(bt)], faces, 3 * f, n_vertices)
        status = torch.empty(2, bt, dtype=torch.int32, device=faces.device)
        return cls._read_back(what, _unique_edges_hip(faces, n_vertices, status), status, n_vertices)

    @classmethod
    def from_edges(cls, edges, n_vertices):
        """Any edge list ``edges`` (E,2) -- shared by the batch -- or (B,E,2), an integer tensor: pairs may repeat, need
        no order and may join a vertex to itself.  Columns beyond the first two are ignored."""
        what = "MeshEdges.from_edges"
        edges = _topology.index_table(what, "edges", edges, "(E, 2) or (B, E, 2)", lambda cols: cols >= 2, keep=2)
        return cls._from_rows(what, edges, int(n_vertices))


def sqrlen_composition(vertices, topo):
    """``mesh_edge_sqrlen`` as torch operations, for any device, floating dtype and D: gather, subtract, square-sum in
    ascending dimension, padding masked to 0."""
    _topology.check_vertices("mesh_edge_sqrlen", vertices, topo, MeshEdges)
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


MeshEdgeSqrLen = _topology.gather_function(
    "MeshEdgeSqrLen", "HIP forward and backward (CUDA fp32, D = 3).", "pp_mesh_edge_sqrlen_forward_f32",
    "pp_mesh_edge_sqrlen_backward_f32", "mesh_edge_sqrlen")


def mesh_edge_sqrlen(vertices, topo):
    """Squared lengths ``(B,Ecap)`` of the edges of ``topo`` (a ``MeshEdges``) over ``vertices`` (B,N,D):
    ``|v[b,edges[e,0]] - v[b,edges[e,1]]|^2`` for ``e < count[b]``, 0 in the padding rows.  A topology of one batch
    element serves every ``b`` without a copy.  Differentiable in ``vertices``.

    CUDA fp32 with D = 3: the HIP kernels (the value is bit-identical to ``knn_edge_lengths(..., squared=True)`` for
    the same vertex pair; the backward gives the same bits on every run, so ``torch.use_deterministic_algorithms``
    changes nothing); anything else: ``sqrlen_composition``.  Nothing synchronises with the host."""
    _topology.check_vertices("mesh_edge_sqrlen", vertices, topo, MeshEdges)
    if (vertices.is_cuda and vertices.dtype == torch.float32 and vertices.shape[2] == 3
            and vertices.shape[0] * max(topo.capacity, vertices.shape[1]) <= _topology.LIMIT):
        return MeshEdgeSqrLen.apply(vertices, topo)
    return sqrlen_composition(vertices, topo)
