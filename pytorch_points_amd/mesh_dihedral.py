"""The face-to-face angle across the edges of a triangle mesh (reference network/geo_operations.py:603-619 get_normals,
:775-789 dihedral_angle) and the (E,4) "edge points" table it works on (reference utils/geometry_utils.py:242-341):

    MeshEdgePoints.from_faces(faces (B,F,3), n_vertices)         the table [a, c, w0, w1] of every unique edge
    MeshEdgePoints.from_edge_points(edge_points (E,4), n_vertices)   the same object over a user's table
    mesh_dihedral_angle(vertices (B,N,3), topo)             ->   (B,Ecap) angles, 0 in the padding

The fourth mesh operator on the pattern of ``mesh_edges``: the topology is an object that is built once (with one
device-to-host copy) and kept; a step on it is two launches and never synchronises with the host.  CUDA fp32 runs the
HIP kernels of csrc/mesh_dihedral.hip (``pp_mesh_edge_points*``, ``pp_mesh_dihedral_*``): a backward that is a gather
over each vertex's sorted list of table entries -- no floating-point atomics, the same bits on every run, one form
only.  CPU tensors and other dtypes go through ``dihedral_composition``, the same contract written as torch
operations.  ``MeshEdgePoints`` is ``_mesh_topology``'s counted row table with four columns and the step its
``gather_function``; here are the table's build chain and the composition.  DESIGN.md "Mesh dihedral angles" states
the contract.
"""
import math

import torch

from . import _lib
from . import _mesh_topology as _topology
from . import mesh_edges as _mesh_edges
from .mesh_normals import _cross

_EPS = 1e-12                      # F.normalize's eps
_LO, _HI = -1 + 1e-6, 1 - 1e-6    # the reference's clamp


def _edge_points_hip(faces, edges, counts, nonmanifold, n_vertices):
    """contiguous int64 CUDA ``faces`` (Bt,F,3) and their unique ``edges`` (Bt,Ecap,2), int32 ``counts`` (Bt) ->
    ``edge_points`` (Bt,Ecap,4); an edge with more than two half-edges is ORed into ``nonmanifold`` (Bt, initialised)"""
    dev = faces.device
    bt, f, ecap = faces.shape[0], faces.shape[1], edges.shape[1]
    _topology.fits("edge points", bt, n_vertices, 4 * ecap)
    edge_points = torch.empty(bt, ecap, 4, dtype=torch.int64, device=dev)
    with _lib.on_device(dev) as stream:
        _lib.check(_lib.lib().pp_mesh_edge_points(_lib.ptr(faces), _lib.ptr(edges), _lib.ptr(counts),
                                                  _lib.ptr(edge_points), _lib.ptr(nonmanifold), bt, f, ecap,
                                                  n_vertices, stream), "mesh edge points")
    return edge_points


def edge_points_composition(faces):
    """The table of ONE triangle list ``faces`` (F,3), an integer tensor, built on the CPU: ``(E,4)`` int64 rows
    ``[a, c, w0, w1]`` -- ``(a,c)`` the unique edges as ``unique_edges_composition`` orders them, ``w0`` / ``w1`` the
    corner opposite the edge in its incident half-edge with the lowest / highest number ``3*f + j`` (half-edge ``j``
    joins corners ``j`` and ``(j+1) % 3``), ``w1 == w0`` on a boundary edge.  ValueError for an edge with more than
    two incident half-edges."""
    faces = faces.detach().cpu().long()
    pairs = torch.sort(torch.stack([faces, faces[:, [1, 2, 0]]], dim=-1), dim=-1)[0].reshape(-1, 2)
    wing = faces[:, [2, 0, 1]].reshape(-1)
    edges, inverse = torch.unique(pairs, dim=0, return_inverse=True)
    e = edges.shape[0]
    if e == 0:
        return faces.new_empty(0, 4)
    if int(torch.bincount(inverse, minlength=e).max()) > 2:
        raise ValueError("edge_points_composition: an edge has more than two incident half-edges (a non-manifold "
                         "edge or a duplicated face)")
    number = torch.arange(pairs.shape[0])
    lowest = torch.full((e,), pairs.shape[0], dtype=torch.int64).scatter_reduce(0, inverse, number, "amin")
    highest = torch.full((e,), -1, dtype=torch.int64).scatter_reduce(0, inverse, number, "amax")
    return torch.cat([edges, wing[lowest][:, None], wing[highest][:, None]], dim=1)


class MeshEdgePoints(_topology.VertexTable):
    """The edge-points topology of a batch of meshes over ``n_vertices`` vertices each.

    ``edge_points`` (Bt,Ecap,4) int64: rows ``[0, count[b])`` are ``[a, c, w0, w1]``, later rows ``-1``; ``counts``
    (Bt,) int32 on the device; ``counts_host`` the same numbers as a tuple of Python ints; ``incidence()`` the
    ``(start (Bt,N+1), entries (Bt,4*Ecap))`` lists of ``4*e + slot`` the backward gathers over (CUDA only).  ``Bt``
    is 1 for a topology that a whole batch shares: a ``faces`` view with batch stride 0, or an un-batched table.

    Building with ``from_faces`` / ``from_edge_points`` makes EXACTLY ONE device-to-host copy -- the counts and both
    flags together -- and nothing that uses the object afterwards synchronises with the host.  An index outside
    ``[0, n_vertices)`` raises IndexError and an edge with more than two incident half-edges ValueError, each naming
    the batch element (the reference's ``build_gemm`` raises IndexError for the latter).  (The shared layer,
    ``_mesh_topology``, keeps this.)"""

    COLS, NAME = 4, "edge_points"
    edge_points = property(lambda self: self._rows)

    def table(self, b):
        """``(E_b,4)`` int64 view of the rows of batch element ``b``"""
        return self._view(b)

    @classmethod
    def from_faces(cls, faces, n_vertices):
        """The table of the triangles ``faces`` (B,F,3) or (F,3), an integer tensor; the edge numbering is that of
        ``MeshEdges.from_faces(faces, n_vertices).edges``."""
        what = "MeshEdgePoints.from_faces"
        faces = _topology.index_table(what, "faces", faces, "(B, F, 3)", None, triangles="")
        n_vertices = int(n_vertices)
        bt, f = faces.shape[0], faces.shape[1]
        if not faces.is_cuda:
            _topology.raise_flagged(what, _topology.out_of_range(faces, n_vertices))
            tables = []
            for b in range(bt):
                try:
                    tables.append(edge_points_composition(faces[b]))
                except ValueError:
                    _topology.raise_flagged(what, (), [0] * b + [1])
            return cls._padded(tables, faces, 3 * f, n_vertices)
        status = torch.empty(3, bt, dtype=torch.int32, device=faces.device)   # counts, range flags, manifold flags
        status[2] = 0
        edges = _mesh_edges._unique_edges_hip(faces, n_vertices, status)
        edge_points = _edge_points_hip(faces, edges, status[0], status[2], n_vertices)
        return cls._read_back(what, edge_points, status, n_vertices)

    @classmethod
    def from_edge_points(cls, edge_points, n_vertices):
        """A user's table ``edge_points`` (E,4) -- shared by the batch -- or (B,E,4), an integer tensor, in any column
        order the reference's ``get_edge_points`` may give (the angle does not depend on it)."""
        what = "MeshEdgePoints.from_edge_points"
        edge_points = _topology.index_table(what, "edge_points", edge_points, "(E, 4) or (B, E, 4)",
                                            lambda cols: cols == 4)
        return cls._from_rows(what, edge_points, int(n_vertices))


def _unit(n):
    """``(n / max(|n|, 1e-12), |n| > 1e-12)``: F.normalize's value; a normal of length <= 1e-12 passes no gradient"""
    sq = (n[..., 0] * n[..., 0] + n[..., 1] * n[..., 1]) + n[..., 2] * n[..., 2]
    ok = torch.sqrt(sq.detach()) > _EPS
    length = torch.sqrt(torch.where(ok, sq, torch.ones_like(sq)))
    return torch.where(ok[..., None], n / length[..., None], n.detach() / _EPS), ok


def dihedral_composition(vertices, topo):
    """``mesh_dihedral_angle`` as torch operations, for any device and floating dtype.  With ``p_k`` the vertices of a
    row taken in canonical order (ends ascending, wings ascending): ``na = cross(p2-p0, p1-p0)``, ``nb = cross(p3-p1,
    p0-p1)``, both through ``F.normalize``'s ``n / max(|n|, 1e-12)``, ``d = clamp(na . nb, -1+1e-6, 1-1e-6)``,
    ``pi - acos(d)``; padding rows 0; a row with an index outside [0, N) NaN.  An edge with a normal of length
    <= 1e-12 (a degenerate face) keeps the reference's value and contributes a zero gradient, where
    ``F.normalize``'s backward would give about 1e12."""
    _topology.check_vertices("mesh_dihedral_angle", vertices, topo, MeshEdgePoints, d3=True)
    b, n, _ = vertices.shape
    ecap = topo.capacity
    valid = torch.arange(ecap, device=vertices.device)[None, :] < topo.counts[:, None].long()      # (Bt,Ecap)
    if n == 0 or ecap == 0:
        out = vertices.new_zeros(b, ecap) + vertices.sum() * 0
        return torch.where(valid.expand(b, -1), torch.full_like(out, float("nan")), out)
    table = topo.edge_points
    bad = ((table < 0) | (table >= n)).any(-1) & valid
    table = torch.cat([torch.sort(table[..., :2], dim=-1)[0], torch.sort(table[..., 2:], dim=-1)[0]], dim=-1)
    table = table.clamp(0, n - 1).expand(b, -1, -1)
    p = [torch.gather(vertices, 1, table[:, :, k:k + 1].expand(-1, -1, 3)) for k in range(4)]
    ua, oka = _unit(_cross(p[2] - p[0], p[1] - p[0]))        # (torch.cross may contract a*b - c*d: a wing with two
    ub, okb = _unit(_cross(p[3] - p[1], p[0] - p[1]))        # equal vertices then has a normal of 1e-9, not 0)
    d = (ua[..., 0] * ub[..., 0] + ua[..., 1] * ub[..., 1]) + ua[..., 2] * ub[..., 2]
    d = torch.where(oka & okb, d, d.detach())
    angle = math.pi - torch.acos(d.clamp(_LO, _HI))
    angle = torch.where(bad.expand(b, -1), torch.full_like(angle, float("nan")), angle)
    return torch.where(valid.expand(b, -1), angle, torch.zeros_like(angle))


MeshDihedralAngle = _topology.gather_function(
    "MeshDihedralAngle", "HIP forward and backward (CUDA fp32).", "pp_mesh_dihedral_forward_f32",
    "pp_mesh_dihedral_backward_f32", "mesh_dihedral_angle")


def mesh_dihedral_angle(vertices, topo):
    """Face-to-face angles ``(B,Ecap)`` across the edges of ``topo`` (a ``MeshEdgePoints``) over ``vertices``
    (B,N,3): ``pi - acos(clamp(na . nb, -1+1e-6, 1-1e-6))`` with the unit normals of the two faces at the edge, for
    ``e < count[b]``; 0 in the padding rows.  A flat interior edge gives ``pi - acos(1-1e-6)``, a boundary edge (its
    one face on both sides) ``pi - acos(-1+1e-6)`` and no gradient.  A topology of one batch element serves every
    ``b`` without a copy.  Differentiable in ``vertices``.

    CUDA fp32: the HIP kernels (the backward gives the same bits on every run, so
    ``torch.use_deterministic_algorithms`` changes nothing); anything else: ``dihedral_composition``.  Nothing
    synchronises with the host."""
    _topology.check_vertices("mesh_dihedral_angle", vertices, topo, MeshEdgePoints, d3=True)
    if (vertices.is_cuda and vertices.dtype == torch.float32
            and vertices.shape[0] * max(topo.capacity, vertices.shape[1]) <= _topology.LIMIT
            and 4 * topo.capacity <= _topology.LIMIT):
        return MeshDihedralAngle.apply(vertices, topo)
    return dihedral_composition(vertices, topo)
