"""Drop-in for the hot-path names of ``pytorch_points.network.geo_operations``: FurthestPointSampling /
furthest_point_sample (reference network/geo_operations.py:11-64), the PCA point normals batch_normals
(:88-126), the cage coordinates mean_value_coordinates_3D (:349-456), mean_value_coordinates (:459-526, the 2-D
polygon cage) and green_coordinates_3D (:625-773), green_coordinates_2D (:622, declared and left empty in the
reference: the contract is this project's, DESIGN.md "Green coordinates, 2-D") with deform_with_green_coordinates_2D,
and the face normals those need, compute_face_normals_and_areas (:529-559), the point-cloud Laplacian
pointUniformLaplacian (:128-152), the mesh Laplacians UniformLaplacian, CotLaplacian and cotangent (:155-346), and
the mesh edge utilities edge_vertex_indices and get_edge_lengths (:562-600), and the face-to-face angles get_normals
(:603-619, without its stray check_values line) and dihedral_angle (:775-789) with the (E,4) table they work on,
get_edge_points (utils/geometry_utils.py:242-341: build_gemm, get_edge_points, get_side_points), and the mesh normals
mesh_face_normals / mesh_vertex_normals (the reference has no vertex normals) with normalize_to_same_area
(utils/geometry_utils.py:15-25), and the step from a mesh to points on its surface, which the reference lacks:
mesh_sample_faces, mesh_interpolate and sample_points_from_meshes of pytorch_points_amd.mesh_sample under their names,
and the exact distances point_face_distance and face_point_distance of pytorch_points_amd.mesh_distance, with the
side of the mesh from pytorch_points_amd.mesh_winding: mesh_winding_number, points_inside_mesh and
point_mesh_signed_distance.
Every function of the reference's geo_operations.py is served."""
import collections

import numpy as np
import torch

from .. import green as _green
from .. import green2d as _green2d
from .. import knn_edges as _knn_edges
from .. import _mesh_topology
from .. import mesh_dihedral as _mesh_dihedral
from .. import mesh_edges as _mesh_edges
from .. import mesh_laplacian as _mesh_laplacian
from .. import mesh_normals as _mesh_normals
from ..mesh_distance import face_point_distance, point_face_distance  # noqa: F401 (no counterpart in the reference)
from ..mesh_sample import mesh_interpolate, mesh_sample_faces, sample_points_from_meshes  # noqa: F401  (no counterpart)
from ..mesh_winding import PointMeshSignedDistance, mesh_winding_number  # noqa: F401 (no counterpart in the reference)
from ..mesh_winding import point_mesh_signed_distance, points_inside_mesh  # noqa: F401
from .. import mvc as _mvc
from .. import mvc2d as _mvc2d
from .. import ops
from .._ext import sampling
from .operations import batch_svd, gather_points

_FAR = 1e10   # initial running minimum of every point (reference :29)


class FurthestPointSampling(torch.autograd.Function):
    """``(xyz (B,N,3), npoint, seedIdx)`` -> int32 ``(B,npoint)``: iterative farthest point sampling started
    at point ``seedIdx``.  Not differentiable."""

    @staticmethod
    def forward(ctx, xyz, npoint, seedIdx):
        batch, n = xyz.shape[0], xyz.shape[1]
        picked = torch.empty((batch, npoint), dtype=torch.int32, device=xyz.device)
        # (the reference fills a temp of 1e10 here, :32-33, and never reads it back: temp=None says exactly that)
        sampling.furthest_sampling(npoint, seedIdx, xyz, None, picked)
        ctx.mark_non_differentiable(picked)
        return picked

    @staticmethod
    def backward(ctx, *unused):
        return None, None, None


_furthest_point_sample = FurthestPointSampling.apply  # type: ignore


class _SampleAndGather(torch.autograd.Function):
    """``furthest_point_sample``'s two steps -- the sampling and ``gather_points`` of the coordinates (reference
    :59-63) -- as ONE launch: ``(points (B,N,3), npoint, seedIdx)`` -> ``(idx (B,npoint) int32,
    chosen (B,3,npoint))``.  The gradient of ``chosen`` is scattered back to ``points`` exactly as
    ``gather_points``' backward does (the ordered form under ``torch.use_deterministic_algorithms``)."""

    @staticmethod
    def forward(ctx, points, npoint, seedIdx):
        batch, n = points.shape[0], points.shape[1]
        picked = torch.empty((batch, npoint), dtype=torch.int32, device=points.device)
        chosen = torch.empty((batch, 3, npoint), dtype=torch.float32, device=points.device)
        sampling.furthest_sampling(npoint, seedIdx, points, None, picked, chosen, True)
        ctx.mark_non_differentiable(picked)
        ctx.save_for_backward(picked)
        ctx.n = n
        return picked, chosen

    @staticmethod
    def backward(ctx, _grad_idx, grad_chosen):
        (picked,) = ctx.saved_tensors
        if grad_chosen is None:
            return None, None, None
        batch, npoint = picked.shape
        grad_cf = grad_chosen.new_zeros((batch, 3, ctx.n))          # the kernel accumulates
        sampling.gather_backward(batch, 3, ctx.n, npoint, grad_chosen.contiguous(), picked, grad_cf)
        return grad_cf.transpose(2, 1), None, None


def furthest_point_sample(xyz, npoint, NCHW=True, seedIdx=0):
    """Sample ``npoint`` points; returns ``(idx (B,npoint) int32, points)`` with ``points`` in the layout of
    the input: ``(B,3,npoint)`` for ``NCHW`` input ``(B,3,N)``, ``(B,npoint,3)`` for ``(B,N,3)``
    (reference :44-64, same messages)."""
    assert (xyz.dim() == 3), "input for furthest sampling must be a 3D-tensor, but xyz.size() is {}".format(xyz.size())
    points_last = xyz.transpose(2, 1) if NCHW else xyz          # (B, N, 3) view
    assert (points_last.size(2) == 3), "furthest sampling is implemented for 3D points"
    points_last = points_last.contiguous()
    if points_last.dtype is torch.float32 and npoint >= 1:
        idx, chosen = _SampleAndGather.apply(points_last, npoint, seedIdx)       # one launch; (B, 3, npoint)
    else:
        idx = _furthest_point_sample(points_last, npoint, seedIdx)
        chosen = gather_points(points_last.transpose(2, 1).contiguous(), idx)   # (B, 3, npoint)
    return idx, (chosen if NCHW else chosen.transpose(2, 1).contiguous())


def batch_normals(points, base=None, nn_size=20, NCHW=True, idx=None):
    """Normals of ``points`` (B,C,M) -- (B,M,C) when not ``NCHW`` -- by PCA of their ``nn_size`` nearest neighbours in
    ``base`` (default: ``points``): the right singular vector of the smallest singular value of each centred
    neighbourhood.  ``idx`` (B,M,nn_size): neighbours given instead of searched.  Returns ``(normals, idx)``, normals in
    the layout of ``points``; the sign of a normal is not defined (reference geo_operations.py:88-126, with
    pytorch_points_amd.ops.knn_points in place of pytorch3d).  Differentiable through batch_svd."""
    if base is None:
        base = points
    if NCHW:
        points = points.transpose(2, 1).contiguous()
        base = base.transpose(2, 1).contiguous()
    assert(nn_size < base.shape[1])
    batch_size, M, C = points.shape
    if idx is None:
        _, idx, grouped_points = ops.knn_points(points, base, K=nn_size, return_nn=True)
    else:
        grouped_points = torch.gather(base.unsqueeze(1).expand(-1, M, -1, -1), 2, idx.unsqueeze(-1).expand(-1, -1, -1, C))
    group_center = torch.mean(grouped_points, dim=2, keepdim=True)
    centred = grouped_points - group_center
    _, _, V = batch_svd(centred.reshape(-1, nn_size, C))
    normals = V[:, :, -1].reshape(batch_size, M, C)
    if NCHW:
        normals = normals.transpose(1, 2)
    return normals, idx


def mean_value_coordinates_3D(query, vertices, faces, verbose=False):
    """Mean value coordinates (Ju et al. 2005) of ``query`` (B,P,3) with respect to the closed triangle cage
    ``vertices`` (B,N,3), ``faces`` (B,F,3): ``wj`` (B,P,N), and ``(wj, wi)`` with ``verbose``, ``wi`` (B,P,F,3) the
    per-face weights.  CUDA fp32 / fp64 run fused HIP kernels; other devices and dtypes a torch composition of the
    same contract (pytorch_points_amd.mvc, DESIGN.md "Mean value coordinates")."""
    return _mvc.mean_value_coordinates_3D(query, vertices, faces, verbose)


def mean_value_coordinates(points, polygon, verbose=False):
    """Mean value coordinates (Floater 2003) of ``points`` (B,2,N) with respect to the closed polygon ``polygon``
    (B,2,M), channel-first: ``phi`` (B,M,N), and ``(phi, w)`` with ``verbose``, ``w`` (B,M,N) the weights before the
    division.  CUDA fp32 / fp64 run fused HIP kernels; other devices and dtypes a torch composition of the same
    contract (pytorch_points_amd.mvc2d, DESIGN.md "Mean value coordinates, 2-D")."""
    return _mvc2d.mean_value_coordinates(points, polygon, verbose)


def compute_face_normals_and_areas(vertices, faces):
    """``(face_normals (B,F,3), face_areas (B,F))`` of the triangles ``faces`` over ``vertices`` (B,N,3); 2-D inputs
    give unbatched outputs (pytorch_points_amd.green)."""
    return _green.compute_face_normals_and_areas(vertices, faces)


def green_coordinates_3D(query, vertices, faces, face_normals=None, verbose=False):
    """Green coordinates (Lipman et al. 2008) of ``query`` (B,P,3) with respect to the closed triangle cage
    ``vertices`` (B,N,3), ``faces`` (B,F,3): ``(GC_vertex (B,P,N), GC_face (B,P,F), exterior_flag (B,P,1))``.
    ``face_normals`` (B,F,3) replaces the normals computed from the cage; ``verbose`` is ignored.  CUDA fp32 / fp64
    run fused HIP kernels; other devices and dtypes a torch composition of the same contract
    (pytorch_points_amd.green, DESIGN.md "Green coordinates")."""
    return _green.green_coordinates_3D(query, vertices, faces, face_normals, verbose)


def green_coordinates_2D(query, vertices, faces, edge_normals=None, verbose=False):
    """Green coordinates (Lipman et al. 2008) of ``query`` (B,P,2) with respect to the polygonal cage ``vertices``
    (B,N,2), ``faces`` (B,F,2) (row ``j`` the directed edge ``(v1, v2)``; outer loops counter-clockwise, holes
    clockwise): ``(phi (B,P,N), psi (B,P,F), exterior_flag (B,P,1))``.  ``edge_normals`` (B,F,2) only orients the
    edges; ``verbose`` is ignored.  CUDA fp32 / fp64 run fused HIP kernels; other devices and dtypes a torch
    composition of the same contract (pytorch_points_amd.green2d, DESIGN.md "Green coordinates, 2-D")."""
    return _green2d.green_coordinates_2D(query, vertices, faces, edge_normals, verbose)


def deform_with_green_coordinates_2D(phi, psi, vertices, new_vertices, faces):
    """``sum_i phi_i v'_i + sum_j psi_j s_j n'_j`` (B,P,2): the queries of ``green_coordinates_2D`` carried along as
    the cage ``vertices`` moves to ``new_vertices``, ``s_j`` the stretch of edge ``j`` and ``n'_j`` its deformed
    normal (pytorch_points_amd.green2d).  Plain torch, differentiable."""
    return _green2d.deform_with_green_coordinates_2D(phi, psi, vertices, new_vertices, faces)


def pointUniformLaplacian(points, knn_idx=None, nn_size=3):
    """Uniform Laplacian of a point cloud: ``(lap (B,N,D), knn_idx (B,N,K))`` with ``lap[n] = -mean_k points[knn_idx[n,k]]
    + points[n]``.  ``knn_idx`` None: the ``nn_size`` nearest neighbours of every point (a search for ``nn_size + 1``
    whose first column, the point itself, is dropped; reference :128-152).  No (B,N,K,D) gather is made
    (pytorch_points_amd.knn_edges, DESIGN.md "k-NN edge operators")."""
    if knn_idx is None:
        assert(nn_size < points.shape[1])
        knn_idx = ops.knn_points(points, points, K=nn_size + 1).idx[:, :, 1:]
    return _knn_edges.knn_laplacian(points, knn_idx), knn_idx


def edge_vertex_indices(F):
    """Unique edges ``(E,2)`` of the triangle list ``F`` (F,3): every face's corner pairs as (min,max), the distinct
    rows in ascending lexicographic order (reference :562-583).  A CUDA integer tensor runs the HIP build with
    ``n_vertices = F.max() + 1`` and is sliced by the count it reports: two host reads (the reference's
    ``torch.unique`` synchronises too); a negative index raises IndexError there.  A CPU tensor goes through the
    torch composition, a numpy array through ``np.unique`` and comes back as numpy.  For a loop that keeps its
    topology, build a ``pytorch_points_amd.mesh_edges.MeshEdges`` once instead."""
    if not isinstance(F, torch.Tensor):
        F = np.asarray(F)
        pairs = np.sort(np.stack([F, F[:, [1, 2, 0]]], axis=-1), axis=-1)
        return np.unique(pairs.reshape([-1, 2]), axis=0)
    if F.dim() != 2 or F.shape[1] != 3:
        raise NotImplementedError("edge_vertex_indices: F must have shape (F, 3) (triangles), got %s" % (tuple(F.shape),))
    if not _mesh_topology.is_index(F):
        raise TypeError("edge_vertex_indices: F must be an integer tensor, got %s" % F.dtype)
    if not F.is_cuda or F.shape[0] == 0:
        return _mesh_edges.unique_edges_composition(F)
    fl = (F if F.dtype == torch.int64 else F.long()).contiguous().unsqueeze(0)
    n_vertices = int(fl.max()) + 1                                        # host read 1
    status = torch.empty(2, 1, dtype=torch.int32, device=F.device)
    edges = _mesh_edges._unique_edges_hip(fl, max(n_vertices, 0), status)
    count, flag = status[:, 0].tolist()                                   # host read 2
    if flag:
        raise IndexError("edge_vertex_indices: F holds a negative vertex index")
    return edges[0, :count].to(F.dtype)


def get_edge_lengths(vertices, edge_points):
    """SQUARED lengths ``(E,)`` of the edges ``edge_points[:, :2]`` over ``vertices`` (N,D), despite the name
    (reference :586-600).  CUDA fp32 with D = 3 runs the HIP kernel; its backward builds the edges' vertex incidence
    when, and only when, a gradient is asked for.  Nothing synchronises with the host: on that path an index outside
    [0, N) gives a NaN length (the reference wraps a negative index and faults on a large one)."""
    if vertices.dim() != 2 or edge_points.dim() != 2 or edge_points.shape[1] < 2:
        raise ValueError("get_edge_lengths: vertices (N, D) and edge_points (E, >= 2), got %s and %s"
                         % (tuple(vertices.shape), tuple(edge_points.shape)))
    if vertices.is_cuda and vertices.dtype == torch.float32 and vertices.shape[1] == 3 and edge_points.is_cuda:
        if not _mesh_topology.is_index(edge_points):
            raise TypeError("get_edge_lengths: edge_points must be an integer tensor, got %s" % edge_points.dtype)
        edges = edge_points[:, :2].long().contiguous().unsqueeze(0)
        topo = _mesh_edges.MeshEdges._unchecked(edges, vertices.shape[0])
        return _mesh_edges.mesh_edge_sqrlen(vertices.unsqueeze(0), topo)[0]
    ends = vertices[edge_points[:, :2]]
    t = ends[:, 0, :] - ends[:, 1, :]
    return torch.sum(t * t, dim=-1)


# -------------------------------------------------------------------------------------- mesh dihedral angles
def get_edge_points(faces_or_mesh, n_vertices=None):
    """The ``(E,4)`` int64 table ``[a, c, w0, w1]`` of a triangle mesh (reference utils/geometry_utils.py:242-341,
    there a Python loop over the faces): ``(a,c)`` the unique edges in ``edge_vertex_indices``' order, ``w0`` / ``w1``
    the corners opposite the edge in its incident half-edge with the lowest / highest number ``3*f + j``, ``w1 == w0``
    on a boundary edge (the reference's ``get_side_points`` there).  ``faces_or_mesh``: a ``(F,3)`` tensor or array,
    or any object with ``fs`` (and ``vs`` for the vertex count); a tensor gives a tensor on its device, anything else
    a numpy array.  The reference's column order follows its face traversal; ``dihedral_angle`` does not depend on it.
    An edge with more than two incident half-edges raises ValueError (the reference's ``build_gemm``: IndexError), an
    index outside ``[0, n_vertices)`` IndexError.  ``n_vertices`` defaults to ``faces.max() + 1`` (on CUDA a second
    host read beside the build's own).  For a loop that keeps its topology, build a
    ``pytorch_points_amd.mesh_dihedral.MeshEdgePoints`` once instead."""
    faces = faces_or_mesh
    if hasattr(faces_or_mesh, "fs"):
        faces = faces_or_mesh.fs
        if n_vertices is None and getattr(faces_or_mesh, "vs", None) is not None:
            n_vertices = len(faces_or_mesh.vs)
    as_tensor = isinstance(faces, torch.Tensor)
    if not as_tensor:
        faces = torch.from_numpy(np.ascontiguousarray(np.asarray(faces)))
    if faces.dim() != 2 or faces.shape[1] != 3:
        raise NotImplementedError("get_edge_points: faces must have shape (F, 3) (triangles), got %s"
                                  % (tuple(faces.shape),))
    if not _mesh_topology.is_index(faces):
        raise TypeError("get_edge_points: faces must be integers, got %s" % faces.dtype)
    if faces.shape[0] == 0:
        table = faces.new_empty((0, 4), dtype=torch.int64)
    else:
        if n_vertices is None:
            n_vertices = max(int(faces.max()) + 1, 0)
        table = _mesh_dihedral.MeshEdgePoints.from_faces(faces, n_vertices).table(0)
    return table if as_tensor else table.numpy()


def get_normals(vertices, edge_points, side):
    """The unit normal ``(E,3)`` of the face on one side of every edge (reference :603-619, without the
    ``check_values`` line it dies on): ``vertices`` (N,3), ``edge_points`` (E,4), ``side`` 0-3 -- sides 0, 1 the face
    with column 2 seen from column 0, sides 2, 3 the face with column 3 seen from column 1.  Torch operations."""
    base, other, wing = (0, 1, 2) if side < 2 else (1, 0, 3)        # the face (base, other end, wing), seen from base
    origin = vertices[edge_points[:, base]]
    to_wing = vertices[edge_points[:, wing]] - origin
    along = vertices[edge_points[:, other]] - origin
    return torch.nn.functional.normalize(torch.cross(to_wing, along, dim=-1), dim=-1)


def dihedral_angle(vertices, edge_points):
    """The face-to-face angle ``(E,)`` across the edges given by their four ``edge_points`` (E,4) over ``vertices``
    (N,3): ``pi - acos(clamp(n_a . n_b, -1+1e-6, 1-1e-6))`` (reference :775-789).  CUDA fp32 runs the HIP kernels; the
    backward builds the table's vertex lists when, and only when, a gradient is asked for.  Nothing synchronises with
    the host: on that path an index outside [0, N) gives a NaN angle (the reference wraps a negative index and faults
    on a large one).  Other devices and dtypes: ``pytorch_points_amd.mesh_dihedral.dihedral_composition``, with an
    IndexError for such an index on the CPU."""
    if vertices.dim() != 2 or vertices.shape[1] != 3 or edge_points.dim() != 2 or edge_points.shape[1] != 4:
        raise ValueError("dihedral_angle: vertices (N, 3) and edge_points (E, 4), got %s and %s"
                         % (tuple(vertices.shape), tuple(edge_points.shape)))
    if not _mesh_topology.is_index(edge_points):
        raise TypeError("dihedral_angle: edge_points must be an integer tensor, got %s" % edge_points.dtype)
    if edge_points.is_cuda:
        topo = _mesh_dihedral.MeshEdgePoints._unchecked(edge_points.long().contiguous().unsqueeze(0), vertices.shape[0])
    else:
        topo = _mesh_dihedral.MeshEdgePoints.from_edge_points(edge_points, vertices.shape[0])
    return _mesh_dihedral.mesh_dihedral_angle(vertices.unsqueeze(0), topo)[0]


# ----------------------------------------------------------------------------------------------- mesh normals
def _corners_of(what, vertices, faces_or_corners):
    """a ``MeshCorners`` as it is; a faces tensor (F,3) / (B,F,3) builds one for this call (one host read)"""
    if isinstance(faces_or_corners, _mesh_laplacian.MeshCorners):
        return faces_or_corners
    if not isinstance(faces_or_corners, torch.Tensor):
        raise TypeError("%s: faces_or_corners must be an integer tensor or a MeshCorners, got %s"
                        % (what, type(faces_or_corners).__name__))
    if vertices.dim() != 3:
        raise ValueError("%s: vertices must have shape (B, N, 3), got %s" % (what, tuple(vertices.shape)))
    return _mesh_laplacian.MeshCorners.from_faces(faces_or_corners.to(vertices.device), vertices.shape[1])


def mesh_face_normals(vertices, faces_or_corners):
    """``(normals (B,F,3), areas (B,F))`` of a triangle mesh: ``compute_face_normals_and_areas``' values through
    ``pytorch_points_amd.mesh_normals.mesh_face_normals`` -- on CUDA fp32 one HIP launch forward and a gather backward
    with no floating-point atomics; a face without area passes no gradient (there: NaN).  ``faces_or_corners``: the
    faces (F,3) or (B,F,3), whose corner lists are then built for this call, or a kept ``MeshCorners``."""
    corners = _corners_of("mesh_face_normals", vertices, faces_or_corners)
    return _mesh_normals.mesh_face_normals(vertices, corners)


def mesh_vertex_normals(vertices, faces_or_corners, weighting="area"):
    """Unit vertex normals ``(B,N,3)`` of a triangle mesh (the reference has none): the normalised sum over a
    vertex's corners of the face's cross product (``weighting="area"``) or unit normal (``"uniform"``); ``+0`` for a
    vertex no face uses (``pytorch_points_amd.mesh_normals.mesh_vertex_normals``).  ``faces_or_corners`` as in
    ``mesh_face_normals``."""
    corners = _corners_of("mesh_vertex_normals", vertices, faces_or_corners)
    return _mesh_normals.mesh_vertex_normals(vertices, corners, weighting)


def normalize_to_same_area(v_ref, f_ref, v, f):
    """``v`` (B,N,3) scaled so that the mesh ``(v, f)`` has the surface area of ``(v_ref, f_ref)``:
    ``v * sqrt(sum(A_ref) / sum(A))`` per batch element (reference utils/geometry_utils.py:15-25).  Differentiable in
    both vertex sets; either face argument is a faces tensor or a kept ``MeshCorners``."""
    area_ref = mesh_face_normals(v_ref, f_ref)[1].sum(dim=-1)
    area = mesh_face_normals(v, f)[1].sum(dim=-1)
    return v * torch.sqrt(area_ref / area).unsqueeze(-1).unsqueeze(-1)


# ------------------------------------------------------------------------------------------- mesh Laplacians
class UniformLaplacian(torch.nn.Module):
    """Uniform Laplacian of a mesh (reference :155-205): ``verts`` (B,N,D), ``faces`` (B,F,L) of any degree L >= 3 ->
    ``L verts / (Lii + 1e-12)`` (B,N,D), with half-edge multiplicities as weights.

    ``self.L`` is built on the first call that finds it None (``faces`` is required then) and kept; assigning
    ``laplacian.L = None`` resets it.  It is a ``pytorch_points_amd.mesh_laplacian.MeshCorners`` -- the sorted
    vertex -> corner lists -- not a sparse matrix; ``self.Lii`` is the reference's (Bt*N,) tensor of ``2 * #corners``.
    An ``L`` built from a single mesh serves a batch (the reference's ``self.L.shape[0] != B*N`` branch).  The build
    makes one device-to-host copy; nothing afterwards touches the host."""

    def __init__(self):
        super().__init__()
        self.L = None

    def computeLaplacian(self, V, F):
        self.L = _mesh_laplacian.MeshCorners.from_faces(F.to(V.device), V.shape[1])
        self.Lii = self.L.lii(V.dtype)

    def forward(self, verts, faces=None):
        if self.L is None:
            assert(faces is not None)
            self.computeLaplacian(verts, faces)
        if self.L.batch != verts.shape[0]:
            # during initialization, used a single batch point set
            assert(self.L.batch == 1)
        return _mesh_laplacian.mesh_uniform_laplacian(verts, self.L)


CotOperator = collections.namedtuple("CotOperator", ["corners", "weights"])
CotOperator.__doc__ = """what ``CotLaplacian.L`` holds: the ``MeshCorners`` of the faces and the detached cotangents
(B,F,3) of the vertices that built it"""


class CotLaplacian(torch.nn.Module):
    """Cotangent Laplacian of a triangle mesh (reference :218-304): ``V`` (B,N,3), ``F`` (B,F,3) -> ``L V`` (B,N,3).

    ``self.L`` is built on the first call that finds it None (``F`` is required then) from THAT call's ``V`` and kept:
    the operator is a constant, later calls reuse its cotangents whatever their ``V``, and the backward is the same
    operator applied to the incoming gradient.  Assigning ``laplacian.L = None`` resets it.  It is a ``CotOperator``
    (corner lists and cotangents on the device), not a scipy matrix, and every apply, forward and backward, stays on
    the device.  The build makes two device-to-host copies: the topology's out-of-range flags and the reference's
    ``check_values`` of the cotangents, which raises ValueError here on a non-finite cotangent (the reference
    asserts); nothing afterwards touches the host.  Unlike the reference's, the build does not print.  The output's
    ``requires_grad`` follows ``V``'s."""

    def __init__(self):
        super().__init__()
        self.L = None

    def computeLaplacian(self, V, F):
        F = F.detach()
        if F.shape[-1] != 3:
            raise NotImplementedError("CotLaplacian: triangles only, got faces of %d corners" % F.shape[-1])
        corners = _mesh_laplacian.MeshCorners.from_faces(F.to(V.device), V.shape[1])
        C = cotangent(V.detach(), corners.faces).detach()
        if not bool(torch.isfinite(C).all()):          # the reference's assert(check_values(C)); once per build
            raise ValueError("CotLaplacian: the cotangents of the mesh are not all finite")
        self.L = CotOperator(corners, C)

    def forward(self, V, F=None):
        if self.L is None:
            assert(F is not None)
            self.computeLaplacian(V, F)
        return _mesh_laplacian.mesh_cot_laplacian(V, self.L.corners, self.L.weights)


def cotangent(V, F):
    """Cotangents ``C`` (B,F,3) of the angles of the triangles ``F`` (B,F,3) over ``V`` (B,N,3), columns for the edges
    23, 31, 12 (reference :306-346): Heron's area, ``(l_a^2 + l_b^2 - l_c^2) / (A + 1e-10) / 4``, exactly 0 for a face
    without area.  CUDA fp32 runs the HIP kernel when no gradient to ``V`` is asked for (``CotLaplacian`` detaches);
    with ``V.requires_grad``, and on other devices and dtypes, the same formula as torch operations
    (pytorch_points_amd.mesh_laplacian)."""
    return _mesh_laplacian.cotangent(V, F)
