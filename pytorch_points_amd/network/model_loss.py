"""Drop-in for the hot-path names of ``pytorch_points.network.model_loss``: NmDistanceFunction /
nndistance and LabeledNmdistanceFunction / labeled_nndistance (reference network/model_loss.py:401-483), and the
point-cloud regularisers PointLaplacianLoss, PointEdgeLengthLoss, PointStretchLoss, SmapeLoss, NormalLoss and
SimplePointRepulsionLoss (:73-163, :310-398) over pytorch_points_amd.knn_edges, and the mesh edge losses
MeshEdgeLengthLoss, MeshStretchLoss and SimpleMeshRepulsionLoss (:166-308) over pytorch_points_amd.mesh_edges, and
the mesh Laplacian losses UniformLaplacianSmoothnessLoss and MeshLaplacianLoss (:8-71) over
pytorch_points_amd.mesh_laplacian, and MeshNormalLoss over pytorch_points_amd.mesh_normals.

``nndistance`` / ``labeled_nndistance`` are the C++ autograd nodes of csrc/torch_bridge.cpp (the reference's
host side is a C++ extension too): at config 2 the step's kernels take less time than Python needs to issue
them through ``torch.autograd.Function``, and the autograd engine has to take the GIL on its device thread for
a Python backward.  The Python classes below are the same operators over the same C ABI (the reference's class
names; ``NmDistanceFunction.apply`` works as in the reference) and are tested to agree bit for bit."""
import torch

from .. import _lib
from .. import knn_edges as _knn_edges
from .. import mesh_dihedral as _mesh_dihedral
from .. import mesh_edges as _mesh_edges
from .. import mesh_laplacian as _mesh_laplacian
from .. import mesh_normals as _mesh_normals
from ..mesh_distance import PointMeshDistanceLoss  # noqa: F401 (no counterpart in the reference)
from ..mesh_sample import SampledMeshChamferLoss  # noqa: F401  (no counterpart in the reference)
from ..mesh_winding import MeshEnclosureLoss  # noqa: F401  (no counterpart in the reference)
from .. import ops
from .._ext import losses


def _inputs(xyz1, xyz2, double_ok=False):
    """contiguous fp32 (double_ok: or fp64) GPU clouds (B,N,C), (B,M,C) on one device -> (xyz1, xyz2, B, N, M, C,
    device); the checks the reference leaves out (its launcher validates nothing, _ext/nmdistance.cpp:13-15)"""
    assert xyz1.dtype == xyz2.dtype
    xyz1, xyz2 = xyz1.contiguous(), xyz2.contiguous()
    if xyz1.dtype is torch.bfloat16:
        raise TypeError("xyz1 is %s: the Chamfer operators serve float32, float64 and float16 (the reference's "
                        "AT_DISPATCH_FLOATING_TYPES_AND_HALF)" % xyz1.dtype)
    if xyz1.dtype is not torch.float32 and not (double_ok and xyz1.dtype in (torch.float64, torch.float16)):
        if xyz1.dtype in (torch.float64, torch.float16):
            raise TypeError("xyz1 is %s: this operator serves float32 only" % xyz1.dtype)
        raise RuntimeError("xyz1 must be a float tensor")
    if not (xyz1.is_cuda and xyz2.is_cuda):
        raise RuntimeError("%s must be a CUDA tensor" % ("xyz2" if xyz1.is_cuda else "xyz1"))
    dev = xyz1.device
    if xyz2.device != dev:
        raise RuntimeError("xyz2 is on %s, expected %s" % (xyz2.device, dev))
    b, n, m, c = losses._shapes(xyz1, xyz2)
    return xyz1, xyz2, b, n, m, c, dev


def _outputs(b, n, m, dev, dtype=torch.float32):
    """(dist1 (B,N), dist2 (B,M), idx1, idx2) uninitialised, on the inputs' device.  The kernels write
    every element (and zero-fill by themselves when one cloud is empty, the only case in which the
    reference's zero initialisation survives), so no fill launches are spent.  The reference allocates on
    the CPU and moves to the *current* device (:412-421)."""
    return (torch.empty((b, n), dtype=dtype, device=dev), torch.empty((b, m), dtype=dtype, device=dev),
            torch.empty((b, n), dtype=torch.int32, device=dev), torch.empty((b, m), dtype=torch.int32, device=dev))


def _finish_forward(ctx, xyz1, xyz2, dist1, dist2, idx1, idx2):
    ctx.save_for_backward(xyz1, xyz2, idx1, idx2)
    ctx.mark_non_differentiable(idx1, idx2)
    ctx.set_materialize_grads(False)   # no zero tensors for the two index outputs on every backward
    return dist1, dist2, idx1, idx2


def _chamfer_backward(ctx, grad1, grad2):
    """d dist1[i] / d xyz1[i] = 2 (xyz1[i] - xyz2[idx1[i]]) and the mirrored terms (reference kernel
    nmdistance_cuda.cu:168-185); a missing upstream gradient counts as zero."""
    xyz1, xyz2, idx1, idx2 = ctx.saved_tensors
    grad1 = xyz1.new_zeros(idx1.shape) if grad1 is None else grad1.contiguous()
    grad2 = xyz2.new_zeros(idx2.shape) if grad2 is None else grad2.contiguous()
    if grad1.dtype is not xyz1.dtype or grad2.dtype is not xyz1.dtype:
        raise RuntimeError("graddist1 must be a %s tensor" % {torch.float64: "double", torch.float16: "half"}.get(xyz1.dtype, "float"))
    dev = xyz1.device
    if grad1.device != dev or grad2.device != dev:
        raise RuntimeError("graddist is on another device than xyz1 (%s)" % (dev,))
    out1, out2 = torch.empty_like(xyz1), torch.empty_like(xyz2)      # fully overwritten by the kernel
    b, n, c = xyz1.shape
    if xyz1.dtype is not torch.float32:
        losses._launch_f64("pp_nmdistance_backward_" + losses._SUFFIX[xyz1.dtype], "nmdistance_backward", dev,
                           xyz1, xyz2, grad1, grad2, idx1, idx2, out1, out2, b, n, xyz2.shape[1], c)
    else:
        losses._launch_backward(xyz1, xyz2, out1, out2, grad1, grad2, idx1, idx2, b, n, xyz2.shape[1], c, dev)
    return out1, out2


class NmDistanceFunction(torch.autograd.Function):
    """``nndistance(xyz1 (B,N,C), xyz2 (B,M,C))`` -> ``(dist1 (B,N), dist2 (B,M), idx1, idx2)``: squared
    distance from every point to its nearest neighbour in the other cloud, and that neighbour's int32 index
    (not differentiable).  Reference :401-439."""

    @staticmethod
    def forward(ctx, xyz1, xyz2):
        xyz1, xyz2, b, n, m, c, dev = _inputs(xyz1, xyz2, double_ok=True)
        out = _outputs(b, n, m, dev, xyz1.dtype)
        if xyz1.dtype is not torch.float32:   # the reference's scalar_t = double / at::Half instantiations (nmdistance_cuda.cu:125)
            losses._launch_f64("pp_nmdistance_forward_" + losses._SUFFIX[xyz1.dtype], "nmdistance_forward", dev,
                               xyz1, xyz2, out[0], out[2], out[1], out[3], b, n, m, c)
        else:
            losses._launch_forward(xyz1, xyz2, *out, b, n, m, c, dev)
        return _finish_forward(ctx, xyz1, xyz2, *out)

    @staticmethod
    def backward(ctx, graddist1, graddist2, *index_grads):
        return _chamfer_backward(ctx, graddist1, graddist2)


def nndistance(xyz1, xyz2):
    """``nndistance(xyz1 (B,N,C), xyz2 (B,M,C))`` -> ``(dist1 (B,N), dist2 (B,M), idx1, idx2)`` (reference :442:
    ``nndistance = NmDistanceFunction.apply``), through the native autograd node.  fp32 is the tuned path; double
    and half clouds (the reference dispatches over the floating types and half, _ext/nmdistance_cuda.cu:125) go through
    the Python node to every-pair kernels with the reference's arithmetic for the type; bfloat16 raises TypeError."""
    if xyz1.dtype is not torch.float32 and xyz1.dtype in (torch.float64, torch.float16, torch.bfloat16):
        return NmDistanceFunction.apply(xyz1, xyz2)
    return _lib.bridge().nndistance(xyz1, xyz2)


class LabeledNmdistanceFunction(torch.autograd.Function):
    """``labeled_nndistance(xyz1, xyz2, label1 (B,N), label2 (B,M))``: nearest neighbour among the points
    of the other cloud that carry the same label; a point without such a partner gets idx -1, dist 0
    (reference :445-481).  The inputs are made contiguous here (the reference omits it);
    labels are compared in the coordinates' dtype, as the reference's kernel does."""

    @staticmethod
    def forward(ctx, xyz1, xyz2, label1, label2):
        xyz1, xyz2, b, n, m, c, dev = _inputs(xyz1, xyz2)
        out = _outputs(b, n, m, dev)
        losses.labeled_nmdistance_forward(xyz1, xyz2, label1.to(xyz1.dtype), label2.to(xyz1.dtype), *out)
        return _finish_forward(ctx, xyz1, xyz2, *out)

    @staticmethod
    def backward(ctx, graddist1, graddist2, *index_grads):
        return _chamfer_backward(ctx, graddist1, graddist2) + (None, None)


def labeled_nndistance(xyz1, xyz2, label1, label2):
    """``labeled_nndistance(xyz1, xyz2, label1 (B,N), label2 (B,M))`` (reference :483), through the native
    autograd node."""
    return _lib.bridge().labeled_nndistance(xyz1, xyz2, label1, label2)


# ------------------------------------------------------------------------------------- point-cloud regularisers
# The reference's modules with its constructor and forward signatures, reductions and constants.  Graphs come from
# ops.knn_points (a search for nn_size + 1 whose first column, the point itself, is dropped); edges and Laplacians
# from pytorch_points_amd.knn_edges, which never makes the (B,N,K,D) gather.  INTEGRATION.md lists the three places
# where the reference's text cannot run and what is done instead.
def _self_graph(points, nn_size):
    assert(nn_size < points.shape[1])
    return ops.knn_points(points, points, K=nn_size + 1).idx[:, :, 1:]


class PointLaplacianLoss(torch.nn.Module):
    """``metric`` between the uniform Laplacians of two clouds in correspondence (reference :73-101): ``point2`` uses
    the connectivity of ``point1``, or, with ``idx12`` (B,N), is gathered by it and searched on its own."""

    def __init__(self, nn_size, metric, use_norm=False):
        super().__init__()
        self.metric = metric
        self.nn_size = nn_size
        self.use_norm = use_norm

    def forward(self, point1, point2, idx12=None, *args, **kwargs):
        from . import geo_operations as geo_op
        lap1, knn_idx = geo_op.pointUniformLaplacian(point1, nn_size=self.nn_size)
        if idx12 is not None:
            point2 = torch.gather(point2, 1, idx12.unsqueeze(-1).expand(-1, -1, point2.shape[-1]))
            lap2, _ = geo_op.pointUniformLaplacian(point2, nn_size=self.nn_size)
        else:
            assert(point2.shape[1] == point1.shape[1])
            lap2, _ = geo_op.pointUniformLaplacian(point2, knn_idx=knn_idx)
        if self.use_norm:
            lap1 = torch.norm(lap1, dim=-1, p=2)
            lap2 = torch.norm(lap2, dim=-1, p=2)
        return self.metric(lap1, lap2)


class PointEdgeLengthLoss(torch.nn.Module):
    """``metric`` between the k-NN edge lengths of ``points_ref`` and the lengths of the same edges in ``points``
    (reference :104-129)."""

    def __init__(self, nn_size, metric):
        super().__init__()
        self.metric = metric
        self.nn_size = nn_size

    def forward(self, points_ref, points):
        knn_idx = _self_graph(points_ref, self.nn_size)
        dist_ref = _knn_edges.knn_edge_lengths(points_ref, knn_idx)
        dist = _knn_edges.knn_edge_lengths(points, knn_idx)
        return self.metric(dist_ref, dist)


class PointStretchLoss(torch.nn.Module):
    """Stretch only: ``max(d / (d_ref + 1e-10) - 1, 0)`` over the k-NN edges of ``points_ref`` (reference :132-163)."""

    def __init__(self, nn_size, reduction="mean"):
        super().__init__()
        self.nn_size = nn_size
        self.reduction = reduction

    def forward(self, points_ref, points):
        knn_idx = _self_graph(points_ref, self.nn_size)
        dist_ref = _knn_edges.knn_edge_lengths(points_ref, knn_idx)
        dist = _knn_edges.knn_edge_lengths(points, knn_idx)
        stretch = torch.max(dist / (dist_ref + 1e-10) - 1, torch.zeros_like(dist))
        if self.reduction == "mean":
            return torch.mean(stretch)
        elif self.reduction == "sum":
            return torch.mean(torch.sum(stretch, dim=-1))
        elif self.reduction == "none":
            return stretch
        elif self.reduction == "max":
            return torch.mean(torch.max(stretch, dim=-1)[0])
        else:
            raise NotImplementedError


class SmapeLoss(torch.nn.Module):
    """Relative L1 norm ``mean(|x - y| / (|x| + |y| + epsilon))`` (reference :310-324)."""

    def __init__(self, epsilon=1e-8):
        super(SmapeLoss, self).__init__()
        self.epsilon = epsilon

    def forward(self, x, y):
        return torch.mean(torch.abs(x - y) / (torch.abs(x) + torch.abs(y) + self.epsilon))


class NormalLoss(torch.nn.Module):
    """``1 - cos`` between the PCA normals of ``gt`` and ``pred`` (B,N,3) in correspondence (reference :326-358):
    ``pred`` uses the neighbourhoods of ``gt``, or, with ``idx12`` (B,N), is gathered by it and searched on its own.
    ``reduction="mean"`` is ``loss.mean()`` (the reference's ``loss.mean(loss)`` cannot run)."""

    def __init__(self, nn_size=10, reduction="mean"):
        super().__init__()
        self.nn_size = nn_size
        self.reduction = reduction
        self.cos = torch.nn.CosineSimilarity(dim=-1, eps=1e-08)

    def forward(self, gt, pred, idx12=None):
        from . import geo_operations as geo_op
        gt_normals, idx = geo_op.batch_normals(gt, nn_size=self.nn_size, NCHW=False)
        if idx12 is not None:
            pred = torch.gather(pred, 1, idx12.unsqueeze(-1).expand(-1, -1, 3))
            pred_normals, _ = geo_op.batch_normals(pred, nn_size=self.nn_size, NCHW=False)
        else:
            pred_normals, _ = geo_op.batch_normals(pred, nn_size=self.nn_size, NCHW=False, idx=idx)
        loss = 1 - self.cos(pred_normals, gt_normals)
        if self.reduction == "mean":
            return loss.mean()
        elif self.reduction == "max":
            return (torch.max(loss, dim=-1)[0]).mean()
        elif self.reduction == "sum":
            return torch.sum(loss, dim=-1).mean()
        elif self.reduction == "none":
            return loss


class SimplePointRepulsionLoss(torch.nn.Module):
    """``1 / sqrt(d^2 + 1e-4)`` over the k-NN edges shorter than ``radius`` (reference :362-398).  Without ``knn_idx``
    the graph is searched here and the neighbours are detached, as in the reference; a supplied ``knn_idx`` (B,N,K)
    passes gradients to both ends.  ``reduction="sum"`` is ``torch.sum(loss, -1).mean()`` (the reference's
    ``loss.mean(torch.sum(...))`` cannot run)."""

    def __init__(self, nn_size, radius, reduction="mean"):
        super().__init__()
        self.nn_size = nn_size
        self.reduction = reduction
        self.radius2 = radius * radius

    def forward(self, points, knn_idx=None):
        if knn_idx is None:
            knn_idx = _self_graph(points, self.nn_size)
            distance2 = _knn_edges.knn_edge_lengths(points, knn_idx, squared=True, detach_neighbors=True)
        else:
            distance2 = _knn_edges.knn_edge_lengths(points, knn_idx, squared=True)
        loss = 1 / torch.sqrt(distance2 + 1e-4)
        loss = torch.where(distance2 < self.radius2, loss, torch.zeros_like(loss))
        if self.reduction == "mean":
            return loss.mean()
        elif self.reduction == "max":
            return torch.mean(torch.max(loss, dim=-1)[0])
        elif self.reduction == "sum":
            return torch.sum(loss, dim=-1).mean()
        elif self.reduction == "none":
            return loss
        else:
            raise NotImplementedError


# ------------------------------------------------------------------------------------------- mesh edge losses
# The reference's modules (:166-308) with its constructor and forward signatures, reductions and constants.  All three
# work on SQUARED edge lengths (geo_operations.get_edge_lengths returns squares).  The unique edges come from
# pytorch_points_amd.mesh_edges.MeshEdges -- one build with one host read for the whole batch, where the reference
# loops over the batch with a torch.unique each -- and the lengths of every batch element from one launch.
def _get_ev(faces, n_vertices):
    """a list of B ``(E_b,2)`` int64 tensors: the unique edges of every batch element of ``faces`` (B,F,3)"""
    topo = _mesh_edges.MeshEdges.from_faces(faces, n_vertices)
    return [topo.edge_list(b) for b in range(faces.shape[0])]


def _edge_mask(topo, like):
    """``(valid (Bt,Ecap) bool, count (Bt,1) in the dtype of ``like``)``, from the device counts: no host read"""
    count = topo.counts[:, None]
    valid = torch.arange(topo.capacity, device=like.device)[None, :] < count
    return valid, count.to(like.dtype)


def _reduce_edges(values, topo, reduction):
    """The reference's per-element reduction of ``values`` (B,Ecap) over each element's own edges, then over the
    batch, as batched operations: padding rows count as 0 and a mean divides by ``count[b]``."""
    if reduction not in ("mean", "none", "max", "sum"):
        raise NotImplementedError
    valid, count = _edge_mask(topo, values)
    values = torch.where(valid, values, torch.zeros_like(values))
    if reduction == "max":
        per = torch.max(values, dim=-1)[0]
    elif reduction == "sum":
        per = torch.sum(values, dim=-1)
    else:
        per = torch.sum(values, dim=-1) / count[:, 0]
    return per if reduction == "none" else per.mean()


class _MeshTopologyLoss(torch.nn.Module):
    """the topology handling the two face-based losses share: ``self.E`` is the ``MeshEdges`` of the last build; it
    is kept, and never checked against later faces, while ``consistent_topology`` is set (reference :195-197)"""

    def __init__(self, consistent_topology):
        super().__init__()
        self.E = None
        self.consistent_topology = consistent_topology

    @staticmethod
    def getEV(faces, n_vertices):
        """return a list of B (E, 2) int64 tensor"""
        return _get_ev(faces, n_vertices)

    def _topology(self, vert1, vert2, face):
        assert(vert1.shape == vert2.shape)
        if (not self.consistent_topology) or (self.E is None):
            assert(face is not None), "Face is required"
            self.E = _mesh_edges.MeshEdges.from_faces(face, vert1.shape[1])
        return self.E


class MeshEdgeLengthLoss(_MeshTopologyLoss):
    """Mean over the batch of ``metric(sq1[b], sq2[b])`` between the squared edge lengths of two meshes of one
    topology, ``vert1`` and ``vert2`` (B,N,3) with ``face`` (B,F,3) (reference :166-209).  ``metric`` is any callable,
    so it is called once per batch element on views of the two ``(B,Ecap)`` length tensors."""

    def __init__(self, metric, consistent_topology=False):
        super().__init__(consistent_topology)
        self.metric = metric

    def forward(self, vert1, vert2, face=None):
        topo = self._topology(vert1, vert2, face)
        sq1 = _mesh_edges.mesh_edge_sqrlen(vert1, topo)
        sq2 = _mesh_edges.mesh_edge_sqrlen(vert2, topo)
        loss = [self.metric(sq1[b, :topo.count(b)], sq2[b, :topo.count(b)]) for b in range(vert1.shape[0])]
        return torch.mean(torch.stack(loss, dim=0))


class MeshStretchLoss(_MeshTopologyLoss):
    """Stretch only: ``max(sq2 / sq1 - 1, 0)`` on the SQUARED edge lengths of ``vert2`` over those of the reference
    ``vert1``, no epsilon (reference :212-266): a zero-length reference edge gives inf or NaN as the division does.
    Per batch element ``mean`` / ``max`` / ``sum``, then the mean over the batch; ``"none"``: the (B,) means."""

    def __init__(self, reduction="mean", consistent_topology=False):
        super().__init__(consistent_topology)
        self.reduction = reduction

    def forward(self, vert1, vert2, face=None):
        if self.reduction not in ("mean", "none", "max", "sum"):
            raise NotImplementedError
        topo = self._topology(vert1, vert2, face)
        sq1 = _mesh_edges.mesh_edge_sqrlen(vert1, topo)
        sq2 = _mesh_edges.mesh_edge_sqrlen(vert2, topo)
        # a padding row divides by 1, not by its own 0: its quotient is masked below, but its NaN gradient would not be
        valid, _ = _edge_mask(topo, sq1)
        sq1 = torch.where(valid, sq1, torch.ones_like(sq1))
        stretch = torch.max(sq2 / sq1 - 1, torch.zeros_like(sq1))
        return _reduce_edges(stretch, topo, self.reduction)


class SimpleMeshRepulsionLoss(torch.nn.Module):
    """``1 / (sq + 1e-6)`` over the edges whose SQUARED length ``sq`` is below ``threshold ** 2`` (reference :269-308:
    the square goes into the comparison and into the reciprocal).  ``edges`` (E,2), shared by the batch; the argument
    of ``forward`` overrides the constructor's.  Reductions as in MeshStretchLoss.  The ``MeshEdges`` of an edge
    tensor is kept for as long as the same tensor, unmodified, comes back.  ``consistent_topology`` is accepted and,
    as in the reference, unused."""

    def __init__(self, threshold, edges=None, reduction="mean", consistent_topology=False):
        super().__init__()
        self.threshold2 = threshold * threshold
        self.edges = edges
        self.reduction = reduction
        self._built = None   # (edge tensor, its _version, n_vertices, MeshEdges)

    def _topology(self, edges, n_vertices):
        built = self._built
        if built is None or built[0] is not edges or built[1] != edges._version or built[2] != n_vertices:
            built = (edges, edges._version, n_vertices, _mesh_edges.MeshEdges.from_edges(edges, n_vertices))
            self._built = built
        return built[3]

    def forward(self, verts, edges=None):
        if self.reduction not in ("mean", "none", "max", "sum"):
            raise NotImplementedError
        if edges is None:
            edges = self.edges
        assert(edges is not None)
        topo = self._topology(edges, verts.shape[1])
        sq = _mesh_edges.mesh_edge_sqrlen(verts, topo)
        tmp = 1 / (sq + 1e-6)
        tmp = torch.where(sq < self.threshold2, tmp, torch.zeros_like(tmp))
        return _reduce_edges(tmp, topo, self.reduction)


class MeshDihedralAngleLoss(torch.nn.Module):
    """A bending / fold-over penalty on the face-to-face angles of a triangle mesh
    (``pytorch_points_amd.mesh_dihedral.mesh_dihedral_angle``: ``pi`` less the angle between the two face normals at
    an edge, the interior angle of a consistently oriented mesh: a flat edge is near ``pi``, a sharp fold near 0).
    The reference has no such module; the signature follows its mesh losses.  ``vert1`` (B,N,3), ``face`` (B,F,3):

    * with ``vert2`` (B,N,3): ``(angle(vert1) - angle(vert2)) ** 2`` per edge;
    * without: ``relu(threshold - angle(vert1)) ** 2``, which penalises the edges folded below ``threshold``.

    Boundary edges have a constant angle and no gradient.  Per batch element ``mean`` / ``max`` / ``sum`` over its own
    edges, then the mean over the batch; ``"none"``: the (B,) means.  ``self.E`` is the ``MeshEdgePoints`` of the last
    build; it is kept, and never checked against later faces, while ``consistent_topology`` is set."""

    def __init__(self, threshold=None, reduction="mean", consistent_topology=False):
        super().__init__()
        self.threshold = threshold
        self.reduction = reduction
        self.consistent_topology = consistent_topology
        self.E = None

    def forward(self, vert1, vert2=None, face=None):
        if self.reduction not in ("mean", "none", "max", "sum"):
            raise NotImplementedError
        if (not self.consistent_topology) or (self.E is None):
            assert(face is not None), "Face is required"
            self.E = _mesh_dihedral.MeshEdgePoints.from_faces(face, vert1.shape[1])
        topo = self.E
        angle1 = _mesh_dihedral.mesh_dihedral_angle(vert1, topo)
        if vert2 is not None:
            assert(vert1.shape == vert2.shape)
            diff = angle1 - _mesh_dihedral.mesh_dihedral_angle(vert2, topo)
        else:
            assert(self.threshold is not None), "threshold is required without vert2"
            diff = torch.relu(self.threshold - angle1)
        return _reduce_edges(diff * diff, topo, self.reduction)


class MeshNormalLoss(torch.nn.Module):
    """``metric`` between the normals of two meshes of one connectivity, ``vert1`` and ``vert2`` (B,N,3) over ``face``
    (B,F,3) or a shared (F,3): the unit vertex normals (B,N,3) of ``pytorch_points_amd.mesh_normals
    .mesh_vertex_normals`` with ``weighting`` "area" or "uniform", or with ``use_face`` the unit face normals (B,F,3)
    of ``mesh_face_normals``.  The reference has no such module; the signature follows its mesh losses.  ``metric`` is
    any callable of two tensors (``torch.nn.MSELoss()``, a cosine loss).  ``self.E`` is the ``MeshCorners`` of the last
    build; it is kept, and never checked against later faces, while ``consistent_topology`` is set."""

    def __init__(self, metric, use_face=False, weighting="area", consistent_topology=False):
        super().__init__()
        self.metric = metric
        self.use_face = use_face
        self.weighting = weighting
        self.consistent_topology = consistent_topology
        self.E = None

    def _normals(self, vert):
        if self.use_face:
            return _mesh_normals.mesh_face_normals(vert, self.E)[0]
        return _mesh_normals.mesh_vertex_normals(vert, self.E, self.weighting)

    def forward(self, vert1, vert2, face=None):
        assert(vert1.shape == vert2.shape)
        if (not self.consistent_topology) or (self.E is None):
            assert(face is not None), "Face is required"
            self.E = _mesh_laplacian.MeshCorners.from_faces(face.to(vert1.device), vert1.shape[1])
        return self.metric(self._normals(vert1), self._normals(vert2))


# ---------------------------------------------------------------------------------------- mesh Laplacian losses
# The reference's modules (:8-71) with their control flow as written, quirks included (DESIGN.md "Mesh Laplacians"
# lists them).  The Laplacians are geo_operations.UniformLaplacian / CotLaplacian: a topology object built with one
# host read, then one launch per apply.
class UniformLaplacianSmoothnessLoss(torch.nn.Module):
    """Encourages minimal mean curvature shapes (reference :8-27): the norm (B,N) of the uniform Laplacian of ``vert``
    over the constructor's ``faces``.  With ``vert_ref`` the reference curvature is computed from ``vert`` again, as in
    the reference, so the result is ``metric(curve, curve)``.  ``num_point`` is unused there too.  The topology is
    built by the first call and kept."""

    def __init__(self, num_point, faces, metric):
        super().__init__()
        from . import geo_operations as geo_op
        self.laplacian = geo_op.UniformLaplacian()
        self.metric = metric
        self.faces = faces

    def forward(self, vert, vert_ref=None):
        lap = self.laplacian(vert, self.faces)
        curve = torch.norm(lap, p=2, dim=-1)
        if vert_ref is not None:
            lap_ref = self.laplacian(vert, self.faces)
            curve_gt = torch.norm(lap_ref, p=2, dim=-1)
            loss = self.metric(curve, curve_gt)
        else:
            loss = curve
        return loss


class MeshLaplacianLoss(torch.nn.Module):
    """``metric`` between the Laplacians of two meshes of one connectivity in correspondence (reference :29-71).
    ``use_cot``: the cotangent Laplacian instead of the uniform one; ``use_norm``: compare the norms (B,N);
    ``consistent_topology``: keep the Laplacian of the first call (and then no call after it touches the host);
    ``precompute_L``: keep the first call's ``lap1`` in ``self.L``.  Without ``consistent_topology`` the Laplacian is
    rebuilt at the start of every call, so a call's cotangent weights come from ``vert1`` and serve ``vert2`` as well
    -- or come from ``vert2`` when ``lap1`` is the kept one.  ``vert2=None`` returns ``lap1.mean()``; the reference's
    ``assert(~self.precompute_L)`` there never fires (``~True`` is -2) and is not kept."""

    def __init__(self, metric, use_cot=False, use_norm=False, consistent_topology=False, precompute_L=False):
        super().__init__()
        from . import geo_operations as geo_op
        if use_cot:
            self.laplacian = geo_op.CotLaplacian()
        else:
            self.laplacian = geo_op.UniformLaplacian()
        self.use_norm = use_norm
        self.consistent_topology = consistent_topology
        self.metric = metric
        self.precompute_L = precompute_L
        self.L = None

    def forward(self, vert1, vert2=None, face=None):
        if not self.consistent_topology:
            self.laplacian.L = None

        if self.L is None or (not self.precompute_L):
            lap1 = self.laplacian(vert1, face)
            if self.use_norm:
                lap1 = torch.norm(lap1, dim=-1, p=2)
            if self.precompute_L:
                self.L = lap1
        else:
            lap1 = self.L

        if vert2 is not None:
            lap2 = self.laplacian(vert2, face)
            if self.use_norm:
                lap2 = torch.norm(lap2, dim=-1, p=2)
            return self.metric(lap1, lap2)
        else:
            return lap1.mean()


class EarthMoverLoss(torch.nn.Module):
    """``emd_distance(xyz1, xyz2) / max(N,M)``, the cost of the approximate matching per unit of mass, reduced over the
    batch by ``"mean"``, ``"sum"`` or ``"none"`` (no counterpart in the reference)."""

    def __init__(self, reduction="mean"):
        super().__init__()
        if reduction not in ("mean", "sum", "none"):
            raise ValueError("EarthMoverLoss: reduction must be 'mean', 'sum' or 'none', got %r" % (reduction,))
        self.reduction = reduction

    def forward(self, xyz1, xyz2):
        from .. import emd as _emd
        per_cloud = _emd.emd_distance(xyz1, xyz2) / max(xyz1.shape[1], xyz2.shape[1], 1)
        if self.reduction == "mean":
            return per_cloud.mean()
        if self.reduction == "sum":
            return per_cloud.sum()
        return per_cloud
