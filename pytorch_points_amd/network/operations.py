"""``pytorch_points.network.operations`` -- the part on the hot path: gather_points, ball_query,
grouping_operation, QueryAndGroup (reference: network/operations.py:38-213), and batch_svd (:215-258), and the
four vector helpers that callers of mean_value_coordinates import beside it: normalize, sqrNorm, dot_product and
cross_product_2D (:260-275).  channel_shuffle, jitter and the other torch one-liners of that file are out of scope
(SURVEY.md §2.1)."""
import torch

from .._ext import linalg, sampling


class GatherFunction(torch.autograd.Function):
    """``gather_points(features (B,C,N), idx (B,npoint))`` -> ``(B,C,npoint)``: columns of ``features``
    picked by ``idx`` (int32; other integer types are converted, reference operations.py:55); the
    gradient is scattered back to ``features`` (reference :38-82)."""

    @staticmethod
    def forward(ctx, features, idx):
        src = features.contiguous()
        cols = idx.contiguous().to(torch.int32)
        batch, channels, n = src.shape
        picked = cols.shape[1]
        out = src.new_empty((batch, channels, picked))
        sampling.gather_forward(batch, channels, n, picked, src, cols, out)
        ctx.save_for_backward(cols)
        ctx.source_shape = (channels, n)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        (cols,) = ctx.saved_tensors
        channels, n = ctx.source_shape
        batch, picked = cols.shape
        # (the fp32 kernel accumulates; the 16-bit entry points write every element)
        grad_features = (grad_out.new_zeros if grad_out.dtype is torch.float32 else grad_out.new_empty)(
            (batch, channels, n))
        sampling.gather_backward(batch, channels, n, picked, grad_out.contiguous(), cols, grad_features)
        return grad_features, None


gather_points = GatherFunction.apply  # type: ignore


class BallQuery(torch.autograd.Function):
    """``ball_query(radius, nsample, xyz (B,N,3), new_xyz (B,npoint,3))`` -> int32 ``(B,npoint,nsample)``:
    per centre the first ``nsample`` points of ``xyz`` (in index order) closer than ``radius``, padded with
    the first hit.  Argument order as the reference's (operations.py:88-111).  Not differentiable."""

    @staticmethod
    def forward(ctx, radius, nsample, xyz, new_xyz):
        members = sampling.ball_query(new_xyz, xyz, radius, nsample)
        ctx.mark_non_differentiable(members)
        return members

    @staticmethod
    def backward(ctx, *unused):
        return None, None, None, None


ball_query = BallQuery.apply  # type: ignore


class GroupingOperation(torch.autograd.Function):
    """``grouping_operation(features (B,C,N), idx (B,npoint,nsample))`` -> ``(B,C,npoint,nsample)``; the
    gradient is scattered back to ``features`` (reference operations.py:117-156)."""

    @staticmethod
    def forward(ctx, features, idx):
        ctx.save_for_backward(idx)
        ctx.source_points = features.shape[2]
        return sampling.group_points(features, idx)

    @staticmethod
    def backward(ctx, grad_out):
        (idx,) = ctx.saved_tensors
        return sampling.group_points_grad(grad_out.contiguous(), idx, ctx.source_points), None


grouping_operation = GroupingOperation.apply  # type: ignore


class _QueryAndGroupFused(torch.autograd.Function):
    """ball_query -> group(xyz) - centre -> group(features) -> concat as ONE output tensor written
    once.  The reference composes four ops and a torch.cat (operations.py:193-204); at B=32, C=128,
    npoint=4096, nsample=64 the cat alone re-reads and re-writes 4.4 GB.  Values are identical."""

    @staticmethod
    def forward(ctx, xyz, new_xyz, features, radius, nsample, use_xyz):
        xyz = xyz.contiguous()
        new_xyz = new_xyz.contiguous()
        idx = sampling.ball_query(new_xyz, xyz, radius, nsample)
        B, N, _ = xyz.shape
        npoint = new_xyz.shape[1]
        C = features.shape[1] if features is not None else 0
        cx = 3 if use_xyz else 0
        # 16-bit features: alone they are grouped as they are; beside the fp32 relative coordinates the
        # output is fp32, torch.cat's promotion in the reference's composition -- the features are widened once
        fdt = features.dtype if features is not None else torch.float32
        if use_xyz and fdt in (torch.float16, torch.bfloat16):
            features = features.float()
        out = torch.empty(B, cx + C, npoint, nsample, dtype=torch.float32 if use_xyz else fdt, device=xyz.device)
        if use_xyz:
            sampling.group_points_into(xyz.transpose(1, 2).contiguous(), idx, out, 0)
            out[:, :3] -= new_xyz.transpose(1, 2).unsqueeze(-1)
        if features is not None:
            sampling.group_points_into(features.contiguous(), idx, out, cx)
        ctx.for_backwards = (idx, N, C, cx, fdt)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        idx, N, C, cx, fdt = ctx.for_backwards
        grad_out = grad_out.contiguous()
        grad_xyz = grad_new_xyz = grad_features = None
        if cx and ctx.needs_input_grad[0]:
            grad_xyz = sampling.group_points_grad_from(grad_out, idx, N, 0, 3).transpose(1, 2).contiguous()
        if cx and ctx.needs_input_grad[1]:
            grad_new_xyz = -grad_out[:, :3].sum(-1).transpose(1, 2).contiguous()
        if C and ctx.needs_input_grad[2]:
            grad_features = sampling.group_points_grad_from(grad_out, idx, N, cx, C).to(fdt)
        return grad_xyz, grad_new_xyz, grad_features, None, None, None


class QueryAndGroup(torch.nn.Module):
    r"""Groups with a ball query of radius (reference operations.py:162-213).

    forward(xyz (B,N,3), new_xyz (B,npoint,3), features (B,C,N) or None)
    -> (B, 3 + C, npoint, nsample)"""

    def __init__(self, radius, nsample, use_xyz=True):
        super(QueryAndGroup, self).__init__()
        self.radius, self.nsample, self.use_xyz = radius, nsample, use_xyz

    def forward(self, xyz, new_xyz, features=None):
        if features is None:
            assert self.use_xyz, "Cannot have not features and not use xyz as a feature!"
        return _QueryAndGroupFused.apply(xyz, new_xyz, features, self.radius, self.nsample, self.use_xyz)

    def forward_unfused(self, xyz, new_xyz, features=None):
        """The same result composed from the public operators the way the reference does it
        (operations.py:193-204: ball_query, two grouping_operations, a subtraction and a concatenation);
        kept as the yardstick of the parity tests and of ``bench.py --workload ball_group``."""
        if features is None and not self.use_xyz:
            raise AssertionError("Cannot have not features and not use xyz as a feature!")
        members = ball_query(self.radius, self.nsample, xyz, new_xyz)
        parts = []
        if self.use_xyz or features is None:
            local = grouping_operation(xyz.transpose(1, 2).contiguous(), members)
            parts.append(local - new_xyz.transpose(1, 2).unsqueeze(-1))     # relative to the centre
        if features is not None:
            parts.append(grouping_operation(features, members))
        return parts[0] if len(parts) == 1 else torch.cat(parts, dim=1)


class BatchSVDFunction(torch.autograd.Function):
    """Batched SVD of (B, M, N) fp32 matrices, M, N <= 32 (reference operations.py:215-245): ``x = U diag(S) V^T`` with
    the thin U (B,M,k), S (B,k) descending, V (B,N,k), k = min(M, N).  A CPU input runs on the GPU and its outputs
    and gradient come back to the CPU, as in the reference.  The kernel writes the thin factors directly
    (pp_batch_svd_f32 with full = 0) where the reference computes full ones and narrows them."""

    @staticmethod
    def forward(ctx, x):
        ctx.device = x.device
        x = x.cuda()
        U, S, V = linalg.batch_svd_forward(x, True, 1e-7, 100, full=False)
        ctx.save_for_backward(x, U, S, V)
        return U.to(ctx.device), S.to(ctx.device), V.to(ctx.device)

    @staticmethod
    def backward(ctx, grad_u, grad_s, grad_v):
        x, U, S, V = ctx.saved_tensors
        dev = x.device
        grads = [g.to(dev) if g is not None else None for g in (grad_u, grad_s, grad_v)]
        grad_out = linalg.batch_svd_backward(grads, x, True, True, U, S, V)
        return grad_out.to(device=ctx.device)


def batch_svd(x):
    """``U, S, V = batch_svd(x)`` for x (B, M, N), so that x = U diag(S) V^T: U (B,M,k), S (B,k) descending,
    V (B,N,k), k = min(M, N) (reference operations.py:248-258)."""
    assert(x.dim() == 3)
    return BatchSVDFunction.apply(x)


# ------------------------------------------------------------------------------------------- vector helpers
def normalize(tensor, dim=-1):
    """``tensor`` scaled to unit L2 length along ``dim`` (lengths below 1e-12 divide by 1e-12)"""
    return torch.nn.functional.normalize(tensor, p=2.0, dim=dim, eps=1e-12)


def sqrNorm(tensor, dim=-1, keepdim=False):
    """squared L2 length along ``dim``"""
    return (tensor * tensor).sum(dim=dim, keepdim=keepdim)


def dot_product(tensor1, tensor2, dim=-1, keepdim=False):
    """inner product along ``dim``"""
    return (tensor1 * tensor2).sum(dim=dim, keepdim=keepdim)


def cross_product_2D(tensor1, tensor2, dim=1):
    """z component ``x1 y2 - y1 x2`` of the cross product of 2-vectors stored along ``dim``; ``dim`` is dropped"""
    if tensor1.shape[dim] != 2 or tensor2.shape[dim] != 2:
        raise AssertionError("cross_product_2D: both tensors need size 2 along dim %d, got %d and %d"
                             % (dim, tensor1.shape[dim], tensor2.shape[dim]))
    x1, y1 = tensor1.unbind(dim)
    x2, y2 = tensor2.unbind(dim)
    return x1 * y2 - y1 * x2
