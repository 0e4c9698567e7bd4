"""The two operators on the edges ``points[idx[n,k]] - points[n]`` of a k-NN graph that the reference's point-cloud
regularisers are made of (network/model_loss.py:73-163,362-398, geo_operations.py:128-152):

    knn_edge_lengths(points (B,N,D), idx (B,N,K))  ->  (B,N,K)   the edges' lengths, or their squares
    knn_laplacian(points (B,N,D), idx (B,N,K))     ->  (B,N,D)   -(sum_k points[idx[n,k]]) / K + points[n]

CUDA fp32 with D <= 32 runs the HIP kernels of csrc/knn_edges.hip (``pp_knn_*``): the (B,N,K,D) gather and its int64
index expansion are never materialised, and the backwards are gathers over the reverse adjacency of ``idx`` with no
floating-point atomics (in ascending edge order under ``torch.use_deterministic_algorithms(True)``).  Every other
device, dtype or D goes through the ``composition`` twins, the same contract written as torch operations.  DESIGN.md
"k-NN edge operators" states the contract.
"""
import ctypes

import torch

from . import _lib

MAX_K = 128   # csrc/knn_edges.hip
MAX_D = 32


def _check(what, points, idx):
    if points.dim() != 3:
        raise ValueError("%s: points must have shape (B, N, D), got %s" % (what, tuple(points.shape)))
    if idx.dim() != 3 or tuple(idx.shape[:2]) != tuple(points.shape[:2]):
        raise ValueError("%s: idx must have shape (B, N, K) with the B and N of points %s, got %s"
                         % (what, tuple(points.shape), tuple(idx.shape)))
    if idx.shape[2] < 1 or points.shape[2] < 1:
        raise ValueError("%s: K and D must be at least 1, got K = %d, D = %d" % (what, idx.shape[2], points.shape[2]))
    if not points.is_floating_point():
        raise RuntimeError("%s: points must be a floating tensor, got %s" % (what, points.dtype))
    if idx.is_floating_point() or idx.is_complex() or idx.dtype == torch.bool:
        raise RuntimeError("%s: idx must be an integer tensor, got %s" % (what, idx.dtype))
    if idx.device != points.device:
        raise RuntimeError("%s: idx is on %s, expected %s" % (what, idx.device, points.device))


def _neighbours(points, idx, detach_neighbors=False):
    """``(nb (B,N,K,D), bad (B,N,K), poison (B,N,1))``: the gathered neighbours (indices clamped into range), the
    out-of-range mask, and a NaN per point that carries NaN into the point's gradient wherever it is selected.  The
    neighbours of a row with an out-of-range index are detached: the row takes no part in the scatter."""
    n, d = points.shape[1], points.shape[2]
    il = idx.long()
    bad = (il < 0) | (il >= n)
    il = il.clamp(0, max(n - 1, 0))
    nb = torch.gather(points.unsqueeze(1).expand(-1, n, -1, -1), 2, il.unsqueeze(-1).expand(-1, -1, -1, d))
    if detach_neighbors:
        nb = nb.detach()
    else:
        nb = torch.where(bad.any(-1)[:, :, None, None], nb.detach(), nb)
    nan = torch.full_like(points[:, :, :1], float("nan"))
    poison = points.sum(-1, keepdim=True) * torch.where(bad.any(-1, keepdim=True), nan, torch.zeros_like(nan))
    return nb, bad, poison


def edge_lengths_composition(points, idx, squared=False, detach_neighbors=False):
    """``knn_edge_lengths`` as torch operations, for any device and floating dtype."""
    _check("knn_edge_lengths", points, idx)
    nb, bad, poison = _neighbours(points, idx, detach_neighbors)
    t = nb - points.unsqueeze(2)
    d2 = t[..., 0] * t[..., 0]
    for c in range(1, points.shape[2]):
        d2 = torch.addcmul(d2, t[..., c], t[..., c])
    if squared:
        out = d2
    else:   # torch.norm's subgradient at a zero length: 0
        zero = d2 == 0
        out = torch.where(zero, torch.zeros_like(d2), torch.sqrt(torch.where(zero, torch.ones_like(d2), d2)))
    return torch.where(bad, poison.expand_as(out), out)


def laplacian_composition(points, idx):
    """``knn_laplacian`` as torch operations, for any device and floating dtype."""
    _check("knn_laplacian", points, idx)
    nb, bad, poison = _neighbours(points, idx)
    k = idx.shape[2]
    total = nb[:, :, 0]
    for j in range(1, k):
        total = total + nb[:, :, j]
    # (a tensor divisor: torch multiplies by the reciprocal of a Python scalar on the GPU, which rounds differently)
    lap = -(total / torch.full_like(points[:1, :1, :1], float(k))) + points
    return torch.where(bad.any(-1, keepdim=True), poison.expand_as(lap), lap)


def _workspace(dev, b, n, k):
    nbytes = int(_lib.lib().pp_knn_edges_workspace_bytes(b, n, k))
    ws = _lib.workspace(dev, "knn_edges", nbytes)
    return (_lib.ptr(ws) if ws is not None else None), ctypes.c_size_t(nbytes), ws


class KnnEdgeLengths(torch.autograd.Function):
    """HIP forward and backward (CUDA fp32, D <= 32, K <= 128)."""

    @staticmethod
    def forward(ctx, points, idx, squared, detach_neighbors):
        dev = _lib.require_cuda(("points", points), ("idx", idx))
        points = points.contiguous()
        il = (idx if idx.dtype == torch.int64 else idx.long()).contiguous()
        b, n, d = points.shape
        k = il.shape[2]
        out = torch.empty(b, n, k, dtype=torch.float32, device=dev)
        with _lib.on_device(dev) as stream:
            _lib.check(_lib.lib().pp_knn_edge_lengths_forward_f32(_lib.ptr(points), _lib.ptr(il), _lib.ptr(out), b, n, k,
                                                                  d, int(squared), stream), "knn_edge_lengths forward")
        ctx.save_for_backward(points, il, out)
        ctx.flags = (int(squared), int(detach_neighbors))
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        if not ctx.needs_input_grad[0]:
            return None, None, None, None
        points, il, out = ctx.saved_tensors
        dev = points.device
        b, n, d = points.shape
        k = il.shape[2]
        grad_out = grad_out.contiguous()
        grad = torch.empty_like(points)
        squared, detach = ctx.flags
        with _lib.on_device(dev) as stream:
            wsp, nbytes, ws = (None, ctypes.c_size_t(0), None) if detach else _workspace(dev, b, n, k)
            _lib.check(_lib.lib().pp_knn_edge_lengths_backward_f32(
                _lib.ptr(points), _lib.ptr(il), _lib.ptr(out), _lib.ptr(grad_out), _lib.ptr(grad), b, n, k, d, squared,
                detach, int(_lib.deterministic()), wsp, nbytes, stream), "knn_edge_lengths backward")
        return grad, None, None, None


class KnnLaplacian(torch.autograd.Function):
    """HIP forward and backward (CUDA fp32, D <= 32, K <= 128)."""

    @staticmethod
    def forward(ctx, points, idx):
        dev = _lib.require_cuda(("points", points), ("idx", idx))
        points = points.contiguous()
        il = (idx if idx.dtype == torch.int64 else idx.long()).contiguous()
        b, n, d = points.shape
        k = il.shape[2]
        lap = torch.empty_like(points)
        with _lib.on_device(dev) as stream:
            _lib.check(_lib.lib().pp_knn_laplacian_forward_f32(_lib.ptr(points), _lib.ptr(il), _lib.ptr(lap), b, n, k, d,
                                                               stream), "knn_laplacian forward")
        ctx.save_for_backward(il)
        ctx.dim = d
        return lap

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_lap):
        if not ctx.needs_input_grad[0]:
            return None, None
        (il,) = ctx.saved_tensors
        dev = il.device
        b, n, k = il.shape
        grad_lap = grad_lap.contiguous()
        grad = torch.empty_like(grad_lap)
        with _lib.on_device(dev) as stream:
            wsp, nbytes, ws = _workspace(dev, b, n, k)
            _lib.check(_lib.lib().pp_knn_laplacian_backward_f32(
                _lib.ptr(il), _lib.ptr(grad_lap), _lib.ptr(grad), b, n, k, ctx.dim, int(_lib.deterministic()), wsp,
                nbytes, stream), "knn_laplacian backward")
        return grad, None


def _hip_serves(what, points, idx):
    """True: the HIP kernels serve this call; False: ``composition`` does.  K beyond the kernels' limit is an error."""
    _check(what, points, idx)
    if idx.shape[2] > MAX_K:
        raise NotImplementedError("%s: 1 <= K <= %d, got %d" % (what, MAX_K, idx.shape[2]))
    return (points.is_cuda and points.dtype == torch.float32 and points.shape[2] <= MAX_D
            and points.shape[1] * idx.shape[2] < 2 ** 31 and points.shape[0] * points.shape[1] < 2 ** 31)


def knn_edge_lengths(points, idx, squared=False, detach_neighbors=False):
    """Lengths ``(B,N,K)`` of the edges ``points[b,idx[b,n,k]] - points[b,n]`` of the graph ``idx`` (B,N,K; integer,
    as ``knn_points`` returns it) over ``points`` (B,N,D); ``squared``: their squares, with an ``idx`` from
    ``knn_points`` bit-identical to its ``dists``.  Differentiable in ``points``; a zero length has gradient 0.
    ``detach_neighbors``: only the centre point ``n`` of an edge receives its gradient.  An index outside [0, N) gives
    a NaN length and a NaN gradient for its centre point, and its row passes no gradient to any other point.

    CUDA fp32 with D <= 32: the HIP kernels; anything else: ``edge_lengths_composition``.  K > 128 raises
    NotImplementedError.  Nothing synchronises with the host."""
    if _hip_serves("knn_edge_lengths", points, idx):
        return KnnEdgeLengths.apply(points, idx, bool(squared), bool(detach_neighbors))
    return edge_lengths_composition(points, idx, squared, detach_neighbors)


def knn_laplacian(points, idx):
    """Uniform Laplacian ``(B,N,D)`` of ``points`` (B,N,D) over the graph ``idx`` (B,N,K):
    ``-(sum_k points[b,idx[b,n,k]]) / K + points[b,n]``, the sum in ascending k.  Differentiable in ``points``.  A row
    with an index outside [0, N) is NaN, as is its centre point's gradient; it passes no gradient to any other point.

    CUDA fp32 with D <= 32: the HIP kernels; anything else: ``laplacian_composition``.  K > 128 raises
    NotImplementedError.  Nothing synchronises with the host."""
    if _hip_serves("knn_laplacian", points, idx):
        return KnnLaplacian.apply(points, idx)
    return laplacian_composition(points, idx)
