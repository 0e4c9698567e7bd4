"""The edge tensor ``[x_i, x_j - x_i]`` of an EdgeConv layer (reference network/layers.py:41-62,88-109), as one operator
over channels-first features:

    knn_edge_features(x (B,C,N), idx (B,P,K) integer, query=None (B,C,P))  ->  (B, 2C, P, K)
        out[b,   c, p, k] = query[b,c,p]
        out[b, C+c, p, k] = x[b,c,idx[b,p,k]] - query[b,c,p]

``query=None`` is the self graph (``query = x``, ``P == N``).  CUDA fp32, fp16 and bf16 run the HIP kernels of
csrc/edge_features.hip (``pp_edge_features_*``): the forward writes every output element once -- no (B,P,K+1,C) gather,
no int64 index expansion, no second pass for the concatenation -- and the backwards are gathers over the reverse
adjacency of ``idx`` with no floating-point atomics (in ascending edge order under
``torch.use_deterministic_algorithms(True)``).  Every other device or dtype goes through ``composition``, the same
contract written as torch operations.  DESIGN.md §4 "Edge features" states the contract.
"""
import ctypes

import torch

from . import _lib

MAX_K = 128   # csrc/edge_features.hip
_DTYPES = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}
_LIMIT = 2 ** 31 - 1


def _check(x, idx, query):
    what = "knn_edge_features"
    if x.dim() != 3:
        raise ValueError("%s: x must have shape (B, C, N), got %s" % (what, tuple(x.shape)))
    if idx.dim() != 3 or idx.shape[0] != x.shape[0]:
        raise ValueError("%s: idx must have shape (B, P, K) with the B of x %s, got %s"
                         % (what, tuple(x.shape), tuple(idx.shape)))
    if query is None:
        if idx.shape[1] != x.shape[2]:
            raise ValueError("%s: the self graph (query=None) needs idx of shape (B, N, K) with the N of x %s, got %s"
                             % (what, tuple(x.shape), tuple(idx.shape)))
    elif query.dim() != 3 or tuple(query.shape) != (x.shape[0], x.shape[1], idx.shape[1]):
        raise ValueError("%s: query must have shape (B, C, P) = %s, got %s"
                         % (what, (x.shape[0], x.shape[1], idx.shape[1]), tuple(query.shape)))
    if idx.shape[2] < 1 or x.shape[1] < 1:
        raise ValueError("%s: K and C must be at least 1, got K = %d, C = %d" % (what, idx.shape[2], x.shape[1]))
    if not x.is_floating_point():
        raise RuntimeError("%s: x must be a floating tensor, got %s" % (what, x.dtype))
    if idx.is_floating_point() or idx.is_complex() or idx.dtype == torch.bool:
        raise RuntimeError("%s: idx must be an integer tensor, got %s" % (what, idx.dtype))
    if idx.device != x.device:
        raise RuntimeError("%s: idx is on %s, expected %s" % (what, idx.device, x.device))
    if query is not None:
        if query.dtype != x.dtype:
            raise RuntimeError("%s: query is %s but x is %s" % (what, query.dtype, x.dtype))
        if query.device != x.device:
            raise RuntimeError("%s: query is on %s, expected %s" % (what, query.device, x.device))


def composition(x, idx, query=None):
    """``knn_edge_features`` as torch operations, for any device and floating dtype."""
    _check(x, idx, query)
    q = x if query is None else query
    c, n = x.shape[1], x.shape[2]
    p, k = idx.shape[1], idx.shape[2]
    il = idx.long()
    bad = (il < 0) | (il >= n)
    bad_row = bad.any(-1)
    il = il.clamp(0, max(n - 1, 0))
    nb = torch.gather(x.unsqueeze(2).expand(-1, -1, p, -1), 3, il.unsqueeze(1).expand(-1, c, -1, -1))
    # a row with an out-of-range index takes no part in the scatter, and its centre's gradient is NaN
    nb = torch.where(bad_row[:, None, :, None], nb.detach(), nb)
    centre = q.unsqueeze(-1).expand(-1, -1, -1, k)
    nan = torch.full_like(q[:1, :1, :1], float("nan"))
    poison = (q * torch.where(bad_row[:, None, :], nan, torch.zeros_like(nan))).unsqueeze(-1)
    diff = torch.where(bad[:, None], poison.expand(-1, -1, -1, k), nb - centre)
    return torch.cat([centre, diff], dim=1)


class KnnEdgeFeatures(torch.autograd.Function):
    """HIP forward and backward (CUDA fp32 / fp16 / bf16, K <= 128).  ``query`` None: the self graph."""

    @staticmethod
    def forward(ctx, x, idx, query):
        named = [("x", x), ("idx", idx)] + ([("query", query)] if query is not None else [])
        dev = _lib.require_cuda(*named)
        x = x.contiguous()
        q = x if query is None else query.contiguous()
        ii = (idx if idx.dtype in (torch.int64, torch.int32) else idx.long()).contiguous()
        b, c, n = x.shape
        p, k = ii.shape[1], ii.shape[2]
        out = torch.empty(b, 2 * c, p, k, dtype=x.dtype, device=dev)
        with _lib.on_device(dev) as stream:
            _lib.check(_lib.lib().pp_edge_features_forward(
                _lib.ptr(x), _lib.ptr(q), _lib.ptr(ii), _lib.ptr(out), b, c, n, p, k, _DTYPES[x.dtype],
                int(ii.dtype == torch.int64), stream), "knn_edge_features forward")
        ctx.save_for_backward(ii)
        ctx.dims = (b, c, n, p, k, x.dtype, query is None)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        (ii,) = ctx.saved_tensors
        b, c, n, p, k, dtype, self_graph = ctx.dims
        need_x = ctx.needs_input_grad[0]
        need_q = (not self_graph) and ctx.needs_input_grad[2]
        if not (need_x or need_q):
            return None, None, None
        dev = ii.device
        grad_out = grad_out.contiguous()
        grad_x = torch.empty(b, c, n, dtype=dtype, device=dev) if need_x else None
        grad_q = torch.empty(b, c, p, dtype=dtype, device=dev) if need_q else None
        with _lib.on_device(dev) as stream:
            nbytes = int(_lib.lib().pp_edge_features_workspace_bytes(b, n, p, k, int(need_x)))
            ws = _lib.workspace(dev, "edge_features", nbytes)
            _lib.check(_lib.lib().pp_edge_features_backward(
                _lib.ptr(ii), _lib.ptr(grad_out), _lib.ptr(grad_x) if need_x else None,
                _lib.ptr(grad_q) if need_q else None, b, c, n, p, k, _DTYPES[dtype], int(ii.dtype == torch.int64),
                int(self_graph), int(_lib.deterministic()), _lib.ptr(ws) if ws is not None else None,
                ctypes.c_size_t(nbytes), stream), "knn_edge_features backward")
        return grad_x, None, grad_q


def _hip_serves(x, idx, query=None):
    """True: the HIP kernels serve this call; False: ``composition`` does.  K beyond the kernels' limit is an error."""
    _check(x, idx, query)
    if idx.shape[2] > MAX_K:
        raise NotImplementedError("knn_edge_features: 1 <= K <= %d, got %d" % (MAX_K, idx.shape[2]))
    b, c, n = x.shape
    p, k = idx.shape[1], idx.shape[2]
    return (x.is_cuda and x.dtype in _DTYPES and min(b, n, p) >= 1
            and max(p * k, b * n, b * p, b * c, b * ((p * k + 255) // 256)) <= _LIMIT and (c + 1) // 2 <= 65535)


def knn_edge_features(x, idx, query=None):
    """Edge features ``(B, 2C, P, K)`` of the graph ``idx`` (B,P,K; integer, as ``knn_points`` returns it -- a strided
    slice such as ``idx[:, :, 1:]`` is fine) over the features ``x`` (B,C,N): channels [0, C) repeat the centre
    ``query[b,c,p]`` along k, channels [C, 2C) hold ``x[b,c,idx[b,p,k]] - query[b,c,p]``.  ``query`` (B,C,P), or None
    for the self graph (``query = x``, ``P == N``).  Differentiable in ``x`` and ``query``.  An index outside [0, N)
    gives NaN differences, a NaN gradient for its centre ``query[b,:,p]``, and its row passes no gradient to ``x``.

    CUDA fp32, fp16 and bf16: the HIP kernels, bit-identical to ``composition`` in the forward; anything else:
    ``composition``.  K > 128 raises NotImplementedError.  Nothing synchronises with the host."""
    if _hip_serves(x, idx, query):
        return KnnEdgeFeatures.apply(x, idx, query)
    return composition(x, idx, query)
