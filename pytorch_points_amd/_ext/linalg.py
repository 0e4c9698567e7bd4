"""``pytorch_points._ext.linalg`` (reference: torch_batch_svd.cpp, bound at pytorch_points/_ext/linalg.cpp).

Same two names and positional signatures as the pybind module.  The forward runs the batched Jacobi SVD of
csrc/linalg.hip (pp_batch_svd_f32) in place of cuSOLVER's gesvdjBatched; the backward is a composition of torch
operations, as the reference's is a composition of ATen ones.  Precondition failures raise RuntimeError (the
reference's TORCH_CHECK).
"""
import torch

from .. import _lib

_MAX_DIM = 32


def batch_svd_forward(a, is_sort, tol=1e-7, max_sweeps=100, *, return_info=False, full=True):
    """batch_svd_forward (torch_batch_svd.cpp:38-140): a (b, m, n) fp32 on the GPU, m, n <= 32 ->
    ``(U (b,m,m), s (b,min(m,n)), V (b,n,n))`` with ``a = U[:, :, :k] diag(s) V[:, :, :k]^T``; ``s`` descending when
    ``is_sort``.

    Deliberate difference from the reference: it copies gesvdj's per-matrix status to the host, synchronises the device
    and prints a warning for each matrix that did not converge.  Here nothing is synchronised and nothing printed (a
    host round trip in every call would stall the stream, and cannot be captured into a graph: the same reasoning as
    for the launches on the caller's stream).  The status is on the device instead: ``return_info=True``
    also returns the int32 ``info`` (b,): sweeps used, -1 not converged within ``max_sweeps``, -2 a NaN or infinity in
    the matrix (its s, U and V are then NaN).

    Beyond the reference's signature: ``full=False`` returns the thin factors U (b,m,k), V (b,n,k) directly (what
    ``network.operations.batch_svd`` needs) instead of computing full ones to narrow them."""
    dev = _lib.require_cuda(("a", a))
    _lib.require_float(("a", a))
    if a.dim() != 3:
        raise RuntimeError("a must be a 3-D tensor (b, m, n)")
    b, m, n = a.shape
    if not (1 <= m <= _MAX_DIM and 1 <= n <= _MAX_DIM):
        raise RuntimeError("batch_svd_forward: m and n must be in 1..%d, got %d x %d" % (_MAX_DIM, m, n))
    if int(max_sweeps) < 1 or not float(tol) >= 0.0:
        raise RuntimeError("batch_svd_forward: tol must be >= 0 and max_sweeps >= 1")
    a = a.contiguous()
    k = min(m, n)
    u = torch.empty(b, m, m if full else k, dtype=torch.float32, device=dev)
    s = torch.empty(b, k, dtype=torch.float32, device=dev)
    v = torch.empty(b, n, n if full else k, dtype=torch.float32, device=dev)
    info = torch.empty(b, dtype=torch.int32, device=dev) if return_info else None
    with _lib.on_device(dev) as stream:
        _lib.check(_lib.lib().pp_batch_svd_f32(
            _lib.ptr(a), _lib.ptr(u), _lib.ptr(s), _lib.ptr(v), _lib.ptr(info) if info is not None else None,
            b, m, n, 1 if full else 0, 1 if is_sort else 0, float(tol), int(max_sweeps), stream), "batch_svd_forward")
    return (u, s, v, info) if return_info else (u, s, v)


def batch_svd_backward(grads, self, some, compute_uv, raw_u, sigma, raw_v):
    """batch_svd_backward (torch_batch_svd.cpp:150-232): the gradient of ``self`` (b, m, n) = U diag(sigma) V^T
    given ``grads = [gU, gS, gV]`` (an undefined gradient is None), by the standard SVD derivative (J. Townsend,
    "Differentiating the Singular Value Decomposition", 2016).  With k = min(m, n), F_ij = 1 / (s_j^2 - s_i^2) off the
    diagonal and 0 on it:

        gA = U [ (F o (U^T gU - gU^T U)) S + diag(gS) + S (F o (V^T gV - gV^T V)) ] V^T
             + (I - U U^T) gU S^-1 V^T      (m > k)
             + U S^-1 gV^T (I - V V^T)      (n > k)

    Only the first k columns of U and V (and of gU, gV) take part, so full factors are accepted; ``compute_uv=False``
    ignores gU and gV.  Any device and floating dtype."""
    g_u, g_s, g_v = (list(grads) + [None, None, None])[:3]
    if not compute_uv:
        g_u = g_v = None
    m, n = self.shape[-2], self.shape[-1]
    k = sigma.shape[-1]
    u = raw_u[..., :k]
    v = raw_v[..., :k]
    if g_u is not None:
        g_u = g_u[..., :k]
    if g_v is not None:
        g_v = g_v[..., :k]
    if g_u is None and g_s is None and g_v is None:
        return torch.zeros_like(self)
    s = sigma
    vt = v.transpose(-2, -1)
    inner = torch.zeros(s.shape[:-1] + (k, k), dtype=s.dtype, device=s.device)
    if g_s is not None:
        inner = inner + torch.diag_embed(g_s)
    if g_u is not None or g_v is not None:
        s2 = s * s
        f = s2.unsqueeze(-2) - s2.unsqueeze(-1)                       # f[i, j] = s_j^2 - s_i^2
        eye = torch.eye(k, dtype=torch.bool, device=s.device)
        f = torch.where(eye, torch.ones_like(f), f).reciprocal().masked_fill(eye, 0)
        if g_u is not None:
            utgu = u.transpose(-2, -1) @ g_u
            inner = inner + (f * (utgu - utgu.transpose(-2, -1))) * s.unsqueeze(-2)
        if g_v is not None:
            vtgv = vt @ g_v
            inner = inner + s.unsqueeze(-1) * (f * (vtgv - vtgv.transpose(-2, -1)))
    grad = u @ inner @ vt
    if g_u is not None and m > k:
        proj = g_u - u @ (u.transpose(-2, -1) @ g_u)                   # (I - U U^T) gU
        grad = grad + (proj / s.unsqueeze(-2)) @ vt
    if g_v is not None and n > k:
        proj = g_v - v @ (vt @ g_v)                                    # (I - V V^T) gV
        grad = grad + (u / s.unsqueeze(-2)) @ proj.transpose(-2, -1)
    return grad
