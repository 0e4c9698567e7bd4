"""Mean value coordinates of query points with respect to a closed triangle cage (Ju, Schaefer and Warren 2005): the
operator behind ``network.geo_operations.mean_value_coordinates_3D`` (reference geo_operations.py:349-456).

CUDA fp32 and fp64 run the fused HIP kernels of csrc/mvc.hip (``pp_mvc3d_*``): no per-(query, face) tensor is
materialised, the forward keeps only the normalised weights plus a sum and a branch code per query, and the backward
evaluates every pair again.  Every other device or dtype goes through ``composition``, the same contract written as
torch operations.  DESIGN.md "Mean value coordinates" states the contract and its deliberate differences from the
reference.
"""
import ctypes

import torch
import torch.nn.functional as tnf

from . import _lib

PI = 3.1415927          # the reference's constant, in the data's precision
_L_CLAMP = 2.0 - 2e-5   # chord lengths >= 2 are clamped here (straight-through)
_C_CLAMP = 1.0 - 1e-5   # cosines outside (-1, 1) are clamped to +-this (straight-through)
_S_EPS = 1e-5           # |s_i| <= this: the face contributes nothing
_H_EPS = 1e-4           # pi - h < this: the query lies on the face
_D_EPS = 1e-8           # d_j < this: the query is on vertex j

# code bits per query row (csrc/mvc.hip)
SUM_REPLACED, ON_FACE, ON_VERTEX, BAD_INDEX = 1, 2, 4, 8

_NEXT, _PREV = [1, 2, 0], [2, 0, 1]


def _check(query, vertices, faces):
    for name, t in (("query", query), ("vertices", vertices), ("faces", faces)):
        if t.dim() != 3 or t.shape[2] != 3:
            raise RuntimeError("mean_value_coordinates_3D: %s must have shape (B, *, 3), got %s" % (name, tuple(t.shape)))
    if not (query.shape[0] == vertices.shape[0] == faces.shape[0]):
        raise RuntimeError("mean_value_coordinates_3D: query, vertices and faces must have the same batch size, got "
                           "%d, %d and %d" % (query.shape[0], vertices.shape[0], faces.shape[0]))
    if not query.is_floating_point() or vertices.dtype != query.dtype:
        raise RuntimeError("mean_value_coordinates_3D: query and vertices must be floating tensors of one dtype, got "
                           "%s and %s" % (query.dtype, vertices.dtype))
    if faces.is_floating_point() or faces.is_complex() or faces.dtype == torch.bool:
        raise RuntimeError("mean_value_coordinates_3D: faces must be an integer tensor, got %s" % faces.dtype)
    if not (query.device == vertices.device == faces.device):
        raise RuntimeError("mean_value_coordinates_3D: query, vertices and faces must be on one device, got %s, %s "
                           "and %s" % (query.device, vertices.device, faces.device))


def composition(query, vertices, faces, verbose=False):
    """The contract as torch operations, for any device and floating dtype: ``wj`` (B,P,N), and with ``verbose`` also
    ``wi`` (B,P,F,3).  Differentiable; where a branch discards a value, its denominators are made safe before the
    division, so the gradients are finite wherever the kept branch is."""
    _check(query, vertices, faces)
    B, P, _ = query.shape
    N, F = vertices.shape[1], faces.shape[1]
    dt = query.dtype
    fl = faces.long()
    bad = ((fl < 0) | (fl >= N)).reshape(B, -1).any(1)                      # (B,)
    if N == 0 or F == 0:
        link = (query.sum() + vertices.sum()) * 0                             # keeps the outputs on the graph
        wj = query.new_zeros(B, P, N) + link
        wi = query.new_zeros(B, P, F, 3) + link
        nan = torch.full_like(wi, float("nan"))
        wi = torch.where(bad[:, None, None, None], nan, wi)
        return (wj, wi) if verbose else wj
    fl = fl.clamp(0, N - 1)
    u = vertices.unsqueeze(1) - query.unsqueeze(2)                            # (B,P,N,3)
    d = torch.linalg.vector_norm(u, dim=-1)                                   # (B,P,N)
    e = tnf.normalize(u, p=2, dim=-1, eps=1e-12)
    on_vertex = d < _D_EPS
    row_vertex = on_vertex.any(-1)                                            # (B,P)
    idx = fl.reshape(B, 1, F * 3)
    ef = torch.gather(e, 2, idx.unsqueeze(-1).expand(B, P, F * 3, 3)).reshape(B, P, F, 3, 3)
    dfc = torch.gather(d, 2, idx.expand(B, P, F * 3)).reshape(B, P, F, 3)
    chord = torch.linalg.vector_norm(ef[..., _NEXT, :] - ef[..., _PREV, :], dim=-1)   # (B,P,F,3)
    chord = torch.where(chord >= 2, chord - (chord.detach() - _L_CLAMP), chord)
    theta = 2 * torch.asin(chord / 2)
    h = theta.sum(-1, keepdim=True) / 2
    sin_t = torch.sin(theta)
    c = 2 * torch.sin(h) * torch.sin(h - theta) / (sin_t[..., _NEXT] * sin_t[..., _PREV]) - 1
    c = torch.where(c >= 1, c - (c.detach() - _C_CLAMP), c)
    c = torch.where(c <= -1, c - (c.detach() + _C_CLAMP), c)
    low = dt in (torch.float16, torch.bfloat16)                               # no LU in these types
    sign = torch.sign(torch.linalg.det(ef.detach().float() if low else ef.detach())).to(dt)   # (B,P,F); no gradient
    s = sign.unsqueeze(-1) * torch.sqrt(1 - c * c)
    num = theta - c[..., _NEXT] * theta[..., _PREV] - c[..., _PREV] * theta[..., _NEXT]
    den = dfc * sin_t[..., _NEXT] * s[..., _PREV]
    zero_face = (s.abs() <= _S_EPS).any(-1)                                   # (B,P,F)
    inside = (PI - h.squeeze(-1)) < _H_EPS                                    # (B,P,F)
    row_inside = inside.any(-1)                                               # (B,P)
    normal = (~zero_face & ~row_inside.unsqueeze(-1)).unsqueeze(-1)          # (B,P,F,1)
    w_normal = torch.where(normal, num / torch.where(normal, den, torch.ones_like(den)), torch.zeros_like(den))
    w_face = sin_t * dfc[..., _PREV] * dfc[..., _NEXT]
    wi = torch.where(inside.unsqueeze(-1), w_face, w_normal)
    # a row overridden to constants (the query on a vertex) passes no gradient, also not through wi
    wi = torch.where(row_vertex[:, :, None, None], wi.detach(), wi)
    wj = query.new_zeros(B, P, N).scatter_add(2, idx.expand(B, P, F * 3), wi.reshape(B, P, F * 3))
    wj = torch.where(row_vertex.unsqueeze(-1), on_vertex.to(dt), wj)
    total = wj.sum(-1, keepdim=True)
    total = torch.where(total == 0, torch.ones_like(total), total)
    wj = wj / total
    nan = float("nan")
    wj = torch.where(bad[:, None, None], torch.full_like(wj, nan), wj)
    if not verbose:
        return wj
    wi = torch.where(bad[:, None, None, None], torch.full_like(wi, nan), wi)
    return wj, wi


class MeanValueCoordinates3D(torch.autograd.Function):
    """HIP forward and backward (CUDA fp32 / fp64).  Outputs ``wj`` and, with ``verbose``, ``wi``."""

    @staticmethod
    def forward(ctx, query, vertices, faces, verbose):
        dev = _lib.require_cuda(("query", query), ("vertices", vertices), ("faces", faces))
        dt = query.dtype
        B, P, _ = query.shape
        N, F = vertices.shape[1], faces.shape[1]
        query = query.contiguous()
        vertices = vertices.contiguous()
        fl, fsb = _lib.faces_arg(faces, B, F, 3)
        wj = torch.empty(B, P, N, dtype=dt, device=dev)
        sums = torch.empty(B, P, dtype=dt, device=dev)
        codes = torch.empty(B, P, dtype=torch.int32, device=dev)
        wi = torch.empty(B, P, F, 3, dtype=dt, device=dev) if verbose else None
        fn = _lib.lib().pp_mvc3d_forward_f64 if dt == torch.float64 else _lib.lib().pp_mvc3d_forward_f32
        with _lib.on_device(dev) as stream:
            _lib.check(fn(_lib.ptr(query), _lib.ptr(vertices), _lib.ptr(fl), fsb, _lib.ptr(wj), _lib.ptr(sums),
                          _lib.ptr(codes), _lib.ptr(wi) if wi is not None else None, B, P, N, F, stream),
                       "mean_value_coordinates_3D forward")
        ctx.save_for_backward(query, vertices, fl, wj, sums, codes)
        ctx.fsb = fsb
        ctx.mark_non_differentiable(codes)
        return (wj, wi) if verbose else wj

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_wj, grad_wi=None):
        query, vertices, fl, wj, sums, codes = ctx.saved_tensors
        dev, dt = query.device, query.dtype
        B, P, _ = query.shape
        N = vertices.shape[1]
        F = fl.shape[-2]
        grad_wj = grad_wj.contiguous() if grad_wj is not None else torch.zeros_like(wj)
        if grad_wi is not None:
            grad_wi = grad_wi.contiguous()
        gq = torch.empty_like(query)
        gv = torch.empty_like(vertices)
        fn = _lib.lib().pp_mvc3d_backward_f64 if dt == torch.float64 else _lib.lib().pp_mvc3d_backward_f32
        with _lib.on_device(dev) as stream:
            nbytes = _lib.lib().pp_mvc3d_workspace_bytes(B, P, N, query.element_size())
            ws = _lib.workspace(dev, "mvc3d", nbytes)
            _lib.check(fn(_lib.ptr(query), _lib.ptr(vertices), _lib.ptr(fl), ctx.fsb, _lib.ptr(wj), _lib.ptr(sums),
                          _lib.ptr(codes), _lib.ptr(grad_wj), _lib.ptr(grad_wi) if grad_wi is not None else None,
                          _lib.ptr(gq), _lib.ptr(gv), B, P, N, F, _lib.ptr(ws) if ws is not None else None,
                          ctypes.c_size_t(nbytes), stream),
                       "mean_value_coordinates_3D backward")
        return (gq if ctx.needs_input_grad[0] else None), (gv if ctx.needs_input_grad[1] else None), None, None


def mean_value_coordinates_3D(query, vertices, faces, verbose=False):
    """Mean value coordinates ``wj`` (B,P,N) of ``query`` (B,P,3) with respect to the closed triangle cage
    ``vertices`` (B,N,3), ``faces`` (B,F,3) (integer vertex indices; a batch-expanded view of one face list is
    read without a copy).  Rows sum to 1 (a row of zeros stays zero).  ``verbose=True`` returns ``(wj, wi)``, ``wi``
    (B,P,F,3) the per-face weights after the face branches.  Differentiable in ``query`` and ``vertices``.

    CUDA fp32 / fp64: the HIP kernels; anything else: ``composition``.  Nothing synchronises with the host:
    non-finite inputs give NaN rows, and an out-of-range face index gives NaN rows for its batch element."""
    _check(query, vertices, faces)
    if query.is_cuda and query.dtype in (torch.float32, torch.float64):
        return MeanValueCoordinates3D.apply(query, vertices, faces, bool(verbose))
    return composition(query, vertices, faces, verbose)
