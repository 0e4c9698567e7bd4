"""Mean value coordinates of 2-D query points with respect to a closed polygon (Floater 2003): the operator behind
``network.geo_operations.mean_value_coordinates`` (reference geo_operations.py:459-526).

CUDA fp32 and fp64 run the fused HIP kernels of csrc/mvc2d.hip (``pp_mvc2d_*``): no per-(vertex, query) temporary is
materialised, the forward keeps only the normalised weights plus a divisor and a branch code per query, and the
backward evaluates every pair again.  Every other device or dtype goes through ``composition``, the same contract
written as torch operations.  DESIGN.md "Mean value coordinates, 2-D" states the contract and its deliberate
differences from the reference.
"""
import ctypes

import torch

from . import _lib

_A_EPS = 1e-5    # |A_i| <= this: pair i contributes no t_i; with D_i < 0 the query lies on edge i
_V_EPS = 1e-8    # r_i < this: the query is on vertex i
_TINY = 1e-10    # the reference's guard added to every denominator

# code bits per query row (csrc/mvc2d.hip)
ZERO_SUM, ON_EDGE, ON_VERTEX, NON_FINITE = 1, 2, 4, 8


def _check(points, polygon):
    for name, t in (("points", points), ("polygon", polygon)):
        if t.dim() != 3 or t.shape[1] != 2:
            raise RuntimeError("mean_value_coordinates: %s must have shape (B, 2, *), got %s" % (name, tuple(t.shape)))
    if points.shape[0] != polygon.shape[0]:
        raise RuntimeError("mean_value_coordinates: points and polygon must have the same batch size, got %d and %d"
                           % (points.shape[0], polygon.shape[0]))
    if not points.is_floating_point() or polygon.dtype != points.dtype:
        raise RuntimeError("mean_value_coordinates: points and polygon must be floating tensors of one dtype, got "
                           "%s and %s" % (points.dtype, polygon.dtype))
    if points.device != polygon.device:
        raise RuntimeError("mean_value_coordinates: points and polygon must be on one device, got %s and %s"
                           % (points.device, polygon.device))


def _next(t, dim):
    """element i+1 at position i, cyclically"""
    return torch.roll(t, -1, dim)


def _prev(t, dim):
    """element i-1 at position i, cyclically"""
    return torch.roll(t, 1, dim)


def composition(points, polygon, verbose=False):
    """The contract as torch operations, for any device and floating dtype: ``phi`` (B,M,N), and with ``verbose`` also
    ``w`` (B,M,N), the row before the division.  Differentiable; where a branch discards a quotient, its denominator
    is made safe before the division, so no discarded infinity reaches a gradient."""
    _check(points, polygon)
    B, _, N = points.shape
    M = polygon.shape[2]
    if N == 0 or M == 0:
        phi = points.new_zeros(B, M, N) + (points.sum() + polygon.sum()) * 0       # keeps the outputs on the graph
        return (phi, phi.clone()) if verbose else phi
    s = polygon.unsqueeze(3) - points.unsqueeze(2)                                  # (B,2,M,N)
    r = torch.linalg.vector_norm(s, dim=1)                                          # (B,M,N)
    s_next, r_next = _next(s, 2), _next(r, 1)
    area = (s[:, 0] * s_next[:, 1] - s[:, 1] * s_next[:, 0]) / 2
    dot = (s * s_next).sum(1)
    big = area.abs() > _A_EPS
    t = torch.where(big, (r_next * r - dot) / torch.where(big, area + _TINY, torch.ones_like(area)),
                    torch.zeros_like(area))
    w = (_prev(t, 1) + t) / (r + _TINY)
    # the query on an edge
    on_edge = (area.abs() <= _A_EPS) & (dot < 0)
    w = torch.where(on_edge.any(1, keepdim=True), torch.zeros_like(w), w)
    length = torch.linalg.vector_norm(polygon - _next(polygon, 2), dim=1).unsqueeze(-1)      # (B,M,1)
    w = torch.where(on_edge, 1 - r / (length + _TINY), w)
    w = torch.where(_prev(on_edge, 1), 1 - w.sum(1, keepdim=True), w)
    # the query on a vertex
    on_vertex = r < _V_EPS
    w = torch.where(on_vertex.any(1, keepdim=True), torch.zeros_like(w), w)
    w = torch.where(on_vertex, torch.ones_like(w), w)
    # a row with a non-finite difference is NaN
    bad = ~torch.isfinite(s).all(1).all(1, keepdim=True)                             # (B,1,N)
    w = torch.where(bad, torch.full_like(w, float("nan")), w)
    total = w.sum(1, keepdim=True)
    total = torch.where(total == 0, torch.ones_like(total), total)
    phi = w / total
    return (phi, w) if verbose else phi


class MeanValueCoordinates2D(torch.autograd.Function):
    """HIP forward and backward (CUDA fp32 / fp64).  Outputs ``phi`` and, with ``verbose``, ``w``."""

    @staticmethod
    def forward(ctx, points, polygon, verbose):
        dev = _lib.require_cuda(("points", points), ("polygon", polygon))
        dt = points.dtype
        B, _, N = points.shape
        M = polygon.shape[2]
        points = points.contiguous()
        polygon = polygon.contiguous()
        phi = torch.empty(B, M, N, dtype=dt, device=dev)
        sums = torch.empty(B, N, dtype=dt, device=dev)
        codes = torch.empty(B, N, dtype=torch.int32, device=dev)
        w = torch.empty(B, M, N, dtype=dt, device=dev) if verbose else None
        fn = _lib.lib().pp_mvc2d_forward_f64 if dt == torch.float64 else _lib.lib().pp_mvc2d_forward_f32
        with _lib.on_device(dev) as stream:
            _lib.check(fn(_lib.ptr(points), _lib.ptr(polygon), _lib.ptr(phi), _lib.ptr(w) if w is not None else None,
                          _lib.ptr(sums), _lib.ptr(codes), B, N, M, stream), "mean_value_coordinates forward")
        ctx.save_for_backward(points, polygon, phi, sums, codes)
        ctx.mark_non_differentiable(codes)
        return (phi, w) if verbose else phi

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_phi, grad_w=None):
        points, polygon, phi, sums, codes = ctx.saved_tensors
        dev = points.device
        B, _, N = points.shape
        M = polygon.shape[2]
        grad_phi = grad_phi.contiguous() if grad_phi is not None else torch.zeros_like(phi)
        if grad_w is not None:
            grad_w = grad_w.contiguous()
        gpoints = torch.empty_like(points)
        gpolygon = torch.empty_like(polygon)
        fn = _lib.lib().pp_mvc2d_backward_f64 if points.dtype == torch.float64 else _lib.lib().pp_mvc2d_backward_f32
        with _lib.on_device(dev) as stream:
            nbytes = _lib.lib().pp_mvc2d_workspace_bytes(B, N, M, points.element_size())
            ws = _lib.workspace(dev, "mvc2d", nbytes)
            _lib.check(fn(_lib.ptr(points), _lib.ptr(polygon), _lib.ptr(phi), _lib.ptr(sums), _lib.ptr(codes),
                          _lib.ptr(grad_phi), _lib.ptr(grad_w) if grad_w is not None else None, _lib.ptr(gpoints),
                          _lib.ptr(gpolygon), B, N, M, _lib.ptr(ws) if ws is not None else None,
                          ctypes.c_size_t(nbytes), stream), "mean_value_coordinates backward")
        return (gpoints if ctx.needs_input_grad[0] else None), (gpolygon if ctx.needs_input_grad[1] else None), None


def mean_value_coordinates(points, polygon, verbose=False):
    """Mean value coordinates ``phi`` (B,M,N) of ``points`` (B,2,N) with respect to the closed polygon ``polygon``
    (B,2,M), both channel-first, vertices taken cyclically.  Rows (over M) sum to 1 (a row whose weights sum to 0 is
    left undivided).  ``verbose=True`` returns ``(phi, w)``, ``w`` (B,M,N) the weights before the division.
    Differentiable in ``points`` and ``polygon``.

    CUDA fp32 / fp64: the HIP kernels; anything else, and an empty input: ``composition``.  Nothing synchronises with
    the host: a non-finite input gives NaN rows."""
    _check(points, polygon)
    if (points.is_cuda and points.dtype in (torch.float32, torch.float64) and points.shape[2] > 0
            and polygon.shape[2] > 0 and points.shape[0] > 0):
        return MeanValueCoordinates2D.apply(points, polygon, bool(verbose))
    return composition(points, polygon, verbose)
