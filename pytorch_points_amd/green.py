"""Green coordinates of query points with respect to a closed triangle cage (Lipman, Levin and Cohen-Or, "Green
Coordinates", 2008): the operator behind ``network.geo_operations.green_coordinates_3D`` (reference
geo_operations.py:625-773, with its helper ``_gcTriInt``).

CUDA fp32 and fp64 run the fused HIP kernels of csrc/green.hip (``pp_gc3d_*``): no per-(query, face) tensor is
materialised, the forward keeps the normalised vertex coordinates, the face coordinates and a row sum and code per
query, and the backward evaluates every pair again.  Every other device or dtype goes through ``composition``, the
same contract written as torch operations.  DESIGN.md "Green coordinates" states the contract and its deliberate
differences from the reference.
"""
import ctypes
import math

import torch
import torch.nn.functional as tnf

from . import _lib

_EPS = 1e-6             # _gcTriInt: cosines within this of +-1 and C within this of 1 are filtered
_ANGLE_EPS = 1e-3       # _gcTriInt: alpha within this of 0 or pi is filtered
_DIV_GUARD = 1e-12      # _gcTriInt: added to denominators and under square roots
_N_EPS = 1e-7           # |N_l| <= this: the edge plane's normal is left unnormalised and II_l is 0
_OMEGA_EPS = 1e-6       # |omega| < this: the face gives no vertex coordinate
_PHI_GUARD = 1e-10      # added to the denominator of phi and to the row sum

# code bits per query row (csrc/green.hip)
BAD_INDEX = 8

_NEXT = [1, 2, 0]


def _check(query, vertices, faces, face_normals=None):
    for name, t in (("query", query), ("vertices", vertices), ("faces", faces)):
        if t.dim() != 3 or t.shape[2] != 3:
            raise RuntimeError("green_coordinates_3D: %s must have shape (B, *, 3), got %s" % (name, tuple(t.shape)))
    if not (query.shape[0] == vertices.shape[0] == faces.shape[0]):
        raise RuntimeError("green_coordinates_3D: query, vertices and faces must have the same batch size, got "
                           "%d, %d and %d" % (query.shape[0], vertices.shape[0], faces.shape[0]))
    if not query.is_floating_point() or vertices.dtype != query.dtype:
        raise RuntimeError("green_coordinates_3D: query and vertices must be floating tensors of one dtype, got "
                           "%s and %s" % (query.dtype, vertices.dtype))
    if faces.is_floating_point() or faces.is_complex() or faces.dtype == torch.bool:
        raise RuntimeError("green_coordinates_3D: faces must be an integer tensor, got %s" % faces.dtype)
    if not (query.device == vertices.device == faces.device):
        raise RuntimeError("green_coordinates_3D: query, vertices and faces must be on one device, got %s, %s "
                           "and %s" % (query.device, vertices.device, faces.device))
    if face_normals is not None:
        if tuple(face_normals.shape) != tuple(faces.shape):
            raise RuntimeError("green_coordinates_3D: face_normals must have shape (B, F, 3) = %s, got %s" % (
                tuple(faces.shape), tuple(face_normals.shape)))
        if face_normals.dtype != query.dtype or face_normals.device != query.device:
            raise RuntimeError("green_coordinates_3D: face_normals must have the dtype and device of query, got %s "
                               "on %s" % (face_normals.dtype, face_normals.device))


def compute_face_normals_and_areas(vertices, faces):
    """``(face_normals (B,F,3), face_areas (B,F))`` of the triangles ``faces`` (B,F,3) over ``vertices`` (B,N,3);
    2-D ``(N,3)`` / ``(F,3)`` inputs give unbatched outputs.  The normal is ``normalize(cross(v1 - v0, v2 - v1))``
    (``F.normalize``, eps 1e-12), the area half the cross product's norm (reference geo_operations.py:529-559, without
    its in-place unsqueeze of the inputs).  Differentiable."""
    unbatched = vertices.dim() == 2 and faces.dim() == 2
    if unbatched:
        vertices, faces = vertices.unsqueeze(0), faces.unsqueeze(0)
    B = vertices.shape[0]
    # (B,F,3,D) corners by advanced indexing, not torch.gather: the same values, and a backward (index_put_ with
    # accumulate, sorted) that is reproducible bit for bit, where gather's scatter-add on the GPU is not
    batch = torch.arange(B, device=vertices.device).view(B, 1, 1)
    fv = vertices[batch, faces.long()]
    cross = torch.cross(fv[:, :, 1, :] - fv[:, :, 0, :], fv[:, :, 2, :] - fv[:, :, 1, :], dim=-1)
    areas = torch.sqrt((cross ** 2).sum(dim=-1)) / 2
    normals = tnf.normalize(cross, p=2, dim=-1, eps=1e-12)
    if unbatched:
        return normals[0], areas[0]
    return normals, areas


def _tri_int(p, v1, v2):
    """``_gcTriInt(p, v1, v2, None)``: p (...,3) broadcast against v1, v2 (...,3,3) -> (...,3); the reference's
    clamps and filters in its order"""
    p = p.unsqueeze(-2)
    p_v1 = p - v1
    v2_p = v2 - p
    v2_v1 = v2 - v1
    p_v1_norm = torch.linalg.vector_norm(p_v1, dim=-1)
    t = (v2_v1 * p_v1).sum(-1) / (p_v1_norm * torch.linalg.vector_norm(v2_v1, dim=-1) + _DIV_GUARD)
    t = t.clamp(-1.0, 1.0)
    mask = t.abs() > (1 - _EPS)
    alpha = torch.acos(t.clamp(-1.0 + _EPS, 1.0 - _EPS))
    mask = mask | ((alpha - math.pi).abs() < _ANGLE_EPS) | (alpha.abs() < _ANGLE_EPS)
    t = (-p_v1 * v2_p).sum(-1) / (p_v1_norm * torch.linalg.vector_norm(v2_p, dim=-1) + _DIV_GUARD)
    t = t.clamp(-1.0, 1.0)
    mask = mask | (t.abs() > (1 - _EPS))
    beta = torch.acos(t.clamp(-1.0 + _EPS, 1.0 - _EPS))
    lambd = (p_v1_norm * torch.sin(alpha)) ** 2
    c = (p * p).sum(-1)
    theta_1 = torch.clamp(math.pi - alpha, 0, math.pi)
    theta_2 = torch.clamp(math.pi - alpha - beta, -math.pi, math.pi)
    S_1, S_2 = torch.sin(theta_1), torch.sin(theta_2)
    C_1, C_2 = torch.cos(theta_1), torch.cos(theta_2)
    sqrt_c = torch.sqrt(c + _DIV_GUARD)
    sqrt_l = torch.sqrt(lambd + _DIV_GUARD)
    flat_1, flat_2 = (C_1 - 1).abs() < _EPS, (C_2 - 1).abs() < _EPS
    mask = mask | flat_1 | flat_2
    # the discarded branch's denominator is made safe, so its gradient is 0 and not NaN
    sqcot_1 = torch.where(flat_1, torch.zeros_like(C_1), S_1 * S_1 / ((1 - C_1) ** 2 + _DIV_GUARD))
    sqcot_2 = torch.where(flat_2, torch.zeros_like(C_2), S_2 * S_2 / ((1 - C_2) ** 2 + _DIV_GUARD))

    def part(S, C, sqcot):
        in_log = sqrt_l * (1 - 2 * c * C / (_DIV_GUARD + c * (1 + C) + lambd + sqrt_l * torch.sqrt(
            lambd + c * S * S + _DIV_GUARD))) * 2 * sqcot
        in_log = in_log.masked_fill(mask | (in_log <= 0), 1.0)
        return -0.5 * torch.sign(S) * (2 * sqrt_c * torch.atan((sqrt_c * C) / torch.sqrt(lambd + S * S * c + _DIV_GUARD))
                                       + sqrt_l * torch.log(in_log))

    I_1, I_2 = part(S_1, C_1, sqcot_1), part(S_2, C_2, sqcot_2)
    return (-1 / (4 * math.pi) * torch.abs(I_1 - I_2 - sqrt_c * beta)).masked_fill(mask, 0.0)


def composition(query, vertices, faces, face_normals=None, verbose=False):
    """The contract as torch operations, for any device and floating dtype: ``(GC_vertex (B,P,N), GC_face (B,P,F),
    exterior_flag (B,P,1))``.  Differentiable in ``query`` and in ``face_normals`` (given) or ``vertices`` (through
    the computed normals).  Where a branch discards a value its denominator is made safe, so the gradients are finite
    where the reference's are NaN (a query on a vertex)."""
    _check(query, vertices, faces, face_normals)
    B, P, _ = query.shape
    N, F = vertices.shape[1], faces.shape[1]
    fl = faces.long()
    bad = ((fl < 0) | (fl >= N)).reshape(B, -1).any(1)                      # (B,)
    nan = float("nan")
    if N == 0 or F == 0:
        link = query.sum() * 0 + vertices.sum() * 0                          # keeps the outputs on the graph
        if face_normals is not None:
            link = link + face_normals.sum() * 0
        gcv = query.new_zeros(B, P, N) + link
        gcf = query.new_zeros(B, P, F) + link
        exterior = torch.ones(B, P, 1, dtype=torch.bool, device=query.device)
        gcv = torch.where(bad[:, None, None], torch.full_like(gcv, nan), gcv)
        gcf = torch.where(bad[:, None, None], torch.full_like(gcf, nan), gcf)
        return gcv, gcf, exterior & ~bad[:, None, None]
    fl = fl.clamp(0, N - 1)
    n_t = face_normals if face_normals is not None else compute_face_normals_and_areas(vertices, fl)[0]
    vd = vertices.detach()
    v = torch.gather(vd, 1, fl.reshape(B, F * 3, 1).expand(-1, -1, 3)).view(B, 1, F, 3, 3) - query.view(B, P, 1, 1, 3)
    n = n_t.unsqueeze(1)                                                       # (B,1,F,3)
    p = (v[:, :, :, 0, :] * n).sum(-1, keepdim=True) * n                      # (B,P,F,3)
    vn = v[:, :, :, _NEXT, :]
    s = torch.sign((torch.cross(v - p.unsqueeze(-2), vn - p.unsqueeze(-2), dim=-1) * n.unsqueeze(-2)).sum(-1))
    I = -torch.abs((s * _tri_int(p, v, vn)).sum(-1))                         # (B,P,F)
    gcf = -I
    II = _tri_int(torch.zeros_like(p), vn, v)
    Nl = torch.cross(vn, v, dim=-1)
    Nl_norm = torch.linalg.vector_norm(Nl, dim=-1)
    big = Nl_norm > _N_EPS
    II = II.masked_fill(Nl_norm < _N_EPS, 0)
    Nl = torch.where(big.unsqueeze(-1), Nl / torch.where(big, Nl_norm, torch.ones_like(Nl_norm)).unsqueeze(-1), Nl)
    omega = n * I.unsqueeze(-1) + (Nl * II.unsqueeze(-1)).sum(-2)            # (B,P,F,3)
    Nn = Nl[:, :, :, _NEXT, :]
    phi = (Nn * omega.unsqueeze(-2)).sum(-1) / ((Nn * v).sum(-1) + _PHI_GUARD)
    phi = phi.masked_fill((torch.linalg.vector_norm(omega, dim=-1) < _OMEGA_EPS).unsqueeze(-1), 0)
    raw = query.new_zeros(B, P, N).scatter_add(2, fl.reshape(B, 1, F * 3).expand(B, P, F * 3), phi.reshape(B, P, F * 3))
    total = raw.sum(2, keepdim=True)
    exterior = total < 0.5
    gcv = raw / (total + _PHI_GUARD)
    gcv = torch.where(bad[:, None, None], torch.full_like(gcv, nan), gcv)
    gcf = torch.where(bad[:, None, None], torch.full_like(gcf, nan), gcf)
    return gcv, gcf, exterior & ~bad[:, None, None]


class GreenCoordinates3D(torch.autograd.Function):
    """HIP forward and backward (CUDA fp32 / fp64) of the pair evaluation, for the vertices detached: inputs
    ``(query, vertices, faces, n_t)``, outputs ``(GC_vertex, GC_face, exterior_flag)``; gradients reach ``query`` and
    ``n_t``."""

    @staticmethod
    def forward(ctx, query, vertices, faces, n_t):
        dev = _lib.require_cuda(("query", query), ("vertices", vertices), ("faces", faces), ("face_normals", n_t))
        dt = query.dtype
        B, P, _ = query.shape
        N, F = vertices.shape[1], faces.shape[1]
        query = query.contiguous()
        vertices = vertices.contiguous()
        n_t = n_t.contiguous()
        fl, fsb = _lib.faces_arg(faces, B, F, 3)
        gcv = torch.empty(B, P, N, dtype=dt, device=dev)
        gcf = torch.empty(B, P, F, dtype=dt, device=dev)
        sums = torch.empty(B, P, dtype=dt, device=dev)
        codes = torch.empty(B, P, dtype=torch.int32, device=dev)
        fn = _lib.lib().pp_gc3d_forward_f64 if dt == torch.float64 else _lib.lib().pp_gc3d_forward_f32
        with _lib.on_device(dev) as stream:
            _lib.check(fn(_lib.ptr(query), _lib.ptr(vertices), _lib.ptr(fl), fsb, _lib.ptr(n_t), _lib.ptr(gcv),
                          _lib.ptr(gcf), _lib.ptr(sums), _lib.ptr(codes), B, P, N, F, stream),
                       "green_coordinates_3D forward")
        exterior = (sums < 0.5).unsqueeze(-1)
        ctx.save_for_backward(query, vertices, fl, n_t, gcv, sums, codes)
        ctx.fsb = fsb
        ctx.mark_non_differentiable(exterior)
        return gcv, gcf, exterior

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_gcv, grad_gcf, _grad_exterior):
        query, vertices, fl, n_t, gcv, sums, codes = ctx.saved_tensors
        dev, dt = query.device, query.dtype
        B, P, _ = query.shape
        N = vertices.shape[1]
        F = n_t.shape[1]
        grad_gcv = grad_gcv.contiguous() if grad_gcv is not None else torch.zeros_like(gcv)
        grad_gcf = grad_gcf.contiguous() if grad_gcf is not None else None
        gq = torch.empty_like(query)
        gn = torch.empty_like(n_t)
        fn = _lib.lib().pp_gc3d_backward_f64 if dt == torch.float64 else _lib.lib().pp_gc3d_backward_f32
        with _lib.on_device(dev) as stream:
            nbytes = _lib.lib().pp_gc3d_workspace_bytes(B, P, F, query.element_size())
            ws = _lib.workspace(dev, "gc3d", nbytes)
            _lib.check(fn(_lib.ptr(query), _lib.ptr(vertices), _lib.ptr(fl), ctx.fsb, _lib.ptr(n_t), _lib.ptr(gcv),
                          _lib.ptr(sums), _lib.ptr(codes), _lib.ptr(grad_gcv),
                          _lib.ptr(grad_gcf) if grad_gcf is not None else None, _lib.ptr(gq), _lib.ptr(gn), B, P, N,
                          F, _lib.ptr(ws) if ws is not None else None, ctypes.c_size_t(nbytes), stream),
                       "green_coordinates_3D backward")
        return (gq if ctx.needs_input_grad[0] else None), None, None, (gn if ctx.needs_input_grad[3] else None)


def green_coordinates_3D(query, vertices, faces, face_normals=None, verbose=False):
    """Green coordinates of ``query`` (B,P,3) with respect to the closed triangle cage ``vertices`` (B,N,3),
    ``faces`` (B,F,3) (integer vertex indices; a batch-expanded view of one face list is read without a copy):
    ``(GC_vertex (B,P,N), GC_face (B,P,F), exterior_flag (B,P,1) bool)``.  A deformed point is
    ``sum_j GC_vertex_j v'_j + sum_f GC_face_f n'_f`` with the deformed cage's normals ``n'``
    (``compute_face_normals_and_areas``).  ``face_normals`` (B,F,3) replaces the normals computed from the cage;
    ``verbose`` is accepted and ignored.  As in the reference, the vertices are detached before the pair evaluation:
    gradients reach ``vertices`` only through the normals computed from them, and a given ``face_normals`` gets its own.

    CUDA fp32 / fp64: the HIP kernels; anything else: ``composition``.  Nothing synchronises with the host: an
    out-of-range face index gives NaN rows (and ``exterior_flag`` False) for its batch element."""
    _check(query, vertices, faces, face_normals)
    if query.is_cuda and query.dtype in (torch.float32, torch.float64):
        B, N, F = query.shape[0], vertices.shape[1], faces.shape[1]
        if face_normals is None:
            fl = faces.long()
            if N > 0:
                fl = fl.clamp(0, N - 1)       # an out-of-range index: NaN rows from the kernel, not a bad gather
            n_t = compute_face_normals_and_areas(vertices, fl)[0] if N > 0 else vertices.new_zeros(B, F, 3)
        else:
            n_t = face_normals
        return GreenCoordinates3D.apply(query, vertices.detach(), faces, n_t)
    return composition(query, vertices, faces, face_normals, verbose)
