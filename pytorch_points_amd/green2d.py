"""Green coordinates of 2-D query points with respect to a closed polygonal cage given as directed edges (Lipman,
Levin and Cohen-Or, "Green Coordinates", 2008, the closed form of their Algorithm 1): the operator behind
``network.geo_operations.green_coordinates_2D``, which the reference declares and leaves empty
(geo_operations.py:622), and the deformation that goes with it.

CUDA fp32 and fp64 run the fused HIP kernels of csrc/green2d.hip (``pp_gc2d_*``): no per-(query, edge) tensor is
materialised, and the backward evaluates every pair again.  Every other device or dtype goes through
``composition``, the same contract written as torch operations.  DESIGN.md "Green coordinates, 2-D" states the
contract.
"""
import ctypes
import math

import torch

from . import _lib

# the most cage vertices whose fp64 accumulator columns fit the 160 KiB of LDS beside the 64-edge tile of psi
# (csrc/green2d.hip, chunk_cap): beyond it the forward walks the edges once per chunk of that many vertices
LDS_VERTICES = {torch.float32: 283, torch.float64: 251}


def _check(query, vertices, faces, edge_normals=None):
    for name, t in (("query", query), ("vertices", vertices), ("faces", faces)):
        if t.dim() != 3 or t.shape[2] != 2:
            raise RuntimeError("green_coordinates_2D: %s must have shape (B, *, 2), got %s" % (name, tuple(t.shape)))
    if not (query.shape[0] == vertices.shape[0] == faces.shape[0]):
        raise RuntimeError("green_coordinates_2D: query, vertices and faces must have the same batch size, got "
                           "%d, %d and %d" % (query.shape[0], vertices.shape[0], faces.shape[0]))
    if not query.is_floating_point() or vertices.dtype != query.dtype:
        raise RuntimeError("green_coordinates_2D: query and vertices must be floating tensors of one dtype, got "
                           "%s and %s" % (query.dtype, vertices.dtype))
    if faces.is_floating_point() or faces.is_complex() or faces.dtype == torch.bool:
        raise RuntimeError("green_coordinates_2D: faces must be an integer tensor, got %s" % faces.dtype)
    if not (query.device == vertices.device == faces.device):
        raise RuntimeError("green_coordinates_2D: query, vertices and faces must be on one device, got %s, %s "
                           "and %s" % (query.device, vertices.device, faces.device))
    if edge_normals is not None:
        if tuple(edge_normals.shape) != tuple(faces.shape):
            raise RuntimeError("green_coordinates_2D: edge_normals must have shape (B, F, 2) = %s, got %s" % (
                tuple(faces.shape), tuple(edge_normals.shape)))
        if edge_normals.dtype != query.dtype or edge_normals.device != query.device:
            raise RuntimeError("green_coordinates_2D: edge_normals must have the dtype and device of query, got %s "
                               "on %s" % (edge_normals.dtype, edge_normals.device))


def _edge_ends(vertices, fl, edge_normals):
    """``(v1, v2)`` (B,F,2): the endpoints of every edge as the pair evaluation takes them, swapped where
    ``edge_normals`` points against the edge's own normal.  Advanced indexing, not torch.gather: a backward that is
    reproducible bit for bit."""
    B = vertices.shape[0]
    i1, i2 = fl[:, :, 0], fl[:, :, 1]
    batch = torch.arange(B, device=vertices.device).view(B, 1)
    if edge_normals is not None:
        vd, en = vertices.detach().double(), edge_normals.detach().double()
        a = vd[batch, i2] - vd[batch, i1]
        flip = (en[:, :, 0] * a[:, :, 1] - en[:, :, 1] * a[:, :, 0]) < 0
        i1, i2 = torch.where(flip, i2, i1), torch.where(flip, i1, i2)
    return vertices[batch, i1], vertices[batch, i2], i1, i2


def composition(query, vertices, faces, edge_normals=None, verbose=False):
    """The contract as torch operations, for any device and floating dtype: ``(phi (B,P,N), psi (B,P,F),
    exterior_flag (B,P,1))``.  Every pair is evaluated in fp64 and the sums rounded once to the inputs' dtype.
    Differentiable in ``query`` and ``vertices``; where a rule discards a value its denominator or argument is made
    safe first, so the gradients of a query on a vertex, an edge or an edge's line are finite."""
    _check(query, vertices, faces, edge_normals)
    B, P, _ = query.shape
    N, F = vertices.shape[1], faces.shape[1]
    dt = query.dtype
    fl = faces.long()
    bad = ((fl < 0) | (fl >= N)).reshape(B, -1).any(1)[:, None, None]        # (B,1,1)
    nan = float("nan")
    if N == 0 or F == 0:
        link = query.sum() * 0 + vertices.sum() * 0                          # keeps the outputs on the graph
        phi = query.new_zeros(B, P, N) + link
        psi = query.new_zeros(B, P, F) + link
        phi = torch.where(bad, torch.full_like(phi, nan), phi)
        psi = torch.where(bad, torch.full_like(psi, nan), psi)
        return phi, psi, torch.ones(B, P, 1, dtype=torch.bool, device=query.device) & ~bad
    fl = fl.clamp(0, N - 1)
    v1, v2, i1, i2 = _edge_ends(vertices, fl, edge_normals)
    v1, v2 = v1.double().unsqueeze(1), v2.double().unsqueeze(1)              # (B,1,F,2)
    q = query.double().unsqueeze(2)                                          # (B,P,1,2)
    a, b, e = v2 - v1, v1 - q, v2 - q
    Q, S, T = (a * a).sum(-1), (b * b).sum(-1), (e * e).sum(-1)              # Q (B,1,F); S, T (B,P,F)
    R = 2 * (a * b).sum(-1)
    c = a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]
    d = (b * e).sum(-1)
    one = torch.ones_like(S)
    zero = torch.zeros_like(S)
    live = (Q != 0).expand_as(S)                                             # (a NaN length is not a zero length)
    Qs = torch.where(Q != 0, Q, torch.ones_like(Q))
    cz = c == 0
    th = torch.where(cz, zero, torch.atan2(torch.where(cz, one, c), d))
    ln_t = torch.log(torch.where(T == 0, one, T))                            # x ln 0 := 0: ln 0 is taken as 0
    ln_s = torch.log(torch.where(S == 0, one, S))
    r = R / Qs
    u = 1 + r / 2
    big_l = u * ln_t + (1 - u) * ln_s
    g = torch.where(cz, zero, c * (ln_t - ln_s) / (2 * Qs))
    h = th / 2
    psi = -torch.sqrt(Qs) / (4 * math.pi) * (2 * c * th / Qs + big_l - 2)
    p1 = (g - h * (2 + r)) / (2 * math.pi)
    p2 = (h * r - g) / (2 * math.pi)
    psi, p1, p2 = torch.where(live, psi, zero), torch.where(live, p1, zero), torch.where(live, p2, zero)
    broken = ~(torch.isfinite(psi) & torch.isfinite(p1) & torch.isfinite(p2)).all(-1, keepdim=True)    # (B,P,1)
    # per vertex in ascending edge order, an edge's first end before its second
    ends = torch.stack([i1, i2], -1).reshape(B, 1, 2 * F).expand(B, P, 2 * F)
    phi = psi.new_zeros(B, P, N).scatter_add(2, ends, torch.stack([p1, p2], -1).reshape(B, P, 2 * F))
    total = phi.sum(-1, keepdim=True)
    dead = bad | broken
    phi = torch.where(dead, torch.full_like(phi, nan), phi).to(dt)
    psi = torch.where(dead, torch.full_like(psi, nan), psi).to(dt)
    return phi, psi, (total < 0.5) & ~dead


class GreenCoordinates2D(torch.autograd.Function):
    """HIP forward and backward (CUDA fp32 / fp64): inputs ``(query, vertices, faces, edge_normals or None)``,
    outputs ``(phi, psi, exterior_flag)``; gradients reach ``query`` and ``vertices``."""

    @staticmethod
    def forward(ctx, query, vertices, faces, edge_normals):
        named = [("query", query), ("vertices", vertices), ("faces", faces)]
        if edge_normals is not None:
            named.append(("edge_normals", edge_normals))
        dev = _lib.require_cuda(*named)
        dt = query.dtype
        B, P, _ = query.shape
        N, F = vertices.shape[1], faces.shape[1]
        query = query.contiguous()
        vertices = vertices.contiguous()
        en = edge_normals.detach().contiguous() if edge_normals is not None else None
        fl, fsb = _lib.faces_arg(faces, B, F, 2)
        phi = torch.empty(B, P, N, dtype=dt, device=dev)
        psi = torch.empty(B, P, F, dtype=dt, device=dev)
        exterior = torch.empty(B, P, 1, dtype=torch.bool, device=dev)
        codes = torch.empty(B, P, dtype=torch.int32, device=dev)
        fn = _lib.lib().pp_gc2d_forward_f64 if dt == torch.float64 else _lib.lib().pp_gc2d_forward_f32
        with _lib.on_device(dev) as stream:
            _lib.check(fn(_lib.ptr(query), _lib.ptr(vertices), _lib.ptr(fl), fsb,
                          _lib.ptr(en) if en is not None else None, _lib.ptr(phi), _lib.ptr(psi),
                          _lib.ptr(exterior), _lib.ptr(codes), B, P, N, F, stream), "green_coordinates_2D forward")
        ctx.save_for_backward(query, vertices, fl, codes, *([en] if en is not None else []))
        ctx.fsb = fsb
        ctx.mark_non_differentiable(exterior)
        return phi, psi, exterior

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_phi, grad_psi, _grad_exterior):
        query, vertices, fl, codes = ctx.saved_tensors[:4]
        en = ctx.saved_tensors[4] if len(ctx.saved_tensors) > 4 else None
        dev, dt = query.device, query.dtype
        B, P, _ = query.shape
        N, F = vertices.shape[1], fl.shape[-2]
        grad_phi = grad_phi.contiguous() if grad_phi is not None else None
        grad_psi = grad_psi.contiguous() if grad_psi is not None else None
        gq = torch.empty_like(query)
        gv = torch.empty_like(vertices)
        fn = _lib.lib().pp_gc2d_backward_f64 if dt == torch.float64 else _lib.lib().pp_gc2d_backward_f32
        with _lib.on_device(dev) as stream:
            nbytes = _lib.lib().pp_gc2d_workspace_bytes(B, P, F, query.element_size())
            ws = _lib.workspace(dev, "gc2d", nbytes)
            _lib.check(fn(_lib.ptr(query), _lib.ptr(vertices), _lib.ptr(fl), ctx.fsb,
                          _lib.ptr(en) if en is not None else None, _lib.ptr(codes),
                          _lib.ptr(grad_phi) if grad_phi is not None else None,
                          _lib.ptr(grad_psi) if grad_psi is not None else None, _lib.ptr(gq), _lib.ptr(gv), B, P, N,
                          F, _lib.ptr(ws) if ws is not None else None, ctypes.c_size_t(nbytes), stream),
                       "green_coordinates_2D backward")
        return (gq if ctx.needs_input_grad[0] else None), (gv if ctx.needs_input_grad[1] else None), None, None


def green_coordinates_2D(query, vertices, faces, edge_normals=None, verbose=False):
    """Green coordinates of ``query`` (B,P,2) with respect to the cage ``vertices`` (B,N,2), ``faces`` (B,F,2): row
    ``j`` of ``faces`` is the directed edge ``(v1, v2)`` (integer vertex indices, any order, any number of closed
    loops; a batch-expanded view of one edge list is read without a copy), with the outward normal
    ``(a_y, -a_x) / |a|``, ``a = v2 - v1``: outer loops counter-clockwise, holes clockwise.  Returns
    ``(phi (B,P,N), psi (B,P,F), exterior_flag (B,P,1) bool)``: inside the cage ``sum_i phi_i = 1`` and
    ``query = sum_i phi_i v_i + sum_j psi_j n_j``; outside ``sum_i phi_i = 0``; ``exterior_flag = sum_i phi_i < 0.5``.
    ``phi`` is not renormalised.  ``edge_normals`` (B,F,2) only orients: an edge whose own normal points against its
    row is taken reversed; it gets no gradient.  ``verbose`` is accepted and ignored.  Differentiable in ``query``
    and ``vertices``.

    CUDA fp32 / fp64 and a non-empty input: the HIP kernels; anything else: ``composition``.  Nothing synchronises
    with the host: an out-of-range index gives NaN rows (and ``exterior_flag`` False) for its batch element, a
    non-finite pair for its query."""
    _check(query, vertices, faces, edge_normals)
    if (query.is_cuda and query.dtype in (torch.float32, torch.float64) and query.shape[0] > 0 and query.shape[1] > 0
            and vertices.shape[1] > 0 and faces.shape[1] > 0):
        return GreenCoordinates2D.apply(query, vertices, faces, edge_normals)
    return composition(query, vertices, faces, edge_normals, verbose)


def deform_with_green_coordinates_2D(phi, psi, vertices, new_vertices, faces):
    """The paper's deformation: ``sum_i phi_i v'_i + sum_j psi_j s_j n'_j`` (B,P,2) for the cage ``vertices`` (B,N,2)
    moved to ``new_vertices`` (B,N,2), with ``s_j = |a'_j| / |a_j|`` the stretch of edge ``j`` and ``n'_j`` the
    deformed edge's normal ``(a'_y, -a'_x) / |a'_j|``.  ``new_vertices = vertices`` gives the queries back; a
    similarity of the cage moves them by that similarity.  Plain torch, differentiable.  A zero-length edge (whose
    ``psi`` is 0) contributes nothing."""
    B = vertices.shape[0]
    fl = faces.long()
    batch = torch.arange(B, device=vertices.device).view(B, 1)
    a = vertices[batch, fl[:, :, 1]] - vertices[batch, fl[:, :, 0]]
    a_new = new_vertices[batch, fl[:, :, 1]] - new_vertices[batch, fl[:, :, 0]]
    length = torch.linalg.vector_norm(a, dim=-1, keepdim=True)
    length = torch.where(length > 0, length, torch.ones_like(length))
    scaled_normal = torch.stack([a_new[:, :, 1], -a_new[:, :, 0]], -1) / length          # s_j n'_j: |a'_j| cancels
    return phi @ new_vertices + psi @ scaled_normal
