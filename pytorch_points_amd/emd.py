"""The earth mover's distance between two point clouds by the approximate matching of Fan, Su and Guibas (2017):

    approx_match(xyz1 (B,N,3), xyz2 (B,M,3))      ->   EmdMatch(a (B,10,N), b (B,10,M));  .dense() -> (B,N,M)
    match_cost(xyz1, xyz2, match)                 ->   cost (B,), differentiable in xyz1 and xyz2
    emd_distance(xyz1, xyz2)                      ->   cost (B,) of the match of the same call
    emd_composition(xyz1, xyz2)                   ->   (EmdMatch, cost (B,)): the contract as torch operations

**The contract.**  The pair value is ``d_kl = (dx dx + dy dy) + dz dz``.  ``multiL = max(N,M) // N`` and ``multiR =
max(N,M) // M`` (integer division, the original's rule: where neither size divides the other some mass stays
unmatched).  From ``remainL[k] = multiL`` and ``remainR[l] = multiR``, for the ten levels ``-4^7, -4^6, ..., -4^-1, 0``
in this order:

    1. a[k] = remainL[k] / (1e-9 + sum_l exp(level d_kl) remainR[l])
    2. s[l] = (sum_k exp(level d_kl) a[k]) remainR[l]
    3. b[l] = min(remainR[l] / (s[l] + 1e-9), 1) remainR[l]
    4. remainR[l] = max(0, remainR[l] - s[l])
    5. remainL[k] = max(0, remainL[k] - a[k] sum_l exp(level d_kl) b[l])

and the match is ``match[k,l] = sum_j (exp(level_j d_kl) a_j[k]) b_j[l]``, ``j`` ascending: a sum of ten kernels scaled
by rank-one factors.  Its whole state is the factors, ``40 B (N + M)`` bytes; the dense ``(B,N,M)`` matrix, with xyz1
along the rows, is built only by ``EmdMatch.dense()``.  (The well-known ``approxmatch`` modules store the transpose,
``(B,M,N)``.)  ``cost[b] = sum_kl match[k,l] sqrt(d_kl)``.  The gradient treats the match as a constant, as the
original does: ``d cost / d xyz1[k] = sum_l (match[k,l] / max(sqrt(d_kl), 1e-20)) (xyz1_k - xyz2_l)`` and for
``xyz2[l]`` the negative of the same terms summed over ``k``; coincident points contribute a zero vector.
``approx_match`` itself is not differentiable.

CUDA fp32 runs the HIP kernels of csrc/emd.hip (``pp_emd_*``): twenty launches for a match, two for a cost, one per
gradient asked for; no floating-point atomics, the same bits on every run, one form only, nothing synchronises with
the host, and the workspace comes from torch's allocator so that a step can be captured.  CPU tensors, fp64 and sizes
beyond the kernels' index limits take ``emd_composition``, the same contract as torch operations.  Bit-equality between
the two is not promised: the sums are long and their association differs.  DESIGN.md "Earth mover's distance".
"""
import torch

from . import _lib

LEVELS = tuple(-(4.0 ** j) for j in range(7, -2, -1)) + (0.0,)
CHUNK_PAIRS = 1 << 22   # pairs of one evaluated block of the composition's (B, N, M) matrix
LIMIT = 2 ** 31 - 1     # B*N and B*M of the kernels


def _check(what, xyz1, xyz2):
    for name, t in (("xyz1", xyz1), ("xyz2", xyz2)):
        if not isinstance(t, torch.Tensor) or t.dtype not in (torch.float32, torch.float64):
            raise TypeError("%s: %s must be a float32 or float64 tensor, got %s"
                            % (what, name, t.dtype if isinstance(t, torch.Tensor) else type(t).__name__))
        if t.dim() != 3 or t.shape[2] != 3:
            raise ValueError("%s: %s must have shape (B, %s, 3), got %s"
                             % (what, name, "N" if name == "xyz1" else "M", tuple(t.shape)))
    if xyz2.shape[0] != xyz1.shape[0]:
        raise ValueError("%s: xyz2 must have shape (B, M, 3) with B = %d, got %s"
                         % (what, xyz1.shape[0], tuple(xyz2.shape)))
    if xyz2.dtype != xyz1.dtype:
        raise TypeError("%s: xyz2 is %s but xyz1 is %s" % (what, xyz2.dtype, xyz1.dtype))
    if xyz2.device != xyz1.device:
        raise RuntimeError("%s: xyz2 is on %s, expected %s" % (what, xyz2.device, xyz1.device))


class EmdMatch(object):
    """The match of ``approx_match`` as its factors: ``a (B,10,N)``, ``b (B,10,M)`` and the clouds they belong to
    (detached).  ``dense()`` gives ``match (B,N,M)``, xyz1 along the rows.  Not differentiable.  ``hip``: the kernels
    made it and serve its ``dense()`` and cost; otherwise the composition does."""

    def __init__(self, xyz1, xyz2, a, b, hip):
        self.xyz1, self.xyz2, self.a, self.b, self.hip = xyz1, xyz2, a, b, hip
        self.batch, self.n, self.m = xyz1.shape[0], xyz1.shape[1], xyz2.shape[1]

    def dense(self):
        if self.hip:
            dev = self.a.device
            out = torch.empty(self.batch, self.n, self.m, dtype=torch.float32, device=dev)
            if out.numel():
                with _lib.on_device(dev) as stream:
                    _lib.check(_lib.lib().pp_emd_dense_f32(
                        _lib.ptr(self.xyz1), _lib.ptr(self.xyz2), _lib.ptr(self.a), _lib.ptr(self.b), _lib.ptr(out),
                        self.batch, self.n, self.m, stream), "emd dense")
            return out
        out = torch.zeros(self.batch, self.n, self.m, dtype=self.a.dtype, device=self.a.device)
        for (k0, k1), match, _ in _match_blocks(self.xyz1, self.xyz2, self.a, self.b):
            out[:, k0:k1] = match
        return out


def _check_match(what, xyz1, xyz2, match):
    if not isinstance(match, EmdMatch):
        raise TypeError("%s: match must be the EmdMatch of approx_match, got %s" % (what, type(match).__name__))
    b, n, m = xyz1.shape[0], xyz1.shape[1], xyz2.shape[1]
    if (match.batch, match.n, match.m) != (b, n, m):
        raise ValueError("%s: match is of clouds (B, N, M) = %s, got %s"
                         % (what, (match.batch, match.n, match.m), (b, n, m)))
    if match.a.dtype != xyz1.dtype:
        raise TypeError("%s: match is %s but xyz1 is %s" % (what, match.a.dtype, xyz1.dtype))
    if match.a.device != xyz1.device:
        raise RuntimeError("%s: match is on %s, expected %s" % (what, match.a.device, xyz1.device))


# ------------------------------------------------------------------------------------------- the composition
def _blocks(b, n, m):
    """row ranges of xyz1 whose (B, rows, M) pair matrix has at most ``CHUNK_PAIRS`` pairs (one row where B M alone is
    beyond that)"""
    step = max(1, CHUNK_PAIRS // max(1, b * m))
    return [(k0, min(n, k0 + step)) for k0 in range(0, n, step)]


def _pair_d(x1, x2):
    """``d (B,rows,M)`` and the three differences ``xyz1 - xyz2``"""
    dx = x1[:, :, None, 0] - x2[:, None, :, 0]
    dy = x1[:, :, None, 1] - x2[:, None, :, 1]
    dz = x1[:, :, None, 2] - x2[:, None, :, 2]
    return (dx * dx + dy * dy) + dz * dz, (dx, dy, dz)


def _pairs(xyz1, xyz2):
    """a function ``(k0, k1) -> d`` over the row blocks; the one block of a small problem is kept"""
    blocks = _blocks(xyz1.shape[0], xyz1.shape[1], xyz2.shape[1])
    kept = {}

    def d_of(k0, k1):
        if len(blocks) == 1:
            if not kept:
                kept[0] = _pair_d(xyz1, xyz2)[0]
            return kept[0]
        return _pair_d(xyz1[:, k0:k1], xyz2)[0]

    return blocks, d_of


def factors_composition(xyz1, xyz2):
    """The ten levels of the contract as torch operations: ``(a (B,10,N), b (B,10,M))``.  The (B,N,M) pair matrix is
    evaluated in row blocks of at most ``CHUNK_PAIRS`` pairs, three times per level, so the peak memory does not grow
    with N M."""
    bsz, n, m = xyz1.shape[0], xyz1.shape[1], xyz2.shape[1]
    dev, dtype = xyz1.device, xyz1.dtype
    a = torch.zeros(bsz, len(LEVELS), n, dtype=dtype, device=dev)
    b = torch.zeros(bsz, len(LEVELS), m, dtype=dtype, device=dev)
    if bsz == 0 or n == 0 or m == 0:
        return a, b
    big = max(n, m)
    remain_l = torch.full((bsz, n), float(big // n), dtype=dtype, device=dev)
    remain_r = torch.full((bsz, m), float(big // m), dtype=dtype, device=dev)
    blocks, d_of = _pairs(xyz1, xyz2)
    for j, level in enumerate(LEVELS):
        for k0, k1 in blocks:                                               # step 1
            e = torch.exp(level * d_of(k0, k1))
            a[:, j, k0:k1] = remain_l[:, k0:k1] / (1e-9 + (e * remain_r[:, None, :]).sum(2))
        v = torch.zeros(bsz, m, dtype=dtype, device=dev)
        for k0, k1 in blocks:                                               # step 2
            e = torch.exp(level * d_of(k0, k1))
            v = v + (e * a[:, j, k0:k1, None]).sum(1)
        s = v * remain_r
        b[:, j] = torch.clamp(remain_r / (s + 1e-9), max=1.0) * remain_r    # step 3
        remain_r = torch.clamp(remain_r - s, min=0.0)                       # step 4
        for k0, k1 in blocks:                                               # step 5
            e = torch.exp(level * d_of(k0, k1))
            taken = a[:, j, k0:k1] * (e * b[:, j, None, :]).sum(2)
            remain_l[:, k0:k1] = torch.clamp(remain_l[:, k0:k1] - taken, min=0.0)
    return a, b


def _match_blocks(xyz1, xyz2, a, b):
    """``((k0, k1), match (B,rows,M), (d, differences))`` per row block: the match from its factors"""
    for k0, k1 in _blocks(xyz1.shape[0], xyz1.shape[1], xyz2.shape[1]):
        d, diff = _pair_d(xyz1[:, k0:k1], xyz2)
        match = torch.zeros_like(d)
        for j, level in enumerate(LEVELS):
            match = match + (torch.exp(level * d) * a[:, j, k0:k1, None]) * b[:, j, None, :]
        yield (k0, k1), match, (d, diff)


def cost_composition(xyz1, xyz2, a, b):
    """``cost (B,)`` of the match given by its factors, as torch operations (no gradient)"""
    cost = torch.zeros(xyz1.shape[0], dtype=xyz1.dtype, device=xyz1.device)
    for _, match, (d, _) in _match_blocks(xyz1, xyz2, a, b):
        cost = cost + (match * torch.sqrt(d)).sum((1, 2))
    return cost


def cost_backward_composition(xyz1, xyz2, a, b, grad_cost, want1=True, want2=True):
    """``(grad_xyz1 or None, grad_xyz2 or None)`` of ``cost_composition`` with the match held constant"""
    g1 = torch.zeros_like(xyz1) if want1 else None
    g2 = torch.zeros_like(xyz2) if want2 else None
    for (k0, k1), match, (d, diff) in _match_blocks(xyz1, xyz2, a, b):
        w = match / torch.clamp(torch.sqrt(d), min=1e-20)
        for c in range(3):
            t = w * diff[c]
            if want1:
                g1[:, k0:k1, c] = t.sum(2)
            if want2:
                g2[:, :, c] -= t.sum(1)
    scale = grad_cost[:, None, None]
    return (g1 * scale if want1 else None, g2 * scale if want2 else None)


# ------------------------------------------------------------------------------------------------- the kernels
def _hip_serves(xyz1, xyz2):
    b, n, m = xyz1.shape[0], xyz1.shape[1], xyz2.shape[1]
    return xyz1.is_cuda and xyz1.dtype == torch.float32 and b * max(n, m) <= LIMIT


def _workspace(dev, b, n, m):
    nbytes = _lib.lib().pp_emd_workspace_bytes(b, n, m)
    return torch.empty(nbytes, dtype=torch.uint8, device=dev), nbytes   # (a capture takes it from its pool)


def approx_match(xyz1, xyz2):
    """The approximate matching of ``xyz1`` (B,N,3) to ``xyz2`` (B,M,3) as an ``EmdMatch``.  The module's docstring
    states the contract.  Not differentiable: the clouds are detached.  A non-contiguous cloud is made contiguous.

    CUDA fp32: the HIP kernels, twenty launches on the current stream; anything else: ``factors_composition``."""
    _check("approx_match", xyz1, xyz2)
    with torch.no_grad():
        xyz1, xyz2 = xyz1.detach().contiguous(), xyz2.detach().contiguous()
        if not _hip_serves(xyz1, xyz2):
            return EmdMatch(xyz1, xyz2, *factors_composition(xyz1, xyz2), hip=False)
        b, n, m = xyz1.shape[0], xyz1.shape[1], xyz2.shape[1]
        dev = xyz1.device
        fa = torch.empty(b, len(LEVELS), n, dtype=torch.float32, device=dev)
        fb = torch.empty(b, len(LEVELS), m, dtype=torch.float32, device=dev)
        if b == 0 or n == 0 or m == 0:
            return EmdMatch(xyz1, xyz2, fa.zero_(), fb.zero_(), hip=True)
        ws, nbytes = _workspace(dev, b, n, m)
        with _lib.on_device(dev) as stream:
            _lib.check(_lib.lib().pp_emd_match_f32(_lib.ptr(xyz1), _lib.ptr(xyz2), _lib.ptr(fa), _lib.ptr(fb), b, n, m,
                                                   _lib.ptr(ws), nbytes, stream), "emd match")
        return EmdMatch(xyz1, xyz2, fa, fb, hip=True)


class MatchCost(torch.autograd.Function):
    """``(xyz1, xyz2, a, b, hip) -> cost (B,)`` with the match held constant in the backward: the HIP kernels with
    ``hip`` (CUDA fp32), the composition otherwise."""

    @staticmethod
    def forward(ctx, xyz1, xyz2, a, b, hip):
        xyz1, xyz2 = xyz1.contiguous(), xyz2.contiguous()
        bsz, n, m = xyz1.shape[0], xyz1.shape[1], xyz2.shape[1]
        ctx.save_for_backward(xyz1, xyz2, a, b)
        ctx.set_materialize_grads(False)
        ctx.hip = hip
        if not hip:
            return cost_composition(xyz1, xyz2, a, b)
        dev = xyz1.device
        if bsz == 0 or n == 0 or m == 0:
            return torch.zeros(bsz, dtype=torch.float32, device=dev)
        cost = torch.empty(bsz, dtype=torch.float32, device=dev)
        ws, nbytes = _workspace(dev, bsz, n, m)
        with _lib.on_device(dev) as stream:
            _lib.check(_lib.lib().pp_emd_cost_f32(_lib.ptr(xyz1), _lib.ptr(xyz2), _lib.ptr(a), _lib.ptr(b),
                                                  _lib.ptr(cost), bsz, n, m, _lib.ptr(ws), nbytes, stream), "emd cost")
        return cost

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_cost):
        want1, want2 = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if grad_cost is None or not (want1 or want2):
            return (None,) * 5
        xyz1, xyz2, a, b = ctx.saved_tensors
        bsz, n, m = xyz1.shape[0], xyz1.shape[1], xyz2.shape[1]
        grad_cost = grad_cost.contiguous()
        if not ctx.hip:
            return cost_backward_composition(xyz1, xyz2, a, b, grad_cost, want1, want2) + (None,) * 3
        if bsz == 0 or n == 0 or m == 0:
            return (torch.zeros_like(xyz1) if want1 else None, torch.zeros_like(xyz2) if want2 else None) + (None,) * 3
        g1 = torch.empty_like(xyz1) if want1 else None
        g2 = torch.empty_like(xyz2) if want2 else None
        opt = lambda t: None if t is None else _lib.ptr(t)   # noqa: E731
        with _lib.on_device(xyz1.device) as stream:
            _lib.check(_lib.lib().pp_emd_cost_backward_f32(
                _lib.ptr(xyz1), _lib.ptr(xyz2), _lib.ptr(a), _lib.ptr(b), _lib.ptr(grad_cost), opt(g1), opt(g2), bsz,
                n, m, stream), "emd cost backward")
        return g1, g2, None, None, None


# ----------------------------------------------------------------------------------------- the public interface
def match_cost(xyz1, xyz2, match):
    """``cost (B,)`` of moving ``xyz1`` onto ``xyz2`` along ``match`` (the ``EmdMatch`` of ``approx_match`` for clouds
    of these sizes): ``sum_kl match[k,l] sqrt(d_kl)``.  Differentiable once in ``xyz1`` and ``xyz2`` with the match
    held constant; only the gradients asked for are computed."""
    _check("match_cost", xyz1, xyz2)
    _check_match("match_cost", xyz1, xyz2, match)
    return MatchCost.apply(xyz1, xyz2, match.a, match.b, match.hip and _hip_serves(xyz1, xyz2))


def emd_distance(xyz1, xyz2):
    """``cost (B,)`` of the approximate matching of ``xyz1`` (B,N,3) to ``xyz2`` (B,M,3): the match under ``no_grad``,
    then ``match_cost``.  The mass moved is ``max(N,M)`` where one size divides the other."""
    _check("emd_distance", xyz1, xyz2)
    return match_cost(xyz1, xyz2, approx_match(xyz1, xyz2))


def emd_composition(xyz1, xyz2):
    """The contract as torch operations, for any device and both floating types: ``(EmdMatch, cost (B,))``, the cost
    differentiable as ``match_cost``'s is.  The oracle of the kernels."""
    _check("emd_composition", xyz1, xyz2)
    with torch.no_grad():
        x1, x2 = xyz1.detach().contiguous(), xyz2.detach().contiguous()
        match = EmdMatch(x1, x2, *factors_composition(x1, x2), hip=False)
    return match, MatchCost.apply(xyz1, xyz2, match.a, match.b, False)
