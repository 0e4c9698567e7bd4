"""GPU tests of green_coordinates_2D (csrc/green2d.hip) against the in-tree fp64 composition, run on the CPU on the same
inputs, and against a numpy.longdouble evaluation of the contract's formulas and of their hand-derived gradients,
which gives the tolerances: 8x the composition's own error on the very cage, as tests/test_green2d_host.py does
(DESIGN.md "Green coordinates, 2-D").  Every cage holds one edge with exactly representable ends (1, -t), (1, t), so
the query (1, 0) lies exactly on it in every precision, and one query sits exactly on a vertex."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DTYPES = {"fp32": torch.float32, "fp64": torch.float64}
FLOOR = 6.1e-16                 # tests/test_green2d_host.py COMPOSITION_ERROR: no tolerance is taken below 8x this
EPS32 = 2.0 ** -24


def lds_vertices(dt):
    from pytorch_points_amd import green2d
    return green2d.LDS_VERTICES[dt]


# ---------------------------------------------------------------------------------------------------------- inputs
def cage(n, seed, np_dtype):
    """a star-shaped counter-clockwise n-gon: vertex k near angle (2k - 1) pi / n, radius in [0.8, 1.2]; vertices 0
    and 1 are (1, -t) and (1, t) exactly"""
    rng = np.random.default_rng(seed)
    ang = (2 * np.arange(n) - 1) * np.pi / n + rng.uniform(-0.2, 0.2, n) * 2 * np.pi / n
    rad = rng.uniform(0.8, 1.2, n)
    v = np.stack([rad * np.cos(ang), rad * np.sin(ang)], 1).astype(np_dtype)
    t = np_dtype(np.tan(np.pi / n)) if n > 3 else np_dtype(0.5)
    v[0] = (1.0, -t)
    v[1] = (1.0, t)
    f = np.stack([np.arange(n), (np.arange(n) + 1) % n], 1)
    return v, f


def make(B, P, n, seed, np_dtype):
    """(query (B,P,2), vertices (B,n,2), faces (B,n,2)); different cages per batch element; the last two queries of
    each element (P >= 3) lie on a vertex and on the exact edge"""
    rng = np.random.default_rng(1000 + seed)
    vs, fs, qs = [], [], []
    for b in range(B):
        v, f = cage(n, seed * 10 + b, np_dtype)
        q = rng.uniform(-1.6, 1.6, (P, 2)).astype(np_dtype)
        if P >= 3:
            q[-2] = v[n // 2]
            q[-1] = (1.0, 0.0)
        vs.append(v)
        fs.append(f)
        qs.append(q)
    return np.stack(qs), np.stack(vs), np.stack(fs)


# ------------------------------------------------------------------------------------------------------- references
def longdouble_reference(q, v, f, w_phi=None, w_psi=None):
    """One batch element in numpy.longdouble: the contract's formulas with its rules -> (phi, psi); with cotangents
    also (grad_query, grad_vertices, the sum of the magnitudes of the terms of grad_vertices), by the reverse-mode
    derivatives of the closed form written out by hand."""
    ld = np.longdouble
    q, v = q.astype(ld), v.astype(ld)
    pi = ld(4) * np.arctan(ld(1))
    k = 1 / (2 * pi)
    P = len(q)
    phi, psi = np.zeros((P, len(v)), ld), np.zeros((P, len(f)), ld)
    gq, gv, gv_abs = np.zeros((P, 2), ld), np.zeros((len(v), 2), ld), np.zeros((len(v), 2), ld)
    for j, (i1, i2) in enumerate(f):
        a = v[i2] - v[i1]
        b, e = v[i1] - q, v[i2] - q
        Q = (a * a).sum()
        if Q == 0:
            continue
        S, T = (b * b).sum(-1), (e * e).sum(-1)
        R = 2 * (b * a).sum(-1)
        c = a[0] * b[:, 1] - a[1] * b[:, 0]
        d = (b * e).sum(-1)
        cz = c == 0
        th = np.where(cz, 0, np.arctan2(np.where(cz, 1, c), d))
        lt, ls = np.log(np.where(T == 0, 1, T)), np.log(np.where(S == 0, 1, S))
        r = R / Q
        u = 1 + r / 2
        D = lt - ls
        g = np.where(cz, 0, c * D / (2 * Q))
        h = th / 2
        sq = np.sqrt(Q)
        M = 2 * c * th / Q + u * lt + (1 - u) * ls - 2
        psi[:, j] = -sq / (4 * pi) * M
        phi[:, i1] += (g - h * (2 + r)) * k
        phi[:, i2] += (h * r - g) * k
        if w_phi is None:
            continue
        w1, w2, wp = w_phi[:, i1].astype(ld), w_phi[:, i2].astype(ld), w_psi[:, j].astype(ld)
        g_g = np.where(cz, 0, k * (w1 - w2))
        g_h = k * (w2 * r - w1 * (2 + r))
        g_r = k * h * (w2 - w1)
        g_M = -wp * sq / (4 * pi)
        g_Q = -wp * M / (4 * pi) / (2 * sq) - g_M * 2 * c * th / (Q * Q) - g_g * g / Q
        g_c = g_M * 2 * th / Q + g_g * D / (2 * Q)
        g_th = g_M * 2 * c / Q + g_h / 2
        g_D = g_g * c / (2 * Q)
        g_T = np.where(T == 0, 0, (g_M * u + g_D) / np.where(T == 0, 1, T))
        g_S = np.where(S == 0, 0, (g_M * (1 - u) - g_D) / np.where(S == 0, 1, S))
        g_r = g_r + g_M * D / 2
        g_R = g_r / Q
        g_Q = g_Q - g_r * r / Q
        den = np.where(cz, 1, c * c + d * d)
        g_c = g_c + np.where(cz, 0, g_th * d / den)
        g_d = np.where(cz, 0, -g_th * c / den)
        ga = np.stack([2 * g_Q * a[0] + 2 * g_R * b[:, 0] + g_c * b[:, 1],
                       2 * g_Q * a[1] + 2 * g_R * b[:, 1] - g_c * b[:, 0]], 1)
        gb = np.stack([2 * g_S * b[:, 0] + 2 * g_R * a[0] - g_c * a[1] + g_d * e[:, 0],
                       2 * g_S * b[:, 1] + 2 * g_R * a[1] + g_c * a[0] + g_d * e[:, 1]], 1)
        ge = np.stack([2 * g_T * e[:, 0] + g_d * b[:, 0], 2 * g_T * e[:, 1] + g_d * b[:, 1]], 1)
        gq -= gb + ge
        gv[i1] += (gb - ga).sum(0)
        gv[i2] += (ge + ga).sum(0)
        gv_abs[i1] += np.abs(gb - ga).sum(0)
        gv_abs[i2] += np.abs(ge + ga).sum(0)
    return phi, psi, gq, gv, gv_abs


class Case:
    """inputs of one shape and dtype with everything the tests compare against, computed once on the CPU"""

    def __init__(self, name, B, P, n, seed):
        from pytorch_points_amd import green2d
        self.dt = DTYPES[name]
        self.B, self.P, self.n = B, P, n
        npdt = np.float32 if name == "fp32" else np.float64
        self.q, self.v, self.f = make(B, P, n, seed, npdt)
        rng = np.random.default_rng(seed)
        self.w_phi = rng.normal(size=(B, P, n)).astype(npdt)
        self.w_psi = rng.normal(size=(B, P, n)).astype(npdt)
        tq = torch.from_numpy(self.q).double().requires_grad_(True)
        tv = torch.from_numpy(self.v).double().requires_grad_(True)
        phi, psi, ext = green2d.composition(tq, tv, torch.from_numpy(self.f))
        loss = (phi * torch.from_numpy(self.w_phi).double()).sum() + (psi * torch.from_numpy(self.w_psi).double()).sum()
        gq, gv = torch.autograd.grad(loss, (tq, tv))
        self.phi, self.psi, self.ext = phi.detach().numpy(), psi.detach().numpy(), ext.numpy()
        self.gq, self.gv = gq.numpy(), gv.numpy()
        # the composition's own error on this cage, against longdouble: what 8x of is allowed (never below 8x FLOOR)
        err = {"out": FLOOR, "gq": FLOOR, "gv": FLOOR}
        self.gv_abs = np.zeros_like(self.gv)
        for b in range(B):
            r = longdouble_reference(self.q[b], self.v[b], self.f[b], self.w_phi[b], self.w_psi[b])
            err["out"] = max(err["out"], float(np.abs(self.phi[b] - r[0]).max()), float(np.abs(self.psi[b] - r[1]).max()))
            err["gq"] = max(err["gq"], float(np.abs(self.gq[b] - r[2]).max()))
            err["gv"] = max(err["gv"], float(np.abs(self.gv[b] - r[3]).max()))
            self.gv_abs[b] = r[4].astype(np.float64)
        self.tol = {key: 8 * val for key, val in err.items()}

    def tensors(self, device, grad=False):
        q = torch.from_numpy(self.q).to(device).requires_grad_(grad)
        v = torch.from_numpy(self.v).to(device).requires_grad_(grad)
        return q, v, torch.from_numpy(self.f).to(device)

    def weights(self, device):
        return torch.from_numpy(self.w_phi).to(device), torch.from_numpy(self.w_psi).to(device)


@functools.lru_cache(maxsize=None)
def case(name, B, P, n, seed=0):
    return Case(name, B, P, n, seed)


def gc2d(*args, **kw):
    from pytorch_points_amd.network.geo_operations import green_coordinates_2D
    return green_coordinates_2D(*args, **kw)


def check_forward(c, phi, psi, ext):
    got_phi, got_psi = phi.detach().cpu().numpy(), psi.detach().cpu().numpy()
    assert got_phi.dtype == c.q.dtype and got_psi.dtype == c.q.dtype and ext.dtype == torch.bool
    assert got_phi.shape == c.phi.shape and got_psi.shape == c.psi.shape and tuple(ext.shape) == (c.B, c.P, 1)
    assert np.isfinite(got_phi).all() and np.isfinite(got_psi).all()
    for name, got, ref in (("phi", got_phi, c.phi), ("psi", got_psi, c.psi)):
        if c.dt == torch.float32:
            # the fp64 composition rounded to fp32, within one fp32 ulp of the larger magnitude: one final rounding,
            # plus fp64 noise that can straddle a rounding boundary
            ref32 = ref.astype(np.float32)
            ulp = np.spacing(np.maximum(np.abs(got), np.abs(ref32)))
            worst = float((np.abs(got.astype(np.float64) - ref32.astype(np.float64)) / ulp).max())
            print("%s: worst %.3g fp32 ulp" % (name, worst))
            assert worst <= 1.0, name
        else:
            worst = float(np.abs(got - ref).max())
            print("%s: worst %.3g, allowed %.3g" % (name, worst, c.tol["out"]))
            assert worst <= c.tol["out"], name
    # the flag: where the fp64 sum is not within the composition's error of 0.5 it must agree
    clear = np.abs(c.phi.sum(-1, keepdims=True) - 0.5) > c.tol["out"] * c.n
    assert np.array_equal(ext.cpu().numpy()[clear], c.ext[clear])


# ---------------------------------------------------------------------------------------------------------- forward
SHAPES = {
    "triangle_p1": (1, 1, 3),
    "p64": (1, 64, 7),
    "p65": (1, 65, 7),
    "p130": (1, 130, 7),
    "f64": (1, 65, 64),
    "f65": (1, 65, 65),
    "f129": (1, 65, 129),
    "b3": (3, 130, 12),
}


@pytest.mark.parametrize("name", sorted(DTYPES))
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_forward_matches_the_composition(cuda, name, shape):
    c = case(name, *SHAPES[shape])
    check_forward(c, *gc2d(*c.tensors(cuda)))


@pytest.mark.parametrize("name", sorted(DTYPES))
@pytest.mark.parametrize("extra", [0, 1])
def test_forward_at_the_last_cage_that_fits_lds_and_the_first_that_does_not(cuda, name, extra):
    c = case(name, 1, 130, lds_vertices(DTYPES[name]) + extra)
    check_forward(c, *gc2d(*c.tensors(cuda)))


@pytest.mark.parametrize("name", sorted(DTYPES))
@pytest.mark.parametrize("chunked", [False, True])
def test_a_row_does_not_depend_on_its_company(cuda, name, chunked):
    """alone, and as member 0, 63, 64 and 129 of 130 queries in element 1 of a batch of 3: the same bits"""
    n = lds_vertices(DTYPES[name]) + 1 if chunked else 12
    c = case(name, 3, 130, n)
    q, v, f = c.tensors(cuda)
    phi, psi, ext = gc2d(q, v, f)
    for member in (0, 63, 64, 129):
        a_phi, a_psi, a_ext = gc2d(q[1:2, member:member + 1], v[1:2], f[1:2])
        assert torch.equal(a_phi[0, 0], phi[1, member]) and torch.equal(a_psi[0, 0], psi[1, member])
        assert bool(a_ext[0, 0, 0]) == bool(ext[1, member, 0])
    # nor on the batch: element 1 twice, as batch-expanded views (one edge list read for both elements)
    expanded = gc2d(q[1:2].expand(2, -1, -1), v[1:2].expand(2, -1, -1), f[1:2].expand(2, -1, -1))
    assert torch.equal(expanded[0][1], phi[1]) and torch.equal(expanded[1][0], psi[1])


def test_reversed_edges_with_the_original_normals(cuda):
    for name in sorted(DTYPES):
        c = case(name, 3, 130, 12)
        q, v, f = c.tensors(cuda, grad=True)
        a = v.detach()[torch.arange(3, device=cuda)[:, None], f[:, :, 1]] - v.detach()[torch.arange(3, device=cuda)[:, None], f[:, :, 0]]
        normals = torch.stack([a[:, :, 1], -a[:, :, 0]], -1)
        w_phi, w_psi = c.weights(cuda)
        ref = gc2d(q, v, f)
        ref_g = torch.autograd.grad((ref[0] * w_phi).sum() + (ref[1] * w_psi).sum(), (q, v))
        mixed = f.clone()
        mixed[:, ::2] = mixed[:, ::2].flip(-1)                               # every other edge reversed
        got = gc2d(q, v, mixed, edge_normals=normals)
        got_g = torch.autograd.grad((got[0] * w_phi).sum() + (got[1] * w_psi).sum(), (q, v))
        for x, y in zip(ref + ref_g, got + got_g):
            assert torch.equal(x, y)
        # without the normals the reversed edges are another cage
        assert not torch.equal(gc2d(q, v, mixed)[0], ref[0])


# --------------------------------------------------------------------------------------------------------- backward
def backward(c, device):
    q, v, f = c.tensors(device, grad=True)
    w_phi, w_psi = c.weights(device)
    phi, psi, _ = gc2d(q, v, f)
    return torch.autograd.grad((phi * w_phi).sum() + (psi * w_psi).sum(), (q, v))


def backward_shapes(name):
    dt = DTYPES[name]
    size = 4 if name == "fp32" else 8
    fits = (160 * 1024 - 64 * 65 * size) // (65 * size)       # the backward stages dL/dphi in the element type
    return {"b3": (3, 130, 12), "p1": (1, 1, 3), "f129": (1, 65, 129), "forward_chunked": (1, 65, lds_vertices(dt) + 1),
            "lds": (1, 65, fits), "global": (1, 65, fits + 1)}


@pytest.mark.parametrize("name", sorted(DTYPES))
@pytest.mark.parametrize("shape", ["b3", "p1", "f129", "forward_chunked", "lds", "global"])
def test_backward_matches_autograd_through_the_composition(cuda, name, shape):
    c = case(name, *backward_shapes(name)[shape])
    gq, gv = backward(c, cuda)
    again = backward(c, cuda)
    assert torch.equal(gq, again[0]) and torch.equal(gv, again[1])          # bit-identical runs
    gq, gv = gq.cpu().numpy(), gv.cpu().numpy()
    assert gq.dtype == c.q.dtype and gv.dtype == c.q.dtype
    assert np.isfinite(gq).all() and np.isfinite(gv).all()
    if c.dt == torch.float64:
        allowed_q = c.tol["gq"]
        # dL/dvertices: the composition's own error, plus the kernel's sums in another order: six levels of the wave's
        # butterfly, the workgroup slices and the (two) edge ends of a vertex, each rounding at most 2^-53 of the sum
        # of the terms' magnitudes
        tiles = (c.P + 63) // 64
        allowed_v = c.tol["gv"] + (6 + tiles + 2) * 2.0 ** -53 * c.gv_abs
    else:
        # fp64 arithmetic on fp32 data, then dL/dquery is rounded once.  dL/dvertices: every workgroup's wave sum is
        # rounded to fp32 (together at most 2^-24 of the sum of the terms' magnitudes), then the slices (tiles - 1
        # additions) and the two edge ends of a vertex (one) are added in fp32, each rounding at most 2^-24 of that
        # sum: tiles + 1 roundings, and one to spare for the second-order terms
        tiles = (c.P + 63) // 64
        allowed_q = c.tol["gq"] + np.spacing(np.maximum(np.abs(gq), np.abs(c.gq.astype(np.float32)))).astype(np.float64)
        allowed_v = c.tol["gv"] + (tiles + 2) * EPS32 * c.gv_abs
    print("dL/dquery worst %.3g (allowed %s), dL/dvertices worst %.3g (allowed >= %.3g)" % (
        np.abs(gq - c.gq).max(), np.max(allowed_q), np.abs(gv - c.gv).max(), np.min(allowed_v)))
    assert (np.abs(gq.astype(np.float64) - c.gq) <= allowed_q).all()
    assert (np.abs(gv.astype(np.float64) - c.gv) <= allowed_v).all()


def test_bit_reproducible_under_deterministic_algorithms(cuda):
    c = case("fp32", 3, 130, 12)
    ref_out = gc2d(*c.tensors(cuda))
    ref_g = backward(c, cuda)
    torch.use_deterministic_algorithms(True)
    try:
        out = gc2d(*c.tensors(cuda))
        g = backward(c, cuda)
    finally:
        torch.use_deterministic_algorithms(False)
    for x, y in zip(ref_out + ref_g, out + g):
        assert torch.equal(x, y)


def test_only_one_cotangent_and_only_one_input(cuda):
    c = case("fp64", 3, 130, 12)
    q, v, f = c.tensors(cuda, grad=True)
    w_phi, w_psi = c.weights(cuda)
    phi, psi, _ = gc2d(q, v, f)
    both = torch.autograd.grad((phi * w_phi).sum() + (psi * w_psi).sum(), (q, v), retain_graph=True)
    only_phi = torch.autograd.grad((phi * w_phi).sum(), (q, v), retain_graph=True)
    only_psi = torch.autograd.grad((psi * w_psi).sum(), (q, v), retain_graph=True)
    for a, b, s in zip(only_phi, only_psi, both):
        assert float((a + b - s).abs().max()) <= 64 * 2.0 ** -52 * float(s.abs().max())
    (gq,) = torch.autograd.grad((phi * w_phi).sum() + (psi * w_psi).sum(), (q,))
    assert torch.equal(gq, both[0])


# ------------------------------------------------------------------------------------------------ graphs and streams
def test_under_graph_capture(cuda):
    from pytorch_points_amd import _lib
    c = case("fp32", 3, 130, 12)
    other = case("fp32", 3, 130, 12, 5)
    q, v, f = c.tensors(cuda, grad=True)
    w_phi, w_psi = c.weights(cuda)

    def step():
        phi, psi, ext = gc2d(q, v, f)
        gq, gv = torch.autograd.grad((phi * w_phi).sum() + (psi * w_psi).sum(), (q, v))
        return phi, psi, ext, gq, gv

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    before = {k: t.data_ptr() for k, t in _lib._WS.items()}
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step()
    assert {k: t.data_ptr() for k, t in _lib._WS.items()} == before          # the graph owns its scratch
    for src in (other, c):
        with torch.no_grad():
            q.copy_(torch.from_numpy(src.q))
            v.copy_(torch.from_numpy(src.v))
        graph.replay()
        torch.cuda.synchronize()
        got = [o.clone() for o in outs]
        for x, y in zip(got, step()):
            assert torch.equal(x, y)
    check_forward(c, *got[:3])


def test_on_a_side_stream(cuda):
    from pytorch_points_amd import _lib
    c = case("fp64", 3, 130, 12)
    ref = gc2d(*c.tensors(cuda)) + backward(c, cuda)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = gc2d(*c.tensors(cuda)) + backward(c, cuda)
    side.synchronize()
    for x, y in zip(ref, got):
        assert torch.equal(x, y)
    assert any(key[2] == "gc2d" and key[1] == side.cuda_stream for key in _lib._WS)      # scratch of its own


# ------------------------------------------------------------------------------------------------- NaN rows, no fault
@pytest.mark.parametrize("name", sorted(DTYPES))
def test_bad_index_and_non_finite_inputs_give_nan_rows(cuda, name):
    c = case(name, 3, 130, 12)
    q, v, f = c.tensors(cuda)
    clean = gc2d(q, v, f)
    bad = f.clone()
    bad[1, 5, 0] = 12                                                        # out of range, element 1 only
    bad[2, 0, 1] = -1
    q2 = q.clone().requires_grad_(True)
    v2 = v.clone().requires_grad_(True)
    phi, psi, ext = gc2d(q2, v2, bad)
    assert torch.equal(phi[0], clean[0][0]) and torch.equal(psi[0], clean[1][0]) and torch.equal(ext[0], clean[2][0])
    assert torch.isnan(phi[1:]).all() and torch.isnan(psi[1:]).all() and not ext[1:].any()
    gq, gv = torch.autograd.grad(phi.sum() + psi.sum(), (q2, v2))
    assert torch.isfinite(gq[0]).all() and torch.isfinite(gv[0]).all()
    assert torch.isnan(gq[1:]).all() and torch.isnan(gv[1:]).all()
    # a non-finite query: its row only; a non-finite vertex: every row of its batch element
    q3 = q.clone()
    q3[0, 3, 1] = float("nan")
    q3[0, 70, 0] = float("inf")
    v3 = v.clone()
    v3[2, 4, 0] = float("inf")
    phi, psi, ext = gc2d(q3, v3, f)
    rows = torch.ones(130, dtype=torch.bool, device=cuda)
    rows[3] = rows[70] = False
    assert torch.equal(phi[0, rows], clean[0][0, rows]) and torch.equal(psi[0, rows], clean[1][0, rows])
    assert torch.isnan(phi[0, ~rows]).all() and torch.isnan(psi[0, ~rows]).all() and not ext[0, ~rows].any()
    assert torch.equal(phi[1], clean[0][1]) and torch.equal(psi[1], clean[1][1])
    assert torch.isnan(phi[2]).all() and torch.isnan(psi[2]).all() and not ext[2].any()
    torch.cuda.synchronize()


def test_half_inputs_take_the_composition_on_the_gpu(cuda):
    c = case("fp32", 1, 65, 7)
    q, v, f = c.tensors(cuda)
    phi, psi, ext = gc2d(q.half(), v.half(), f)
    assert phi.dtype == torch.float16 and phi.is_cuda and torch.isfinite(phi).all()
