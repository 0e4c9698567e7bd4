"""CPU tests (no GPU) of green_coordinates_2D: the drop-in names import, the C ABI declares and exports the pp_gc2d_*
entry points, and the in-tree torch composition (the path of CPU tensors and of dtypes the kernels do not serve) is
checked against the defining boundary integrals by quadrature, against the coordinates' own identities (partition of
unity, reproduction, conformality of the deformation) and at the boundary and degenerate rules of the contract
(DESIGN.md "Green coordinates, 2-D").  The reference gives nothing to compare with: its function is an empty stub."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from pytorch_points_amd import _build, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["pp_gc2d_workspace_bytes", "pp_gc2d_forward_f32", "pp_gc2d_forward_f64", "pp_gc2d_backward_f32",
           "pp_gc2d_backward_f64"]

# DESIGN.md "Green coordinates, 2-D", accuracy: the largest error of the fp64 composition against a numpy.longdouble
# evaluation of the same formulas over the cages and queries of this file was 6.1e-16 (coordinates of magnitude <= 1,
# cages of diameter ~2; a handful of fp64 roundings through ln, atan2 and the cancelling sums).  The identity tests
# allow 8x that per unit of what they sum: see tol().
COMPOSITION_ERROR = 6.1e-16


def tol(scale=1.0):
    return 8 * COMPOSITION_ERROR * scale


def polygon(n, seed):
    """a fixed-seed star-shaped counter-clockwise n-gon around the origin, radii in [0.7, 1.3]"""
    rng = np.random.default_rng(seed)
    ang = np.sort(rng.uniform(0, 2 * np.pi, n))
    ang = ang + np.linspace(0, 0.3, n)                                   # keeps neighbouring angles apart
    rad = rng.uniform(0.7, 1.3, n)
    v = np.stack([rad * np.cos(ang), rad * np.sin(ang)], 1)
    f = np.stack([np.arange(n), (np.arange(n) + 1) % n], 1)
    return v, f


def boundary_distance(q, v, f):
    a, b = v[f[:, 0]], v[f[:, 1]]
    t = np.clip(((q[:, None] - a) * (b - a)).sum(-1) / ((b - a) ** 2).sum(-1), 0, 1)
    return np.linalg.norm(q[:, None] - (a + t[..., None] * (b - a)), axis=-1).min(1)


def inside(q, v, f):
    """winding number != 0, by the angles the edges subtend"""
    b, e = v[f[:, 0]] - q[:, None], v[f[:, 1]] - q[:, None]
    ang = np.arctan2(b[..., 0] * e[..., 1] - b[..., 1] * e[..., 0], (b * e).sum(-1)).sum(1)
    return np.abs(ang) > np.pi


def queries(v, f, n, seed, margin=0.05):
    """n interior and n exterior queries at least ``margin`` from the boundary"""
    rng = np.random.default_rng(seed)
    q = rng.uniform(-2.0, 2.0, (40 * n, 2))
    q = q[boundary_distance(q, v, f) >= margin]
    ins = inside(q, v, f)
    qi, qe = q[ins][:n], q[~ins][:n]
    assert len(qi) == n and len(qe) == n
    return qi, qe


def normals_of(v, f):
    a = v[f[:, 1]] - v[f[:, 0]]
    return np.stack([a[:, 1], -a[:, 0]], 1) / np.linalg.norm(a, axis=1, keepdims=True)


def run(q, v, f, **kw):
    from pytorch_points_amd import green2d
    phi, psi, ext = green2d.composition(torch.from_numpy(q)[None], torch.from_numpy(v)[None],
                                        torch.from_numpy(f)[None], **kw)
    return phi[0].numpy(), psi[0].numpy(), ext[0, :, 0].numpy()


def evaluate_longdouble(q, v, f):
    """the contract's formulas in numpy.longdouble (queries off the boundary): (phi, psi)"""
    ld = np.longdouble
    q, v = q.astype(ld), v.astype(ld)
    pi = ld(4) * np.arctan(ld(1))
    phi = np.zeros((len(q), len(v)), ld)
    psi = np.zeros((len(q), len(f)), ld)
    for j, (i1, i2) in enumerate(f):
        a = v[i2] - v[i1]
        b, e = v[i1] - q, v[i2] - q
        Q, S, T = (a * a).sum(), (b * b).sum(-1), (e * e).sum(-1)
        R = 2 * (b * a).sum(-1)
        c = a[0] * b[:, 1] - a[1] * b[:, 0]
        th = np.arctan2(c, (b * e).sum(-1))
        u = 1 + R / (2 * Q)
        big_l = u * np.log(T) + (1 - u) * np.log(S)
        g = c * (np.log(T) - np.log(S)) / (2 * Q)
        h = th / 2
        psi[:, j] = -np.sqrt(Q) / (4 * pi) * (2 * c * th / Q + big_l - 2)
        phi[:, i1] += (g - h * (2 + R / Q)) / (2 * pi)
        phi[:, i2] += (h * R / Q - g) / (2 * pi)
    return phi, psi


# ------------------------------------------------------------------------------------------------ 1. names and ABI
def test_drop_in_names_import():
    from pytorch_points_amd.network.geo_operations import deform_with_green_coordinates_2D, green_coordinates_2D
    assert callable(green_coordinates_2D) and callable(deform_with_green_coordinates_2D)
    import pytorch_points_amd
    pytorch_points_amd.install_as_pytorch_points()
    from pytorch_points.network.geo_operations import green_coordinates_2D as through_install
    assert through_install is green_coordinates_2D


def test_header_declares_and_library_exports_gc2d():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pp_hip.h")).read(), flags=re.S)
    _build.build()
    handle = ctypes.CDLL(_build.LIB)
    for s in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, text), s
        assert s in _lib.SIGNATURES, s
        assert hasattr(handle, s), s


def test_workspace_query_and_argument_checks_are_host_only():
    L = _lib.lib()
    assert L.pp_gc2d_workspace_bytes(8, 16384, 64, 4) == 8 * 256 * 64 * 4 * 4
    assert L.pp_gc2d_workspace_bytes(2, 65, 10, 8) == 2 * 2 * 10 * 4 * 8
    assert L.pp_gc2d_workspace_bytes(0, 10, 10, 4) == 0
    assert L.pp_gc2d_workspace_bytes(1, 10, 10, 2) == 0
    none9 = [None] * 5
    assert L.pp_gc2d_forward_f32(None, None, None, 0, *none9, -1, 4, 4, 4, None) != 0
    assert L.pp_gc2d_forward_f32(None, None, None, 0, *none9, 2, 0, 4, 4, None) == 0
    assert L.pp_gc2d_forward_f64(None, None, None, -1, *none9, 1, 1, 4, 4, None) != 0
    assert L.pp_gc2d_forward_f64(None, None, None, 0, *none9, 1, 1, 4, 4, None) != 0          # null pointers
    assert L.pp_gc2d_backward_f32(None, None, None, 0, None, None, None, None, None, None, 1, 4, 4, 4, None, 0,
                                  None) != 0
    assert L.pp_gc2d_backward_f64(None, None, None, 0, None, None, None, None, None, None, 1, -4, 4, 4, None, 0,
                                  None) != 0
    # a P whose tile count would overflow an int: refused before any arithmetic on it
    big = 2 ** 31 - 1
    assert L.pp_gc2d_workspace_bytes(1, big, 10, 4) == 0
    for fwd in (L.pp_gc2d_forward_f32, L.pp_gc2d_forward_f64):
        assert fwd(None, None, None, 0, *none9, 1, big, 4, 4, None) != 0
    for bwd in (L.pp_gc2d_backward_f32, L.pp_gc2d_backward_f64):
        assert bwd(None, None, None, 0, *[None] * 6, 1, big, 4, 4, None, 0, None) != 0


def test_lds_vertex_counts_match_the_kernel_formula():
    """green2d.LDS_VERTICES mirrors chunk_cap of csrc/green2d.hip: (160 KiB - the 64 x 65 psi tile) / (65 x 8)"""
    from pytorch_points_amd import green2d
    for dt, size in ((torch.float32, 4), (torch.float64, 8)):
        assert green2d.LDS_VERTICES[dt] == (160 * 1024 - 64 * 65 * size) // (65 * 8)


# ------------------------------------------------------------------------------------------------ 2. quadrature
def quadrature(q, v, f, m):
    """phi_i = the integral of dG/dn over the two edges at vertex i against its hat function, psi_j = -the integral
    of G over edge j, G = ln|xi - eta| / (2 pi), by the midpoint rule with m points per edge"""
    t = (np.arange(m) + 0.5) / m
    n = normals_of(v, f)
    phi = np.zeros((len(q), len(v)))
    psi = np.zeros((len(q), len(f)))
    for j, (i1, i2) in enumerate(f):
        length = np.linalg.norm(v[i2] - v[i1])
        xi = v[i1] + t[:, None] * (v[i2] - v[i1])                        # (m,2)
        d = xi[None] - q[:, None]                                        # (P,m,2)
        r2 = (d * d).sum(-1)
        dgdn = (d * n[j]).sum(-1) / (2 * np.pi * r2)
        psi[:, j] = -(np.log(r2) / (4 * np.pi)).mean(1) * length
        phi[:, i1] += (dgdn * (1 - t)).mean(1) * length
        phi[:, i2] += (dgdn * t).mean(1) * length
    return phi, psi


def test_composition_matches_quadrature_of_the_defining_integrals():
    v, f = polygon(7, 1)
    qi, qe = queries(v, f, 6, 2)
    q = np.concatenate([qi, qe])
    phi, psi, _ = run(q, v, f)
    coarse, fine = quadrature(q, v, f, 20000), quadrature(q, v, f, 40000)
    own = max(np.abs(coarse[0] - fine[0]).max(), np.abs(coarse[1] - fine[1]).max())      # the quadrature's own error
    err = max(np.abs(phi - fine[0]).max(), np.abs(psi - fine[1]).max())
    print("quadrature: own error %.3g, composition against it %.3g" % (own, err))
    assert own < 1e-8
    assert err <= 10 * own


# ------------------------------------------------------------------------------------------------ 3. identities
def test_recorded_composition_error_against_longdouble():
    """the figure the identity tolerances are derived from (COMPOSITION_ERROR) still holds"""
    worst = 0.0
    for n, seed in ((7, 1), (5, 3), (12, 4)):
        v, f = polygon(n, seed)
        q = np.concatenate(queries(v, f, 8, seed + 10))
        phi, psi, _ = run(q, v, f)
        rphi, rpsi = evaluate_longdouble(q, v, f)
        worst = max(worst, float(np.abs(phi - rphi).max()), float(np.abs(psi - rpsi).max()))
    print("fp64 composition against longdouble: %.3g" % worst)
    assert worst <= COMPOSITION_ERROR


@pytest.mark.parametrize("n,seed", [(7, 1), (12, 4)])
def test_partition_of_unity_reproduction_and_exterior_flag(n, seed):
    v, f = polygon(n, seed)
    qi, qe = queries(v, f, 8, seed + 10)
    phi, psi, ext = run(qi, v, f)
    # N + F terms of magnitude <= ~1 (coordinates times cage coordinates <= 1.3), each within the composition's error
    assert np.abs(phi.sum(1) - 1).max() <= tol(n)
    assert np.abs(phi @ v + psi @ normals_of(v, f) - qi).max() <= tol(2 * n * 1.3)
    assert not ext.any()
    phi, psi, ext = run(qe, v, f)
    assert np.abs(phi.sum(1)).max() <= tol(n)
    assert ext.all()


# ------------------------------------------------------------------------------------------------ 4. conformality
def test_deformation_by_a_similarity_moves_the_queries_by_it():
    from pytorch_points_amd import green2d
    v, f = polygon(7, 1)
    qi, _ = queries(v, f, 8, 11)
    ang, scale, shift = 0.7, 1.8, np.array([0.4, -2.5])
    rot = np.array([[np.cos(ang), -np.sin(ang)], [np.sin(ang), np.cos(ang)]])
    move = lambda x: scale * x @ rot.T + shift
    tq, tv, tf = torch.from_numpy(qi)[None], torch.from_numpy(v)[None], torch.from_numpy(f)[None]
    phi, psi, _ = green2d.composition(tq, tv, tf)
    out = green2d.deform_with_green_coordinates_2D(phi, psi, tv, torch.from_numpy(move(v))[None], tf)[0].numpy()
    # 2n terms, the deformed cage within |shift| + scale * 1.3 of the origin
    assert np.abs(out - move(qi)).max() <= tol(2 * 7 * (np.abs(shift).max() + scale * 1.3))
    same = green2d.deform_with_green_coordinates_2D(phi, psi, tv, tv, tf)[0].numpy()
    assert np.abs(same - qi).max() <= tol(2 * 7 * 1.3)
    # differentiable
    nv = torch.from_numpy(move(v))[None].requires_grad_(True)
    green2d.deform_with_green_coordinates_2D(phi, psi, tv, nv, tf).sum().backward()
    assert torch.isfinite(nv.grad).all() and nv.grad.abs().sum() > 0


# ------------------------------------------------------------------------------------------------ 5. a hole
def square_with_hole():
    outer = np.array([[-1.0, -1.0], [1.0, -1.0], [1.0, 1.0], [-1.0, 1.0]])
    hole = 0.4 * outer[::-1]                                             # clockwise
    v = np.concatenate([outer, hole])
    f = np.array([[0, 1], [1, 2], [2, 3], [3, 0], [4, 5], [5, 6], [6, 7], [7, 4]])
    return v, f


def test_square_with_a_clockwise_hole():
    v, f = square_with_hole()
    annulus = np.array([[0.7, 0.0], [-0.6, 0.65], [0.0, -0.8], [0.9, 0.9], [0.45, 0.1]])
    in_hole = np.array([[0.0, 0.0], [0.3, -0.2], [-0.35, 0.35]])
    phi, psi, ext = run(annulus, v, f)
    assert np.abs(phi.sum(1) - 1).max() <= tol(8)
    assert np.abs(phi @ v + psi @ normals_of(v, f) - annulus).max() <= tol(16)
    assert not ext.any()
    phi, psi, ext = run(in_hole, v, f)
    assert np.abs(phi.sum(1)).max() <= tol(8)
    assert ext.all()
    # every edge reversed, the original normals given: the same outputs
    q = np.concatenate([annulus, in_hole])
    ref = run(q, v, f)
    got = run(q, v, f[:, ::-1].copy(), edge_normals=torch.from_numpy(normals_of(v, f))[None])
    for a, b in zip(ref, got):
        assert np.array_equal(a, b)
    # normals that agree with the edges change nothing
    got = run(q, v, f, edge_normals=torch.from_numpy(normals_of(v, f))[None])
    for a, b in zip(ref, got):
        assert np.array_equal(a, b)


# ------------------------------------------------------------------------------------------------ 6. rules
def test_boundary_and_degenerate_rules_give_finite_rows_and_gradients():
    from pytorch_points_amd import green2d
    # a square (coordinates exact in binary, so "on an edge" is exact too) plus vertex 4 = vertex 2: edge (2,4) has
    # length 0
    v = np.array([[-1.0, -1.0], [1.0, -1.0], [1.0, 1.0], [-1.0, 1.0], [1.0, 1.0]])
    f = np.array([[0, 1], [1, 2], [2, 3], [3, 0], [2, 4]])
    q = np.array([[1.0, 1.0], [1.0, 0.25], [1.0, 2.5], [0.05, 0.02]])    # a vertex, on an edge, on its line, inside
    tq = torch.from_numpy(q)[None].requires_grad_(True)
    tv = torch.from_numpy(v)[None].requires_grad_(True)
    phi, psi, ext = green2d.composition(tq, tv, torch.from_numpy(f)[None])
    assert torch.isfinite(phi).all() and torch.isfinite(psi).all()
    assert (psi[0, :, 4] == 0).all() and (phi[0, :, 4] == 0).all()       # the zero-length edge and its own vertex
    sums = phi[0].detach().sum(1).numpy()
    assert abs(sums[0] - 0.25) <= tol(5)                                 # on a right-angled vertex: the angle inside
    assert abs(sums[1] - 0.5) <= tol(5)                                  # on an edge: half the full angle
    assert abs(sums[2]) <= tol(5)                                        # on the edge's line, outside
    assert abs(sums[3] - 1) <= tol(5)
    assert ext[0, :, 0].tolist() == [True, False, True, False]
    w = torch.from_numpy(np.random.default_rng(0).normal(size=(4, 10)))
    (torch.cat([phi[0], psi[0]], 1) * w).sum().backward()
    assert torch.isfinite(tq.grad).all() and torch.isfinite(tv.grad).all()
    assert tq.grad.abs().sum() > 0 and tv.grad.abs().sum() > 0


def test_bad_index_and_non_finite_inputs_give_nan_rows():
    from pytorch_points_amd import green2d
    v, f = polygon(5, 3)
    q = np.array([[0.0, 0.1], [1.9, 0.3]])
    tq = torch.from_numpy(np.stack([q, q]))
    tv = torch.from_numpy(np.stack([v, v]))
    tf = torch.from_numpy(np.stack([f, f])).clone()
    tf[1, 3, 1] = 5                                                      # out of range, second batch element only
    phi, psi, ext = green2d.composition(tq, tv, tf)
    assert torch.isfinite(phi[0]).all() and torch.isfinite(psi[0]).all() and ext[0, :, 0].tolist() == [False, True]
    assert torch.isnan(phi[1]).all() and torch.isnan(psi[1]).all() and not ext[1].any()
    tf[1, 3, 1] = -1
    assert torch.isnan(green2d.composition(tq, tv, tf)[0][1]).all()
    tq2 = tq[:1].clone()
    tq2[0, 1, 0] = float("nan")
    phi, psi, ext = green2d.composition(tq2, tv[:1], tf[:1])
    assert torch.isfinite(phi[0, 0]).all() and torch.isfinite(psi[0, 0]).all()
    assert torch.isnan(phi[0, 1]).all() and torch.isnan(psi[0, 1]).all() and not ext[0, 1, 0]
    tv2 = tv[:1].clone()
    tv2[0, 2, 1] = float("inf")
    phi, psi, ext = green2d.composition(tq[:1], tv2, tf[:1])
    assert torch.isnan(phi).all() and torch.isnan(psi).all() and not ext.any()


def test_empty_inputs_and_other_dtypes():
    from pytorch_points_amd import green2d
    v, f = polygon(5, 3)
    tq, tv, tf = torch.zeros(1, 3, 2), torch.from_numpy(v)[None].float(), torch.from_numpy(f)[None]
    phi, psi, ext = green2d.green_coordinates_2D(tq[:, :0], tv, tf)
    assert phi.shape == (1, 0, 5) and psi.shape == (1, 0, 5) and ext.shape == (1, 0, 1)
    phi, psi, ext = green2d.green_coordinates_2D(tq, tv, tf[:, :0])
    assert phi.shape == (1, 3, 5) and psi.shape == (1, 3, 0) and (phi == 0).all() and ext.all()
    phi, psi, ext = green2d.green_coordinates_2D(tq.half(), tv.half(), tf.int(), verbose=True)
    assert phi.dtype == torch.float16 and psi.dtype == torch.float16 and ext.dtype == torch.bool
    assert abs(float(phi[0, 0].float().sum()) - 1) < 5e-3
    ref = green2d.composition(tq.double(), tv.half().double(), tf)
    assert torch.equal(phi, ref[0].half())                               # fp64 pairs, one rounding


def test_shape_dtype_and_device_errors():
    from pytorch_points_amd.network.geo_operations import green_coordinates_2D as gc2d
    q = torch.zeros(2, 4, 2)
    v = torch.zeros(2, 6, 2)
    f = torch.zeros(2, 6, 2, dtype=torch.long)
    with pytest.raises(RuntimeError, match="query must have shape"):
        gc2d(torch.zeros(2, 4, 3), v, f)
    with pytest.raises(RuntimeError, match="vertices must have shape"):
        gc2d(q, torch.zeros(2, 6), f)
    with pytest.raises(RuntimeError, match="faces must have shape"):
        gc2d(q, v, torch.zeros(2, 6, 3, dtype=torch.long))
    with pytest.raises(RuntimeError, match="same batch size"):
        gc2d(q, torch.zeros(3, 6, 2), f)
    with pytest.raises(RuntimeError, match="one dtype"):
        gc2d(q, v.double(), f)
    with pytest.raises(RuntimeError, match="floating tensors"):
        gc2d(q.long(), v.long(), f)
    with pytest.raises(RuntimeError, match="integer tensor"):
        gc2d(q, v, f.float())
    with pytest.raises(RuntimeError, match="edge_normals must have shape"):
        gc2d(q, v, f, edge_normals=torch.zeros(2, 5, 2))
    with pytest.raises(RuntimeError, match="dtype and device of query"):
        gc2d(q, v, f, edge_normals=torch.zeros(2, 6, 2, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="one device"):
        gc2d(q, v, f.to("meta"))


# ------------------------------------------------------------------------------------------------ 7. gradcheck
def test_gradcheck_of_the_composition():
    from pytorch_points_amd import green2d
    v, f = polygon(5, 3)
    qi, qe = queries(v, f, 2, 13)
    q = torch.from_numpy(np.concatenate([qi, qe[:1]]))[None].requires_grad_(True)         # P = 3
    tv = torch.from_numpy(v)[None].requires_grad_(True)
    tf = torch.from_numpy(f)[None]
    assert torch.autograd.gradcheck(lambda a, b: green2d.composition(a, b, tf)[:2], (q, tv))
    en = torch.from_numpy(normals_of(v, f))[None]
    rev = torch.from_numpy(f[:, ::-1].copy())[None]
    assert torch.autograd.gradcheck(lambda a, b: green2d.composition(a, b, rev, en)[:2], (q, tv))
