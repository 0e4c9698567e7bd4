"""CPU tests (no GPU) of the 2-D mean_value_coordinates: the drop-in names import, the C ABI declares, binds and
exports the pp_mvc2d_* entry points, and the in-tree torch composition (the path of CPU tensors and of dtypes the
kernels do not serve) matches the reference's own fp64 results recorded in tests/golden/mvc2d_*.npz
(tools/gen_mvc2d_golden.py)."""
import ctypes
import glob
import os
import re

import numpy as np
import pytest
import torch

from pytorch_points_amd import _build, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "mvc2d_*.npz")))
SYMBOLS = ["pp_mvc2d_workspace_bytes", "pp_mvc2d_forward_f32", "pp_mvc2d_forward_f64", "pp_mvc2d_backward_f32",
           "pp_mvc2d_backward_f64"]
INTERIOR, EXTERIOR, FAR10, FAR100, VERTEX, EDGE, EXTENSION, CENTROID, NEAR_EDGE, NEAR_VERTEX = range(10)


def test_drop_in_names_import():
    import pytorch_points_amd
    pytorch_points_amd.install_as_pytorch_points()
    from pytorch_points.network.geo_operations import mean_value_coordinates
    from pytorch_points.network.operations import normalize, sqrNorm, dot_product, cross_product_2D
    assert all(callable(f) for f in (mean_value_coordinates, normalize, sqrNorm, dot_product, cross_product_2D))


def test_helpers_compute_what_their_names_say():
    from pytorch_points_amd.network.operations import normalize, sqrNorm, dot_product, cross_product_2D
    a = torch.tensor([[3.0, 4.0], [0.0, 0.0]], dtype=torch.float64)
    b = torch.tensor([[1.0, 2.0], [5.0, 6.0]], dtype=torch.float64)
    assert torch.equal(normalize(a), torch.tensor([[0.6, 0.8], [0.0, 0.0]], dtype=torch.float64))
    assert torch.equal(normalize(a, dim=0)[0], torch.tensor([1.0, 1.0], dtype=torch.float64))
    assert torch.equal(sqrNorm(a), torch.tensor([25.0, 0.0], dtype=torch.float64))
    assert sqrNorm(a, dim=1, keepdim=True).shape == (2, 1)
    assert torch.equal(dot_product(a, b), torch.tensor([11.0, 0.0], dtype=torch.float64))
    assert dot_product(a, b, dim=0, keepdim=True).shape == (1, 2)
    assert torch.equal(cross_product_2D(a, b, dim=1), torch.tensor([2.0, 0.0], dtype=torch.float64))
    x = torch.randn(3, 2, 4, 5)
    assert cross_product_2D(x, x.flip(1)).shape == (3, 4, 5)
    with pytest.raises(AssertionError):
        cross_product_2D(torch.zeros(2, 3), torch.zeros(2, 3))


def test_header_declares_and_library_exports_mvc2d():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pp_hip.h")).read(), flags=re.S)
    _build.build()
    handle = ctypes.CDLL(_build.LIB)
    for s in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, text), s
        assert s in _lib.SIGNATURES, s
        assert hasattr(handle, s), s


def test_workspace_query_and_argument_checks_are_host_only():
    L = _lib.lib()
    assert L.pp_mvc2d_workspace_bytes(8, 16384, 64, 4) == 8 * 256 * 64 * 2 * 4
    assert L.pp_mvc2d_workspace_bytes(2, 65, 10, 8) == 2 * 2 * 10 * 2 * 8
    assert L.pp_mvc2d_workspace_bytes(0, 10, 10, 4) == 0
    assert L.pp_mvc2d_workspace_bytes(1, 10, 10, 2) == 0
    none6, none9 = [None] * 6, [None] * 9
    for fwd in (L.pp_mvc2d_forward_f32, L.pp_mvc2d_forward_f64):
        assert fwd(*none6, -1, 4, 4, None) != 0
        assert fwd(*none6, 1, -4, 4, None) != 0
        assert fwd(*none6, 1, 4, -4, None) != 0
        assert fwd(*none6, 2, 0, 4, None) == 0          # zero sizes: success, nothing touched
        assert fwd(*none6, 2, 4, 0, None) == 0
        assert fwd(*none6, 0, 4, 4, None) == 0
        assert fwd(*none6, 1, 4, 4, None) != 0          # null pointers with work to do
    for bwd in (L.pp_mvc2d_backward_f32, L.pp_mvc2d_backward_f64):
        assert bwd(*none9, -1, 4, 4, None, 0, None) != 0
        assert bwd(*none9, 1, 4, -1, None, 0, None) != 0
        assert bwd(*none9, 0, 4, 4, None, 0, None) == 0
        assert bwd(*none9, 2, 0, 0, None, 0, None) == 0
        assert bwd(*none9, 1, 4, 4, None, 0, None) != 0
    # an N whose tile count would overflow an int: refused before any arithmetic on it
    big = 2 ** 31 - 1
    assert L.pp_mvc2d_workspace_bytes(1, big, 10, 4) == 0
    for fwd in (L.pp_mvc2d_forward_f32, L.pp_mvc2d_forward_f64):
        assert fwd(*none6, 1, big, 4, None) != 0
    for bwd in (L.pp_mvc2d_backward_f32, L.pp_mvc2d_backward_f64):
        assert bwd(*none9, 1, big, 4, None, 0, None) != 0


def row_error(got, ref):
    """max over the vertices of |got - ref| per query (B,N); NaN where both are NaN counts as equal"""
    err = np.abs(got - ref)
    err[np.isnan(got) & np.isnan(ref)] = 0.0
    return np.nan_to_num(err, nan=np.inf).max(1)


def compose(z, dtype=torch.float64):
    from pytorch_points_amd import mvc2d
    q = torch.tensor(z["points"], dtype=dtype, requires_grad=True)
    p = torch.tensor(z["polygon"], dtype=dtype, requires_grad=True)
    phi, w = mvc2d.composition(q, p, verbose=True)
    return q, p, phi, w


@pytest.mark.parametrize("path", GOLDEN, ids=lambda p: os.path.basename(p)[6:-4])
def test_composition_matches_reference_fp64(path):
    z = dict(np.load(path))
    q, p, phi, w = compose(z)
    st = z["stable"]
    phi_n, w_n = phi.detach().numpy(), w.detach().numpy()
    same = (row_error(phi_n, z["phi64"]) <= 1e-12) & (row_error(w_n, z["w64"]) <= 1e-12)
    assert same[st].all(), np.argwhere(st & ~same)
    # rows the reference decides by rounding: finite wherever the reference's are
    for got, ref in ((phi_n, z["phi64"]), (w_n, z["w64"])):
        got, ref = got.transpose(0, 2, 1)[~same], ref.transpose(0, 2, 1)[~same]
        assert np.isfinite(got[np.isfinite(ref)]).all()
    # G is zero on the unstable rows, so both gradients are comparable as a whole
    gq, gp = torch.autograd.grad((phi * torch.from_numpy(z["G"])).sum(), (q, p))
    for got, ref in ((gq.numpy(), z["gq64"]), (gp.numpy(), z["gp64"])):
        assert np.isfinite(got).all()
        assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max()


@pytest.mark.parametrize("path", GOLDEN, ids=lambda p: os.path.basename(p)[6:-4])
def test_linear_precision_and_partition_of_unity(path):
    z = dict(np.load(path))
    _, _, phi, _ = compose(z)
    phi = phi.detach().numpy()
    poly, pts, kind = z["polygon"].astype(np.float64), z["points"].astype(np.float64), z["kind"]
    # every row sums to 1; relative to its largest weight (weights of both signs cancel outside the polygon)
    scale = np.maximum(1.0, np.abs(phi).max(1))
    assert (np.abs(phi.sum(1) - 1) <= 1e-12 * scale * phi.shape[1]).all()
    # polygon @ phi gives the query back, on interior and exterior rows (the near exterior and the far field at 10x).
    # The bound: without the 1e-10 guards sum_i phi_i (p_i - q) is 0; a guard moves t_i by the fraction 1e-10 / |A_i|
    # and w_i by 1e-10 / r_i, so phi_i by at most d = 1e-10 (2 / min|A| + 1 / min r) of itself to first order, and
    # the sum by at most d sum_i |phi_i| r_i; doubled for the second order, plus the rounding of M terms of that size
    s = poly[:, :, :, None] - pts[:, :, None, :]
    r = np.linalg.norm(s, axis=1)
    s_next = np.roll(s, -1, axis=2)
    area = np.abs(s[:, 0] * s_next[:, 1] - s[:, 1] * s_next[:, 0]) / 2
    rec = np.einsum("bcm,bmn->bcn", poly, phi)
    sel = np.isin(kind, (INTERIOR, EXTERIOR, FAR10, CENTROID))
    with np.errstate(divide="ignore"):                       # rows on a vertex or an edge are not selected
        d = 1e-10 * (2 / area.min(1) + 1 / r.min(1))
    bound = (2 * d + 1e-14 * phi.shape[1]) * (np.abs(phi) * r).sum(1)
    err = np.abs(rec - pts).max(1)
    assert (err[sel] <= bound[sel]).all(), (err[sel] / bound[sel]).max()
    assert (bound[kind == INTERIOR] < 1e-6).all()
    assert sel.sum() >= 100


def test_golden_fixtures_cover_the_issue():
    names = {os.path.basename(p)[6:-4] for p in GOLDEN}
    assert {"triangle", "pentagon", "star12", "gon64", "b2"} <= names
    assert sum(os.path.getsize(p) for p in GOLDEN) < 1 << 20
    shapes = {os.path.basename(p)[6:-4]: np.load(p)["polygon"].shape for p in GOLDEN}
    assert shapes["triangle"][2] == 3 and shapes["pentagon"][2] == 5 and shapes["star12"][2] == 12
    assert shapes["gon64"][2] == 64 and shapes["b2"][0] == 2
    for p in GOLDEN:
        z = np.load(p)
        assert set(range(10)) <= set(z["kind"].ravel().tolist()), p
        assert z["points"].dtype == np.float32 and z["polygon"].dtype == np.float32
        for key in ("w64", "w32"):                  # no zero-sum row: the reference's other divisor was never taken
            assert (z[key].sum(1) != 0).all(), (p, key)
        # the reference decides by rounding only at 100 x the polygon's size and at the on-vertex threshold
        assert set(z["kind"][~z["stable"]].tolist()) <= {FAR100, NEAR_VERTEX}
        assert z["stable"][z["kind"] == FAR10].all() and z["stable"][z["kind"] == NEAR_EDGE].all()


def test_zero_sum_row_is_divided_by_one_and_leaves_its_neighbours():
    """A polygon so small that every |A_i| <= 1e-5 seen from a query outside it: every t_i is 0, the row is 0 and its
    sum is 0.  The reference then divides EVERY row of the tensor by its own weights; here that row is divided by 1
    and the other rows are what they are without it."""
    from pytorch_points_amd import mvc2d
    big = torch.tensor([[[0.0, 1.0, 0.3], [0.0, 0.1, 0.9]]], dtype=torch.float64)
    small = big * 1e-6
    pts = torch.tensor([[[0.3, 0.5, 0.4], [0.2, 0.3, 0.5]]], dtype=torch.float64)
    poly = torch.cat([big, small])                                 # B = 2: a zero-sum batch element beside a plain one
    q = torch.cat([pts, pts]).requires_grad_(True)
    phi, w = mvc2d.composition(q, poly, verbose=True)
    assert (w[1] == 0).all() and (phi[1] == 0).all()
    alone = mvc2d.composition(pts, big)
    assert torch.equal(phi[0], alone[0])
    assert torch.allclose(phi[0].sum(0), torch.ones(3, dtype=torch.float64), atol=1e-14)
    (gq,) = torch.autograd.grad(phi.sum() + w.sum(), q)
    assert torch.isfinite(gq).all() and (gq[1] == 0).all()
    # one zero-sum row beside a plain row of the same batch element: |A_i| is about r times the polygon's size / 2, so
    # a 1e-3 triangle seen from 7e-3 away has every |A_i| <= 1e-5, seen from 1.4 away none
    q2 = torch.tensor([[[1.0, 5e-3], [1.0, -5e-3]]], dtype=torch.float64)
    both = mvc2d.composition(q2, big * 1e-3)
    assert (both[0, :, 1] == 0).all()
    assert torch.equal(both[0, :, 0], mvc2d.composition(q2[:, :, :1], big * 1e-3)[0, :, 0])
    assert abs(float(both[0, :, 0].sum()) - 1) < 1e-12


def test_composition_other_dtypes_devices_and_empty_inputs():
    from pytorch_points_amd.network.geo_operations import mean_value_coordinates
    from pytorch_points_amd import mvc2d
    z = dict(np.load(GOLDEN[0]))
    st = z["stable"]
    for dt, tol in ((torch.float32, None), (torch.float16, None), (torch.bfloat16, None)):
        q = torch.from_numpy(z["points"]).to(dt)
        p = torch.from_numpy(z["polygon"]).to(dt)
        phi = mean_value_coordinates(q, p)
        assert phi.dtype == dt and phi.shape == z["phi64"].shape
    # the fp32 composition is the reference's fp32 chain: the same bits on the stable rows
    phi32, w32 = mean_value_coordinates(torch.from_numpy(z["points"]), torch.from_numpy(z["polygon"]), verbose=True)
    assert np.array_equal(phi32.numpy().transpose(0, 2, 1)[st], z["phi32"].transpose(0, 2, 1)[st])
    assert np.array_equal(w32.numpy().transpose(0, 2, 1)[st], z["w32"].transpose(0, 2, 1)[st])
    # empty inputs stay on the autograd graph
    q = torch.zeros(2, 2, 0, dtype=torch.float64, requires_grad=True)
    p = torch.randn(2, 2, 5, dtype=torch.float64, requires_grad=True)
    phi, w = mvc2d.composition(q, p, verbose=True)
    assert phi.shape == (2, 5, 0) and w.shape == (2, 5, 0) and phi.requires_grad
    gq, gp = torch.autograd.grad(phi.sum(), (q, p))
    assert gq.shape == q.shape and (gp == 0).all()
    phi = mvc2d.composition(p, q)                                   # M == 0
    assert phi.shape == (2, 0, 5) and phi.requires_grad
    # non-finite inputs: NaN rows, the other rows untouched
    p = torch.tensor(z["polygon"], dtype=torch.float64)
    q = torch.tensor(z["points"], dtype=torch.float64)[:, :, :4].clone()
    clean = mvc2d.composition(q, p)
    q[0, 0, 1] = float("nan")
    q[0, 1, 2] = float("inf")
    phi = mvc2d.composition(q, p)
    assert torch.isnan(phi[0, :, 1]).all() and torch.isnan(phi[0, :, 2]).all()
    assert torch.equal(phi[0, :, [0, 3]], clean[0, :, [0, 3]])
    p[0, 1, 0] = float("-inf")
    assert torch.isnan(mvc2d.composition(q, p)[0]).all()


def test_shape_and_dtype_errors():
    from pytorch_points_amd.network.geo_operations import mean_value_coordinates as mvc2
    q = torch.zeros(2, 2, 4)
    p = torch.zeros(2, 2, 6)
    with pytest.raises(RuntimeError, match="points must have shape"):
        mvc2(torch.zeros(2, 3, 4), p)
    with pytest.raises(RuntimeError, match="polygon must have shape"):
        mvc2(q, torch.zeros(2, 3, 6))
    with pytest.raises(RuntimeError, match="polygon must have shape"):
        mvc2(q, torch.zeros(2, 2))
    with pytest.raises(RuntimeError, match="same batch size"):
        mvc2(q, torch.zeros(3, 2, 6))
    with pytest.raises(RuntimeError, match="one dtype"):
        mvc2(q, p.double())
    with pytest.raises(RuntimeError, match="floating"):
        mvc2(q.long(), p.long())
    with pytest.raises(RuntimeError, match="one device"):
        mvc2(q, p.to("meta"))
