"""CPU tests (no GPU) of the k-NN edge operators' torch compositions (pytorch_points_amd/knn_edges.py), which state the
contract the HIP kernels are tested against, and of the reference's point-cloud regularisers built on them
(network/model_loss.py, network/geo_operations.py)."""
import collections

import numpy as np
import pytest
import torch

from pytorch_points_amd import _lib, knn_edges, ops
from pytorch_points_amd.network import geo_operations, model_loss
from test_mesh_edges_host import bucket_scratch_bytes

F32 = np.float32
EPS = 2.0 ** -23


# ------------------------------------------------------------------------------------------ numpy restatements
def np_sq_lengths(p, idx):
    """t0*t0, then fma(t_c, t_c, acc) in ascending dimension; the fused step is made in fp64 (the product of two fp32
    numbers is exact there) and rounded to fp32 once"""
    b = np.arange(p.shape[0])[:, None, None]
    t = p[b, idx] - p[:, :, None, :]
    d = t[..., 0] * t[..., 0]
    for c in range(1, p.shape[2]):
        d = (t[..., c].astype(np.float64) * t[..., c].astype(np.float64) + d.astype(np.float64)).astype(F32)
    return d


def np_laplacian(p, idx):
    b = np.arange(p.shape[0])[:, None]
    total = p[b, idx[:, :, 0]]
    for k in range(1, idx.shape[2]):
        total = total + p[b, idx[:, :, k]]
    return -(total / F32(idx.shape[2])) + p


def graph(rng, b, n, k):
    idx = rng.integers(0, n, size=(b, n, k))
    idx[0, 3, 0] = 3                       # a self-loop
    if k > 1:
        idx[1, 5, 1] = idx[1, 5, 0]        # a duplicate neighbour
    return idx


@pytest.mark.parametrize("d", [2, 3, 5])
@pytest.mark.parametrize("k", [1, 3, 8])
def test_compositions_match_the_numpy_restatement(k, d):
    rng = np.random.default_rng(100 * k + d)
    p = rng.normal(size=(2, 70, d)).astype(F32)
    idx = graph(rng, 2, 70, k)
    tp, ti = torch.from_numpy(p), torch.from_numpy(idx)
    # the Laplacian's sums are sequential fp32 additions: bitwise
    lap = knn_edges.laplacian_composition(tp, ti).numpy()
    assert np.array_equal(lap, np_laplacian(p, idx))
    # the lengths: the composition's addcmul may or may not fuse; each of the d - 1 steps then differs by at most one
    # rounding of a growing positive sum, the root adds half an ulp
    ref = np_sq_lengths(p, idx)
    sq = knn_edges.edge_lengths_composition(tp, ti, squared=True).numpy()
    np.testing.assert_allclose(sq, ref, rtol=d * EPS, atol=0)
    ln = knn_edges.edge_lengths_composition(tp, ti).numpy()
    np.testing.assert_allclose(ln, np.sqrt(ref), rtol=d * EPS, atol=0)
    assert sq[0, 3, 0] == 0 and ln[0, 3, 0] == 0
    # the public names take the composition on the CPU
    assert torch.equal(knn_edges.knn_laplacian(tp, ti), torch.from_numpy(lap))
    assert torch.equal(knn_edges.knn_edge_lengths(tp, ti, squared=True), torch.from_numpy(sq))


def test_zero_length_has_zero_gradient_and_no_nan():
    p = torch.randn(1, 6, 3, requires_grad=True)
    idx = torch.tensor([[[0, 1], [1, 1], [0, 2], [3, 0], [4, 4], [5, 2]]])
    knn_edges.edge_lengths_composition(p, idx).sum().backward()
    assert torch.isfinite(p.grad).all()
    g = p.grad.clone()
    p.grad = None
    keep = torch.tensor([[[0., 1], [0, 0], [1, 0], [0, 1], [0, 0], [0, 1]]])     # the same sum without the self-loops
    (knn_edges.edge_lengths_composition(p, idx) * keep).sum().backward()
    assert torch.equal(g, p.grad)


def test_out_of_range_index_contract():
    rng = np.random.default_rng(5)
    p = torch.from_numpy(rng.normal(size=(2, 70, 3))).requires_grad_(True)
    idx = torch.from_numpy(graph(rng, 2, 70, 4))
    bad = idx.clone()
    bad[0, 7, 1], bad[1, 9, 3] = -1, 70
    # the run the rest is compared with: the two rows contribute nothing (self-loops, zero upstream gradient)
    quiet = idx.clone()
    quiet[0, 7], quiet[1, 9] = 7, 9
    w_len = torch.from_numpy(rng.uniform(-1, 1, size=(2, 70, 4)))
    w_lap = torch.from_numpy(rng.uniform(-1, 1, size=(2, 70, 3)))
    rows = torch.ones(2, 70, dtype=torch.bool)
    rows[0, 7] = rows[1, 9] = False
    for squared in (False, True):
        out = knn_edges.edge_lengths_composition(p, bad, squared=squared)
        isnan = torch.zeros(2, 70, 4, dtype=torch.bool)
        isnan[0, 7, 1] = isnan[1, 9, 3] = True
        assert torch.equal(torch.isnan(out), isnan)
        ref = knn_edges.edge_lengths_composition(p, quiet, squared=squared)
        assert torch.equal(out[rows], ref[rows])
        g, = torch.autograd.grad((out * w_len).sum(), p)
        gr, = torch.autograd.grad((ref * w_len * rows[..., None]).sum(), p)
        assert torch.isnan(g[~rows]).all() and torch.equal(g[rows], gr[rows])
    lap = knn_edges.laplacian_composition(p, bad)
    assert torch.equal(torch.isnan(lap), (~rows)[..., None].expand(-1, -1, 3))
    ref = knn_edges.laplacian_composition(p, quiet)
    assert torch.equal(lap[rows], ref[rows])
    g, = torch.autograd.grad((lap * w_lap).sum(), p)
    gr, = torch.autograd.grad((ref * w_lap * rows[..., None]).sum(), p)
    assert torch.isnan(g[~rows]).all() and torch.equal(g[rows], gr[rows])


def test_gradcheck_fp64():
    rng = np.random.default_rng(7)
    p = torch.from_numpy(rng.normal(size=(1, 12, 3))).requires_grad_(True)
    idx = torch.from_numpy((np.arange(12)[:, None] + rng.integers(1, 12, size=(12, 3))) % 12)[None]   # no self-loops
    idx[0, 4, 1] = idx[0, 4, 0]
    fixed = p.detach().clone()
    w = torch.from_numpy(rng.uniform(-1, 1, size=(1, 12, 3)))
    for squared in (False, True):
        assert torch.autograd.gradcheck(lambda x: knn_edges.edge_lengths_composition(x, idx, squared), (p,))
        # detach_neighbors: the function of the centre points alone, the neighbours held where they are
        def held(x):
            d2 = ((fixed[0][idx[0]] - x[0][:, None]) ** 2).sum(-1)[None]
            return d2 if squared else d2.sqrt()
        assert torch.autograd.gradcheck(held, (p,))
        g, = torch.autograd.grad((knn_edges.edge_lengths_composition(p, idx, squared, True) * w).sum(), p)
        gh, = torch.autograd.grad((held(p) * w).sum(), p)
        torch.testing.assert_close(g, gh, rtol=1e-12, atol=1e-12)
    assert torch.autograd.gradcheck(lambda x: knn_edges.laplacian_composition(x, idx), (p,))


def test_validation():
    p = torch.zeros(2, 10, 3)
    idx = torch.zeros(2, 10, 4, dtype=torch.int64)
    for fn in (knn_edges.knn_edge_lengths, knn_edges.knn_laplacian):
        with pytest.raises(ValueError, match="idx must have shape"):
            fn(p, idx[:, :9])
        with pytest.raises(ValueError, match="idx must have shape"):
            fn(p, idx[0])
        with pytest.raises(ValueError, match="points must have shape"):
            fn(p[0], idx)
        with pytest.raises(ValueError, match="at least 1"):
            fn(p, idx[:, :, :0])
        with pytest.raises(RuntimeError, match="integer tensor"):
            fn(p, idx.float())
        with pytest.raises(RuntimeError, match="floating tensor"):
            fn(p.long(), idx)
        with pytest.raises(RuntimeError, match="expected"):
            fn(p, idx.to("meta"))
        with pytest.raises(NotImplementedError, match="K <= 128"):
            fn(p, torch.zeros(2, 10, 129, dtype=torch.int64))
        assert fn(p, torch.zeros(2, 10, 128, dtype=torch.int32)).shape[:2] == (2, 10)


def test_workspace_bytes_follow_the_layout():
    """pure host arithmetic, callable without a GPU: N*K entries per batch element and no owner region"""
    size = _lib.lib().pp_knn_edges_workspace_bytes
    assert bucket_scratch_bytes(2, 70, 70 * 8, False) == 6656
    # B*N a multiple of 64 and not, B*N*K on both sides of a multiple of 256
    for b, n, k in [(2, 70, 8), (1, 64, 4), (3, 85, 1), (1, 257, 20), (3, 5000, 33), (1, 1, 128)]:
        assert size(b, n, k) == bucket_scratch_bytes(b, n, n * k, False), (b, n, k)
    for b, n, k in [(0, 70, 8), (2, 0, 8), (-1, 70, 8), (2, -1, 8), (2, 70, 0), (2, 70, 129),
                    (2, 1 << 30, 1), (1, 1 << 28, 8)]:             # B*N or N*K beyond 2^31 - 1
        assert size(b, n, k) == 0, (b, n, k)


# ------------------------------------------------------------------------------------------------- the losses
_KNN = collections.namedtuple("KNN", "dists idx knn")


def topk_knn(p1, p2, lengths1=None, lengths2=None, K=1, version=-1, return_nn=False, return_sorted=True):
    """ops.knn_points' contract on any device (the product's runs on the GPU only)"""
    d = ((p1[:, :, None] - p2[:, None]) ** 2).sum(-1)
    dists, idx = d.topk(K, dim=-1, largest=False)
    nn = ops.knn_gather(p2, idx) if return_nn else None
    return _KNN(dists, idx, nn)


def svd_normals(points, base=None, nn_size=20, NCHW=True, idx=None):
    """geo_operations.batch_normals' contract (NCHW=False) on any device, sign fixed by the largest component"""
    assert not NCHW
    base = points if base is None else base
    if idx is None:
        idx = topk_knn(points, base, K=nn_size).idx
    g = ops.knn_gather(base, idx)
    g = g - g.mean(2, keepdim=True)
    v = torch.linalg.svd(g, full_matrices=False).Vh[..., -1, :]
    return v, idx


@pytest.fixture
def cpu_graphs(monkeypatch):
    monkeypatch.setattr(ops, "knn_points", topk_knn)
    monkeypatch.setattr(geo_operations, "batch_normals", svd_normals)


def clouds(seed, b=2, n=40, d=3):
    rng = np.random.default_rng(seed)
    ref = torch.from_numpy(rng.normal(size=(b, n, d)).astype(F32))
    pred = (ref + torch.from_numpy(rng.normal(scale=0.05, size=(b, n, d)).astype(F32))).requires_grad_(True)
    return ref.requires_grad_(True), pred


def gathered(points, knn_idx):     # the reference's gather, network/model_loss.py:126
    return torch.gather(points.unsqueeze(1).expand(-1, knn_idx.shape[1], -1, -1), 2,
                        knn_idx.unsqueeze(-1).expand(-1, -1, -1, points.shape[-1]))


def agree(loss, ref, inputs, rtol=1e-5):
    torch.testing.assert_close(loss, ref, rtol=rtol, atol=1e-6)
    got = torch.autograd.grad(loss.sum(), inputs, allow_unused=True, retain_graph=True)
    want = torch.autograd.grad(ref.sum(), inputs, allow_unused=True, retain_graph=True)
    for a, b in zip(got, want):
        assert (a is None) == (b is None)
        if a is not None:
            torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-6)


@pytest.mark.parametrize("d", [3, 5])
def test_point_uniform_laplacian_and_loss(cpu_graphs, d):
    ref, pred = clouds(1, d=d)
    lap, idx = geo_operations.pointUniformLaplacian(ref, nn_size=4)
    assert idx.shape == (2, 40, 4) and not (idx == torch.arange(40)[None, :, None]).any()
    want = -torch.sum(gathered(ref, idx), dim=2) / 4 + ref                        # geo_operations.py:151
    agree(lap, want, (ref,))
    lap2, idx2 = geo_operations.pointUniformLaplacian(pred, knn_idx=idx)
    assert idx2 is idx
    agree(lap2, -torch.sum(gathered(pred, idx), dim=2) / 4 + pred, (pred,))
    for use_norm in (False, True):
        mod = model_loss.PointLaplacianLoss(4, torch.nn.L1Loss(), use_norm=use_norm)
        a, b = want, -torch.sum(gathered(pred, idx), dim=2) / 4 + pred
        if use_norm:
            a, b = torch.norm(a, dim=-1, p=2), torch.norm(b, dim=-1, p=2)
        agree(mod(ref, pred), torch.nn.functional.l1_loss(a, b), (ref, pred))
    # with a correspondence: point2 is gathered (over all D coordinates) and searched on its own
    idx12 = torch.from_numpy(np.random.default_rng(2).permutation(40))[None].expand(2, -1)
    p2 = torch.gather(pred, 1, idx12.unsqueeze(-1).expand(-1, -1, d))
    i2 = topk_knn(p2, p2, K=5).idx[:, :, 1:]
    b = -torch.sum(gathered(p2, i2), dim=2) / 4 + p2
    agree(model_loss.PointLaplacianLoss(4, torch.nn.MSELoss())(ref, pred, idx12), torch.nn.functional.mse_loss(want, b),
          (ref, pred))


def _ref_lengths(points_ref, points, nn_size):       # network/model_loss.py:120-127
    _, knn_idx, group = topk_knn(points_ref, points_ref, K=nn_size + 1, return_nn=True)
    knn_idx, group = knn_idx[:, :, 1:], group[:, :, 1:, :]
    dist_ref = torch.norm(group - points_ref.unsqueeze(2), dim=-1, p=2)
    dist = torch.norm(gathered(points, knn_idx) - points.unsqueeze(2), dim=-1, p=2)
    return dist_ref, dist


def test_point_edge_length_loss(cpu_graphs):
    ref, pred = clouds(3)
    dist_ref, dist = _ref_lengths(ref, pred, 5)
    agree(model_loss.PointEdgeLengthLoss(5, torch.nn.L1Loss())(ref, pred), torch.nn.functional.l1_loss(dist_ref, dist),
          (ref, pred))


@pytest.mark.parametrize("reduction", ["mean", "sum", "none", "max"])
def test_point_stretch_loss(cpu_graphs, reduction):
    ref, pred = clouds(4)
    dist_ref, dist = _ref_lengths(ref, pred, 5)
    stretch = torch.max(dist / (dist_ref + 1e-10) - 1, torch.zeros_like(dist))
    want = {"mean": torch.mean(stretch), "sum": torch.mean(torch.sum(stretch, dim=-1)), "none": stretch,
            "max": torch.mean(torch.max(stretch, dim=-1)[0])}[reduction]
    agree(model_loss.PointStretchLoss(5, reduction)(ref, pred), want, (ref, pred))
    with pytest.raises(NotImplementedError):
        model_loss.PointStretchLoss(5, "median")(ref, pred)


@pytest.mark.parametrize("supplied", [False, True])
@pytest.mark.parametrize("reduction", ["mean", "sum", "none", "max"])
def test_simple_point_repulsion_loss(cpu_graphs, reduction, supplied):
    points, _ = clouds(5)
    radius = 0.9
    _, knn_idx, knn_points = topk_knn(points, points, K=5, return_nn=True)       # network/model_loss.py:378-387
    knn_idx = knn_idx[:, :, 1:].contiguous()
    if supplied:
        knn_points = gathered(points, knn_idx)
    else:
        knn_points = knn_points[:, :, 1:, :].contiguous().detach()
    knn_v = knn_points - points.unsqueeze(dim=2)
    distance2 = torch.sum(knn_v * knn_v, dim=-1)
    loss = 1 / torch.sqrt(distance2 + 1e-4)
    loss = torch.where(distance2 < radius * radius, loss, torch.zeros_like(loss))
    assert 0 < (loss == 0).sum() < loss.numel()          # the radius cuts through the edges
    want = {"mean": loss.mean(), "max": torch.mean(torch.max(loss, dim=-1)[0]),
            "sum": torch.sum(loss, dim=-1).mean(), "none": loss}[reduction]      # "sum": the repaired reduction
    mod = model_loss.SimplePointRepulsionLoss(4, radius, reduction)
    agree(mod(points, knn_idx) if supplied else mod(points), want, (points,))
    # gradients reach the neighbours only with a supplied graph: one edge's gradient, looked at on its far end
    out = model_loss.SimplePointRepulsionLoss(4, 10.0, "none")(points, *([knn_idx] if supplied else []))
    g, = torch.autograd.grad(out[0, 0, 0], points)
    far = int(knn_idx[0, 0, 0])
    assert g[0, 0].abs().sum() > 0 and (g[0, far].abs().sum() > 0) == supplied
    with pytest.raises(NotImplementedError):
        model_loss.SimplePointRepulsionLoss(4, radius, "median")(points)


@pytest.mark.parametrize("reduction", ["mean", "sum", "none", "max"])
def test_normal_loss(cpu_graphs, reduction):
    gt, pred = clouds(6)
    gn, idx = svd_normals(gt, nn_size=6, NCHW=False)                               # network/model_loss.py:342-358
    pn, _ = svd_normals(pred, nn_size=6, NCHW=False, idx=idx)
    loss = 1 - torch.nn.functional.cosine_similarity(pn, gn, dim=-1, eps=1e-8)
    want = {"mean": loss.mean(), "max": torch.max(loss, dim=-1)[0].mean(), "sum": torch.sum(loss, dim=-1).mean(),
            "none": loss}[reduction]                                                 # "mean": the repaired reduction
    got = model_loss.NormalLoss(6, reduction)(gt, pred)
    assert got.shape == ((2, 40) if reduction == "none" else ())
    agree(got, want, (pred,))
    idx12 = torch.from_numpy(np.random.default_rng(8).permutation(40))[None].expand(2, -1)
    p2, _ = svd_normals(torch.gather(pred, 1, idx12.unsqueeze(-1).expand(-1, -1, 3)), nn_size=6, NCHW=False)
    want = (1 - torch.nn.functional.cosine_similarity(p2, gn, dim=-1, eps=1e-8)).mean()
    torch.testing.assert_close(model_loss.NormalLoss(6, "mean")(gt, pred, idx12), want)


def test_smape_loss():
    x, y = torch.randn(50, 3, requires_grad=True), torch.randn(50, 3)
    agree(model_loss.SmapeLoss()(x, y), torch.mean(torch.abs(x - y) / (torch.abs(x) + torch.abs(y) + 1e-8)), (x,))
    assert model_loss.SmapeLoss(0.5).epsilon == 0.5


def test_graph_size_is_asserted(cpu_graphs):
    p = torch.randn(1, 4, 3)
    for call in (lambda: geo_operations.pointUniformLaplacian(p, nn_size=4),
                 lambda: model_loss.PointEdgeLengthLoss(4, torch.nn.L1Loss())(p, p),
                 lambda: model_loss.PointStretchLoss(4)(p, p), lambda: model_loss.SimplePointRepulsionLoss(4, 1.0)(p)):
        with pytest.raises(AssertionError):
            call()


def test_drop_in_names_resolve():
    import pytorch_points_amd
    pytorch_points_amd.install_as_pytorch_points()
    from pytorch_points.network.geo_operations import pointUniformLaplacian  # noqa: F401
    from pytorch_points.network.model_loss import (NormalLoss, PointEdgeLengthLoss, PointLaplacianLoss,  # noqa: F401
                                                   PointStretchLoss, SimplePointRepulsionLoss, SmapeLoss)
