"""GPU tests of the k-NN edge operators (csrc/knn_edges.hip through pytorch_points_amd/knn_edges.py) and of the
point-cloud regularisers over them: forwards bit for bit against knn_points / the oracle / a numpy restatement,
backwards against the fp64 composition (default form) and against a sequential numpy loop (ordered form), the
out-of-range contract, the losses against the compositions, graph capture and a side stream."""
import contextlib
import functools

import numpy as np
import pytest
import torch

import oracle
from pytorch_points_amd import knn_edges, ops, synthetic
from pytorch_points_amd.network import geo_operations, model_loss
from topology_fuzz import np_lap_backward, np_laplacian, np_len_backward

pytestmark = pytest.mark.gpu

F32 = np.float32
SHAPES = [(2, 70), (1, 257), (3, 5000)]
KS = [1, 3, 20, 33]


def dev_t(a, dev, grad=False):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev).requires_grad_(grad)


@functools.lru_cache(maxsize=None)
def cloud(b, n, d=3):
    return synthetic.unit_sphere(11 + n + d, b, n, d)


@functools.lru_cache(maxsize=None)
def searched(b, n, k):
    """(points, idx (B,N,K) without the self column, dists) of the product's own search, as numpy"""
    p = cloud(b, n)
    res = ops.knn_points(dev_t(p, "cuda"), dev_t(p, "cuda"), K=k + 1)
    return p, res.idx[:, :, 1:].cpu().numpy(), res.dists[:, :, 1:].cpu().numpy()


def measure(got, ref):
    """test_gpu_mvc.py's rel_close measure: the largest absolute error over the largest absolute reference"""
    return float(np.abs(got - ref).max(initial=0.0)) / max(float(np.abs(ref).max(initial=0.0)), 1e-30)


@contextlib.contextmanager
def deterministic():
    torch.use_deterministic_algorithms(True)
    try:
        yield
    finally:
        torch.use_deterministic_algorithms(False)


def grads(fn, p, idx, w, device, dtype):
    x = torch.from_numpy(p).to(device=device, dtype=dtype).requires_grad_(True)
    out = fn(x, torch.from_numpy(idx).to(device))
    g, = torch.autograd.grad(out, x, torch.from_numpy(w).to(device=device, dtype=dtype))
    return g.cpu().numpy()


# ------------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("b,n", SHAPES)
def test_forward_bit_exact_d3(cuda, b, n, k):
    p, idx, dists = searched(b, n, k)
    tp, ti = dev_t(p, "cuda"), dev_t(idx, "cuda")
    sq = knn_edges.knn_edge_lengths(tp, ti, squared=True).cpu().numpy()
    assert np.array_equal(sq, dists)
    ln = knn_edges.knn_edge_lengths(tp, ti).cpu().numpy()
    assert np.array_equal(ln, np.sqrt(dists))
    lap = knn_edges.knn_laplacian(tp, ti).cpu().numpy()
    assert np.array_equal(lap, np_laplacian(p, idx))
    # int32 indices are accepted
    assert np.array_equal(knn_edges.knn_edge_lengths(tp, ti.int(), squared=True).cpu().numpy(), dists)


@pytest.mark.parametrize("d", [2, 5, 32])
def test_forward_bit_exact_runtime_d(cuda, d):
    p = cloud(2, 257, d)
    for k in (3, 33):
        dist, idx = oracle.knn(p, p, k + 1)
        dist, idx = dist[:, :, 1:], idx[:, :, 1:].astype(np.int64)
        tp, ti = dev_t(p, "cuda"), dev_t(idx, "cuda")
        assert np.array_equal(knn_edges.knn_edge_lengths(tp, ti, squared=True).cpu().numpy(), dist)
        assert np.array_equal(knn_edges.knn_edge_lengths(tp, ti).cpu().numpy(), np.sqrt(dist))
        assert np.array_equal(knn_edges.knn_laplacian(tp, ti).cpu().numpy(), np_laplacian(p, idx))


# ------------------------------------------------------------------------------------------- backward: graphs
def hub_graph():
    return cloud(1, 1000), np.zeros((1, 1000, 8), np.int64)


def odd_graph():
    """self-loops and duplicate neighbours within a row"""
    p, idx, _ = searched(2, 70, 3)
    idx = idx.copy()
    idx[0, 5, 1] = 5
    idx[1, :, 0] = np.arange(70)
    idx[0, 9, 2] = idx[0, 9, 0]
    idx[1, 11, 1:] = idx[1, 11, 1]
    return p, idx


def threshold_graph():
    """in-degrees 256, 257 and 87: on both sides of the longest list that one lane sorts (256 entries)"""
    idx = np.full((1, 600, 1), 2, np.int64)
    idx[0, :256] = 0
    idx[0, 256:513] = 1
    return cloud(1, 600), idx


def backward_cases():
    cases = [("b%d_n%d_k%d" % (b, n, k), (lambda b=b, n=n, k=k: searched(b, n, k)[:2])) for b, n in SHAPES for k in KS]
    return cases + [("hub", hub_graph), ("loops_and_duplicates", odd_graph), ("threshold", threshold_graph)]


def operators():
    return [("lengths", lambda x, i: knn_edges.knn_edge_lengths(x, i), knn_edges.edge_lengths_composition, "k"),
            ("squared", lambda x, i: knn_edges.knn_edge_lengths(x, i, squared=True),
             lambda x, i: knn_edges.edge_lengths_composition(x, i, squared=True), "k"),
            ("detached", lambda x, i: knn_edges.knn_edge_lengths(x, i, detach_neighbors=True),
             lambda x, i: knn_edges.edge_lengths_composition(x, i, detach_neighbors=True), "k"),
            ("laplacian", knn_edges.knn_laplacian, knn_edges.laplacian_composition, "d")]


@pytest.mark.parametrize("name,make", backward_cases(), ids=[c[0] for c in backward_cases()])
def test_backward_default_form(cuda, name, make):
    """against the fp64 composition's autograd; the bound is 4x the error of the fp32 CPU composition on the same
    inputs by the same measure (the summation order differs over up to in-degree terms), floor 1e-6"""
    p, idx = make()
    rng = np.random.default_rng(3)
    for op, hip, comp, wshape in operators():
        w = rng.uniform(-1, 1, size=idx.shape if wshape == "k" else p.shape).astype(F32)
        ref = grads(comp, p, idx, w, "cpu", torch.float64)
        cpu32 = grads(comp, p, idx, w, "cpu", torch.float32)
        got = grads(hip, p, idx, w, "cuda", torch.float32)
        assert np.isfinite(got).all()
        bound = max(4 * measure(cpu32, ref), 1e-6)
        err = measure(got, ref)
        print("%s %s: error %.3g, fp32 CPU composition %.3g, bound %.3g" % (name, op, err, measure(cpu32, ref), bound))
        assert err <= bound, (op, err, bound)


def test_zero_length_gives_zero_gradient(cuda):
    p, idx = odd_graph()
    x = dev_t(p, "cuda", True)
    out = knn_edges.knn_edge_lengths(x, dev_t(idx, "cuda"))
    assert (out[1, :, 0] == 0).all() and out[0, 5, 1] == 0
    mask = torch.zeros_like(out)
    mask[1, :, 0] = 1
    mask[0, 5, 1] = 1
    g, = torch.autograd.grad(out, x, mask)
    assert (g == 0).all()


ORDERED = [("hub", hub_graph), ("n257", lambda: searched(1, 257, 20)[:2]), ("n5000", lambda: searched(3, 5000, 20)[:2]),
           ("loops_and_duplicates", odd_graph), ("threshold", threshold_graph)]


@pytest.mark.parametrize("name,make", ORDERED, ids=[c[0] for c in ORDERED])
def test_backward_ordered_form(cuda, name, make):
    """torch.use_deterministic_algorithms(True): the same bits twice, and the bits of a sequential numpy loop"""
    p, idx = make()
    rng = np.random.default_rng(4)
    wk = rng.uniform(-1, 1, size=idx.shape).astype(F32)
    wd = rng.uniform(-1, 1, size=p.shape).astype(F32)
    tp, ti = dev_t(p, "cuda"), dev_t(idx, "cuda")
    with deterministic():
        for squared in (False, True):
            out = knn_edges.knn_edge_lengths(tp, ti, squared=squared).cpu().numpy()
            for detach in (False, True):
                fn = lambda x, i: knn_edges.knn_edge_lengths(x, i, squared=squared, detach_neighbors=detach)  # noqa: E731
                a = grads(fn, p, idx, wk, "cuda", torch.float32)
                assert np.array_equal(a, grads(fn, p, idx, wk, "cuda", torch.float32))
                assert np.array_equal(a, np_len_backward(p, idx, out, wk, squared, detach))
        a = grads(knn_edges.knn_laplacian, p, idx, wd, "cuda", torch.float32)
        assert np.array_equal(a, grads(knn_edges.knn_laplacian, p, idx, wd, "cuda", torch.float32))
        assert np.array_equal(a, np_lap_backward(idx, wd))


def test_backward_runtime_d(cuda):
    """the (point, dimension) form of the backwards, ordered: the bits of the sequential loop"""
    for d in (2, 5, 32):
        p = cloud(2, 257, d)
        idx = oracle.knn(p, p, 8)[1][:, :, 1:].astype(np.int64)
        rng = np.random.default_rng(d)
        wk = rng.uniform(-1, 1, size=idx.shape).astype(F32)
        wd = rng.uniform(-1, 1, size=p.shape).astype(F32)
        with deterministic():
            out = knn_edges.knn_edge_lengths(dev_t(p, "cuda"), dev_t(idx, "cuda")).cpu().numpy()
            a = grads(knn_edges.knn_edge_lengths, p, idx, wk, "cuda", torch.float32)
            assert np.array_equal(a, np_len_backward(p, idx, out, wk, False))
            a = grads(knn_edges.knn_laplacian, p, idx, wd, "cuda", torch.float32)
            assert np.array_equal(a, np_lap_backward(idx, wd))


# ------------------------------------------------------------------------------------------------ out of range
def test_out_of_range_index(cuda):
    """defined behaviour: NaN exactly where the contract says, everything else as if the two rows were not there"""
    p, idx, _ = searched(2, 70, 3)
    bad = idx.copy()
    bad[0, 7, 1], bad[1, 9, 2] = -1, 70
    quiet = idx.copy()                      # the rows contribute nothing: self-loops, and no upstream gradient below
    quiet[0, 7], quiet[1, 9] = 7, 9
    rows = np.ones((2, 70), bool)
    rows[0, 7] = rows[1, 9] = False
    rng = np.random.default_rng(6)
    wk = rng.uniform(-1, 1, size=idx.shape).astype(F32)
    wd = rng.uniform(-1, 1, size=p.shape).astype(F32)
    tp = dev_t(p, "cuda")
    isnan = np.zeros(idx.shape, bool)
    isnan[0, 7, 1] = isnan[1, 9, 2] = True
    with deterministic():
        for squared in (False, True):
            fn = lambda x, i: knn_edges.knn_edge_lengths(x, i, squared=squared)   # noqa: E731
            out = fn(tp, dev_t(bad, "cuda")).cpu().numpy()
            assert np.array_equal(np.isnan(out), isnan)
            assert np.array_equal(out[rows], fn(tp, dev_t(quiet, "cuda")).cpu().numpy()[rows])
            g = grads(fn, p, bad, wk, "cuda", torch.float32)
            gq = grads(fn, p, quiet, wk * rows[..., None], "cuda", torch.float32)
            assert np.isnan(g[~rows]).all() and np.array_equal(g[rows], gq[rows])
        lap = knn_edges.knn_laplacian(tp, dev_t(bad, "cuda")).cpu().numpy()
        assert np.array_equal(np.isnan(lap), np.broadcast_to(~rows[..., None], lap.shape))
        assert np.array_equal(lap[rows], knn_edges.knn_laplacian(tp, dev_t(quiet, "cuda")).cpu().numpy()[rows])
        g = grads(knn_edges.knn_laplacian, p, bad, wd, "cuda", torch.float32)
        gq = grads(knn_edges.knn_laplacian, p, quiet, wd * rows[..., None], "cuda", torch.float32)
        assert np.isnan(g[~rows]).all() and np.array_equal(g[rows], gq[rows])


def test_dispatch(cuda):
    """fp64 and D > 32 take the composition on the GPU; K > 128 raises"""
    p = torch.randn(1, 40, 3, device="cuda", dtype=torch.float64, requires_grad=True)
    idx = torch.randint(0, 40, (1, 40, 4), device="cuda")
    assert torch.equal(knn_edges.knn_edge_lengths(p, idx), knn_edges.edge_lengths_composition(p, idx))
    wide = torch.randn(1, 40, 33, device="cuda")
    assert torch.equal(knn_edges.knn_laplacian(wide, idx), knn_edges.laplacian_composition(wide, idx))
    with pytest.raises(NotImplementedError):
        knn_edges.knn_laplacian(wide, torch.zeros(1, 40, 129, dtype=torch.int64, device="cuda"))
    with pytest.raises(RuntimeError, match="expected"):
        knn_edges.knn_laplacian(wide, idx.cpu())


# ------------------------------------------------------------------------------------------------------ losses
def loss_cases():
    l1 = torch.nn.L1Loss()
    cases = [("laplacian", lambda: model_loss.PointLaplacianLoss(6, l1), 2),
             ("laplacian_norm", lambda: model_loss.PointLaplacianLoss(6, torch.nn.MSELoss(), use_norm=True), 2),
             ("edge_length", lambda: model_loss.PointEdgeLengthLoss(6, l1), 2)]
    cases += [("stretch_" + r, (lambda r=r: model_loss.PointStretchLoss(6, r)), 2) for r in ("mean", "sum", "none", "max")]
    cases += [("repulsion_" + r, (lambda r=r: model_loss.SimplePointRepulsionLoss(6, 0.12, r)), 1)
              for r in ("mean", "sum", "none", "max")]
    return cases


@pytest.mark.parametrize("name,make,nargs", loss_cases(), ids=[c[0] for c in loss_cases()])
def test_losses_match_the_compositions(cuda, monkeypatch, name, make, nargs):
    ref = cloud(2, 700)
    pred = (ref + 0.01 * synthetic.unit_sphere(5, 2, 700)).astype(F32)

    def run(composed):
        with monkeypatch.context() as m:
            if composed:
                m.setattr(knn_edges, "knn_edge_lengths", knn_edges.edge_lengths_composition)
                m.setattr(knn_edges, "knn_laplacian", knn_edges.laplacian_composition)
            xs = [dev_t(a, "cuda", True) for a in (ref, pred)[:nargs]]
            loss = make()(*xs)
            return loss, torch.autograd.grad(loss.sum(), xs)

    loss, g = run(False)
    loss_c, g_c = run(True)
    torch.testing.assert_close(loss, loss_c, rtol=1e-5, atol=1e-5)
    for a, b in zip(g, g_c):
        a64, b64 = a.double().cpu().numpy(), b.double().cpu().numpy()
        print("%s: gradient error %.3g" % (name, measure(a64, b64)))
        # two fp32 evaluations of the same sums in different orders: an entry adds about K + in-degree ~ 2K terms (a
        # few more through the reductions), each rounded to 2^-24 relative: well under 64 * 2^-23 = 7.6e-6 of the
        # largest entry
        assert measure(a64, b64) <= 1e-5
    if name == "repulsion_none":
        assert 0 < int((loss == 0).sum()) < loss.numel()      # the radius cuts through the edges
        # with a supplied graph the gradients reach the neighbours too
        x = dev_t(ref, "cuda", True)
        idx = ops.knn_points(x, x, K=7).idx[:, :, 1:]
        mod = make()
        ga, = torch.autograd.grad(mod(x, idx).sum(), x)
        with monkeypatch.context() as m:
            m.setattr(knn_edges, "knn_edge_lengths", knn_edges.edge_lengths_composition)
            gb, = torch.autograd.grad(mod(x, idx).sum(), x)
        assert measure(ga.double().cpu().numpy(), gb.double().cpu().numpy()) <= 1e-5
        assert not torch.equal(ga, g[0])


def test_point_uniform_laplacian(cuda):
    x = dev_t(cloud(2, 700), "cuda")
    lap, idx = geo_operations.pointUniformLaplacian(x, nn_size=5)
    assert idx.shape == (2, 700, 5) and lap.shape == (2, 700, 3)
    assert not bool((idx == torch.arange(700, device="cuda")[None, :, None]).any())
    assert torch.equal(lap, knn_edges.laplacian_composition(x, idx))       # the same sequential sums
    lap2, idx2 = geo_operations.pointUniformLaplacian(x, knn_idx=idx)
    assert idx2 is idx and torch.equal(lap2, lap)


def test_normal_loss(cuda):
    gt = dev_t(cloud(2, 700), "cuda")
    loss = model_loss.NormalLoss(10, "none")(gt, gt)
    assert loss.shape == (2, 700) and float(loss.max()) <= 1e-5
    pred = dev_t((cloud(2, 700) * F32(1.05)).astype(F32), "cuda", True)
    none = model_loss.NormalLoss(10, "none")(gt, pred)
    torch.testing.assert_close(model_loss.NormalLoss(10, "mean")(gt, pred), none.mean())
    torch.testing.assert_close(model_loss.NormalLoss(10, "sum")(gt, pred), none.sum(-1).mean())
    torch.testing.assert_close(model_loss.NormalLoss(10, "max")(gt, pred), none.max(-1)[0].mean())
    idx12 = torch.arange(700, device="cuda")[None].expand(2, -1).flip(1)
    assert model_loss.NormalLoss(10)(gt, pred, idx12).shape == ()


# --------------------------------------------------------------------------------------- capture, side stream
def _step(x, idx, wk, wd):
    """each operator's forward and backward with a gradient call of its own: two gradients summed into one leaf by a
    single torch.autograd.grad would be added by the engine on the default stream, outside the capturing one"""
    out = knn_edges.knn_edge_lengths(x, idx)
    g_out, = torch.autograd.grad(out, x, wk)
    lap = knn_edges.knn_laplacian(x, idx)
    g_lap, = torch.autograd.grad(lap, x, wd)
    return out, g_out, lap, g_lap


def test_capture_and_side_stream(cuda):
    p, idx, _ = searched(1, 257, 20)
    x, ti = dev_t(p, "cuda", True), dev_t(idx, "cuda")
    wk = torch.rand(idx.shape, device="cuda") * 2 - 1
    wd = torch.rand(p.shape, device="cuda") * 2 - 1
    with deterministic():
        eager = [t.detach().clone() for t in _step(x, ti, wk, wd)]
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            got = _step(x, ti, wk, wd)                                    # also the warm-up, as test_gpu_mvc.py's
        torch.cuda.current_stream().wait_stream(side)
        for a, b in zip(got, eager):
            assert torch.equal(a.detach(), b)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            held = _step(x, ti, wk, wd)
        for _ in range(2):
            with torch.no_grad():
                for t in held:
                    t.fill_(7.0)
            graph.replay()
            torch.cuda.synchronize()
            for a, b in zip(held, eager):
                assert torch.equal(a.detach(), b)
