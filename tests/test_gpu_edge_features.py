"""GPU tests of knn_edge_features (csrc/edge_features.hip through pytorch_points_amd/edge_features.py) and of the modules
over it (network/layers.py, network/pointnet2_modules.py): the forward bit for bit against numpy in fp32, fp16 and
bf16, the ordered backward bit for bit against a sequential numpy loop, the default backward against the fp64
composition, the out-of-range contract, needs_input_grad, graph capture and a side stream, and the modules against
their compositions.

Figures of the default backward on the MI355X (printed by test_backward_default_form; measure = largest absolute error
over largest absolute reference): see DESIGN.md §4 "Edge features"."""
import contextlib
import copy
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from pytorch_points_amd import edge_features, ops, synthetic
from pytorch_points_amd.network import geo_operations, layers, operations, pointnet2_modules, pointnet2_utils
from topology_fuzz import np_ef_backward as np_backward, np_ef_forward as np_forward, round_to

pytestmark = pytest.mark.gpu

F32 = np.float32
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
ROUNDING = {torch.float32: 0.0, torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
SHAPES = [(2, 70), (1, 257), (3, 1030)]
KS = [1, 3, 16, 33]
CS = [1, 3, 24, 65]


# ------------------------------------------------------------------------------------------------ numpy side
def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def same_bits(got, want):
    """a torch tensor of any of the three types against an fp32 array of that type's values (widening is exact)"""
    return np.array_equal(bits(got.detach().float().cpu().numpy()), bits(want))


def by_row(a):
    """(B,C,P[,K]) -> (B,P[,K],C): a (B,P) mask then picks rows"""
    return np.moveaxis(a, 1, -1)


def measure(got, ref):
    """tests/test_gpu_knn_edges.py's measure: the largest absolute error over the largest absolute reference"""
    return float(np.abs(got - ref).max(initial=0.0)) / max(float(np.abs(ref).max(initial=0.0)), 1e-30)


@contextlib.contextmanager
def deterministic():
    torch.use_deterministic_algorithms(True)
    try:
        yield
    finally:
        torch.use_deterministic_algorithms(False)


def dev_t(a, dtype=None, grad=False):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    if dtype is not None:
        t = t.to(dtype)
    return t.requires_grad_(grad)


# ---------------------------------------------------------------------------------------------------- inputs
@functools.lru_cache(maxsize=None)
def features(b, c, n, dtype, seed=0):
    """(B,C,N) fp32 array of values of ``dtype``"""
    return round_to(synthetic.normal(17 + seed + 3 * c + n, (b, c, n)), dtype)


@functools.lru_cache(maxsize=None)
def searched(b, c, n, k):
    """the product's own feature-space graph of the fp32 features: (padded idx (B,N,K+1) on the device, numpy idx
    (B,N,K) without the self column)"""
    xt = dev_t(features(b, c, n, torch.float32)).transpose(1, 2).contiguous()
    full = ops.knn_points(xt, xt, K=k + 1).idx
    return full, full[:, :, 1:].cpu().numpy()


def query_graph(c, dtype):
    """P = 40 centres over N = 257 points, with a duplicate neighbour and rows that share neighbours"""
    rng = np.random.default_rng(c)
    idx = rng.integers(0, 257, size=(2, 40, 5))
    idx[0, 3, 1] = idx[0, 3, 0]
    idx[1, :, 2] = 11
    return features(2, c, 257, dtype), idx, features(2, c, 40, dtype, seed=5)


def odd_graph(c, dtype):
    """self-loops and duplicate neighbours within a row"""
    idx = searched(2, c, 70, 3)[1].copy()
    idx[0, 5, 1] = 5
    idx[1, :, 0] = np.arange(70)
    idx[0, 9, 2] = idx[0, 9, 0]
    idx[1, 11, 1:] = idx[1, 11, 1]
    return features(2, c, 70, dtype), idx, None


def hub_graph(c, dtype):
    """every row points at one point: in-degree 900"""
    return features(1, c, 300, dtype), np.full((1, 300, 3), 7, np.int64), None


def threshold_graph(c, dtype):
    """in-degrees 256, 257 and 87: on both sides of the longest list that one lane sorts (256 entries)"""
    idx = np.full((1, 600, 1), 2, np.int64)
    idx[0, :256] = 0
    idx[0, 256:513] = 1
    return features(1, c, 600, dtype), idx, None


def generic(b, c, n, k):
    return lambda _c, dtype: (features(b, c, n, dtype), searched(b, c, n, k)[1], None)


BACKWARD = [("b2_n70_k3_c3", generic(2, 3, 70, 3), 3), ("b1_n257_k16_c24", generic(1, 24, 257, 16), 24),
            ("b3_n1030_k33_c65", generic(3, 65, 1030, 33), 65), ("b2_n70_k1_c1", generic(2, 1, 70, 1), 1),
            ("query_c3", query_graph, 3), ("query_c24", query_graph, 24), ("loops_and_duplicates", odd_graph, 3),
            ("hub", hub_graph, 3), ("threshold", threshold_graph, 3)]


def hip_grads(x, idx, q, w, dtype):
    """(grad_x, grad_query | None) of the HIP operator as fp32 numpy"""
    tx = dev_t(x, dtype, True)
    tq = None if q is None else dev_t(q, dtype, True)
    out = edge_features.knn_edge_features(tx, dev_t(idx), tq)
    assert out.dtype == dtype and isinstance(out.grad_fn, torch.autograd.function.BackwardCFunction)
    got = torch.autograd.grad(out, (tx,) if q is None else (tx, tq), dev_t(w, dtype))
    assert all(t.dtype == dtype for t in got)
    return [t.float().cpu().numpy() for t in got] + ([None] if q is None else [])


def composition_grads(x, idx, q, w, dtype):
    tx = torch.from_numpy(x).to(dtype).requires_grad_(True)
    tq = None if q is None else torch.from_numpy(q).to(dtype).requires_grad_(True)
    out = edge_features.composition(tx, torch.from_numpy(idx), tq)
    got = torch.autograd.grad(out, (tx,) if q is None else (tx, tq), torch.from_numpy(w).to(dtype))
    return [t.numpy() for t in got] + ([None] if q is None else [])


# --------------------------------------------------------------------------------------------------- forward
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("b,n", SHAPES)
def test_forward_bit_exact_self_graph(cuda, b, n, k):
    """every C and type; idx is the strided [:, :, 1:] slice of the search's result, in int64 and in int32"""
    for c in CS:
        full, idx = searched(b, c, n, k)
        for dtype in DTYPES:
            x = features(b, c, n, dtype)
            want = np_forward(x, idx, x, dtype)
            tx = dev_t(x, dtype)
            sliced = full[:, :, 1:]
            assert not sliced.is_contiguous()
            out = edge_features.knn_edge_features(tx, sliced)
            assert out.dtype == dtype and tuple(out.shape) == (b, 2 * c, n, k)
            assert same_bits(out, want), (c, dtype)
            assert same_bits(edge_features.knn_edge_features(tx, full.int()[:, :, 1:]), want), (c, dtype, "int32")
            assert torch.equal(out, edge_features.composition(tx, sliced))


@pytest.mark.parametrize("dtype", DTYPES)
def test_forward_bit_exact_query_graph_loops_and_duplicates(cuda, dtype):
    for make, c in ((query_graph, 3), (query_graph, 65), (odd_graph, 3), (odd_graph, 24), (hub_graph, 1)):
        x, idx, q = make(c, dtype)
        tq = None if q is None else dev_t(q, dtype)
        out = edge_features.knn_edge_features(dev_t(x, dtype), dev_t(idx), tq)
        assert same_bits(out, np_forward(x, idx, x if q is None else q, dtype)), (make.__name__, c)
        assert torch.equal(out, edge_features.composition(dev_t(x, dtype), dev_t(idx), tq))


# -------------------------------------------------------------------------------------------------- backward
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name,make,c", BACKWARD, ids=[c[0] for c in BACKWARD])
def test_backward_ordered_form(cuda, name, make, c, dtype):
    """torch.use_deterministic_algorithms(True): the same bits twice, and the bits of a sequential numpy loop"""
    x, idx, q = make(c, dtype)
    p, k = idx.shape[1], idx.shape[2]
    w = round_to(np.random.default_rng(4).uniform(-1, 1, size=(x.shape[0], 2 * c, p, k)), dtype)
    with deterministic():
        a = hip_grads(x, idx, q, w, dtype)
        again = hip_grads(x, idx, q, w, dtype)
    want = np_backward(w, idx, x.shape[2], q is None, dtype)
    assert np.array_equal(bits(a[0]), bits(again[0])) and np.array_equal(bits(a[0]), bits(want[0]))
    if q is not None:
        assert np.array_equal(bits(a[1]), bits(again[1])) and np.array_equal(bits(a[1]), bits(want[1]))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name,make,c", BACKWARD, ids=[c[0] for c in BACKWARD])
def test_backward_default_form(cuda, name, make, c, dtype):
    """against the fp64 composition's autograd on the widened inputs.  fp32 bound: 4x the error of the fp32 CPU
    composition by the same measure, floor 1e-6 (the project's rule for the k-NN edge backwards); 16-bit: one rounding
    of the reference to the type (2^-11 fp16, 2^-8 bf16, relative to the largest entry) plus that bound"""
    x, idx, q = make(c, dtype)
    p, k = idx.shape[1], idx.shape[2]
    w = round_to(np.random.default_rng(3).uniform(-1, 1, size=(x.shape[0], 2 * c, p, k)), dtype)
    ref = composition_grads(x, idx, q, w, torch.float64)
    cpu32 = composition_grads(x, idx, q, w, torch.float32)
    got = hip_grads(x, idx, q, w, dtype)
    for what, g, r, c32 in zip(("grad_x", "grad_query"), got, ref, cpu32):
        if g is None:
            continue
        assert np.isfinite(g).all()
        fp32_bound = max(4 * measure(c32, r), 1e-6)
        bound = ROUNDING[dtype] + fp32_bound
        err = measure(g, r)
        print("%s %s %s: error %.3g, fp32 CPU composition %.3g, bound %.3g" % (name, dtype, what, err, measure(c32, r), bound))
        assert err <= bound, (what, err, bound)


def test_needs_input_grad_combinations(cuda):
    x, idx, q = query_graph(3, torch.float32)
    w = dev_t(np.random.default_rng(8).uniform(-1, 1, size=(2, 6, 40, 5)).astype(F32))
    with deterministic():
        both = hip_grads(x, idx, q, w.cpu().numpy(), torch.float32)
        for need_x, need_q in ((True, False), (False, True)):
            tx, tq = dev_t(x, grad=need_x), dev_t(q, grad=need_q)
            out = edge_features.knn_edge_features(tx, dev_t(idx), tq)
            gx, _, gq = out.grad_fn.apply(w)            # the node's own answers: None where no gradient is needed
            assert (gx is None) == (not need_x) and (gq is None) == (not need_q)
            out.backward(w)
            if need_x:
                assert tq.grad is None and np.array_equal(bits(tx.grad.cpu().numpy()), bits(both[0]))
            else:
                assert tx.grad is None and np.array_equal(bits(tq.grad.cpu().numpy()), bits(both[1]))
        # the self graph without a gradient: nothing to do
        out = edge_features.knn_edge_features(dev_t(x), dev_t(searched(2, 3, 257, 3)[1]))
        assert not out.requires_grad


# ---------------------------------------------------------------------------------------------- out of range
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("int32", [False, True])
def test_out_of_range_index(cuda, dtype, int32):
    """NaN exactly where the contract says, everything else as if the rows were not there.  The bad indices are only
    compared in the kernels, never used as addresses."""
    huge = 2 ** 31 - 1 if int32 else 2 ** 40
    for self_graph in (True, False):
        if self_graph:
            x, idx, q = odd_graph(3, dtype)
            n_rows = 70
        else:
            x, idx, q = query_graph(3, dtype)
            n_rows = 40
        n = x.shape[2]
        bad = idx.copy()
        bad[0, 7, 1], bad[1, 9, 2], bad[1, 20, 0] = -1, n, huge
        rows = np.ones((2, n_rows), bool)
        rows[0, 7] = rows[1, 9] = rows[1, 20] = False
        quiet = idx.copy()            # the rows contribute nothing: no upstream gradient on their differences below
        quiet[0, 7], quiet[1, 9], quiet[1, 20] = 7, 9, 20
        isnan = np.zeros((2, 6) + idx.shape[1:], bool)
        isnan[0, 3:, 7, 1] = isnan[1, 3:, 9, 2] = isnan[1, 3:, 20, 0] = True
        ti = (lambda a: dev_t(a).int()) if int32 else dev_t
        tx = dev_t(x, dtype)
        tq = None if q is None else dev_t(q, dtype)
        out = edge_features.knn_edge_features(tx, ti(bad), tq).float().cpu().numpy()
        ref = edge_features.knn_edge_features(tx, ti(quiet), tq).float().cpu().numpy()
        same = edge_features.knn_edge_features(tx, ti(idx), tq).float().cpu().numpy()      # without the bad indices
        assert np.array_equal(np.isnan(out), isnan)
        assert np.array_equal(bits(out[~isnan]), bits(same[~isnan]))
        assert np.array_equal(bits(by_row(out)[rows]), bits(by_row(ref)[rows]))
        w = round_to(np.random.default_rng(6).uniform(-1, 1, size=out.shape), dtype)
        wq = w.copy()
        wq[:, 3:] = np.where(rows[:, None, :, None], wq[:, 3:], 0)

        def grads(index, weight):
            a = dev_t(x, dtype, True)
            b = None if q is None else dev_t(q, dtype, True)
            o = edge_features.knn_edge_features(a, ti(index), b)
            g = torch.autograd.grad(o, (a,) if q is None else (a, b), dev_t(weight, dtype))
            return [t.float().cpu().numpy() for t in g]

        with deterministic():
            g, gr = grads(bad, w), grads(quiet, wq)
        if self_graph:
            assert np.isnan(by_row(g[0])[~rows]).all()
            assert np.array_equal(bits(by_row(g[0])[rows]), bits(by_row(gr[0])[rows]))
        else:
            assert np.array_equal(bits(g[0]), bits(gr[0]))
            assert np.isnan(by_row(g[1])[~rows]).all()
            assert np.array_equal(bits(by_row(g[1])[rows]), bits(by_row(gr[1])[rows]))


def test_dispatch(cuda):
    """fp64 takes the composition on the GPU; K > 128 raises; tensors on two devices raise"""
    x = torch.randn(1, 4, 40, device="cuda", dtype=torch.float64, requires_grad=True)
    idx = torch.randint(0, 40, (1, 40, 4), device="cuda")
    out = edge_features.knn_edge_features(x, idx)
    assert torch.equal(out, edge_features.composition(x, idx))
    assert not isinstance(out.grad_fn, torch.autograd.function.BackwardCFunction)
    with pytest.raises(NotImplementedError):
        edge_features.knn_edge_features(x.float(), torch.zeros(1, 40, 129, dtype=torch.int64, device="cuda"))
    with pytest.raises(RuntimeError, match="expected"):
        edge_features.knn_edge_features(x.float(), idx.cpu())
    # another integer type is converted
    assert torch.equal(edge_features.knn_edge_features(x.float(), idx.to(torch.int16)),
                       edge_features.composition(x.float(), idx))


# --------------------------------------------------------------------------------------- capture, side stream
def _step(x, q, idx_self, idx_query, w_self, w_query):
    out = edge_features.knn_edge_features(x, idx_self)
    g_self, = torch.autograd.grad(out, x, w_self)
    out_q = edge_features.knn_edge_features(x, idx_query, q)
    g_x, g_q = torch.autograd.grad(out_q, (x, q), w_query)
    return out, g_self, out_q, g_x, g_q


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_capture_and_side_stream(cuda, dtype):
    xs, idx_q, qs = query_graph(24, dtype)
    x, q = dev_t(xs, dtype, True), dev_t(qs, dtype, True)
    ti_self = searched(2, 24, 257, 16)[0][:, :, 1:]
    ti_q = dev_t(idx_q)
    w_self = (torch.rand(2, 48, 257, 16, device="cuda") * 2 - 1).to(dtype)
    w_q = (torch.rand(2, 48, 40, 5, device="cuda") * 2 - 1).to(dtype)
    args = (x, q, ti_self, ti_q, w_self, w_q)
    with deterministic():
        eager = [t.detach().clone() for t in _step(*args)]
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            got = _step(*args)                                             # also the warm-up
        torch.cuda.current_stream().wait_stream(side)
        for a, b in zip(got, eager):
            assert torch.equal(a.detach(), b)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            held = _step(*args)
        for _ in range(2):
            with torch.no_grad():
                for t in held:
                    t.fill_(7.0)
            graph.replay()
            torch.cuda.synchronize()
            for a, b in zip(held, eager):
                assert torch.equal(a.detach(), b)


# --------------------------------------------------------------------------------------------------- modules
def first_layer_input(module, call):
    seen = []
    handle = module.mlps[0].register_forward_hook(lambda m, inp, out: seen.append(inp[0].detach().clone()))
    try:
        result = call()
    finally:
        handle.remove()
    return seen[0], result


def outputs_and_grads(module, y, x):
    w = torch.from_numpy(np.random.default_rng(9).uniform(-1, 1, size=tuple(y.shape))).to(device=y.device, dtype=y.dtype)
    grads = torch.autograd.grad(y, [x] + list(module.parameters()), w)
    return [y.detach().double().cpu().numpy()] + [g.double().cpu().numpy() for g in grads]


def within_the_rule(name, got, cpu32, ref):
    for i, (g, c, r) in enumerate(zip(got, cpu32, ref)):
        bound = max(4 * measure(c, r), 1e-6)
        err = measure(g, r)
        print("%s [%d]: error %.3g, fp32 CPU %.3g, bound %.3g" % (name, i, err, measure(c, r), bound))
        assert err <= bound, (name, i, err, bound)


def test_dense_edge_conv(cuda):
    torch.manual_seed(0)
    module = layers.DenseEdgeConv(24, 12, 3, 8).cuda()
    xs = features(2, 24, 300, torch.float32)
    x = dev_t(xs, grad=True)
    fed, (y, idx) = first_layer_input(module, lambda: module(x))
    fed_u, (y_u, idx_u) = first_layer_input(module, lambda: module.forward_unfused(x))
    assert tuple(fed.shape) == (2, 48, 300, 8) and torch.equal(fed, fed_u)
    assert tuple(y.shape) == (2, module.out_channels, 300) and torch.equal(idx, idx_u) and tuple(idx.shape) == (2, 300, 8)
    assert torch.equal(y, y_u)
    # a given graph is used as it is
    y_g, idx_g = module(x, idx)
    assert idx_g is idx and torch.equal(y_g, y)
    got = outputs_and_grads(module, y, x)
    cpu32, ref = [], []
    for dtype, dest in ((torch.float32, cpu32), (torch.float64, ref)):
        twin = copy.deepcopy(module).cpu().to(dtype)
        xc = torch.from_numpy(xs).to(dtype).requires_grad_(True)
        yc, _ = twin.forward_unfused(xc, idx.cpu())
        dest.extend(outputs_and_grads(twin, yc, xc))
    within_the_rule("DenseEdgeConv", got, cpu32, ref)


@pytest.mark.parametrize("nsample", [16, 1])
def test_sampled_dense_edge_conv(cuda, nsample):
    torch.manual_seed(1)
    module = layers.SampledDenseEdgeConv(24, 12, 3, 8).cuda()
    xs = features(2, 24, 300, torch.float32)
    xyz = dev_t(synthetic.unit_sphere(3, 2, 300)).transpose(1, 2).contiguous()          # (B,3,N)
    x = dev_t(xs, grad=True)
    fed, (y, s_xyz, s_idx) = first_layer_input(module, lambda: module(x, nsample, xyz))
    fed_u, (y_u, s_xyz_u, s_idx_u) = first_layer_input(module, lambda: module.forward_unfused(x, nsample, xyz))
    assert tuple(fed.shape) == (2, 48, nsample, 8) and torch.equal(fed, fed_u)
    assert torch.equal(y, y_u) and torch.equal(s_idx, s_idx_u) and torch.equal(s_xyz, s_xyz_u)
    assert tuple(y.shape) == (2, module.out_channels, nsample) and tuple(s_idx.shape) == (2, nsample)
    assert tuple(s_xyz.shape) == ((2, 1, 3) if nsample == 1 else (2, 3, nsample))       # the reference's two layouts
    picked = s_idx.long()
    if nsample == 1:
        assert torch.equal(s_xyz, torch.gather(xyz, 2, picked[:, None, :].expand(-1, 3, -1)).transpose(1, 2))
    else:
        assert torch.equal(s_idx, geo_operations.furthest_point_sample(xyz, nsample, NCHW=True)[0])
    # the graph the module searched: the centres are columns of x, their nearest column is dropped
    centres = torch.gather(x.detach(), 2, picked[:, None, :].expand(-1, 24, -1))
    graph = ops.knn_points(centres.transpose(1, 2).contiguous(), x.detach().transpose(1, 2).contiguous(), K=9).idx[:, :, 1:]
    got = outputs_and_grads(module, y, x)
    cpu32, ref = [], []
    for dtype, dest in ((torch.float32, cpu32), (torch.float64, ref)):
        twin = copy.deepcopy(module).cpu().to(dtype)
        xc = torch.from_numpy(xs).to(dtype).requires_grad_(True)
        cc = torch.gather(xc, 2, picked.cpu()[:, None, :].expand(-1, 24, -1))
        edges, _ = twin.get_local_graph(cc, xc, 8, idx=graph.cpu(), fused=False)
        dest.extend(outputs_and_grads(twin, twin._dense(edges, cc), xc))
    within_the_rule("SampledDenseEdgeConv nsample=%d" % nsample, got, cpu32, ref)


def test_dense_edge_conv_bf16_autocast(cuda):
    torch.manual_seed(2)
    module = layers.DenseEdgeConv(24, 12, 3, 8).cuda()
    x = dev_t(features(2, 24, 300, torch.bfloat16), torch.bfloat16, True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        y, idx = module(x)
    assert y.dtype == torch.bfloat16 and idx.dtype == torch.int64
    y.float().sum().backward()
    assert x.grad.dtype == torch.bfloat16 and bool(torch.isfinite(x.grad.float()).all())
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in module.parameters())


def shared_mlp_eval(mlp, t):
    """a SharedMLP in eval mode from its own weights: convolution, batch norm over the running statistics, ReLU"""
    for layer in mlp:
        t = F.conv2d(t, layer.conv.weight)
        t = F.batch_norm(t, layer.norm.running_mean, layer.norm.running_var, layer.norm.weight, layer.norm.bias,
                         training=False, momentum=0.01, eps=0.001)
        t = F.relu(t)
    return t


def randomise_norms(module):
    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.normal_(0, 0.1)
                m.running_var.uniform_(0.5, 1.5)
                m.weight.uniform_(0.5, 1.5)
                m.bias.normal_(0, 0.1)


def test_pointnet_sa_module_msg(cuda):
    torch.manual_seed(3)
    module = pointnet2_modules.PointnetSAModuleMSG(npoint=32, radii=[0.3, 0.6], nsamples=[8, 16],
                                                   mlps=[[5, 8, 12], [5, 16]]).cuda().eval()
    randomise_norms(module)
    xyz = dev_t(synthetic.unit_sphere(4, 2, 256))
    feats = dev_t(features(2, 5, 256, torch.float32))
    new_xyz, out = module(xyz, feats)
    want_xyz = geo_operations.furthest_point_sample(xyz, 32, NCHW=False)[1]
    parts = []
    for i, (radius, nsample) in enumerate(((0.3, 8), (0.6, 16))):
        members = operations.ball_query(radius, nsample, xyz, want_xyz)
        local = operations.grouping_operation(xyz.transpose(1, 2).contiguous(), members)
        grouped = torch.cat([local - want_xyz.transpose(1, 2).unsqueeze(-1),
                             operations.grouping_operation(feats, members)], dim=1)
        parts.append(F.max_pool2d(shared_mlp_eval(module.mlps[i], grouped), kernel_size=[1, nsample]).squeeze(-1))
    assert torch.equal(new_xyz, want_xyz) and tuple(out.shape) == (2, 28, 32)
    assert torch.equal(out, torch.cat(parts, dim=1))
    # given centres are used as they are
    given, out2 = module(xyz, feats, want_xyz)
    assert given is want_xyz and torch.equal(out2, out)


def test_pointnet_sa_module(cuda):
    torch.manual_seed(4)
    xyz = dev_t(synthetic.unit_sphere(5, 2, 256))
    feats = dev_t(features(2, 5, 256, torch.float32))
    # npoint=None: the whole cloud as one group
    module = pointnet2_modules.PointnetSAModule(mlp=[5, 16]).cuda().eval()
    randomise_norms(module)
    new_xyz, out = module(xyz, feats)
    grouped = torch.cat([xyz.transpose(1, 2).unsqueeze(2), feats.unsqueeze(2)], dim=1)
    assert new_xyz is None and tuple(out.shape) == (2, 16, 1)
    assert torch.equal(out, F.max_pool2d(shared_mlp_eval(module.mlps[0], grouped), kernel_size=[1, 256]).squeeze(-1))
    # features=None: the relative coordinates alone; avg_pool
    module = pointnet2_modules.PointnetSAModule(mlp=[0, 8], npoint=32, radius=0.4, nsample=8,
                                                pool_method="avg_pool").cuda().eval()
    randomise_norms(module)
    new_xyz, out = module(xyz)
    members = operations.ball_query(0.4, 8, xyz, new_xyz)
    local = operations.grouping_operation(xyz.transpose(1, 2).contiguous(), members) - new_xyz.transpose(1, 2).unsqueeze(-1)
    assert tuple(out.shape) == (2, 8, 32)
    assert torch.equal(out, F.avg_pool2d(shared_mlp_eval(module.mlps[0], local), kernel_size=[1, 8]).squeeze(-1))
    module.pool_method = "median"
    with pytest.raises(NotImplementedError):
        module(xyz)


def test_pointnet_fp_module(cuda):
    torch.manual_seed(5)
    unknown = dev_t(synthetic.unit_sphere(6, 2, 64))
    known = dev_t(synthetic.unit_sphere(7, 2, 16))
    unknown_feats = dev_t(features(2, 3, 64, torch.float32))
    known_feats = dev_t(features(2, 5, 16, torch.float32))
    module = pointnet2_modules.PointnetFPModule(mlp=[8, 12, 6]).cuda().eval()
    randomise_norms(module)
    dist, idx = pointnet2_utils.three_nn(unknown, known)
    recip = 1.0 / (dist + 1e-8)
    interpolated = pointnet2_utils.three_interpolate(known_feats, idx, recip / torch.sum(recip, dim=2, keepdim=True))
    out = module(unknown, known, unknown_feats, known_feats)
    want = shared_mlp_eval(module.mlp, torch.cat([interpolated, unknown_feats], dim=1).unsqueeze(-1)).squeeze(-1)
    assert tuple(out.shape) == (2, 6, 64) and torch.equal(out, want)
    # unknow_feats=None
    module = pointnet2_modules.PointnetFPModule(mlp=[5, 6]).cuda().eval()
    randomise_norms(module)
    out = module(unknown, known, None, known_feats)
    assert torch.equal(out, shared_mlp_eval(module.mlp, interpolated.unsqueeze(-1)).squeeze(-1))
    # known=None: one global feature repeated
    one = known_feats[:, :, :1].contiguous()
    out = module(unknown, None, None, one)
    assert torch.equal(out, shared_mlp_eval(module.mlp, one.expand(-1, -1, 64).unsqueeze(-1)).squeeze(-1))
