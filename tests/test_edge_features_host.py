"""CPU tests (no GPU) of knn_edge_features' torch composition (pytorch_points_amd/edge_features.py), which states the
contract the HIP kernels are tested against, of its dispatch, and of the modules of network/layers.py and
network/pointnet2_modules.py: import names, state_dict() keys and shapes, constructor defaults and quirks."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from pytorch_points_amd import _lib, edge_features
from pytorch_points_amd.network import layers, pointnet2_modules
from test_abi_and_host import declared_symbols
from test_mesh_edges_host import bucket_scratch_bytes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------ numpy restatement
def np_forward(x, idx, q):
    """the contract, element by element; an index outside [0, N) gives NaN differences"""
    b, c, n = x.shape
    p, k = idx.shape[1:]
    out = np.empty((b, 2 * c, p, k), x.dtype)
    for bi in range(b):
        for pi in range(p):
            for ki in range(k):
                j = idx[bi, pi, ki]
                out[bi, :c, pi, ki] = q[bi, :, pi]
                out[bi, c:, pi, ki] = x[bi, :, j] - q[bi, :, pi] if 0 <= j < n else np.nan
    return out


def np_backward(g, idx, n, self_graph):
    """(grad_x, grad_query): a row with a bad index scatters nothing and has a NaN centre gradient"""
    b, c2, p, k = g.shape
    c = c2 // 2
    gq = np.zeros((b, c, p), g.dtype)
    gx = np.zeros((b, c, n), g.dtype)
    for bi in range(b):
        for pi in range(p):
            row_bad = ((idx[bi, pi] < 0) | (idx[bi, pi] >= n)).any()
            for ki in range(k):
                gq[bi, :, pi] += g[bi, :c, pi, ki] - g[bi, c:, pi, ki]
                if not row_bad:
                    gx[bi, :, idx[bi, pi, ki]] += g[bi, c:, pi, ki]
            if row_bad:
                gq[bi, :, pi] = np.nan
    if self_graph:
        gx = gx + gq
    return gx, gq


def cases(rng, dtype):
    x = rng.normal(size=(2, 3, 9)).astype(dtype)
    q = rng.normal(size=(2, 3, 5)).astype(dtype)
    idx_self = rng.integers(0, 9, size=(2, 9, 4))
    idx_self[0, 3, 0] = 3                              # a self-loop
    idx_self[1, 5, 1] = idx_self[1, 5, 0]              # a duplicate neighbour
    idx_query = rng.integers(0, 9, size=(2, 5, 4))
    return [(x, idx_self, None), (x, idx_query, q)]


@pytest.mark.parametrize("bad", [False, True])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_composition_matches_the_numpy_restatement(dtype, bad):
    rng = np.random.default_rng(1)
    for x, idx, q in cases(rng, dtype):
        idx = idx.copy()
        if bad:
            idx[0, 2, 1], idx[1, 4, 3], idx[1, 0, 0] = -1, 9, 2 ** 40
        tx = torch.from_numpy(x).requires_grad_(True)
        tq = None if q is None else torch.from_numpy(q).requires_grad_(True)
        out = edge_features.composition(tx, torch.from_numpy(idx), tq)
        want = np_forward(x, idx, x if q is None else q)
        assert out.dtype == tx.dtype and np.array_equal(out.detach().numpy(), want, equal_nan=True)     # one subtraction
        assert np.isnan(want).any() == bad
        assert torch.equal(edge_features.knn_edge_features(tx, torch.from_numpy(idx), tq).detach(), out.detach()) or bad
        w = rng.uniform(-1, 1, size=want.shape).astype(dtype)
        got = torch.autograd.grad(out, (tx,) if q is None else (tx, tq), torch.from_numpy(w))
        gx, gq = np_backward(w, idx, 9, q is None)
        tol = dict(rtol=0, atol=64 * np.finfo(dtype).eps)           # sums of 4 + in-degree terms of size <= 2
        np.testing.assert_allclose(got[0].numpy(), gx, equal_nan=True, **tol)
        if q is not None:
            np.testing.assert_allclose(got[1].numpy(), gq, equal_nan=True, **tol)
            assert np.isnan(gq).any() == bad and not np.isnan(gx).any()
        else:
            assert np.isnan(gx).any() == bad


def test_16_bit_composition_rounds_once():
    """the difference is made in fp32 on the widened operands and rounded once: torch's own 16-bit subtraction"""
    rng = np.random.default_rng(2)
    for dtype in (torch.float16, torch.bfloat16):
        x = torch.from_numpy(rng.normal(size=(1, 3, 20)).astype(np.float32)).to(dtype)
        idx = torch.from_numpy(rng.integers(0, 20, size=(1, 20, 3)))
        out = edge_features.composition(x, idx)
        wide = edge_features.composition(x.float(), idx)
        assert out.dtype == dtype and torch.equal(out, wide.to(dtype))


def test_gradcheck_fp64():
    rng = np.random.default_rng(7)
    x = torch.from_numpy(rng.normal(size=(1, 2, 6))).requires_grad_(True)
    q = torch.from_numpy(rng.normal(size=(1, 2, 6))).requires_grad_(True)
    idx = torch.from_numpy(rng.integers(0, 6, size=(1, 6, 2)))
    idx[0, 4, 1] = idx[0, 4, 0]
    assert torch.autograd.gradcheck(lambda a: edge_features.composition(a, idx), (x,))
    assert torch.autograd.gradcheck(lambda a, c: edge_features.composition(a, idx, c), (x, q))


def test_hip_serves_and_validation():
    x = torch.zeros(2, 4, 10)
    idx = torch.zeros(2, 10, 3, dtype=torch.int64)
    q = torch.zeros(2, 4, 7)
    serves = edge_features._hip_serves
    assert not serves(x, idx) and not serves(x, idx[:, :7], q)                  # CPU tensors: the composition
    meta = lambda t: t.to("meta")                                               # noqa: E731
    # (a device check alone cannot be made without a GPU: the decision is stated on the other criteria)
    assert edge_features._DTYPES == {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}
    assert torch.float64 not in edge_features._DTYPES
    with pytest.raises(NotImplementedError, match="K <= 128"):
        serves(x, torch.zeros(2, 10, 129, dtype=torch.int64))
    with pytest.raises(NotImplementedError, match="K <= 128"):
        edge_features.knn_edge_features(x, torch.zeros(2, 10, 129, dtype=torch.int64))
    assert edge_features.knn_edge_features(x, torch.zeros(2, 10, 128, dtype=torch.int32)).shape == (2, 8, 10, 128)
    with pytest.raises(ValueError, match="x must have shape"):
        serves(x[0], idx)
    with pytest.raises(ValueError, match="idx must have shape"):
        serves(x, idx[0])
    with pytest.raises(ValueError, match="self graph"):
        serves(x, idx[:, :9])
    with pytest.raises(ValueError, match="query must have shape"):
        serves(x, idx, q)
    with pytest.raises(ValueError, match="at least 1"):
        serves(x, idx[:, :, :0])
    with pytest.raises(RuntimeError, match="integer tensor"):
        serves(x, idx.float())
    with pytest.raises(RuntimeError, match="floating tensor"):
        serves(x.long(), idx)
    with pytest.raises(RuntimeError, match="expected"):
        serves(x, meta(idx))
    with pytest.raises(RuntimeError, match="query is"):
        serves(x, idx[:, :7], q.double())


class _Shape:
    """stands in for a CUDA tensor where only the dispatch criteria are read"""

    def __init__(self, shape, dtype, cuda=True):
        self.shape, self.dtype, self.is_cuda = torch.Size(shape), dtype, cuda


def test_hip_serves_decisions(monkeypatch):
    monkeypatch.setattr(edge_features, "_check", lambda *a: None)
    serves = edge_features._hip_serves
    idx = _Shape((2, 10, 3), torch.int64)
    for dtype in (torch.float32, torch.float16, torch.bfloat16):
        assert serves(_Shape((2, 4, 10), dtype), idx)
        assert not serves(_Shape((2, 4, 10), dtype, cuda=False), idx)
    assert not serves(_Shape((2, 4, 10), torch.float64), idx)
    assert serves(_Shape((2, 1, 10), torch.float32), idx) and serves(_Shape((2, 1000, 10), torch.float32), idx)
    # index products beyond 2^31 - 1: P*K, B*N, B*P, B*C
    assert serves(_Shape((1, 4, 2 ** 24), torch.float32), _Shape((1, 2 ** 24, 127), torch.int64))
    assert not serves(_Shape((1, 4, 2 ** 24), torch.float32), _Shape((1, 2 ** 24, 128), torch.int64))
    assert not serves(_Shape((2 ** 16, 4, 2 ** 15), torch.float32), _Shape((2 ** 16, 8, 3), torch.int64))
    assert not serves(_Shape((2 ** 16, 4, 8), torch.float32), _Shape((2 ** 16, 2 ** 15, 3), torch.int64))
    assert not serves(_Shape((2 ** 16, 2 ** 15, 8), torch.float32), _Shape((2 ** 16, 8, 3), torch.int64))
    assert not serves(_Shape((0, 4, 10), torch.float32), _Shape((0, 10, 3), torch.int64))


def test_entry_points_are_declared_exported_and_bound():
    names = ["pp_edge_features_backward", "pp_edge_features_forward", "pp_edge_features_workspace_bytes"]
    assert [s for s in declared_symbols() if s.startswith("pp_edge_features")] == names
    lib = _lib.lib()
    for name in names:
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert _lib._RESTYPES["pp_edge_features_workspace_bytes"] is _lib._c_size_t
    # the workspace: a flag byte per row of idx, then (where grad_x is wanted) the bucket scratch of N buckets and
    # P*K items per batch element; host arithmetic, callable without a GPU
    size = lib.pp_edge_features_workspace_bytes
    for b, n, p, k in [(2, 70, 70, 8), (1, 257, 40, 5), (3, 1030, 1030, 33), (1, 1, 1, 128)]:
        flags = (b * p + 255) // 256 * 256
        assert size(b, n, p, k, 0) == flags
        assert size(b, n, p, k, 1) == flags + bucket_scratch_bytes(b, n, p * k, False)
    for b, n, p, k in [(0, 70, 70, 8), (2, 0, 70, 8), (2, 70, 0, 8), (2, 70, 70, 0), (2, 70, 70, 129), (2, 1 << 30, 4, 1)]:
        assert size(b, n, p, k, 1) == 0


# ------------------------------------------------------------------------------------------------- imports
def test_reference_import_names_resolve_without_an_install_call():
    code = ("from pytorch_points.network.layers import DenseEdgeConv, SampledDenseEdgeConv, SharedMLP, Conv2d, Conv1d, "
            "Linear, ShuffleBlock\n"
            "from pytorch_points.network.pointnet2_modules import PointnetSAModuleMSG, PointnetSAModule, "
            "PointnetFPModule\n"
            "import pytorch_points_amd.network.layers as L, pytorch_points_amd.network.pointnet2_modules as M\n"
            "assert DenseEdgeConv is L.DenseEdgeConv and PointnetFPModule is M.PointnetFPModule\n"
            "print('ok')")
    env = dict(os.environ, PYTHONPATH=ROOT)
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, cwd=ROOT)
    assert res.returncode == 0 and res.stdout.strip() == "ok", res.stderr


# --------------------------------------------------------------------------------------------- state dicts
def shapes(module):
    return [(k, tuple(v.shape)) for k, v in module.state_dict().items()]


def norm_keys(prefix, channels, running=True):
    keys = [(prefix + ".weight", (channels,)), (prefix + ".bias", (channels,))]
    if running:
        keys += [(prefix + ".running_mean", (channels,)), (prefix + ".running_var", (channels,)),
                 (prefix + ".num_batches_tracked", ())]
    return keys


def test_wrapper_state_dicts_and_defaults():
    assert shapes(layers.Conv2d(3, 5, 1)) == [("conv.weight", (5, 3, 1, 1)), ("conv.bias", (5,))]
    assert shapes(layers.Conv2d(3, 5, 1, bias=False)) == [("conv.weight", (5, 3, 1, 1))]
    m = layers.Conv2d(3, 5, 1, normalization="batch", activation="relu")
    assert shapes(m) == [("conv.weight", (5, 3, 1, 1))] + norm_keys("norm", 5)          # no conv bias beside a norm
    assert isinstance(m.norm, torch.nn.BatchNorm2d) and (m.norm.eps, m.norm.momentum, m.norm.affine) == (0.001, 0.01, True)
    assert isinstance(m.act, torch.nn.ReLU)
    m = layers.Conv1d(3, 5, 1, normalization="instance", activation="lrelu", momentum=0.2)
    assert shapes(m) == [("conv.weight", (5, 3, 1))] + norm_keys("norm", 5, running=False)
    assert isinstance(m.norm, torch.nn.InstanceNorm1d) and (m.norm.eps, m.norm.momentum, m.norm.affine) == (0.001, 0.2, True)
    assert isinstance(m.act, torch.nn.LeakyReLU) and m.act.negative_slope == 0.1
    m = layers.Linear(3, 5, normalization="batch", activation="elu")
    assert shapes(m) == [("linear.weight", (5, 3))] + norm_keys("norm", 5)
    assert isinstance(m.norm, torch.nn.BatchNorm1d) and isinstance(m.act, torch.nn.ELU) and m.act.alpha == 1.0
    assert shapes(layers.Linear(3, 5, activation="tanh")) == [("linear.weight", (5, 3)), ("linear.bias", (5,))]
    assert isinstance(layers.Conv2d(3, 5, 1, normalization="instance").norm, torch.nn.InstanceNorm2d)
    for make in (lambda **kw: layers.Conv2d(3, 5, 1, **kw), lambda **kw: layers.Conv1d(3, 5, 1, **kw),
                 lambda **kw: layers.Linear(3, 5, **kw)):
        with pytest.raises(ValueError, match='only "batch/instance" normalization permitted.'):
            make(normalization="layer")
        with pytest.raises(ValueError, match='only "relu/elu/lrelu/tanh" implemented'):
            make(activation="gelu")
    # forward: convolution, normalisation, activation; `epoch` is accepted
    m = layers.Conv1d(3, 5, 1, normalization="batch", activation="tanh").eval()
    x = torch.randn(2, 3, 7)
    assert torch.equal(m(x, epoch=3), torch.tanh(m.norm(m.conv(x))))
    x = torch.arange(2 * 6 * 1 * 2, dtype=torch.float32).view(2, 6, 1, 2)
    assert torch.equal(layers.ShuffleBlock(2)(x)[:, :, 0, 0] % 12, torch.tensor([[0., 6, 2, 8, 4, 10]] * 2))


def test_module_state_dicts():
    m = layers.SharedMLP([3, 8, 9], activation="relu", normalization="batch")
    assert shapes(m) == ([("layer0.conv.weight", (8, 3, 1, 1))] + norm_keys("layer0.norm", 8)
                         + [("layer1.conv.weight", (9, 8, 1, 1))] + norm_keys("layer1.norm", 9))
    assert shapes(layers.SharedMLP([3, 8])) == [("layer0.conv.weight", (8, 3, 1, 1)), ("layer0.conv.bias", (8,))]
    for cls in (layers.DenseEdgeConv, layers.SampledDenseEdgeConv):
        m = cls(4, 3, 3, 2, unused="accepted")
        assert shapes(m) == [("mlps.0.weight", (3, 8, 1, 1)), ("mlps.0.bias", (3,)), ("mlps.1.weight", (3, 7, 1, 1)),
                             ("mlps.1.bias", (3,)), ("mlps.2.weight", (3, 10, 1, 1)), ("mlps.2.bias", (3,))]
        assert (m.out_channels, m.growth_rate, m.n, m.k) == (13, 3, 3, 2)
    m = pointnet2_modules.PointnetSAModuleMSG(npoint=4, radii=[0.1, 0.2], nsamples=[2, 3], mlps=[[3, 8], [3, 8, 9]])
    assert shapes(m) == ([("mlps.0.layer0.conv.weight", (8, 6, 1, 1))] + norm_keys("mlps.0.layer0.norm", 8)
                         + [("mlps.1.layer0.conv.weight", (8, 6, 1, 1))] + norm_keys("mlps.1.layer0.norm", 8)
                         + [("mlps.1.layer1.conv.weight", (9, 8, 1, 1))] + norm_keys("mlps.1.layer1.norm", 9))
    assert len(m.groupers) == 2 and (m.groupers[1].radius, m.groupers[1].nsample, m.groupers[1].use_xyz) == (0.2, 3, True)
    assert (m.npoint, m.pool_method) == (4, "max_pool")
    m = pointnet2_modules.PointnetSAModule(mlp=[3, 8], npoint=4, radius=0.1, nsample=2, normalization="instance")
    assert shapes(m) == [("mlps.0.layer0.conv.weight", (8, 6, 1, 1))] + norm_keys("mlps.0.layer0.norm", 8, running=False)
    m = pointnet2_modules.PointnetFPModule(mlp=[6, 5, 4])
    assert shapes(m) == ([("mlp.layer0.conv.weight", (5, 6, 1, 1))] + norm_keys("mlp.layer0.norm", 5)
                         + [("mlp.layer1.conv.weight", (4, 5, 1, 1))] + norm_keys("mlp.layer1.norm", 4))


def test_constructor_quirks_are_kept():
    # with use_xyz the constructor adds 3 to the first entry of the caller's list
    spec = [3, 8]
    pointnet2_modules.PointnetSAModule(mlp=spec, npoint=4, radius=0.1, nsample=2)
    assert spec == [6, 8]
    specs = [[3, 8], [3, 9]]
    pointnet2_modules.PointnetSAModuleMSG(npoint=4, radii=[0.1, 0.2], nsamples=[2, 3], mlps=specs, use_xyz=False)
    assert specs == [[3, 8], [3, 9]]
    # bn is accepted and ignored: normalization decides
    m = pointnet2_modules.PointnetSAModule(mlp=[3, 8], npoint=4, radius=0.1, nsample=2, bn=False)
    assert isinstance(m.mlps[0].layer0.norm, torch.nn.BatchNorm2d)
    m = pointnet2_modules.PointnetSAModule(mlp=[3, 8], npoint=4, radius=0.1, nsample=2, bn=True, normalization=None)
    assert not hasattr(m.mlps[0].layer0, "norm") and m.mlps[0].layer0.conv.bias is not None
    # npoint=None: the whole cloud is one group
    m = pointnet2_modules.PointnetSAModule(mlp=[3, 8])
    assert type(m.groupers[0]).__name__ == "GroupAll" and m.npoint is None
    with pytest.raises(AssertionError):
        pointnet2_modules.PointnetSAModuleMSG(npoint=4, radii=[0.1], nsamples=[2, 3], mlps=[[3, 8]])
    with pytest.raises(TypeError):
        pointnet2_modules.PointnetSAModule([3, 8])                                  # keyword-only, as in the reference


def test_dense_edge_conv_with_a_given_graph_on_cpu():
    """forward(x, idx=given) -- a NameError in the reference -- gathers with the given graph: bit for bit the
    reference's composition"""
    torch.manual_seed(0)
    m = layers.DenseEdgeConv(4, 3, 3, 2)
    x = torch.randn(2, 4, 9, requires_grad=True)
    idx = torch.randint(0, 9, (2, 9, 2))
    y, got_idx = m(x, idx)
    y_u, idx_u = m.forward_unfused(x, idx)
    assert got_idx is idx and idx_u is idx and tuple(y.shape) == (2, 13, 9) and torch.equal(y, y_u)
    g, = torch.autograd.grad(y.sum(), x)
    g_u, = torch.autograd.grad(y_u.sum(), x)
    torch.testing.assert_close(g, g_u)
    # one layer: the first layer's ReLU applies; the edge tensor itself
    edges, _ = m.get_local_graph(x, 2, idx)
    nb = torch.gather(x.unsqueeze(2).expand(-1, -1, 9, -1), 3, idx.unsqueeze(1).expand(-1, 4, -1, -1))
    assert torch.equal(edges, torch.cat([x.unsqueeze(-1).expand(-1, -1, -1, 2), nb - x.unsqueeze(-1)], dim=1))
    one = layers.DenseEdgeConv(4, 3, 1, 2)
    y1, _ = one(x, idx)
    want = torch.cat([torch.relu(one.mlps[0](edges)), x.unsqueeze(-1).expand(-1, -1, -1, 2)], dim=1).max(-1)[0]
    assert torch.equal(y1, want)
    # the sampled module's graph over given centres
    s = layers.SampledDenseEdgeConv(4, 3, 2, 2)
    q = torch.randn(2, 4, 5)
    idx_q = torch.randint(0, 9, (2, 5, 2))
    a, _ = s.get_local_graph(q, x, 2, idx=idx_q)
    b, _ = s.get_local_graph(q, x, 2, idx=idx_q, fused=False)
    assert tuple(a.shape) == (2, 8, 5, 2) and torch.equal(a, b)
