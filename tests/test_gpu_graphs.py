"""Every operator under graph capture (``torch.cuda.graph``, its default ``global`` error mode) and on concurrent streams.

The library keeps its scratch per (device, stream) and caches none while a stream is capturing, so that every graph
owns its scratch and no two streams share any ("Graphs and streams").  These tests pin that contract,
and the capture-time host paths behind it, against the CPU oracle with the equality the eager tests use for each operator: indices,
distances, gathers and groupings bit-exact; atomic-order gradients within the eager tolerance; the ordered backwards of
deterministic mode bit-exact.  Deterministic outputs of a replay are also compared bit for bit with the eager call.

  1. warm capture of every operator and path, replayed with input sets written in place;
  2. two graphs of one operator replayed side by side on two streams, and a replay beside an eager call;
  3. four eager streams running an operator chain with no synchronisation between them, and a pass over 20 streams
     that makes both scratch tables evict while earlier streams still have work in flight;
  4. cold capture: in fresh child processes, the operator's capture is the first library call of the process.

Debug knobs are host globals read when a launch is recorded: each test sets them before capture and the ``knobs``
fixture resets them to automatic afterwards."""
import contextlib
import ctypes
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import oracle
from pytorch_points_amd import synthetic as S

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


# ------------------------------------------------------------------------------------------------------------ helpers
def _set_knob(name, value):
    from pytorch_points_amd import _lib
    fn = getattr(_lib.lib(), "pp_debug_set_" + name)
    fn.argtypes = [ctypes.c_int]
    fn.restype = None
    fn(value)


@pytest.fixture
def knobs():
    """knobs(name=value, ...) before a capture; every knob touched is back at 0 (automatic) after the test"""
    touched = set()

    def set_(**kw):
        for k, v in kw.items():
            touched.add(k)
            _set_knob(k, v)
    yield set_
    for k in touched:
        _set_knob(k, 0)


@contextlib.contextmanager
def deterministic():
    before = torch.are_deterministic_algorithms_enabled()
    before_warn = torch.is_deterministic_algorithms_warn_only_enabled()
    torch.use_deterministic_algorithms(True)
    try:
        yield
    finally:
        torch.use_deterministic_algorithms(before, warn_only=before_warn)


_ORACLE = {}


def cached(what, fn, *arrays):
    """oracle results by content of their inputs (the large shapes are checked several times per session)"""
    h = hashlib.sha1(what.encode())
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
        h.update(str(a.shape).encode())
    key = h.hexdigest()
    if key not in _ORACLE:
        _ORACLE[key] = fn(*arrays)
    return _ORACLE[key]


def _grad(outputs, inputs, grads):
    return torch.autograd.grad(outputs, inputs, grads)


# ------------------------------------------------------------------------------------------------------------ families
# A family: make(k) -> input set k (numpy arrays); which inputs are leaves requiring grad; step(*tensors) -> outputs;
# check(inputs, outputs, det) asserts against the oracle / fp64; `exact` = outputs that are deterministic (compared bit
# for bit with the eager call); `knobs` = debug knobs the path needs.
class Family:
    def __init__(self, make, step, check, grad=(), exact=(), knobs=None):
        self.make, self.step, self.check, self.grad, self.exact = make, step, check, tuple(grad), tuple(exact)
        self.knobs = dict(knobs or {})

    def tensors(self, arrays, device):
        out = []
        for i, a in enumerate(arrays):
            t = torch.from_numpy(np.ascontiguousarray(a)).to(device)
            out.append(t.requires_grad_(True) if i in self.grad else t)
        return out


def _chamfer_shell(seed, b, n, m):
    """a shell against its core (test_gpu_chamfer_grid.py's adversarial pair): every direction is routed"""
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((b, n, 3))
    a /= np.linalg.norm(a, axis=-1, keepdims=True)
    return a.astype(np.float32), (rng.standard_normal((b, m, 3)) * 1e-3).astype(np.float32)


def _chamfer_grad_bound(x1, x2, g1, g2, i1, i2):
    """per coordinate: the sum of the magnitudes of the terms the Chamfer backward adds into it"""
    x1, x2, g1, g2 = (a.astype(np.float64) for a in (x1, x2, g1, g2))
    b1, b2 = np.zeros_like(x1), np.zeros_like(x2)
    for k in range(x1.shape[0]):
        t1 = np.abs(2 * g1[k][:, None] * (x1[k] - x2[k][i1[k]]))
        t2 = np.abs(2 * g2[k][:, None] * (x2[k] - x1[k][i2[k]]))
        b1[k] += t1
        np.add.at(b2[k], i1[k], t1)
        b2[k] += t2
        np.add.at(b1[k], i2[k], t2)
    return b1, b2


def chamfer(b, n, m, fn="node", adversarial=False, dtype=np.float32, routing=None):
    from pytorch_points_amd.network import model_loss as ml
    f = {"node": ml.nndistance, "python": ml.NmDistanceFunction.apply}[fn]

    def make(k):
        if adversarial and k == 1:
            x1, x2 = _chamfer_shell(960 + k, b, n, m)
        else:
            x1, x2 = S.unit_sphere(100 + 2 * k, b, n), S.unit_sphere(101 + 2 * k, b, m)
        return [x1.astype(dtype), x2.astype(dtype), S.normal(110 + k, (b, n)).astype(dtype),
                S.normal(120 + k, (b, m)).astype(dtype)]

    def step(x1, x2, g1, g2):
        d1, d2, i1, i2 = f(x1, x2)
        return (d1, d2, i1, i2) + _grad([d1, d2], [x1, x2], [g1, g2])

    def check(inp, out, det=False):
        x1, x2, g1, g2 = inp
        if dtype == np.float64:
            e = cached("chamfer64", oracle.chamfer_forward_f64, x1, x2)
            eg = oracle.chamfer_backward_f64(x1, x2, g1, g2, e[1], e[3])
        else:
            e = cached("chamfer", oracle.chamfer_forward, x1, x2)
            eg = cached("chamfer_bwd", lambda *a: oracle.chamfer_backward(*a), x1, x2, g1, g2, e[1], e[3])
        for got, want, what in zip(out[:4], (e[0], e[2], e[1], e[3]), ("dist1", "dist2", "idx1", "idx2")):
            assert np.array_equal(got, want), "%s differs at %d places" % (what, int((got != want).sum()))
        shell = adversarial and dtype == np.float32 and np.array_equal(x2, _chamfer_shell(961, b, n, m)[1])
        bound = _chamfer_grad_bound(x1, x2, g1, g2, e[1], e[3]) if shell else (None, None)
        for got, want, mag in zip(out[4:], eg, bound):
            if det:
                assert np.array_equal(got, want)
            elif shell:  # thousands of shell terms cancel on each core point: 1e-5 of the sum of the terms' magnitudes
                err = np.abs(got.astype(np.float64) - want)
                assert (err <= 1e-5 * mag + 1e-6).all(), (err / (mag + 1e-30)).max()
            else:        # the eager tests' equality (test_gpu_chamfer.py)
                assert np.allclose(got, want, rtol=1e-5, atol=1e-6), np.abs(got - want).max()
    knobs = {} if routing is None else {"nmdistance_routing": routing}
    return Family(make, step, check, grad=(0, 1), exact=(0, 1, 2, 3), knobs=knobs)


def labeled(b, n, m):
    from pytorch_points_amd.network import model_loss as ml

    def make(k):
        return [S.unit_sphere(130 + 2 * k, b, n), S.unit_sphere(131 + 2 * k, b, m),
                (S.uniform01(140 + k, (b, n)) * 3).astype(np.int64).reshape(b, n),
                (S.uniform01(150 + k, (b, m)) * 3).astype(np.int64).reshape(b, m),
                S.normal(160 + k, (b, n)), S.normal(170 + k, (b, m))]

    def step(x1, x2, l1, l2, g1, g2):
        d1, d2, i1, i2 = ml.labeled_nndistance(x1, x2, l1, l2)
        return (d1, d2, i1, i2) + _grad([d1, d2], [x1, x2], [g1, g2])

    def check(inp, out, det=False):
        x1, x2, l1, l2, g1, g2 = inp
        e = cached("labeled", oracle.labeled_chamfer_forward, x1, x2, l1.astype(np.float32), l2.astype(np.float32))
        for got, want in zip(out[:4], (e[0], e[2], e[1], e[3])):
            assert np.array_equal(got, want)
        eg = oracle.chamfer_backward(x1, x2, g1, g2, e[1], e[3])
        for got, want in zip(out[4:], eg):
            assert np.array_equal(got, want) if det else np.allclose(got, want, rtol=1e-5, atol=1e-6)
    return Family(make, step, check, grad=(0, 1), exact=(0, 1, 2, 3))


_FPS_FORMS = {"bucket_batched": {"fps_v1": 3, "fps_bucket_chain": 2}, "bucket_one_pick": {"fps_v1": 3, "fps_bucket_chain": 1},
              "cluster": {"fps_v1": 2}, "single_block": {"fps_v1": 1}, "auto": {}}


def fps(b, n, m, form="auto"):
    from pytorch_points_amd.network.geo_operations import furthest_point_sample

    def make(k):
        return [S.unit_sphere(200 + n + k, b, n), S.normal(210 + k, (b, m, 3))]

    def step(x, w):
        idx, chosen = furthest_point_sample(x, m, NCHW=False)
        return (idx, chosen) + _grad([chosen], [x], [w])

    def check(inp, out, det=False):
        x, w = inp
        e_idx, _ = cached("fps%d" % m, lambda a: oracle.furthest_sampling(a, m, 0), x)
        assert np.array_equal(out[0], e_idx)
        assert np.array_equal(out[1], np.take_along_axis(x, e_idx[..., None].astype(np.int64), 1))
        eg = oracle.gather_backward(np.ascontiguousarray(w.transpose(0, 2, 1)), e_idx, n).transpose(0, 2, 1)
        assert np.array_equal(out[2], eg) if det else np.allclose(out[2], eg, rtol=1e-5, atol=1e-6)
    return Family(make, step, check, grad=(0,), exact=(0, 1), knobs=_FPS_FORMS[form])


def gather(b, c, n, m, scatter="sorted"):
    from pytorch_points_amd.network.operations import gather_points

    def make(k):
        return [S.normal(220 + k, (b, c, n)), (S.uniform01(230 + k, (b, m)).reshape(b, m) * n).astype(np.int32),
                S.normal(240 + k, (b, c, m))]

    def step(f, idx, go):
        out = gather_points(f, idx)
        return (out,) + _grad([out], [f], [go])

    def check(inp, out, det=False):
        f, idx, go = inp
        assert np.array_equal(out[0], oracle.gather_forward(f, idx))
        eg = oracle.gather_backward(go, idx, n)
        assert np.array_equal(out[1], eg) if det else np.allclose(out[1], eg, rtol=1e-5, atol=1e-5)
    return Family(make, step, check, grad=(0,), exact=(0,), knobs={"scatter_mode": 0 if scatter == "sorted" else 1})


_GROUP_GRAD = {"auto": {}, "global_atomics": {"group_points_grad_variant": 1, "scatter_mode": 1},
               "lds_columns": {"group_points_grad_variant": 2, "scatter_mode": 1}}


def group(b, c, n, p, ns, variant="auto"):
    from pytorch_points_amd.network.operations import grouping_operation

    def make(k):
        return [S.normal(250 + k, (b, c, n)), (S.uniform01(260 + k, (b, p, ns)).reshape(b, p, ns) * n).astype(np.int32),
                S.normal(270 + k, (b, c, p, ns))]

    def step(f, idx, go):
        out = grouping_operation(f, idx)
        return (out,) + _grad([out], [f], [go])

    def check(inp, out, det=False):
        f, idx, go = inp
        assert np.array_equal(out[0], oracle.group_points(f, idx))
        eg = oracle.group_points_grad(go, idx, n)
        bad = ~np.isclose(out[1], eg, rtol=1e-5, atol=1e-5)
        assert np.array_equal(out[1], eg) if det else not bad.any(), "%d of %d differ, first at %s: %r vs %r" % (
            bad.sum(), bad.size, np.argwhere(bad)[:1].tolist(), out[1][bad][:4], eg[bad][:4])
    return Family(make, step, check, grad=(0,), exact=(0,), knobs=_GROUP_GRAD[variant])


def query_and_group(b, c, n, p, r, ns):
    from pytorch_points_amd.network.operations import QueryAndGroup
    qg = QueryAndGroup(r, ns)

    def make(k):
        x = S.unit_sphere(280 + k, b, n)
        return [x, np.ascontiguousarray(x[:, ::n // p][:, :p]) + np.float32(1e-3), S.normal(290 + k, (b, c, n)),
                S.normal(300 + k, (b, 3 + c, p, ns))]

    def step(xyz, centres, feats, go):
        out = qg(xyz, centres, feats)
        return (out,) + _grad([out], [feats], [go])

    def check(inp, out, det=False):
        xyz, centres, feats, go = inp
        bq = cached("bq", lambda a, q: oracle.ball_query(a, q, r, ns), centres, xyz)
        rel = oracle.group_points(np.ascontiguousarray(xyz.transpose(0, 2, 1)), bq) - centres.transpose(0, 2, 1)[..., None]
        assert np.array_equal(out[0][:, :3], rel)
        assert np.array_equal(out[0][:, 3:], oracle.group_points(feats, bq))
        eg = oracle.group_points_grad(np.ascontiguousarray(go[:, 3:]), bq, n)
        assert np.array_equal(out[1], eg) if det else np.allclose(out[1], eg, rtol=1e-5, atol=1e-5)
    return Family(make, step, check, grad=(2,), exact=(0,))


def ball_query(b, n, p, r, ns, search="grid"):
    from pytorch_points_amd.network.operations import ball_query as bq_op

    def make(k):
        x = S.unit_sphere(310 + k, b, n)
        x[:, n // 2:n // 2 + 50] = x[:, :50]                       # duplicates
        return [x, S.unit_sphere(320 + k, b, p)]

    def step(xyz, centres):
        return (bq_op(r, ns, xyz, centres),)

    def check(inp, out, det=False):
        xyz, centres = inp
        assert np.array_equal(out[0], cached("bq", lambda a, q: oracle.ball_query(a, q, r, ns), centres, xyz))
    return Family(make, step, check, exact=(0,), knobs={"ball_query_search": 2 if search == "grid" else 1})


def three_nn(b, n, m, c, search="grid", interp_grad=None):
    from pytorch_points_amd.network.pointnet2_utils import three_nn as tn, three_interpolate

    def make(k):
        u = S.unit_sphere(330 + k, b, n)
        kn = S.unit_sphere(340 + k, b, m)
        kn[:, m // 2:m // 2 + 5] = kn[:, :5]                       # exact ties
        u[:, :7] = kn[:, 10:17]                                     # zero distances
        return [u, kn, S.normal(350 + k, (b, c, m)), S.normal(360 + k, (b, c, n))]

    def step(u, kn, feats, go):
        dist, idx = tn(u, kn)
        w = 1.0 / (dist + 1e-8)
        w = (w / w.sum(-1, keepdim=True)).contiguous()
        out = three_interpolate(feats, idx, w)
        return (dist, idx, w, out) + _grad([out], [feats], [go])

    def check(inp, out, det=False):
        u, kn, feats, go = inp
        e_d2, e_idx = cached("three_nn", oracle.three_nn, u, kn)
        assert np.array_equal(out[1], e_idx) and np.array_equal(out[0], np.sqrt(e_d2))
        w = out[2]
        w64 = 1.0 / (np.sqrt(e_d2.astype(np.float64)) + 1e-8)
        assert np.allclose(w, w64 / w64.sum(-1, keepdims=True), rtol=1e-5, atol=1e-7)
        assert np.array_equal(out[3], oracle.three_interpolate(feats, e_idx, w))
        eg = oracle.three_interpolate_grad(go, e_idx, w, m)
        assert np.array_equal(out[4], eg) if det else np.allclose(out[4], eg, rtol=1e-5, atol=1e-5)
    kb = {"three_nn_search": 0 if search == "grid" else 1}
    if interp_grad is not None:
        kb["three_interpolate_grad_variant"] = interp_grad
    return Family(make, step, check, grad=(2,), exact=(0, 1, 2, 3), knobs=kb)


def knn(b, n, m, dim, K, search="grid"):
    from pytorch_points_amd.ops import knn_points

    def make(k):
        p1, p2 = (S.unit_sphere(370 + k, b, n), S.unit_sphere(371 + k, b, m)) if dim == 3 else \
            (S.normal(370 + k, (b, n, dim)), S.normal(371 + k, (b, m, dim)))
        p2[:, m // 2:m // 2 + 20] = p2[:, :20]                     # exact ties
        p1[:, :5] = p2[:, 7:12]                                     # zero distances
        return [p1, p2, S.normal(380 + k, (b, n, K))]

    def step(p1, p2, gd):
        out = knn_points(p1, p2, K=K)
        return (out.dists, out.idx) + _grad([out.dists], [p1, p2], [gd])

    def check(inp, out, det=False):
        p1, p2, gd = inp
        e_d, e_i = cached("knn%d" % K, lambda a, c: oracle.knn(a, c, K), p1, p2)
        assert np.array_equal(out[0], e_d) and np.array_equal(out[1], e_i)
        nb = np.take_along_axis(p2.astype(np.float64)[:, None], e_i[..., None].astype(np.int64), 2)   # (b, n, K, dim)
        diff = 2 * gd[..., None].astype(np.float64) * (p1.astype(np.float64)[:, :, None] - nb)
        g2 = np.zeros(p2.shape)
        for i in range(b):
            np.add.at(g2[i], e_i[i].reshape(-1), -diff[i].reshape(-1, dim))
        assert np.allclose(out[2], diff.sum(2), rtol=1e-5, atol=1e-5)
        assert np.allclose(out[3], g2, rtol=1e-5, atol=1e-5)
    return Family(make, step, check, grad=(0, 1), exact=(0, 1), knobs={"knn_search": 0 if search == "grid" else 1})


def svd(batch, m, n, full=True):
    from pytorch_points_amd._ext import linalg
    from test_gpu_linalg import check_contract

    def make(k):
        a = np.random.default_rng(390 + k).standard_normal((batch, m, n)).astype(np.float32)
        if k == 1:
            a[5, m - 1, n - 1] = np.nan                             # one replay sees a NaN in one matrix
        return [a]

    def step(a):
        return linalg.batch_svd_forward(a, True, 1e-7, 100, return_info=True, full=full)

    def check(inp, out, det=False):
        a = inp[0]
        u, s, v, info = out
        bad = ~np.isfinite(a).all(axis=(1, 2))
        for x in (u, s, v):
            assert np.isnan(x[bad]).all()
        assert (info[bad] == -2).all() and (info[~bad] >= -1).all()
        check_contract(a[~bad], u[~bad], s[~bad], v[~bad], full)
    return Family(make, step, check, exact=(0, 1, 2, 3))


def normals(b, n, nn):
    from pytorch_points_amd.network.geo_operations import batch_normals

    def make(k):
        return [S.unit_sphere(400 + k, b, n)]

    def step(p):
        nrm, idx = batch_normals(p, nn_size=nn, NCHW=False)
        return nrm, idx

    def check(inp, out, det=False):
        p = inp[0]
        _, e_i = cached("knn%d" % nn, lambda a, c: oracle.knn(a, c, nn), p, p)
        assert np.array_equal(out[1], e_i)
        g = np.take_along_axis(p.astype(np.float64)[:, None], e_i[..., None].astype(np.int64), 2)
        g -= g.mean(2, keepdims=True)
        _, s64, vt64 = np.linalg.svd(g)
        sep = (s64[..., 1] - s64[..., 2]) >= 1e-2 * s64[..., 0]
        cos = np.abs(np.einsum("bnc,bnc->bn", out[0].astype(np.float64), vt64[..., 2, :]))
        assert sep.mean() > 0.9 and (cos[sep] >= 1 - 1e-4).all()
    return Family(make, step, check, exact=(0, 1))


# ------------------------------------------------------------------------------------------------------------ capture
class Captured:
    """static inputs, warm-up on a side stream, one capture in the default (global) error mode"""

    def __init__(self, fam, device, warmup=2):
        self.fam = fam
        self.inputs = fam.tensors(fam.make(0), device)
        if warmup:
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(warmup):
                    fam.step(*self.inputs)
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
        from pytorch_points_amd import _lib
        before = {k: v.data_ptr() for k, v in _lib._WS.items()}
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.outputs = fam.step(*self.inputs)
        # every graph owns its scratch: the capture neither cached a buffer nor took one from the table
        after = {k: v.data_ptr() for k, v in _lib._WS.items()}
        assert after == before, "the capture changed the scratch table: %s" % sorted(set(after.items()) ^ set(before.items()))

    def load(self, arrays):
        with torch.no_grad():
            for t, a in zip(self.inputs, arrays):
                t.copy_(torch.from_numpy(np.ascontiguousarray(a)))

    def read(self):
        return [o.detach().cpu().numpy() for o in self.outputs]

    def run(self, arrays):
        self.load(arrays)
        self.graph.replay()
        torch.cuda.synchronize()
        return self.read()


def eager(fam, arrays, device):
    out = fam.step(*fam.tensors(arrays, device))
    torch.cuda.synchronize()
    return [o.detach().cpu().numpy() for o in out]


def replay_and_check(fam, device, sets=(0, 1), det=False):
    cap = Captured(fam, device)
    for k in sets:
        arrays = fam.make(k)
        got = cap.run(arrays)
        fam.check(arrays, got, det)
        ref = eager(fam, arrays, device)
        for i in (range(len(got)) if det else fam.exact):
            assert np.array_equal(got[i], ref[i], equal_nan=True), "input set %d: output %d differs from the eager call" % (k, i)
    return cap


# ------------------------------------------------------------------------------------------------ 1. warm capture
GRID = (8, 8192, 4096)


@pytest.mark.parametrize("fn", ["node", "python"])
def test_chamfer_brute_force_shape(cuda, fn):
    replay_and_check(chamfer(2, 300, 500, fn), cuda)


@pytest.mark.parametrize("routing", [0, 1, 2])
@pytest.mark.parametrize("fn", ["node", "python"])
def test_chamfer_grid_shape_every_routing_form(cuda, knobs, fn, routing):
    """the routing form is baked into the graph; the bits must not depend on it (second input set: shell vs core)"""
    fam = chamfer(*GRID, fn=fn, adversarial=True, routing=routing)
    knobs(**fam.knobs)
    replay_and_check(fam, cuda)


def test_labeled_chamfer_grid_shape(cuda):
    replay_and_check(labeled(*GRID), cuda)


def test_chamfer_fp64(cuda):
    replay_and_check(chamfer(2, 300, 500, fn="python", dtype=np.float64), cuda)


@pytest.mark.parametrize("form", ["bucket_batched", "bucket_one_pick", "cluster", "single_block"])
@pytest.mark.parametrize("b,n,m", [(1, 70000, 64), (16, 8192, 200)])
def test_furthest_point_sample(cuda, knobs, form, b, n, m):
    from pytorch_points_amd._ext import sampling
    fam = fps(b, n, m, form)
    knobs(**fam.knobs)
    replay_and_check(fam, cuda)
    assert sampling.furthest_sampling_status(cuda) == 0


@pytest.mark.parametrize("scatter", ["sorted", "atomics"])
def test_gather_points(cuda, knobs, scatter):
    fam = gather(9, 16, 16384, 8192, scatter)
    knobs(**fam.knobs)
    if scatter == "sorted":
        _assert_sorted_scatter_runs(fam, cuda)
    replay_and_check(fam, cuda)


@pytest.mark.parametrize("variant", ["auto", "sorted", "global_atomics", "lds_columns"])
def test_grouping_operation(cuda, knobs, variant):
    """auto at this shape: the LDS column kernel; sorted: a shape the sorted scatter-add serves"""
    fam = group(*SORTED_GROUP) if variant == "sorted" else group(4, 16, 4096, 1024, 32, variant)
    knobs(**fam.knobs)
    if variant == "sorted":
        _assert_sorted_scatter_runs(fam, cuda)
    replay_and_check(fam, cuda)


def test_query_and_group(cuda):
    replay_and_check(query_and_group(2, 8, 8192, 512, 0.15, 32), cuda)


@pytest.mark.parametrize("search", ["grid", "scan"])
def test_ball_query(cuda, knobs, search):
    fam = ball_query(2, 8192, 512, 0.1, 32, search)
    knobs(**fam.knobs)
    replay_and_check(fam, cuda)


@pytest.mark.parametrize("search", ["grid", "scan"])
def test_three_nn_and_interpolate(cuda, knobs, search):
    fam = three_nn(2, 8192, 1024, 16, search)
    knobs(**fam.knobs)
    replay_and_check(fam, cuda)


@pytest.mark.parametrize("path", ["grid", "scan", "nd"])
def test_knn_points(cuda, knobs, path):
    fam = knn(2, 1000, 2000, 24, 17) if path == "nd" else knn(2, 2048, 8192, 3, 8, path)
    knobs(**fam.knobs)
    replay_and_check(fam, cuda)


@pytest.mark.parametrize("full", [True, False], ids=["full", "thin"])
@pytest.mark.parametrize("m,n", [(20, 3), (3, 3), (17, 31), (32, 32)])
def test_batch_svd(cuda, m, n, full):
    """per-lane (K <= 4) and per-column kernels; the second replay has a NaN in matrix 5: NaN factors and info -2
    there, and every other matrix bit-equal to the first replay's"""
    fam = svd(256, m, n, full)
    cap = replay_and_check(fam, cuda)
    clean = cap.run(fam.make(0))
    a0 = fam.make(0)[0].copy()
    a0[5, m - 1, n - 1] = np.nan
    dirty = cap.run([a0])
    for x, y in zip(dirty, clean):
        assert np.array_equal(np.delete(x, 5, 0), np.delete(y, 5, 0))
    assert np.isnan(dirty[1][5]).all() and dirty[3][5] == -2


def test_batch_normals(cuda):
    replay_and_check(normals(2, 2048, 16), cuda)


@pytest.mark.parametrize("family", ["chamfer", "labeled", "gather", "group", "query_and_group", "three_interpolate"])
def test_deterministic_mode_ordered_backwards(cuda, family):
    """under torch.use_deterministic_algorithms(True) the captured backwards are the ordered forms: equal to the
    oracle bit for bit, and every output equal to the eager call's"""
    fam = {"chamfer": lambda: chamfer(*GRID), "labeled": lambda: labeled(*GRID),
           "gather": lambda: gather(9, 16, 16384, 8192), "group": lambda: group(4, 16, 4096, 1024, 32),
           "query_and_group": lambda: query_and_group(2, 8, 8192, 512, 0.15, 32),
           "three_interpolate": lambda: three_nn(2, 8192, 1024, 16)}[family]()
    with deterministic():
        replay_and_check(fam, cuda, det=True)


# ------------------------------------------------------------------------------- 2. scratch between graphs and streams
SORTED_GROUP = (8, 16, 8192, 512, 32)   # P = 16384 <= 4 N and B P C >= 2^20: grouping's sorted scatter-add backward


def _assert_sorted_scatter_runs(fam, device):
    """the eager call writes the per-stream "scatter" scratch (the sorted scatter-add's triples): zeroed before, not
    after -- so the family's shape takes the sorted form, whatever the heuristic becomes"""
    from pytorch_points_amd import _lib
    eager(fam, fam.make(0), device)
    bufs = _lib.cached_workspaces("scatter", device)
    assert bufs, "no scatter scratch: the sorted form does not serve this shape"
    for buf in bufs:
        buf.zero_()
    eager(fam, fam.make(0), device)
    assert any(int(buf.count_nonzero()) > 0 for buf in bufs), "the sorted scatter-add did not run"


def _assert_streams_get_their_own_scratch(device):
    """the scratch table gives every stream a buffer of its own (checked before any unsynchronised run)"""
    from pytorch_points_amd import _lib
    ptrs = []
    for _ in range(2):
        with torch.cuda.stream(torch.cuda.Stream()):
            ptrs.append(_lib.workspace(device, "fps", 1 << 16).data_ptr())
    assert ptrs[0] != ptrs[1], "two streams were handed the same scratch"
SCRATCH_FAMILIES = {
    "chamfer_grid": lambda: chamfer(*GRID),
    "labeled_grid": lambda: labeled(*GRID),
    "ball_query_grid": lambda: ball_query(2, 8192, 512, 0.1, 32),
    "three_nn_grid": lambda: three_nn(2, 8192, 1024, 16),
    "knn_grid": lambda: knn(2, 2048, 8192, 3, 8),
    "fps_cluster": lambda: fps(16, 8192, 200, "cluster"),
    "fps_bucket": lambda: fps(16, 8192, 200, "bucket_batched"),
    "group_sorted_scatter": lambda: group(*SORTED_GROUP),
    "gather_sorted_scatter": lambda: gather(9, 16, 16384, 8192),
}


@pytest.mark.parametrize("name", sorted(SCRATCH_FAMILIES))
def test_two_graphs_side_by_side_and_beside_eager(cuda, knobs, name):
    from pytorch_points_amd._ext import sampling
    fam = SCRATCH_FAMILIES[name]()
    knobs(**fam.knobs)
    if name.endswith("sorted_scatter"):
        _assert_sorted_scatter_runs(fam, cuda)
    _assert_streams_get_their_own_scratch(cuda)
    a, b = Captured(fam, cuda), Captured(fam, cuda)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    sets = [fam.make(k) for k in (1, 2, 3, 4)]
    for rnd in range(2):
        a.load(sets[0])
        b.load(sets[1])
        s1.wait_stream(torch.cuda.current_stream())
        s2.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s1):
            a.graph.replay()
        with torch.cuda.stream(s2):
            b.graph.replay()
        torch.cuda.synchronize()
        fam.check(sets[0], a.read())
        fam.check(sets[1], b.read())
        # one replay beside the eager operator on another stream, with other inputs
        a.load(sets[2])
        eager_in = fam.tensors(sets[3], cuda)
        s1.wait_stream(torch.cuda.current_stream())
        s2.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s1):
            a.graph.replay()
        with torch.cuda.stream(s2):
            eager_out = fam.step(*eager_in)
        torch.cuda.synchronize()
        fam.check(sets[2], a.read())
        fam.check(sets[3], [o.detach().cpu().numpy() for o in eager_out])
        sets = sets[2:] + sets[:2]
    if name.startswith("fps"):
        assert sampling.furthest_sampling_status(cuda) == 0


# --------------------------------------------------------------------------------------- 3. concurrent eager streams
CHAIN_N, CHAIN_P, CHAIN_C, CHAIN_R, CHAIN_NS, CHAIN_K = 8192, 512, 8, 0.15, 32, 8


def _chain_inputs(seed):
    n, p, c, ns = CHAIN_N, CHAIN_P, CHAIN_C, CHAIN_NS
    return [S.unit_sphere(seed, 1, n), S.unit_sphere(seed + 1, 1, n), S.normal(seed + 2, (1, n)),
            S.normal(seed + 3, (1, n)), S.normal(seed + 4, (1, c, n)), S.normal(seed + 5, (1, 3 + c, p, ns)),
            S.normal(seed + 6, (1, c, p)), S.normal(seed + 7, (1, c, n))]


def _chain(cuda, arrays):
    """Chamfer forward + backward at a grid shape, FPS, ball query + group (+ backward), three_nn + interpolate
    (+ backward), knn -- on the current stream"""
    from pytorch_points_amd.network.model_loss import nndistance
    from pytorch_points_amd.network.geo_operations import furthest_point_sample
    from pytorch_points_amd.network.operations import QueryAndGroup
    from pytorch_points_amd.network.pointnet2_utils import three_nn as tn, three_interpolate
    from pytorch_points_amd.ops import knn_points
    x1, x2, g1, g2, feats, gq, fc, gi = [torch.from_numpy(a).to(cuda) for a in arrays]
    x1.requires_grad_(True)
    x2.requires_grad_(True)
    feats.requires_grad_(True)
    fc.requires_grad_(True)
    d1, d2, i1, i2 = nndistance(x1, x2)
    gx1, gx2 = _grad([d1, d2], [x1, x2], [g1, g2])
    xd = x1.detach()
    fidx, centres = furthest_point_sample(xd, CHAIN_P, NCHW=False)
    grouped = QueryAndGroup(CHAIN_R, CHAIN_NS)(xd, centres, feats)
    gf, = _grad([grouped], [feats], [gq])
    dist, nidx = tn(xd, centres)
    w = 1.0 / (dist + 1e-8)
    w = (w / w.sum(-1, keepdim=True)).contiguous()
    interp = three_interpolate(fc, nidx, w)
    gfc, = _grad([interp], [fc], [gi])
    kd = knn_points(centres, xd, K=CHAIN_K)
    return [d1, d2, i1, i2, gx1, gx2, fidx, centres, grouped, gf, nidx, w, interp, gfc, kd.dists, kd.idx]


def _check_chain(arrays, out):
    x1, x2, g1, g2, feats, gq, fc, gi = arrays
    out = [o.detach().cpu().numpy() for o in out]
    d1, d2, i1, i2, gx1, gx2, fidx, centres, grouped, gf, nidx, w, interp, gfc, kdist, kidx = out
    e = oracle.chamfer_forward(x1, x2)
    assert np.array_equal(d1, e[0]) and np.array_equal(i1, e[1]) and np.array_equal(d2, e[2]) and np.array_equal(i2, e[3])
    eg = oracle.chamfer_backward(x1, x2, g1, g2, e[1], e[3])
    assert np.allclose(gx1, eg[0], rtol=1e-5, atol=1e-6) and np.allclose(gx2, eg[1], rtol=1e-5, atol=1e-6)
    e_f, _ = oracle.furthest_sampling(x1, CHAIN_P, 0)
    e_c = np.take_along_axis(x1, e_f[..., None].astype(np.int64), 1)
    assert np.array_equal(fidx, e_f) and np.array_equal(centres, e_c)
    bq = oracle.ball_query(e_c, x1, CHAIN_R, CHAIN_NS)
    assert np.array_equal(grouped[:, 3:], oracle.group_points(feats, bq))
    assert np.allclose(gf, oracle.group_points_grad(np.ascontiguousarray(gq[:, 3:]), bq, CHAIN_N), rtol=1e-5, atol=1e-5)
    _, e_n = oracle.three_nn(x1, e_c)
    assert np.array_equal(nidx, e_n)
    assert np.array_equal(interp, oracle.three_interpolate(fc, e_n, w))
    assert np.allclose(gfc, oracle.three_interpolate_grad(gi, e_n, w, CHAIN_P), rtol=1e-5, atol=1e-5)
    e_kd, e_ki = oracle.knn(e_c, x1, CHAIN_K)
    assert np.array_equal(kdist, e_kd) and np.array_equal(kidx, e_ki)


def test_four_streams_run_the_chain_concurrently(cuda):
    _assert_streams_get_their_own_scratch(cuda)
    streams = [torch.cuda.Stream() for _ in range(4)]
    inputs = [_chain_inputs(500 + 10 * i) for i in range(4)]
    last = [None] * 4
    for it in range(3):
        for i, s in enumerate(streams):
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                last[i] = _chain(cuda, inputs[i])
    torch.cuda.synchronize()
    for i in range(4):
        _check_chain(inputs[i], last[i])


def test_twenty_streams_evict_the_scratch_tables(cuda):
    """20 streams in turn, no synchronisation: the Python table (16 entries) drops, and the C++ table (cleared beyond 16)
    forgets, scratch of streams whose work is still in flight"""
    from pytorch_points_amd import _lib
    _assert_streams_get_their_own_scratch(cuda)
    streams = [torch.cuda.Stream() for _ in range(20)]
    inputs = [_chain_inputs(700 + 10 * i) for i in range(20)]
    outs = []
    for i, s in enumerate(streams):
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            outs.append(_chain(cuda, inputs[i]))
    assert len(_lib._WS) <= _lib._WS_MAX
    torch.cuda.synchronize()
    for i in range(20):
        _check_chain(inputs[i], outs[i])


# ------------------------------------------------------------------------------------------- 4. cold capture
COLD_FAMILIES = {
    "chamfer_node_grid": lambda: chamfer(*GRID),
    "chamfer_python_grid": lambda: chamfer(*GRID, fn="python"),
    "chamfer_brute_force": lambda: chamfer(2, 300, 500),
    "chamfer_fp64": lambda: chamfer(2, 300, 500, fn="python", dtype=np.float64),
    "labeled_grid": lambda: labeled(*GRID),
    "fps_bucket": lambda: fps(16, 8192, 200),                 # (automatic: the bucketed kernel)
    "fps_cluster": lambda: fps(4, 70000, 64),                 # (automatic beyond 65536 points: the CU cluster)
    "fps_single_block": lambda: fps(2, 1000, 64),             # (automatic below the cluster's 512 points per workgroup)
    "gather": lambda: gather(9, 16, 16384, 8192),
    "group": lambda: group(4, 16, 4096, 1024, 32),
    "query_and_group": lambda: query_and_group(2, 8, 8192, 512, 0.15, 32),
    "ball_query": lambda: ball_query(2, 8192, 512, 0.1, 32),
    "three_nn_interpolate": lambda: three_nn(2, 8192, 1024, 16),
    "knn_grid": lambda: knn(2, 2048, 8192, 3, 8),
    "knn_nd": lambda: knn(2, 1000, 2000, 24, 17),
    "batch_svd": lambda: svd(256, 32, 32),
    "batch_normals": lambda: normals(2, 2048, 16),
}


def cold_child(name, path):
    """body of a child process: torch warmed up (its autograd engine included), the library untouched; the capture of
    family ``name`` is the library's first call in the process; two replays go to ``path``"""
    from pytorch_points_amd import _lib
    dev = torch.device("cuda:0")
    x = torch.randn(256, device=dev, requires_grad=True)
    (x * x).sum().backward()
    torch.cuda.synchronize()
    fam = COLD_FAMILIES[name]()
    assert _lib._lib is None and _lib._bridge is None, "the library was loaded before the capture"
    cap = Captured(fam, dev, warmup=0)
    res = {}
    for k in (0, 1):
        arrays = fam.make(k)
        for i, o in enumerate(cap.run(arrays)):
            res["out%d_%d" % (k, i)] = o
    np.savez(path, **res)


_CHILD = """import sys
sys.path[:0] = [%r, %r]
import test_gpu_graphs
test_gpu_graphs.cold_child(sys.argv[1], sys.argv[2])
print("cold capture ok")
""" % (ROOT, HERE)


def test_cold_capture_in_fresh_processes(cuda, tmp_path):
    script = tmp_path / "cold_child.py"
    script.write_text(_CHILD)
    env = dict(os.environ)
    env["PYTHONPATH"] = os.pathsep.join([ROOT, HERE] + ([env["PYTHONPATH"]] if env.get("PYTHONPATH") else []))
    flags = ["-s"] if sys.flags.no_user_site else []
    failed = []
    for name in COLD_FAMILIES:
        out = tmp_path / (name + ".npz")
        try:
            r = subprocess.run([sys.executable] + flags + [str(script), name, str(out)], cwd=ROOT, env=env,
                               capture_output=True, text=True, timeout=240)
        except subprocess.TimeoutExpired:
            pytest.fail("cold capture of %s timed out: no further child started" % name)
        if r.returncode < 0:
            pytest.fail("cold capture of %s ended with signal %d: no further child started\n%s" % (
                name, -r.returncode, r.stderr[-3000:]))
        if r.returncode != 0:   # (a HIP error surfaces as an exit status of 1: start nothing more on the device)
            pytest.fail("cold capture of %s failed (exit %d): no further child started\n%s" % (
                name, r.returncode, r.stderr[-3000:]))
        fam = COLD_FAMILIES[name]()
        got = np.load(out)
        for k in (0, 1):
            outs = [got["out%d_%d" % (k, i)] for i in range(len(got.files) // 2)]
            try:
                fam.check(fam.make(k), outs)
            except AssertionError as exc:
                failed.append("%s, input set %d: %r" % (name, k, exc))
    assert not failed, "\n\n".join(failed)
