"""GPU tests of mean_value_coordinates_3D (csrc/mvc.hip, pp_mvc3d_*): accuracy against the reference's own results
(tests/golden/mvc_*.npz, tools/gen_mvc_golden.py) and against the in-tree torch composition, gradients, determinism,
memory, graph capture and concurrent streams.

fp64 contract: wj / wi within 1e-10 of the reference's fp64 results, gradients within 1e-8 relative.  fp32 contract,
per query: max_j |w - w64| <= 2 max_j |w_ref32 - w64| + 1e-5.  On random sets, fp64 rows of queries outside the cage
within 1e-9 (both fp64 chains lose digits to cancellation there: measured 2e-10), wi relative to the row's largest
face weight.  Gradients against the fp64 composition: 1e-6 relative on the fixtures; on random sets 1e-5 for the query
gradient and 1e-3 for the vertex gradient (measured up to 5e-6 and 1.6e-4, where large per-pair terms cancel outside the
cage); the vertex gradient of the interior queries alone within 1e-8; gradcheck pins the backward itself.  Fixture rows the reference decides by rounding (its
fp64 row moves under a translation of the scene by 1e-9: ``stable`` False) are held to the weaker checks named where
they are used (DESIGN.md "Mean value coordinates")."""
import functools
import glob
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from cage_checks import rel_close, same_bits
from pytorch_points_amd import mvc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "mvc_*.npz")))
INTERIOR, VERTEX, CENTROID = 0, 2, 3


def load(path, dev):
    z = dict(np.load(path))
    faces = torch.from_numpy(z["faces"]).to(dev)
    if z["expand"]:
        faces = faces[:1].expand(z["query"].shape[0], -1, -1)
    return z, faces


def run(q, v, f, G=None, verbose=True, Gwi=None):
    """forward (and backward with cotangent G) of the kernel path; numpy outputs"""
    q = q.detach().clone().requires_grad_(G is not None)
    v = v.detach().clone().requires_grad_(G is not None)
    out = mvc.mean_value_coordinates_3D(q, v, f, verbose=verbose)
    wj, wi = out if verbose else (out, None)
    res = [wj.detach(), None if wi is None else wi.detach()]
    if G is not None:
        outs, grads = [wj], [G]
        if Gwi is not None:
            outs.append(wi)
            grads.append(Gwi)
        res += list(torch.autograd.grad(outs, (q, v), grads))
    torch.cuda.synchronize()
    return [None if t is None else t.cpu().numpy() for t in res]


def comp(q, v, f, G=None, verbose=True):
    q = q.detach().clone().requires_grad_(G is not None)
    v = v.detach().clone().requires_grad_(G is not None)
    wj, wi = mvc.composition(q, v, f, verbose=True)
    res = [wj.detach(), wi.detach()]
    if G is not None:
        res += list(torch.autograd.grad((wj * G).sum(), (q, v)))
    return [t.cpu().numpy() for t in res]


# --------------------------------------------------------------------------------------------- golden fixtures
@pytest.mark.parametrize("path", GOLDEN, ids=lambda p: os.path.basename(p)[4:-4])
def test_golden_fp64(cuda, path):
    z, f = load(path, cuda)
    q = torch.tensor(z["query"], dtype=torch.float64, device=cuda)
    v = torch.tensor(z["vertices"], dtype=torch.float64, device=cuda)
    st = z["stable"]
    G = torch.from_numpy(z["G"] * st[..., None]).to(cuda)      # rows the reference decides by rounding: no cotangent
    wj, wi, gq, gv = run(q, v, f, G)
    np.testing.assert_allclose(wj[st], z["wj64"][st], rtol=0, atol=1e-10)
    np.testing.assert_allclose(wi[st], z["wi64"][st], rtol=0, atol=1e-10)
    # unstable rows: finite wherever the reference's are
    assert np.isfinite(wj[~st][np.isfinite(z["wj64"][~st])]).all()
    assert np.isfinite(gq).all() and np.isfinite(gv).all()
    fin = np.isfinite(z["gq64"]) & st[..., None]
    rel_close(gq[fin], z["gq64"][fin], 1e-8)
    assert (gq[z["kind"] == VERTEX] == 0).all()
    # the vertex gradient: the reference's where finite (every row of its batch element stable), and the fp64
    # composition's (the same formulas, pinned to the reference on the CPU) everywhere
    for b in range(q.shape[0]):
        if st[b].all() and z["gv_stable"][b] and np.isfinite(z["gv64"][b]).all():
            rel_close(gv[b], z["gv64"][b], 1e-6)
    cw, cwi, cq, cv = comp(q, v, f, G)
    rel_close(gv, cv, 1e-6)
    rel_close(gq, cq, 1e-6)


@pytest.mark.parametrize("path", GOLDEN, ids=lambda p: os.path.basename(p)[4:-4])
def test_golden_fp32(cuda, path):
    z, f = load(path, cuda)
    q = torch.from_numpy(z["query"]).to(cuda)
    v = torch.from_numpy(z["vertices"]).to(cuda)
    wj, wi = run(q, v, f)
    st = z["stable"] & np.isfinite(z["wj32"]).all(-1)
    kind = z["kind"]
    bound = 2 * np.abs(z["wj32"] - z["wj64"]).max(-1) + 1e-5
    err = np.abs(wj - z["wj64"]).max(-1)
    assert (err[st] <= bound[st]).all(), (err[st] - bound[st]).max()
    # branch decisions on vertices and face centroids: the same faces contribute, the same rows are one-hot
    sel = (kind == VERTEX) | (kind == CENTROID)
    np.testing.assert_array_equal(wi[sel] != 0, z["wi32"][sel] != 0)
    onehot = z["wj32"] == 1
    np.testing.assert_array_equal(wj[kind == VERTEX] == 1, onehot[kind == VERTEX])
    # linear precision for interior queries (at least 1e-2 from the cage)
    verts = z["vertices"].astype(np.float64)
    diam = max(np.ptp(verts[b], axis=0).max() for b in range(verts.shape[0]))
    rec = np.einsum("bpn,bnc->bpc", wj.astype(np.float64), verts)
    inner = kind == INTERIOR
    assert (np.linalg.norm(rec - z["query"], axis=-1)[inner] <= 1e-4 * diam).all()


# --------------------------------------------------------------------------------------------- random sets
def cage(name):
    import importlib.util
    spec = importlib.util.spec_from_file_location("gen_mvc_golden", os.path.join(ROOT, "tools", "gen_mvc_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    return {"octahedron": (gen.octahedron, 0.5), "ico1": (lambda: gen.icosphere(1), 0.85),
            "ico2": (lambda: gen.icosphere(2), 0.9), "star": (gen.star, 0.7), "cube": (gen.cube, 0.9),
            "ico4": (lambda: gen.icosphere(4), 0.9)}[name]


def random_set(name, B, P, seed):
    make, inner = cage(name)
    v0, f0 = make()
    rng = np.random.default_rng(seed)
    vs, qs, outside = [], [], []
    for b in range(B):
        vs.append(v0 * rng.uniform(0.8, 1.2, 3) + rng.normal(scale=0.05, size=3))
        dirs = rng.normal(size=(P, 3))
        dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
        r = np.where(rng.uniform(size=P) < 0.75, rng.uniform(0.05, 0.75, P) * inner, rng.uniform(1.5, 3.0, P))
        outside.append(r > 1)
        qs.append(vs[-1].mean(0) + dirs * r[:, None])
    return (np.stack(qs).astype(np.float32), np.stack(vs).astype(np.float32),
            torch.from_numpy(f0)[None].expand(B, -1, -1), rng.normal(size=(B, P, len(v0))),
            np.stack(outside).reshape(B, P))


RANDOM = [(name, B, P) for name in ("octahedron", "ico1", "ico2", "star", "cube") for B in (1, 3)
          for P in (0, 1, 63, 64, 65, 1000, 4097)] + [("ico4", B, P) for B in (1, 3) for P in (0, 1, 63, 64, 65)]


@pytest.mark.parametrize("name,B,P", RANDOM)
def test_random_sets(cuda, name, B, P):
    q32, v32, f, G, outside = random_set(name, B, P, seed=B * 10007 + P)
    f = f.to(cuda)
    q64, v64 = torch.from_numpy(q32).double().to(cuda), torch.from_numpy(v32).double().to(cuda)
    Gt = torch.from_numpy(G).to(cuda)
    ref = comp(q64, v64, f, Gt)
    got = run(q64, v64, f, Gt)
    tol = np.where(outside, 1e-9, 1e-10)
    F = f.shape[1]
    assert (np.abs(got[0] - ref[0]).max(-1, initial=0) <= tol).all()
    wi_scale = np.maximum(1.0, np.abs(ref[1]).reshape(B, P, F * 3).max(-1, initial=0))
    assert (np.abs(got[1] - ref[1]).reshape(B, P, F * 3).max(-1, initial=0) <= tol * wi_scale).all()
    rel_close(got[2], ref[2], 1e-5)
    rel_close(got[3], ref[3], 1e-3)
    # the vertex gradient of the queries inside the cage alone, where the per-pair terms do not cancel
    G_in = Gt * torch.from_numpy(~outside).to(cuda)[..., None]
    rel_close(run(q64, v64, f, G_in)[3], comp(q64, v64, f, G_in)[3], 1e-8)
    c32 = comp(torch.from_numpy(q32).to(cuda), torch.from_numpy(v32).to(cuda), f)[0]
    w32 = run(torch.from_numpy(q32).to(cuda), torch.from_numpy(v32).to(cuda), f, verbose=False)[0]
    ref_err = np.abs(c32 - ref[0]).max(-1, initial=0)
    bound = 2 * ref_err + 1e-5
    assert (np.abs(w32 - ref[0]).max(-1, initial=0) <= bound).all()


@pytest.mark.parametrize("B", [1, 2])
def test_gradcheck_fp64(cuda, B):
    q32, v32, f, _, _ = random_set("octahedron", B, 6, seed=5 + B)
    q = torch.from_numpy(q32).double().to(cuda).requires_grad_(True)
    v = torch.from_numpy(v32).double().to(cuda).requires_grad_(True)
    f = f.to(cuda)
    assert torch.autograd.gradcheck(lambda a, b: mvc.mean_value_coordinates_3D(a, b, f, verbose=True), (q, v),
                                    eps=1e-6, atol=1e-6, rtol=1e-5)


def test_wi_cotangent_matches_composition(cuda):
    q32, v32, f, G, _ = random_set("ico1", 2, 100, seed=3)
    f = f.to(cuda)
    q, v = torch.from_numpy(q32).double().to(cuda), torch.from_numpy(v32).double().to(cuda)
    Gwi = torch.randn(2, 100, f.shape[1], 3, dtype=torch.float64, device=cuda)
    Gt = torch.from_numpy(G).to(cuda)
    got = run(q, v, f, Gt, Gwi=Gwi)
    qc, vc = q.clone().requires_grad_(True), v.clone().requires_grad_(True)
    wj, wi = mvc.composition(qc, vc, f, verbose=True)
    gq, gv = torch.autograd.grad((wj * Gt).sum() + (wi * Gwi).sum(), (qc, vc))
    rel_close(got[2], gq.cpu().numpy(), 1e-8)
    rel_close(got[3], gv.cpu().numpy(), 1e-8)


def test_bad_index_gives_nan_rows(cuda):
    q32, v32, f, G, _ = random_set("octahedron", 2, 10, seed=1)
    f = f.clone()
    f[1, 3, 1] = 6
    wj, wi, gq, gv = run(torch.from_numpy(q32).to(cuda), torch.from_numpy(v32).to(cuda), f.to(cuda),
                         torch.from_numpy(G).float().to(cuda))
    assert np.isnan(wj[1]).all() and np.isnan(wi[1]).all() and np.isnan(gq[1]).all() and np.isnan(gv[1]).all()
    assert np.isfinite(wj[0]).all() and np.isfinite(gq[0]).all() and np.isfinite(gv[0]).all()


# --------------------------------------------------------------------------------------------- determinism
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("det_mode", [False, True])
def test_bitwise_reproducible(cuda, dtype, det_mode):
    q32, v32, f, G, _ = random_set("ico2", 3, 4097, seed=11)
    q, v, f = torch.from_numpy(q32).to(cuda, dtype), torch.from_numpy(v32).to(cuda, dtype), f.to(cuda)
    Gt = torch.from_numpy(G).to(cuda, dtype)
    prev = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(det_mode)
    try:
        a = run(q, v, f, Gt)
        b = run(q, v, f, Gt)
    finally:
        torch.use_deterministic_algorithms(prev)
    for x, y in zip(a, b):
        assert np.array_equal(x, y, equal_nan=True)
    # a query's row alone equals its row inside P = 4097 and inside B = 3
    for bi, pi in ((0, 0), (1, 2049), (2, 4096)):
        one = run(q[bi:bi + 1, pi:pi + 1], v[bi:bi + 1], f[bi:bi + 1])
        assert np.array_equal(one[0][0, 0], a[0][bi, pi]) and np.array_equal(one[1][0, 0], a[1][bi, pi])


# --------------------------------------------------------------------------------------------- LDS and global paths
# mvc.hip keeps a tile's accumulators in LDS while they fit: N * 65 * sizeof(T) bytes in the forward, N * 68 *
# sizeof(T) in the backward (fwd_lds, bwd_lds); above 64 KiB the launch needs the big-LDS attribute, above kMaxLds =
# 160 KiB the kernels take the global-memory path (the backward's with a zero-filled workspace).  Padding the ico1 cage
# with isolated vertices far away moves N across each threshold without changing any (query, face) pair.
def lds_thresholds(elem):
    ns = set()
    for words in (65, 68):
        for cap in (64 << 10, 160 << 10):
            last = cap // (words * elem)          # the largest N that fits
            ns |= {last, last + 1}
    return ns


PATH_N = sorted(lds_thresholds(4) | lds_thresholds(8) | {2600})
PATH_CAGE_N, PATH_P = 42, 4097                    # ico1; 65 tiles of 64 queries, the last one partial


@functools.lru_cache(maxsize=None)
def path_set():
    """ico1, B = 3, P = 4097: the random queries of test_random_sets("ico1", 3, 4097) with the first 242 of each batch
    element replaced by the 42 vertices, the 80 face centroids and the 120 edge midpoints of its cage"""
    q, v, f, _, _ = random_set("ico1", 3, PATH_P, seed=3 * 10007 + PATH_P)
    f0 = f[0].numpy()
    edges = np.unique(np.sort(np.concatenate([f0[:, [0, 1]], f0[:, [1, 2]], f0[:, [2, 0]]]), axis=1), axis=0)
    assert v.shape[1] == PATH_CAGE_N and len(f0) == 80 and len(edges) == 120
    for b in range(3):
        vb = v[b].astype(np.float64)
        special = np.concatenate([vb, vb[f0].mean(1), vb[edges].mean(1)]).astype(np.float32)
        q[b, :len(special)] = special
    return q, v, f0


def path_faces(dev, faces):
    """the one face list of path_set on ``dev``: a batch-expanded view (faces_batch_stride 0) or one copy per batch
    element (stride 3 F).  Expanded on the device: ``.to`` would materialise an expanded tensor."""
    f = torch.from_numpy(path_set()[2]).to(dev)[None].expand(3, -1, -1)
    return f.contiguous() if faces == "per_batch" else f


@functools.lru_cache(maxsize=None)
def path_baseline(dev, dtype):
    """cotangents for the largest N (the first 42 columns are the unpadded run's) and the unpadded run itself"""
    q, v, f0 = path_set()
    gen = torch.Generator(device=dev).manual_seed(17)
    G = torch.randn(3, PATH_P, max(PATH_N), dtype=dtype, device=dev, generator=gen)
    Gwi = torch.randn(3, PATH_P, len(f0), 3, dtype=dtype, device=dev, generator=gen)
    q, v = torch.from_numpy(q).to(dev, dtype), torch.from_numpy(v).to(dev, dtype)
    return G, Gwi, run(q, v, path_faces(dev, "expanded"), G[..., :PATH_CAGE_N], Gwi=Gwi)


@pytest.mark.parametrize("faces", ["expanded", "per_batch"])
@pytest.mark.parametrize("N", PATH_N)
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_lds_and_global_paths_are_bitwise_equal(cuda, dtype, N, faces):
    """Every query row is the same bits on the LDS and the global path (mvc.hip's header): the cage padded to N
    vertices gives the unpadded run's wj, wi and both gradients, and zeros for the isolated vertices.  The unpadded
    run's random queries are held to the fp64 composition by test_random_sets("ico1", 3, 4097)."""
    q, v, _ = path_set()
    G, Gwi, (wj0, wi0, gq0, gv0) = path_baseline(cuda, dtype)
    far = np.stack([50.0 + 0.5 * np.arange(N - PATH_CAGE_N), np.full(N - PATH_CAGE_N, -40.0),
                    np.full(N - PATH_CAGE_N, 30.0)], axis=1)
    vp = np.concatenate([v, np.broadcast_to(far, (3,) + far.shape)], axis=1)
    wj, wi, gq, gv = run(torch.from_numpy(q).to(cuda, dtype), torch.from_numpy(vp).to(cuda, dtype),
                         path_faces(cuda, faces), G[..., :N], Gwi=Gwi)
    assert same_bits(wj[..., :PATH_CAGE_N], wj0) and (wj[..., PATH_CAGE_N:] == 0).all()
    assert same_bits(wi, wi0)
    assert same_bits(gq, gq0)
    assert same_bits(gv[:, :PATH_CAGE_N], gv0) and (gv[:, PATH_CAGE_N:] == 0).all()


# --------------------------------------------------------------------------------------------- memory
def test_memory_at_neural_cages_size(cuda):
    B, P = 8, 16384
    q32, v32, f, _, _ = random_set("ico2", B, P, seed=2)
    q = torch.from_numpy(q32).to(cuda).requires_grad_(True)
    v = torch.from_numpy(v32).to(cuda).requires_grad_(True)
    f = f.to(cuda)
    N = v.shape[1]
    G = torch.randn(B, P, N, device=cuda)
    mvc.mean_value_coordinates_3D(q[:, :64], v, f).sum().backward()     # library loaded, workspace table warm
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    wj = mvc.mean_value_coordinates_3D(q, v, f)
    gq, gv = torch.autograd.grad(wj, (q, v), G)
    torch.cuda.synchronize()
    growth = torch.cuda.max_memory_allocated() - base
    assert growth <= 4 * B * P * N * 4 + (64 << 20), growth
    assert torch.isfinite(gq).all() and torch.isfinite(gv).all()


# --------------------------------------------------------------------------------------------- graphs and streams
def _step(q, v, f, G):
    wj = mvc.mean_value_coordinates_3D(q, v, f)
    gq, gv = torch.autograd.grad(wj, (q, v), G)
    return wj, gq, gv


def test_graph_capture_replay_matches_eager(cuda):
    q32, v32, f, G, _ = random_set("ico2", 2, 1000, seed=21)
    q = torch.from_numpy(q32).to(cuda).requires_grad_(True)
    v = torch.from_numpy(v32).to(cuda).requires_grad_(True)
    f, G = f.to(cuda), torch.from_numpy(G).float().to(cuda)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _step(q, v, f, G)                                                   # warm
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = _step(q, v, f, G)
    q2, v2, _, _, _ = random_set("ico2", 2, 1000, seed=22)
    with torch.no_grad():
        q.copy_(torch.from_numpy(q2))
        v.copy_(torch.from_numpy(v2))
    g.replay()
    torch.cuda.synchronize()
    eager = _step(q, v, f, G)
    for a, b in zip(out, eager):
        assert torch.equal(a, b)


COLD = r"""
import sys, numpy as np, torch
sys.path.insert(0, sys.argv[1])
from pytorch_points_amd import mvc
dev = torch.device("cuda:0")
rng = np.random.default_rng(0)
q = torch.from_numpy(rng.normal(scale=0.3, size=(2, 300, 3)).astype(np.float32)).to(dev).requires_grad_(True)
v0 = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float32)
v = torch.from_numpy(np.stack([v0, v0 * 1.1])).to(dev).requires_grad_(True)
f = torch.tensor([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]],
                 device=dev)[None].expand(2, -1, -1)
G = torch.randn(2, 300, 6, device=dev)
g = torch.cuda.CUDAGraph()
s = torch.cuda.Stream()
with torch.cuda.stream(s):
    with torch.cuda.graph(g):
        wj = mvc.mean_value_coordinates_3D(q, v, f)
        gq, gv = torch.autograd.grad(wj, (q, v), G)
g.replay()
torch.cuda.synchronize()
wj2 = mvc.mean_value_coordinates_3D(q, v, f)
gq2, gv2 = torch.autograd.grad(wj2, (q, v), G)
assert torch.equal(wj, wj2) and torch.equal(gq, gq2) and torch.equal(gv, gv2)
print("COLD_OK")
"""


def test_cold_capture_in_fresh_process(cuda, tmp_path):
    script = tmp_path / "cold_mvc.py"
    script.write_text(COLD)
    r = subprocess.run([sys.executable, str(script), ROOT], cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0 and "COLD_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def test_two_streams_unsynchronised(cuda):
    sets = [random_set("ico1", 2, 3000, seed=s) for s in (31, 32)]
    inputs = []
    for q32, v32, f, G, _ in sets:
        inputs.append((torch.from_numpy(q32).to(cuda).requires_grad_(True),
                       torch.from_numpy(v32).to(cuda).requires_grad_(True), f.to(cuda),
                       torch.from_numpy(G).float().to(cuda)))
    eager = [_step(*x) for x in inputs]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs = [None, None]
    for _ in range(3):
        for i in range(2):
            streams[i].wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(streams[i]):
                outs[i] = _step(*inputs[i])
    torch.cuda.synchronize()
    for i in range(2):
        for a, b in zip(outs[i], eager[i]):
            assert torch.equal(a, b)
