"""GPU tests of green_coordinates_3D (csrc/green.hip, pp_gc3d_*): accuracy against the reference's own results
(tests/golden/gc_*.npz, tools/gen_gc_golden.py) and against the in-tree torch composition, gradients, layouts,
determinism, memory, graph capture and concurrent streams.

fp64 contract: GC_vertex / GC_face within 1e-10 of the reference's fp64 results on stable rows, exterior_flag
identical, gradients within 1e-8 relative and finite on every row.  fp32 contract, per query and output:
max |x - x64| <= 2 max |x_ref32 - x64| + 1e-5.  Rows the reference decides by rounding (``stable`` False; among them
every query outside the cage, whose row sum is ~0 and whose GC_vertex is raw / (S + 1e-10)) are held to finiteness
of the gradients (DESIGN.md "Green coordinates")."""
import functools
import glob
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from cage_checks import rel_close
from pytorch_points_amd import green

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "gc_*.npz")))


def load(path, dev):
    z = dict(np.load(path))
    faces = torch.from_numpy(z["faces"]).to(dev)
    if z["expand"]:
        faces = faces[:1].expand(z["query"].shape[0], -1, -1)
    return z, faces


def run(fn, q, v, f, Gv=None, Gf=None, n=None):
    """outputs (and with cotangents, the gradients with respect to query and vertices -- or normals, if given)"""
    grad = Gv is not None
    q = q.detach().clone().requires_grad_(grad)
    v = v.detach().clone().requires_grad_(grad and n is None)
    if n is not None:
        n = n.detach().clone().requires_grad_(grad)
    gcv, gcf, ext = fn(q, v, f, face_normals=n)
    res = [gcv.detach(), gcf.detach(), ext]
    if grad:
        res += list(torch.autograd.grad((gcv * Gv).sum() + (gcf * Gf).sum(), (q, v if n is None else n)))
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in res]


kern = green.green_coordinates_3D
comp = green.composition


def row_err(got, ref):
    err = np.abs(got - ref)
    err[np.isnan(got) & np.isnan(ref)] = 0
    return np.nan_to_num(err, nan=np.inf).max(-1, initial=0)


# --------------------------------------------------------------------------------------------- golden fixtures
@pytest.mark.parametrize("path", GOLDEN, ids=lambda p: os.path.basename(p)[3:-4])
def test_golden_fp64(cuda, path):
    z, f = load(path, cuda)
    q = torch.tensor(z["query"], dtype=torch.float64, device=cuda)
    v = torch.tensor(z["vertices"], dtype=torch.float64, device=cuda)
    st = z["stable"]
    Gv = torch.from_numpy(z["Gv"]).double().to(cuda)
    Gf = torch.from_numpy(z["Gf"]).double().to(cuda)
    gcv, gcf, ext, gq, gv = run(kern, q, v, f, Gv, Gf)
    assert (row_err(gcv, z["gcv64"])[st] <= 1e-10).all()
    assert (row_err(gcf, z["gcf64"])[st] <= 1e-10).all()
    np.testing.assert_array_equal(ext, z["ext64"])
    assert np.isfinite(gq).all() and np.isfinite(gv).all()
    fin = np.isfinite(z["gq64"]) & st[..., None]
    rel_close(gq[fin], z["gq64"][fin], 1e-8)
    # the normals passed in
    n = torch.from_numpy(z["normals"]).to(cuda)
    _, _, _, gqn, gn = run(kern, q, v, f, Gv, Gf, n=n)
    assert np.isfinite(gqn).all() and np.isfinite(gn).all()
    fin = np.isfinite(z["gqn64"]) & st[..., None]
    rel_close(gqn[fin], z["gqn64"][fin], 1e-8)
    # normals and vertices take every row's cotangent: against the reference where all of a batch element's rows are
    # stable and finite, against the fp64 composition (pinned to the reference on the CPU) with stable rows only
    for b in range(q.shape[0]):
        if st[b].all() and np.isfinite(z["gn64"][b]).all():
            rel_close(gn[b], z["gn64"][b], 1e-8)
    m = torch.from_numpy(st).to(cuda)[..., None]
    got = run(kern, q, v, f, Gv * m, Gf * m)
    ref = run(comp, q, v, f, Gv * m, Gf * m)
    rel_close(got[3], ref[3], 1e-8)
    rel_close(got[4], ref[4], 1e-8)
    got = run(kern, q, v, f, Gv * m, Gf * m, n=n)
    ref = run(comp, q, v, f, Gv * m, Gf * m, n=n)
    rel_close(got[4], ref[4], 1e-8)


@pytest.mark.parametrize("path", GOLDEN, ids=lambda p: os.path.basename(p)[3:-4])
def test_golden_fp32(cuda, path):
    z, f = load(path, cuda)
    gcv, gcf, ext = run(kern, torch.from_numpy(z["query"]).to(cuda), torch.from_numpy(z["vertices"]).to(cuda), f)
    st = z["stable"]
    for got, r32, r64 in ((gcv, z["gcv32"], z["gcv64"]), (gcf, z["gcf32"], z["gcf64"])):
        bound = 2 * row_err(r32.astype(np.float64), r64) + 1e-5
        err = row_err(got.astype(np.float64), r64)
        assert (err[st] <= bound[st]).all(), (err[st] - bound[st]).max()
    np.testing.assert_array_equal(ext[st], z["ext64"][st])


# --------------------------------------------------------------------------------------------- random sets
@functools.lru_cache(maxsize=None)
def gen():
    import importlib.util
    spec = importlib.util.spec_from_file_location("gen_mvc_golden", os.path.join(ROOT, "tools", "gen_mvc_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def cage(name):
    g = gen()
    return {"octahedron": (g.octahedron, 0.5), "ico1": (lambda: g.icosphere(1), 0.85),
            "ico2": (lambda: g.icosphere(2), 0.9), "star": (g.star, 0.7), "cube": (g.cube, 0.9),
            "ico4": (lambda: g.icosphere(4), 0.9)}[name]


def random_set(name, B, P, seed):
    """(q, v) fp32, faces expanded over B, cotangents (Gv, Gf) and the queries outside the cage"""
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
            rng.normal(size=(B, P, len(f0))), np.stack(outside).reshape(B, P))


RANDOM = [(name, B, P) for name in ("octahedron", "ico1", "ico2", "star", "cube") for B in (1, 3)
          for P in (0, 1, 63, 64, 65, 1000)] + [("ico4", B, P) for B in (1, 2) for P in (1, 65)]


@pytest.mark.parametrize("name,B,P", RANDOM)
def test_random_sets(cuda, name, B, P):
    q32, v32, f, Gv, Gf, outside = random_set(name, B, P, seed=B * 10007 + P)
    f = f.to(cuda)
    q64, v64 = torch.from_numpy(q32).double().to(cuda), torch.from_numpy(v32).double().to(cuda)
    inside = torch.from_numpy(~outside).to(cuda)[..., None]
    Gv, Gf = torch.from_numpy(Gv).to(cuda) * inside, torch.from_numpy(Gf).to(cuda) * inside
    ref = run(comp, q64, v64, f, Gv, Gf)
    got = run(kern, q64, v64, f, Gv, Gf)
    ins = ~outside
    assert (row_err(got[0], ref[0])[ins] <= 1e-10).all()
    assert (row_err(got[1], ref[1]) <= 1e-10).all()                  # GC_face is not divided by the row sum
    np.testing.assert_array_equal(got[2][ins], ref[2][ins])
    assert not got[2][ins].any()
    rel_close(got[3], ref[3], 1e-8)
    rel_close(got[4], ref[4], 1e-8)
    c32 = run(comp, torch.from_numpy(q32).to(cuda), torch.from_numpy(v32).to(cuda), f)
    k32 = run(kern, torch.from_numpy(q32).to(cuda), torch.from_numpy(v32).to(cuda), f)
    for i in (0, 1):
        bound = 2 * row_err(c32[i].astype(np.float64), ref[i]) + 1e-5
        assert (row_err(k32[i].astype(np.float64), ref[i])[ins] <= bound[ins]).all()


@pytest.mark.parametrize("B", [1, 2])
def test_gradcheck_fp64(cuda, B):
    q32, v32, f, _, _, outside = random_set("octahedron", B, 8, seed=5 + B)
    keep = np.flatnonzero(~outside.any(0))[:4]                       # interior queries in every batch element
    q = torch.from_numpy(q32[:, keep]).double().to(cuda).requires_grad_(True)
    v = torch.from_numpy(v32).double().to(cuda).requires_grad_(True)
    f = f.to(cuda)
    # (the vertices reach the pair evaluation detached, as in the reference: only the normals carry their gradient)
    assert torch.autograd.gradcheck(lambda a: kern(a, v.detach(), f)[:2], (q,), eps=1e-6, atol=1e-6, rtol=1e-5)
    n = green.compute_face_normals_and_areas(v.detach(), f)[0].requires_grad_(True)
    assert torch.autograd.gradcheck(lambda a, c: kern(a, v.detach(), f, face_normals=c)[:2], (q, n), eps=1e-6,
                                    atol=1e-6, rtol=1e-5)


def test_query_on_vertex_has_finite_gradient(cuda):
    """the reference's query gradient is NaN on a vertex (0/0 of a discarded branch); here it is that of the branch
    taken, and the composition's is the same"""
    v0, f0 = gen().octahedron()
    q = torch.tensor(v0[None, :3], device=cuda)
    v = torch.tensor(v0[None], device=cuda)
    f = torch.from_numpy(f0)[None].to(cuda)
    Gv, Gf = torch.ones(1, 3, 6, dtype=torch.float64, device=cuda), torch.ones(1, 3, 8, dtype=torch.float64, device=cuda)
    got, ref = run(kern, q, v, f, Gv, Gf), run(comp, q, v, f, Gv, Gf)
    assert np.isfinite(got[3]).all() and np.isfinite(got[4]).all() and got[2].all()
    rel_close(got[3], ref[3], 1e-8)
    rel_close(got[4], ref[4], 1e-8)


def test_bad_index_gives_nan_rows(cuda):
    q32, v32, f, Gv, Gf, _ = random_set("octahedron", 2, 10, seed=1)
    f = f.clone()
    f[1, 3, 1] = 6
    gcv, gcf, ext, gq, gv = run(kern, torch.from_numpy(q32).to(cuda), torch.from_numpy(v32).to(cuda), f.to(cuda),
                                torch.from_numpy(Gv).float().to(cuda), torch.from_numpy(Gf).float().to(cuda))
    assert np.isnan(gcv[1]).all() and np.isnan(gcf[1]).all() and np.isnan(gq[1]).all() and not ext[1].any()
    assert np.isfinite(gcv[0]).all() and np.isfinite(gq[0]).all() and np.isfinite(gv[0]).all()
    f[1, 3, 1] = -1
    assert np.isnan(run(kern, torch.from_numpy(q32).to(cuda), torch.from_numpy(v32).to(cuda), f.to(cuda))[0][1]).all()


def test_empty_sizes_and_non_contiguous(cuda):
    q32, v32, f, Gv, Gf, _ = random_set("ico1", 2, 100, seed=4)
    q, v, f = torch.from_numpy(q32).to(cuda), torch.from_numpy(v32).to(cuda), f.to(cuda)
    out = run(kern, q[:, :0], v, f, torch.zeros(2, 0, 42, device=cuda), torch.zeros(2, 0, 80, device=cuda))
    assert [o.shape for o in out] == [(2, 0, 42), (2, 0, 80), (2, 0, 1), (2, 0, 3), (2, 42, 3)]
    assert (out[4] == 0).all()
    out = run(kern, q, v, f[:, :0], torch.ones(2, 100, 42, device=cuda), torch.zeros(2, 100, 0, device=cuda))
    assert (out[0] == 0).all() and out[1].shape == (2, 100, 0) and out[2].all() and (out[3] == 0).all()
    out = run(kern, q, v[:, :0], f[:, :0])
    assert out[0].shape == (2, 100, 0) and out[2].all()
    # non-contiguous query, vertices, faces and normals
    qn = torch.from_numpy(q32).to(cuda).transpose(1, 2).contiguous().transpose(1, 2)
    vn = torch.stack([v, v], dim=3)[..., 0]
    fn = torch.cat([f, f], dim=2)[..., :3]
    assert not (qn.is_contiguous() or vn.is_contiguous() or fn.is_contiguous())
    Gv, Gf = torch.from_numpy(Gv).float().to(cuda), torch.from_numpy(Gf).float().to(cuda)
    a, b = run(kern, qn, vn, fn, Gv, Gf), run(kern, q, v, f.contiguous(), Gv, Gf)
    assert all(same_bits(x, y) for x, y in zip(a, b))
    n = green.compute_face_normals_and_areas(v, f)[0]
    nn = torch.stack([n, n], dim=3)[..., 0]
    assert not nn.is_contiguous()
    a, b = run(kern, q, v, f, Gv, Gf, n=nn), run(kern, q, v, f, Gv, Gf, n=n)
    assert all(same_bits(x, y) for x, y in zip(a, b))


# --------------------------------------------------------------------------------------------- determinism
def same_bits(x, y):
    if x.dtype == np.bool_:
        return np.array_equal(x, y)
    it = {4: np.int32, 8: np.int64}[x.dtype.itemsize]
    return x.shape == y.shape and np.array_equal(np.ascontiguousarray(x).view(it), np.ascontiguousarray(y).view(it))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("det_mode", [False, True])
def test_bitwise_reproducible(cuda, dtype, det_mode):
    q32, v32, f, Gv, Gf, _ = random_set("ico1", 3, 1100, seed=11)
    q, v, f = torch.from_numpy(q32).to(cuda, dtype), torch.from_numpy(v32).to(cuda, dtype), f.to(cuda)
    Gv, Gf = torch.from_numpy(Gv).to(cuda, dtype), torch.from_numpy(Gf).to(cuda, dtype)
    prev = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(det_mode)
    try:
        a = run(kern, q, v, f, Gv, Gf)
        b = run(kern, q, v, f, Gv, Gf)
    finally:
        torch.use_deterministic_algorithms(prev)
    assert all(same_bits(x, y) for x, y in zip(a, b))
    # a query's row alone equals its row inside P = 1100 and inside B = 3
    for bi, pi in ((0, 0), (1, 513), (2, 1099)):
        one = run(kern, q[bi:bi + 1, pi:pi + 1], v[bi:bi + 1], f[bi:bi + 1])
        assert same_bits(one[0][0, 0], a[0][bi, pi]) and same_bits(one[1][0, 0], a[1][bi, pi])


# --------------------------------------------------------------------------------------------- LDS and global paths
# green.hip keeps a tile's vertex accumulators in LDS while (N + 64) * 65 * sizeof(T) bytes fit in 160 KiB (the 64
# rows are the face tile); above 64 KiB the launch needs the big-LDS attribute.  Padding the ico1 cage with isolated
# vertices far away moves N across each threshold without changing any (query, face) pair.
def thresholds(elem):
    ns = set()
    for cap in (64 << 10, 160 << 10):
        last = cap // (65 * elem) - 64
        ns |= {last, last + 1}
    return ns


PATH_N = sorted(n for n in thresholds(4) | thresholds(8) | {1200} if n >= 42)


@functools.lru_cache(maxsize=None)
def path_baseline(dev, dtype):
    q, v, f, Gv, Gf, _ = random_set("ico1", 3, 200, seed=3)
    gen_ = torch.Generator(device=dev).manual_seed(17)
    G = torch.randn(3, 200, max(PATH_N), dtype=dtype, device=dev, generator=gen_)
    Gf = torch.from_numpy(Gf).to(dev, dtype)
    q, v = torch.from_numpy(q).to(dev, dtype), torch.from_numpy(v).to(dev, dtype)
    return q, v, f[0], G, Gf, run(kern, q, v, f.to(dev), G[..., :42], Gf)


@pytest.mark.parametrize("faces", ["expanded", "per_batch"])
@pytest.mark.parametrize("N", PATH_N)
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_lds_and_global_paths_are_bitwise_equal(cuda, dtype, N, faces):
    q, v, f0, G, Gf, base = path_baseline(cuda, dtype)
    far = torch.stack([50.0 + 0.5 * torch.arange(N - 42, device=cuda, dtype=dtype),
                       torch.full((N - 42,), -40.0, device=cuda, dtype=dtype),
                       torch.full((N - 42,), 30.0, device=cuda, dtype=dtype)], dim=1)
    vp = torch.cat([v, far[None].expand(3, -1, -1)], dim=1)
    f = f0.to(cuda)[None].expand(3, -1, -1)
    if faces == "per_batch":
        f = f.contiguous()
    # normals from the unpadded cage (the padded vertices belong to no face: the same normals)
    gcv, gcf, ext, gq, gv = run(kern, q, vp, f, G[..., :N], Gf)
    assert same_bits(gcv[..., :42], base[0]) and (gcv[..., 42:] == 0).all()
    assert same_bits(gcf, base[1]) and same_bits(ext, base[2]) and same_bits(gq, base[3])
    assert same_bits(gv[:, :42], base[4]) and (gv[:, 42:] == 0).all()


# --------------------------------------------------------------------------------------------- memory
def test_memory_at_neural_cages_size(cuda):
    B, P = 8, 16384
    q32, v32, f, _, _, _ = random_set("ico2", B, P, seed=2)
    q = torch.from_numpy(q32).to(cuda).requires_grad_(True)
    v = torch.from_numpy(v32).to(cuda).requires_grad_(True)
    f = f.to(cuda)
    N, F = v.shape[1], f.shape[1]
    Gv, Gf = torch.randn(B, P, N, device=cuda), torch.randn(B, P, F, device=cuda)
    a, b, _ = kern(q[:, :64], v, f)
    (a.sum() + b.sum()).backward()                                       # library loaded, workspace table warm
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    gcv, gcf, ext = kern(q, v, f)
    gq, gv = torch.autograd.grad((gcv, gcf), (q, v), (Gv, Gf))
    torch.cuda.synchronize()
    growth = torch.cuda.max_memory_allocated() - base
    # outputs and their gradient buffers (B*P*(N+F) each), the workspace (B*256*F*3): no per-pair tensor
    assert growth <= 3 * B * P * (N + F) * 4 + B * 256 * F * 3 * 4 + (64 << 20), growth
    assert torch.isfinite(gq).all() and torch.isfinite(gv).all()


# --------------------------------------------------------------------------------------------- graphs and streams
def _step(q, v, f, Gv, Gf):
    gcv, gcf, ext = kern(q, v, f)
    gq, gv = torch.autograd.grad((gcv, gcf), (q, v), (Gv, Gf))
    return gcv, gcf, ext, gq, gv


def test_graph_capture_replay_matches_eager(cuda):
    q32, v32, f, Gv, Gf, _ = random_set("ico2", 2, 300, seed=21)
    q = torch.from_numpy(q32).to(cuda).requires_grad_(True)
    v = torch.from_numpy(v32).to(cuda).requires_grad_(True)
    f, Gv, Gf = f.to(cuda), torch.from_numpy(Gv).float().to(cuda), torch.from_numpy(Gf).float().to(cuda)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _step(q, v, f, Gv, Gf)                                          # warm
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = _step(q, v, f, Gv, Gf)
    q2, v2, _, _, _, _ = random_set("ico2", 2, 300, seed=22)
    with torch.no_grad():
        q.copy_(torch.from_numpy(q2))
        v.copy_(torch.from_numpy(v2))
    g.replay()
    torch.cuda.synchronize()
    eager = _step(q, v, f, Gv, Gf)
    for a, b in zip(out, eager):
        assert torch.equal(a, b)


COLD = r"""
import sys, numpy as np, torch
sys.path.insert(0, sys.argv[1])
from pytorch_points_amd import green
dev = torch.device("cuda:0")
rng = np.random.default_rng(0)
q = torch.from_numpy(rng.normal(scale=0.3, size=(2, 300, 3)).astype(np.float32)).to(dev).requires_grad_(True)
v0 = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float32)
v = torch.from_numpy(np.stack([v0, v0 * 1.1])).to(dev).requires_grad_(True)
f = torch.tensor([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]],
                 device=dev)[None].expand(2, -1, -1)
Gv, Gf = torch.randn(2, 300, 6, device=dev), torch.randn(2, 300, 8, device=dev)
g = torch.cuda.CUDAGraph()
s = torch.cuda.Stream()
with torch.cuda.stream(s):
    with torch.cuda.graph(g):
        a, b, e = green.green_coordinates_3D(q, v, f)
        gq, gv = torch.autograd.grad((a, b), (q, v), (Gv, Gf))
g.replay()
torch.cuda.synchronize()
a2, b2, e2 = green.green_coordinates_3D(q, v, f)
gq2, gv2 = torch.autograd.grad((a2, b2), (q, v), (Gv, Gf))
assert torch.equal(a, a2) and torch.equal(b, b2) and torch.equal(e, e2) and torch.equal(gq, gq2) and torch.equal(gv, gv2)
print("COLD_OK")
"""


def test_cold_capture_in_fresh_process(cuda, tmp_path):
    script = tmp_path / "cold_gc.py"
    script.write_text(COLD)
    r = subprocess.run([sys.executable, str(script), ROOT], cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0 and "COLD_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def test_two_streams_unsynchronised(cuda):
    inputs = []
    for s in (31, 32):
        q32, v32, f, Gv, Gf, _ = random_set("ico1", 2, 1000, seed=s)
        inputs.append((torch.from_numpy(q32).to(cuda).requires_grad_(True),
                       torch.from_numpy(v32).to(cuda).requires_grad_(True), f.to(cuda),
                       torch.from_numpy(Gv).float().to(cuda), torch.from_numpy(Gf).float().to(cuda)))
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
