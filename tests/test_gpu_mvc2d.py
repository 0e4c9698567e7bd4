"""GPU tests of the 2-D mean_value_coordinates (csrc/mvc2d.hip, pp_mvc2d_*): accuracy against the reference's own
results (tests/golden/mvc2d_*.npz, tools/gen_mvc2d_golden.py) and against the in-tree torch composition, gradients,
determinism, graph capture and concurrent streams.

fp64 contract, on the rows the reference does not decide by rounding (``stable``): phi and w within
1e-10 max(1, max_j |.|) of the reference's fp64 row, gradients within 1e-8 of the same scale.  fp32 contract,
per query: max_j |w - w64| <= 2 max_j |w_ref32 - w64| + 1e-5 max(1, max_j |w64_j|).  These are the 3-D operator's
bounds (DESIGN.md "Mean value coordinates, 2-D")."""
import glob
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from cage_checks import same_bits
from pytorch_points_amd import mvc2d

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "mvc2d_*.npz")))
INTERIOR, EXTERIOR, FAR10, FAR100, VERTEX, EDGE, EXTENSION, CENTROID, NEAR_EDGE, NEAR_VERTEX = range(10)


def run(q, p, G=None, Gw=None, fn=mvc2d.mean_value_coordinates):
    """forward (and backward with the cotangents G of phi and Gw of w); numpy outputs [phi, w, gq, gp]"""
    q = q.detach().clone().requires_grad_(G is not None)
    p = p.detach().clone().requires_grad_(G is not None)
    phi, w = fn(q, p, verbose=True)
    res = [phi.detach(), w.detach()]
    if G is not None:
        outs, grads = [phi], [G]
        if Gw is not None:
            outs.append(w)
            grads.append(Gw)
        res += list(torch.autograd.grad(outs, (q, p), grads))
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in res]


def comp(q, p, G=None, Gw=None):
    return run(q, p, G, Gw, fn=mvc2d.composition)


def row_scale(ref):
    """max(1, max_j |ref_j|) per query row of a (B,M,N) array -> (B,1,N)"""
    return np.maximum(1.0, np.abs(ref).max(1, keepdims=True))


# --------------------------------------------------------------------------------------------- golden fixtures
@pytest.mark.parametrize("path", GOLDEN, ids=lambda p: os.path.basename(p)[6:-4])
def test_golden_fp64(cuda, path):
    z = dict(np.load(path))
    q = torch.tensor(z["points"], dtype=torch.float64, device=cuda)
    p = torch.tensor(z["polygon"], dtype=torch.float64, device=cuda)
    st = z["stable"][:, None, :]
    phi, w, gq, gp = run(q, p, torch.from_numpy(z["G"]).to(cuda))          # G is zero on the unstable rows
    worst = []
    for got, ref in ((phi, z["phi64"]), (w, z["w64"])):
        rel = np.where(st, np.abs(got - ref) / row_scale(ref), 0.0)
        worst.append(rel.max())
        # unstable rows: finite wherever the reference's are
        assert np.isfinite(got[np.broadcast_to(~st, got.shape) & np.isfinite(ref)]).all()
    # "the same scale": a query's gradient against max(1, max_j |phi_j|) of its row, the polygon's (a sum over the
    # stable rows of its batch element; G is zero on the others) against the largest such scale among them
    scale = row_scale(z["phi64"])[:, 0]                                      # (B,N)
    big = np.where(z["stable"], scale, 1.0).max(1)                           # (B,)
    gworst = [(np.abs(gq - z["gq64"]).max(1) / scale).max(), (np.abs(gp - z["gp64"]).reshape(len(big), -1).max(1) / big).max()]
    print("fp64 golden %s: phi %.3g w %.3g (bound 1e-10) | grad points %.3g polygon %.3g (bound 1e-8)"
          % (os.path.basename(path), worst[0], worst[1], gworst[0], gworst[1]))
    assert max(worst) <= 1e-10, worst
    assert np.isfinite(gq).all() and np.isfinite(gp).all()
    assert max(gworst) <= 1e-8, gworst
    assert (gq.transpose(0, 2, 1)[z["kind"] == VERTEX] == 0).all()


@pytest.mark.parametrize("path", GOLDEN, ids=lambda p: os.path.basename(p)[6:-4])
def test_golden_fp32(cuda, path):
    z = dict(np.load(path))
    q = torch.from_numpy(z["points"]).to(cuda)
    p = torch.from_numpy(z["polygon"]).to(cuda)
    phi, w = run(q, p)
    kind = z["kind"]
    st = z["stable"] & np.isfinite(z["phi32"]).all(1) & np.isfinite(z["w32"]).all(1)
    for name, got, ref32, ref64 in (("phi", phi, z["phi32"], z["phi64"]), ("w", w, z["w32"], z["w64"])):
        ref_err = np.abs(ref32 - ref64).max(1)
        err = np.abs(got - ref64).max(1)
        bound = 2 * ref_err + 1e-5 * row_scale(ref64)[:, 0]
        for far in (FAR10, FAR100):       # every row of the kind: at 100 x the reference's fp64 rows are unstable at
            sel = (kind == far) & np.isfinite(ref32).all(1)   # the 1e-7 level, far below either fp32 error
            print("fp32 golden %s %s kind %d: kernel error max %.3g median %.3g | reference fp32 error max %.3g median "
                  "%.3g | ratio of the medians %.3g" % (os.path.basename(path), name, far, err[sel].max(),
                                                        np.median(err[sel]), ref_err[sel].max(),
                                                        np.median(ref_err[sel]),
                                                        np.median(ref_err[sel]) / max(np.median(err[sel]), 1e-300)))
        print("fp32 golden %s %s: worst err / bound %.3g" % (os.path.basename(path), name, (err[st] / bound[st]).max()))
        assert (err[st] <= bound[st]).all(), (name, np.argwhere(st & (err > bound)), (err[st] / bound[st]).max())
    # branch decisions on vertices, edge midpoints and the centroid: the same entries are zero, the same rows one-hot
    sel = np.isin(kind, (VERTEX, EDGE, CENTROID))
    got_rows, ref_rows = w.transpose(0, 2, 1)[sel], z["w32"].transpose(0, 2, 1)[sel]
    np.testing.assert_array_equal(got_rows != 0, ref_rows != 0)
    vert = kind == VERTEX
    np.testing.assert_array_equal(phi.transpose(0, 2, 1)[vert] == 1, z["phi32"].transpose(0, 2, 1)[vert] == 1)
    assert (phi.transpose(0, 2, 1)[vert].sum(-1) == 1).all()


# --------------------------------------------------------------------------------------------- random sets
def random_set(B, N, M, seed):
    """random star-shaped polygons (B,2,M) and queries (B,2,N) in and around them, fp32 values; cotangents (B,M,N)"""
    rng = np.random.default_rng(seed)
    ang = 2 * np.pi * (np.arange(M) + 0.8 * (rng.uniform(size=(B, M)) - 0.5)) / M       # strictly increasing
    rad = rng.uniform(0.6, 1.4, (B, M))
    centre = rng.normal(scale=0.2, size=(B, 2, 1))
    poly = centre + np.stack([rad * np.cos(ang), rad * np.sin(ang)], 1)
    qa = rng.uniform(0, 2 * np.pi, (B, N))
    qr = np.where(rng.uniform(size=(B, N)) < 0.7, rng.uniform(0.02, 0.5, (B, N)), rng.uniform(1.6, 3.0, (B, N)))
    pts = centre + np.stack([qr * np.cos(qa), qr * np.sin(qa)], 1)
    return pts.astype(np.float32), poly.astype(np.float32), rng.normal(size=(B, M, N)), rng.normal(size=(B, M, N))


RANDOM = [(B, N, M) for B in (1, 3) for N in (1, 63, 64, 65, 130) for M in (3, 4, 63, 64, 65, 200)]


@pytest.mark.parametrize("B,N,M", RANDOM)
def test_random_sets(cuda, B, N, M):
    """Values and both gradients against the fp64 composition on the device.  Both are fp64 evaluations of the same
    chain in different summation orders, so they differ by rounding times the chain's conditioning: a weight row is
    held to 1e-10 of its largest entry (the golden bound), a gradient to 1e-8 of its largest entry."""
    q32, p32, G, Gw = random_set(B, N, M, seed=B * 10007 + N * 101 + M)
    q, p = torch.from_numpy(q32).double().to(cuda), torch.from_numpy(p32).double().to(cuda)
    Gt, Gwt = torch.from_numpy(G).to(cuda), torch.from_numpy(Gw).to(cuda)
    ref = comp(q, p, Gt, Gwt)
    got = run(q, p, Gt, Gwt)
    for i in (0, 1):
        assert (np.abs(got[i] - ref[i]) <= 1e-10 * row_scale(ref[i])).all(), np.abs(got[i] - ref[i]).max()
    for i in (2, 3):
        assert got[i].shape == ref[i].shape
        assert np.abs(got[i] - ref[i]).max() <= 1e-8 * max(1.0, np.abs(ref[i]).max()), (i, np.abs(got[i] - ref[i]).max())
    # fp32 data: the project's rule against the fp32 composition's own error
    c32 = comp(q.float(), p.float())[0]
    k32 = run(q.float(), p.float())[0]
    bound = 2 * np.abs(c32 - ref[0]).max(1) + 1e-5 * row_scale(ref[0])[:, 0]
    assert (np.abs(k32 - ref[0]).max(1) <= bound).all()


@pytest.mark.parametrize("B", [1, 2])
def test_gradcheck_fp64(cuda, B):
    q32, p32, _, _ = random_set(B, 5, 6, seed=40 + B)
    q = torch.from_numpy(q32).double().to(cuda).requires_grad_(True)
    p = torch.from_numpy(p32).double().to(cuda).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda a, b: mvc2d.mean_value_coordinates(a, b, verbose=True), (q, p),
                                    eps=1e-6, atol=1e-6, rtol=1e-5)


def test_w_cotangent_matches_composition(cuda):
    q32, p32, G, Gw = random_set(2, 100, 12, seed=3)
    q, p = torch.from_numpy(q32).double().to(cuda), torch.from_numpy(p32).double().to(cuda)
    zero = torch.zeros(2, 12, 100, dtype=torch.float64, device=cuda)
    Gwt = torch.from_numpy(Gw).to(cuda)
    got, ref = run(q, p, zero, Gwt), comp(q, p, zero, Gwt)               # the cotangent of w alone
    for i in (2, 3):
        assert np.abs(ref[i]).max() > 0
        assert np.abs(got[i] - ref[i]).max() <= 1e-8 * max(1.0, np.abs(ref[i]).max())


def test_special_rows_gradients_match_composition(cuda):
    """the hand-written backward on the rows the plain random sets do not hold: on an edge (with the path through the
    edge's length), on an edge's extension, on a vertex, and a zero-sum row"""
    z = dict(np.load([g for g in GOLDEN if g.endswith("star12.npz")][0]))
    sel = np.isin(z["kind"][0], (VERTEX, EDGE, EXTENSION, NEAR_EDGE, NEAR_VERTEX, INTERIOR))
    q = torch.tensor(z["points"][:, :, sel], dtype=torch.float64, device=cuda)
    p = torch.tensor(z["polygon"], dtype=torch.float64, device=cuda)
    q = torch.cat([q, q * 1e-9 + 5.0], dim=2)              # far from a polygon scaled below: zero-sum rows
    scale = torch.tensor([1.0, 1e-7], dtype=torch.float64, device=cuda).reshape(2, 1, 1)
    q, p = q.expand(2, -1, -1) * 1.0, p.expand(2, -1, -1) * scale
    gen = torch.Generator(device=cuda).manual_seed(5)
    G = torch.randn(2, p.shape[2], q.shape[2], dtype=torch.float64, device=cuda, generator=gen)
    Gw = torch.randn(2, p.shape[2], q.shape[2], dtype=torch.float64, device=cuda, generator=gen)
    got, ref = run(q, p, G, Gw), comp(q, p, G, Gw)
    assert (ref[1][1].sum(0) == 0).any() and (got[1][1].sum(0) == 0).sum() == (ref[1][1].sum(0) == 0).sum()
    for i in (0, 1):
        assert (np.abs(got[i] - ref[i]) <= 1e-10 * row_scale(ref[i])).all()
    for i in (2, 3):
        assert np.isfinite(got[i]).all()
        assert np.abs(got[i] - ref[i]).max() <= 1e-8 * max(1.0, np.abs(ref[i]).max()), (i, np.abs(got[i] - ref[i]).max())


# --------------------------------------------------------------------------------------------- determinism
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("det_mode", [False, True])
def test_bitwise_reproducible_and_rows_independent(cuda, dtype, det_mode):
    q32, p32, G, Gw = random_set(3, 130, 65, seed=11)
    q, p = torch.from_numpy(q32).to(cuda, dtype), torch.from_numpy(p32).to(cuda, dtype)
    Gt, Gwt = torch.from_numpy(G).to(cuda, dtype), torch.from_numpy(Gw).to(cuda, dtype)
    prev = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(det_mode)
    try:
        runs = [run(q, p, Gt, Gwt) for _ in range(3)]
    finally:
        torch.use_deterministic_algorithms(prev)
    for other in runs[1:]:
        for x, y in zip(runs[0], other):
            assert same_bits(x, y)
    # the query at position 70 of 130: the same forward row alone (N = 1) and in a batch of 1
    for b in range(3):
        alone = run(q[b:b + 1, :, 70:71], p[b:b + 1])
        assert same_bits(alone[0][0, :, 0], runs[0][0][b, :, 70]) and same_bits(alone[1][0, :, 0], runs[0][1][b, :, 70])


# --------------------------------------------------------------------------------------------- graphs and streams
def _step(q, p, G):
    phi = mvc2d.mean_value_coordinates(q, p)
    gq, gp = torch.autograd.grad(phi, (q, p), G)
    return phi, gq, gp


def test_graph_capture_replay_matches_eager(cuda):
    q32, p32, G, _ = random_set(2, 130, 20, seed=21)
    q = torch.from_numpy(q32).to(cuda).requires_grad_(True)
    p = torch.from_numpy(p32).to(cuda).requires_grad_(True)
    G = torch.from_numpy(G).float().to(cuda)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _step(q, p, G)                                                      # warm
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = _step(q, p, G)
    q2, p2, _, _ = random_set(2, 130, 20, seed=22)
    with torch.no_grad():
        q.copy_(torch.from_numpy(q2))
        p.copy_(torch.from_numpy(p2))
    g.replay()
    torch.cuda.synchronize()
    eager = _step(q, p, G)
    for a, b in zip(out, eager):
        assert torch.equal(a, b)


COLD = r"""
import sys, numpy as np, torch
sys.path.insert(0, sys.argv[1])
from pytorch_points_amd import mvc2d
dev = torch.device("cuda:0")
rng = np.random.default_rng(0)
ang = 2 * np.pi * np.arange(7) / 7
poly = np.stack([np.stack([np.cos(ang), np.sin(ang)]), np.stack([1.2 * np.cos(ang), 0.8 * np.sin(ang)])])
p = torch.from_numpy(poly.astype(np.float32)).to(dev).requires_grad_(True)
q = torch.from_numpy(rng.normal(scale=0.3, size=(2, 2, 130)).astype(np.float32)).to(dev).requires_grad_(True)
G = torch.randn(2, 7, 130, device=dev)
g = torch.cuda.CUDAGraph()
s = torch.cuda.Stream()
with torch.cuda.stream(s):
    with torch.cuda.graph(g):
        phi = mvc2d.mean_value_coordinates(q, p)
        gq, gp = torch.autograd.grad(phi, (q, p), G)
g.replay()
torch.cuda.synchronize()
phi2 = mvc2d.mean_value_coordinates(q, p)
gq2, gp2 = torch.autograd.grad(phi2, (q, p), G)
assert torch.equal(phi, phi2) and torch.equal(gq, gq2) and torch.equal(gp, gp2)
assert torch.isfinite(phi).all() and float(phi.sum(1).sub(1).abs().max()) < 1e-4
print("COLD_OK")
"""


def test_cold_capture_in_fresh_process(cuda, tmp_path):
    script = tmp_path / "cold_mvc2d.py"
    script.write_text(COLD)
    r = subprocess.run([sys.executable, str(script), ROOT], cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0 and "COLD_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def test_two_streams_unsynchronised(cuda):
    inputs = []
    for seed in (31, 32):
        q32, p32, G, _ = random_set(2, 1000, 33, seed=seed)
        inputs.append((torch.from_numpy(q32).to(cuda).requires_grad_(True),
                       torch.from_numpy(p32).to(cuda).requires_grad_(True), torch.from_numpy(G).float().to(cuda)))
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


# --------------------------------------------------------------------------------------------- inputs
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_nonfinite_inputs_give_nan_rows(cuda, dtype):
    q32, p32, G, _ = random_set(2, 70, 9, seed=51)
    q, p = torch.from_numpy(q32).to(cuda, dtype), torch.from_numpy(p32).to(cuda, dtype)
    Gt = torch.from_numpy(G).to(cuda, dtype)
    clean = run(q, p, Gt)
    qb = q.clone()
    qb[0, 0, 3] = float("nan")
    qb[0, 1, 66] = float("inf")
    pb = p.clone()
    pb[1, 0, 4] = float("-inf")
    phi, w, gq, gp = run(qb, pb, Gt)
    assert np.isnan(phi[0, :, 3]).all() and np.isnan(phi[0, :, 66]).all() and np.isnan(w[0, :, 3]).all()
    assert np.isnan(phi[1]).all() and np.isnan(w[1]).all()
    keep = np.setdiff1d(np.arange(70), [3, 66])
    assert same_bits(phi[0][:, keep], clean[0][0][:, keep]) and same_bits(gq[0][:, keep], clean[2][0][:, keep])
    assert np.isfinite(gq).all() and np.isfinite(gp).all()        # a NaN row is a constant: it passes no gradient
    again = run(q, p, Gt)                                          # the next call on the stream is unaffected
    for x, y in zip(again, clean):
        assert same_bits(x, y)


def test_empty_and_noncontiguous_inputs(cuda):
    q32, p32, G, _ = random_set(2, 70, 9, seed=52)
    q, p = torch.from_numpy(q32).to(cuda), torch.from_numpy(p32).to(cuda)
    for qq, pp in ((q[:, :, :0], p), (q, p[:, :, :0])):
        qq, pp = qq.clone().requires_grad_(True), pp.clone().requires_grad_(True)
        phi, w = mvc2d.mean_value_coordinates(qq, pp, verbose=True)
        assert phi.shape == (2, pp.shape[2], qq.shape[2]) == w.shape and phi.requires_grad
        gq, gp = torch.autograd.grad(phi.sum() + w.sum(), (qq, pp))
        assert (gq == 0).all() and (gp == 0).all()
    assert mvc2d.mean_value_coordinates(q[:0], p[:0]).shape == (0, 9, 70)
    # transposed views (the points-last layout of the rest of the library) are accepted
    qt = q.transpose(1, 2).contiguous().transpose(1, 2)
    pt = p.transpose(1, 2).contiguous().transpose(1, 2)
    assert not qt.is_contiguous() and not pt.is_contiguous()
    Gt = torch.from_numpy(G).float().to(cuda)
    for x, y in zip(run(qt, pt, Gt), run(q, p, Gt)):
        assert same_bits(x, y)
    # a non-contiguous cotangent too
    Gs = torch.from_numpy(G).float().to(cuda).transpose(1, 2).contiguous().transpose(1, 2)
    for x, y in zip(run(q, p, Gs), run(q, p, Gt)):
        assert same_bits(x, y)
