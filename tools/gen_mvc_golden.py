"""Writes tests/golden/mvc_*.npz: mean value coordinates computed by the reference's own
``network.geo_operations.mean_value_coordinates_3D`` on CPU torch.  CPU machine only.

    python tools/gen_mvc_golden.py <reference checkout>

The reference module is read from the checkout at run time (nothing of it is stored here); its compiled ``_ext``
and the ``pytorch3d`` and ``scipy`` imports, which the function does not use, are replaced by empty modules.

Per fixture: query (B,P,3) fp32, vertices (B,N,3) fp32, faces (B,F,3) int64 (``expand``: the tests pass faces[:1]
expanded over B), ``kind`` (B,P) of each query (KINDS), the reference's wj / wi in fp64 (inputs upcast) and in fp32,
a cotangent G (B,P,N) and the reference's fp64 gradients of sum(G * wj) (NaN kept), and ``stable`` (B,P): the
reference's fp64 row moves by at most 1e-9 (and its gradient by 1e-6 relative) when the whole scene is translated by
a few 1e-9, or the queries alone by ~1e-11 -- where it does not, the reference's answer is decided by rounding.
"""
import importlib
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden")
KINDS = {"interior": 0, "exterior": 1, "vertex": 2, "centroid": 3, "edge": 4, "coplanar": 5, "near": 6}


def load_reference(checkout):
    pkg_dir = os.path.join(checkout, "pytorch_points")
    if not os.path.isdir(pkg_dir):
        raise SystemExit("%s has no pytorch_points/ directory" % checkout)
    for name in [n for n in sys.modules if n == "pytorch_points" or n.startswith("pytorch_points.")]:
        del sys.modules[name]

    def stub(name, **attrs):
        mod = types.ModuleType(name)
        mod.__path__ = []
        mod.__dict__.update(attrs)
        sys.modules[name] = mod
        return mod

    for name in ["pytorch3d", "pytorch3d.ops", "scipy", "scipy.sparse"]:
        stub(name)
    sys.modules["pytorch3d"].ops = sys.modules["pytorch3d.ops"]
    sys.modules["scipy"].sparse = sys.modules["scipy.sparse"]
    top = stub("pytorch_points")
    top.__path__ = [pkg_dir]
    ext = stub("pytorch_points._ext", sampling=stub("pytorch_points._ext.sampling"),
               linalg=stub("pytorch_points._ext.linalg"), losses=stub("pytorch_points._ext.losses"))
    top._ext = ext
    stub("pytorch_points.misc", logger=stub("pytorch_points.misc.logger"))
    return importlib.import_module("pytorch_points.network.geo_operations").mean_value_coordinates_3D


# ------------------------------------------------------------------------------------------------ cages
def octahedron():
    v = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float64)
    f = [[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]]
    return v, np.array(f, np.int64)


def icosphere(level):
    t = (1 + 5 ** 0.5) / 2
    v = [[-1, t, 0], [1, t, 0], [-1, -t, 0], [1, -t, 0], [0, -1, t], [0, 1, t], [0, -1, -t], [0, 1, -t],
         [t, 0, -1], [t, 0, 1], [-t, 0, -1], [-t, 0, 1]]
    f = [[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6],
         [7, 1, 8], [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10],
         [8, 6, 7], [9, 8, 1]]
    v = [list(np.array(p) / np.linalg.norm(p)) for p in v]
    for _ in range(level):
        mid = {}

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = (np.array(v[a]) + np.array(v[b])) / 2
                v.append(list(p / np.linalg.norm(p)))
                mid[key] = len(v) - 1
            return mid[key]

        nf = []
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [[a, ab, ca], [b, bc, ab], [c, ca, bc], [ab, bc, ca]]
        f = nf
    return np.array(v, np.float64), np.array(f, np.int64)


def star():
    v, f = icosphere(1)
    radius = np.where(np.arange(len(v)) < 12, 1.6, 0.8)       # the 12 icosahedron corners pushed out: non-convex
    return v * radius[:, None], f


def cube():
    v = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], np.float64)
    f = [[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4],
         [1, 5, 7], [1, 7, 3]]
    return v, np.array(f, np.int64)


def queries(rng, v, f, inner, coplanar=None):
    """(P,3) fp32 queries and their kinds for the cage (v, f); ``inner``: radius of a ball inside the cage"""
    pts, kinds = [], []

    def add(p, kind):
        pts.append(np.asarray(p, np.float64))
        kinds.append(KINDS[kind])

    for _ in range(12):
        dvec = rng.normal(size=3)
        add(dvec / np.linalg.norm(dvec) * inner * rng.uniform(0.05, 0.9), "interior")
    for _ in range(6):
        dvec = rng.normal(size=3)
        add(dvec / np.linalg.norm(dvec) * np.abs(v).max() * rng.uniform(1.8, 3.0), "exterior")
    for j in rng.choice(len(v), 3, replace=False):
        add(v[j], "vertex")
    for k in rng.choice(len(f), 4, replace=False):
        add(v[f[k]].mean(0), "centroid")
    for k in rng.choice(len(f), 3, replace=False):
        add((v[f[k][0]] + v[f[k][1]]) / 2, "edge")
    for k in rng.choice(len(f), 3, replace=False):
        a, b, c = v[f[k]]
        add(a + 1.5 * (b - a) + 0.7 * (c - a), "coplanar")        # in the face's plane, outside the triangle
    for p in coplanar or []:
        add(p, "coplanar")
    for k in rng.choice(len(f), 4, replace=False):
        a, b, c = v[f[k]]
        n = np.cross(b - a, c - a)
        add((a + b + c) / 3 + rng.choice([-1, 1]) * 1e-3 * n / np.linalg.norm(n), "near")
    return np.stack(pts).astype(np.float32), np.array(kinds, np.int8)


# ------------------------------------------------------------------------------------------------ recording
def run(mvc, q, v, f, dtype, grad_of=None):
    qt = torch.tensor(q, dtype=dtype, requires_grad=grad_of is not None)
    vt = torch.tensor(v, dtype=dtype, requires_grad=grad_of is not None)
    wj, wi = mvc(qt, vt, f, verbose=True)
    if grad_of is None:
        return wj.detach().numpy(), wi.detach().numpy()
    gq, gv = torch.autograd.grad((wj * torch.tensor(grad_of)).sum(), (qt, vt), allow_unused=True)
    gq = torch.zeros_like(qt) if gq is None else gq
    gv = torch.zeros_like(vt) if gv is None else gv
    return wj.detach().numpy(), wi.detach().numpy(), gq.numpy(), gv.numpy()


def record(mvc, name, q, v, f, kind, expand=False, seed=0):
    rng = np.random.default_rng(seed + 1000)
    B, P = q.shape[:2]
    N = v.shape[1]
    ft = torch.from_numpy(f)
    if expand:
        ft = ft[:1].expand(B, -1, -1)
    q64, v64 = q.astype(np.float64), v.astype(np.float64)
    G = rng.normal(size=(B, P, N))
    wj64, wi64, gq64, gv64 = run(mvc, q64, v64, ft, torch.float64, G)
    wj32, wi32 = run(mvc, q, v, ft, torch.float32)
    stable = np.ones((B, P), bool)
    gv_stable = np.ones(B, bool)
    moves = [(t, t) for t in ([1e-9, -2e-9, 3e-9], [-3e-9, 1e-9, 2e-9], [2e-9, 2e-9, -1e-9])]
    moves += [(rng.normal(scale=1e-11, size=q.shape), 0.0) for _ in range(2)]     # the queries alone, by ~1e-11
    for tq, tv in moves:
        wj_t, _, gq_t, gv_t = run(mvc, q64 + tq, v64 + tv, ft, torch.float64, G)
        row = np.abs(wj_t - wj64).max(-1) <= 1e-9
        row &= np.isnan(wj_t).any(-1) == np.isnan(wj64).any(-1)
        gerr = np.abs(gq_t - gq64).max(-1) <= 1e-6 * (1 + np.abs(gq64).max(-1))
        gerr |= np.isnan(gq64).any(-1)                               # a NaN reference gradient is recorded as such
        stable &= row & gerr
        gv_stable &= (np.abs(gv_t - gv64) <= 1e-6 * (1 + np.abs(gv64))).reshape(B, -1).all(1) | np.isnan(gv64).reshape(B, -1).any(1)
    path = os.path.join(OUT, "mvc_%s.npz" % name)
    np.savez_compressed(path, query=q, vertices=v, faces=f, expand=np.array(expand), kind=kind, wj64=wj64, wi64=wi64,
                        wj32=wj32, wi32=wi32, G=G, gq64=gq64, gv64=gv64, stable=stable, gv_stable=gv_stable)
    print("%-18s B=%d P=%3d N=%3d F=%3d  unstable rows %d, NaN gradient rows %d, %d bytes" % (
        name, B, P, N, f.shape[1], (~stable).sum(), np.isnan(gq64).any(-1).sum(), os.path.getsize(path)))


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    mvc = load_reference(os.path.abspath(sys.argv[1]))
    rng = np.random.default_rng(7)
    cube_coplanar = [[1.0, 2.5, 0.25], [-0.5, -1.0, 3.0], [0.75, 1.5, -1.0]]     # exactly in the planes x=1, y=-1, z=-1
    cages = [("octahedron", octahedron(), 0.5, None), ("ico1", icosphere(1), 0.85, None),
             ("ico2", icosphere(2), 0.9, None), ("star", star(), 0.7, None), ("cube", cube(), 0.9, cube_coplanar)]
    for seed, (name, (v, f), inner, extra) in enumerate(cages):
        q, kind = queries(rng, v, f, inner, extra)
        record(mvc, name, q[None], v.astype(np.float32)[None], f[None], kind[None], seed=seed)
    # B = 2, a different cage in each batch element (same sizes): an octahedron and a rotated, stretched one with its
    # faces listed in another order and their corners rotated
    v0, f0 = octahedron()
    rot = np.linalg.qr(rng.normal(size=(3, 3)))[0]
    v1 = (v0 * [1.3, 0.8, 1.1]) @ rot.T
    f1 = np.roll(f0[::-1], 1, axis=1)
    qa, ka = queries(rng, v0, f0, 0.5)
    qb, kb = queries(rng, v1, f1, 0.4)
    record(mvc, "b2_two_cages", np.stack([qa, qb]), np.stack([v0, v1]).astype(np.float32), np.stack([f0, f1]),
           np.stack([ka, kb]), seed=10)
    # B = 2, one face list expanded over B, two cages of that topology
    v2, f2 = icosphere(1)
    v3 = v2 * [1.2, 0.9, 1.0] + [0.1, -0.2, 0.05]
    qa, ka = queries(rng, v2, f2, 0.85)
    qb, kb = queries(rng, v3, f2, 0.75)
    record(mvc, "b2_expanded", np.stack([qa, qb]), np.stack([v2, v3]).astype(np.float32), f2[None].copy(),
           np.stack([ka, kb]), expand=True, seed=11)


if __name__ == "__main__":
    main()
