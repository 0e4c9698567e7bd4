"""Writes tests/golden/gc_*.npz: Green coordinates computed by the reference's own
``network.geo_operations.green_coordinates_3D`` on CPU torch.  CPU machine only.

    python tools/gen_gc_golden.py <reference checkout>

The reference module is loaded by ``load_reference`` of tools/gen_mvc_golden.py (read from the checkout at run time;
nothing of it is stored here), and the cages and query kinds are that tool's.

Per fixture: query (B,P,3) fp32, vertices (B,N,3) fp32, faces (B,F,3) int64 (``expand``: the tests pass faces[:1]
expanded over B), ``kind`` (B,P) of each query (KINDS), ``normals`` (B,F,3) the fp64 face normals of the cage, the
reference's outputs in fp64 (inputs upcast: gcv64, gcf64, ext64) and in fp32 (gcv32, gcf32, ext32), cotangents Gv
(B,P,N) and Gf (B,P,F) (fp32 values), the reference's fp64 gradients of sum(Gv * GC_vertex) + sum(Gf * GC_face) with
respect to query and vertices (normals computed inside: gq64, gv64) and with respect to query and face_normals
(``normals`` passed: gqn64, gn64), NaN kept, and ``stable`` (B,P): the reference's fp64 row (both outputs) moves by at
most 1e-9, its flag not at all and its query gradients by at most 1e-6 relative when the whole scene is translated by
a few 1e-9 or the queries alone by ~1e-11 -- where it does not, the reference's answer is decided by rounding.
"""
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden")


def _mvc_tool():
    spec = importlib.util.spec_from_file_location("gen_mvc_golden", os.path.join(ROOT, "tools", "gen_mvc_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


mvc_tool = _mvc_tool()
KINDS = mvc_tool.KINDS


def load_reference(checkout):
    mvc_tool.load_reference(checkout)
    geo = sys.modules["pytorch_points.network.geo_operations"]
    return geo.green_coordinates_3D, geo.compute_face_normals_and_areas


def run(gc, normals_fn, q, v, f, dtype, G=None, pass_normals=False):
    """the reference's outputs (numpy), and with cotangents G = (Gv, Gf) its gradients with respect to query and
    vertices (normals computed inside) or query and face_normals (``pass_normals``)"""
    grad = G is not None
    qt = torch.tensor(q, dtype=dtype, requires_grad=grad)
    vt = torch.tensor(v, dtype=dtype, requires_grad=grad and not pass_normals)
    nt = None
    if pass_normals:
        nt = normals_fn(vt.detach().clone(), f.clone())[0].detach().requires_grad_(True)
    gcv, gcf, ext = gc(qt, vt, f, face_normals=nt)
    out = [gcv.detach().numpy(), gcf.detach().numpy(), ext.numpy()]
    if grad:
        wrt = (qt, nt if pass_normals else vt)
        loss = (gcv * torch.from_numpy(G[0]).to(dtype)).sum() + (gcf * torch.from_numpy(G[1]).to(dtype)).sum()
        g = torch.autograd.grad(loss, wrt, allow_unused=True)
        out += [(torch.zeros_like(w) if x is None else x).numpy() for w, x in zip(wrt, g)]
    return out


def record(fns, name, q, v, f, kind, expand=False, seed=0):
    gc, normals_fn = fns
    rng = np.random.default_rng(seed + 2000)
    B, P = q.shape[:2]
    N, F = v.shape[1], f.shape[1]
    ft = torch.from_numpy(f)
    if expand:
        ft = ft[:1].expand(B, -1, -1)
    q64, v64 = q.astype(np.float64), v.astype(np.float64)
    G = (rng.normal(size=(B, P, N)).astype(np.float32), rng.normal(size=(B, P, F)).astype(np.float32))
    gcv64, gcf64, ext64, gq64, gv64 = run(gc, normals_fn, q64, v64, ft, torch.float64, G)
    _, _, _, gqn64, gn64 = run(gc, normals_fn, q64, v64, ft, torch.float64, G, pass_normals=True)
    gcv32, gcf32, ext32 = run(gc, normals_fn, q, v, ft, torch.float32)
    normals = normals_fn(torch.from_numpy(v64), ft.clone())[0].numpy()
    stable = np.ones((B, P), bool)
    moves = [(t, t) for t in ([1e-9, -2e-9, 3e-9], [-3e-9, 1e-9, 2e-9], [2e-9, 2e-9, -1e-9])]
    moves += [(rng.normal(scale=1e-11, size=q.shape), 0.0) for _ in range(2)]     # the queries alone, by ~1e-11
    for tq, tv in moves:
        a, b, e, gq_t, _ = run(gc, normals_fn, q64 + tq, v64 + tv, ft, torch.float64, G)
        row = (np.abs(a - gcv64).max(-1, initial=0) <= 1e-9) & (np.abs(b - gcf64).max(-1, initial=0) <= 1e-9)
        row &= (np.isnan(a).any(-1) == np.isnan(gcv64).any(-1)) & (e[..., 0] == ext64[..., 0])
        gerr = np.abs(gq_t - gq64).max(-1) <= 1e-6 * (1 + np.abs(gq64).max(-1))
        gerr |= np.isnan(gq64).any(-1)                               # a NaN reference gradient is recorded as such
        stable &= row & gerr
    path = os.path.join(OUT, "gc_%s.npz" % name)
    np.savez_compressed(path, query=q, vertices=v, faces=f, expand=np.array(expand), kind=kind, normals=normals,
                        gcv64=gcv64, gcf64=gcf64, ext64=ext64, gcv32=gcv32, gcf32=gcf32, ext32=ext32, Gv=G[0],
                        Gf=G[1], gq64=gq64, gv64=gv64, gqn64=gqn64, gn64=gn64, stable=stable)
    print("%-18s B=%d P=%3d N=%3d F=%3d  unstable rows %d, NaN gradient rows %d, exterior %d, %d bytes" % (
        name, B, P, N, F, (~stable).sum(), np.isnan(gq64).any(-1).sum(), ext64.sum(), os.path.getsize(path)))


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    fns = load_reference(os.path.abspath(sys.argv[1]))
    t = mvc_tool
    rng = np.random.default_rng(9)
    cube_coplanar = [[1.0, 2.5, 0.25], [-0.5, -1.0, 3.0], [0.75, 1.5, -1.0]]     # exactly in the planes x=1, y=-1, z=-1
    cages = [("octahedron", t.octahedron(), 0.5, None), ("ico1", t.icosphere(1), 0.85, None),
             ("ico2", t.icosphere(2), 0.9, None), ("star", t.star(), 0.7, None), ("cube", t.cube(), 0.9, cube_coplanar)]
    for seed, (name, (v, f), inner, extra) in enumerate(cages):
        q, kind = t.queries(rng, v, f, inner, extra)
        record(fns, name, q[None], v.astype(np.float32)[None], f[None], kind[None], seed=seed)
    # B = 2, a different cage in each batch element (same sizes): an octahedron and a rotated, stretched one with its
    # faces listed in another order and their corners rotated
    v0, f0 = t.octahedron()
    rot = np.linalg.qr(rng.normal(size=(3, 3)))[0]
    v1 = (v0 * [1.3, 0.8, 1.1]) @ rot.T
    f1 = np.roll(f0[::-1], 1, axis=1)
    qa, ka = t.queries(rng, v0, f0, 0.5)
    qb, kb = t.queries(rng, v1, f1, 0.4)
    record(fns, "b2_two_cages", np.stack([qa, qb]), np.stack([v0, v1]).astype(np.float32), np.stack([f0, f1]),
           np.stack([ka, kb]), seed=10)
    # B = 2, one face list expanded over B, two cages of that topology
    v2, f2 = t.icosphere(1)
    v3 = v2 * [1.2, 0.9, 1.0] + [0.1, -0.2, 0.05]
    qa, ka = t.queries(rng, v2, f2, 0.85)
    qb, kb = t.queries(rng, v3, f2, 0.75)
    record(fns, "b2_expanded", np.stack([qa, qb]), np.stack([v2, v3]).astype(np.float32), f2[None].copy(),
           np.stack([ka, kb]), expand=True, seed=11)


if __name__ == "__main__":
    main()
