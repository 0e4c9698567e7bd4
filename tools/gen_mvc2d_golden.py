"""Writes tests/golden/mvc2d_*.npz: 2-D mean value coordinates computed by the reference's own
``network.geo_operations.mean_value_coordinates`` on CPU torch.  CPU machine only.

    python tools/gen_mvc2d_golden.py <reference checkout>

The reference module is read from the checkout at run time, with the imports stubbed as tools/gen_mvc_golden.py stubs
them; nothing of it is stored here.

Per fixture: points (B,2,N) fp32, polygon (B,2,M) fp32, ``kind`` (B,N) of each query (KINDS), the reference's phi / w
(``verbose=True``) in fp64 (inputs upcast) and in fp32, and ``stable`` (B,N): the reference's fp64 row moves by at
most 1e-9, and its query gradient by at most 1e-6 relative, when the whole scene is translated by a few 1e-9, or the
queries alone by ~1e-11 (the moves of tools/gen_mvc_golden.py) -- where it does not, the reference's answer is decided
by rounding.  The second kind of move matters far from the polygon: a translation shifts every r_i of a query
together, while moving the query draws the roundings of r_i r_{i+1} - D_i anew.  The cotangent G (B,M,N) is zero on the unstable rows, and
gq64 (B,2,N), gp64 (B,2,M) are the reference's fp64 gradients of sum(G * phi); ``gp_stable`` (B,) says that the polygon
gradient keeps to 1e-6 relative under the same translations.

No recorded row has a zero weight sum: the reference would switch the divisor of the whole tensor there (DESIGN.md
"Mean value coordinates, 2-D"), which this project deliberately does not do.
"""
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden")
KINDS = {"interior": 0, "exterior": 1, "far10": 2, "far100": 3, "vertex": 4, "edge": 5, "extension": 6, "centroid": 7,
         "near_edge": 8, "near_vertex": 9}
OFFSETS = [1e-3, 1e-4, 1e-5, 1e-6, 1e-7, 1e-8]


def load_reference(checkout):
    spec = importlib.util.spec_from_file_location("gen_mvc_golden", os.path.join(ROOT, "tools", "gen_mvc_golden.py"))
    gen3d = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen3d)
    gen3d.load_reference(checkout)                       # stubs the imports and loads the module
    return sys.modules["pytorch_points.network.geo_operations"].mean_value_coordinates


# ------------------------------------------------------------------------------------------------ cages
# (M,2) counter-clockwise polygons, star-shaped about their vertex mean, moved so that vertex 0 is the origin: queries
# a few 1e-9 from it are then fp32 numbers, and the on-vertex threshold (1e-8) is bracketed
def at_origin(p):
    p = np.asarray(p, np.float64)
    return p - p[0]


def triangle():
    return at_origin([[0.0, 0.0], [1.0, 0.1], [0.3, 0.9]])


def pentagon():
    ang = 2 * np.pi * (np.arange(5) + 0.13) / 5
    return at_origin(np.stack([1.1 * np.cos(ang), 0.8 * np.sin(ang)], 1))


def star12():
    ang = 2 * np.pi * np.arange(12) / 12
    rad = np.where(np.arange(12) % 2 == 0, 1.0, 0.45)
    return at_origin(np.stack([rad * np.cos(ang), rad * np.sin(ang)], 1))


def gon(m, radius=1.0, phase=0.0):
    ang = 2 * np.pi * np.arange(m) / m + phase
    return at_origin(np.stack([radius * np.cos(ang), radius * np.sin(ang)], 1))


def dented8():
    ang = 2 * np.pi * np.arange(8) / 8 + 0.2
    rad = np.array([1.0, 0.9, 0.5, 1.2, 0.8, 0.4, 1.1, 0.7])
    return at_origin(np.stack([1.3 * rad * np.cos(ang), rad * np.sin(ang)], 1))


def boundary_radius(poly, centre, direction):
    """distance from ``centre`` to the polygon's boundary along the unit vector ``direction``"""
    best = np.inf
    for a, b in zip(poly, np.roll(poly, -1, axis=0)):
        e = b - a
        den = direction[0] * e[1] - direction[1] * e[0]
        if abs(den) < 1e-14:
            continue
        rel = a - centre
        t = (rel[0] * e[1] - rel[1] * e[0]) / den
        u = (rel[0] * direction[1] - rel[1] * direction[0]) / den
        if t > 0 and -1e-12 <= u <= 1 + 1e-12:
            best = min(best, t)
    return best


def queries(rng, poly, n_interior=60, n_exterior=30, n_far=16):
    """(N,2) fp32 queries and their kinds for the fp32-rounded polygon ``poly`` (M,2)"""
    poly = poly.astype(np.float32).astype(np.float64)
    M = len(poly)
    centre = poly.mean(0)
    size = np.linalg.norm(poly - centre, axis=1).max()
    pts, kinds = [], []

    def add(p, kind):
        pts.append(np.asarray(p, np.float64))
        kinds.append(KINDS[kind])

    def unit():
        a = rng.uniform(0, 2 * np.pi)
        return np.array([np.cos(a), np.sin(a)])

    for _ in range(n_interior):
        d = unit()
        add(centre + d * boundary_radius(poly, centre, d) * rng.uniform(0.05, 0.9), "interior")
    for _ in range(n_exterior):
        d = unit()
        add(centre + d * size * rng.uniform(1.2, 2.0), "exterior")
    for _ in range(n_far):
        add(centre + unit() * size * 10 * rng.uniform(0.8, 1.2), "far10")
    for _ in range(n_far):
        add(centre + unit() * size * 100 * rng.uniform(0.8, 1.2), "far100")
    some = rng.choice(M, min(3, M), replace=False)
    for j in some:
        add(poly[j], "vertex")
    for j in some:
        add((poly[j] + poly[(j + 1) % M]) / 2, "edge")
    for j in some:
        add(poly[j] + 1.5 * (poly[(j + 1) % M] - poly[j]), "extension")
    add(centre, "centroid")
    j = int(some[0])
    a, b = poly[j], poly[(j + 1) % M]
    normal = np.array([(b - a)[1], -(b - a)[0]]) / np.linalg.norm(b - a)
    for off in OFFSETS:
        for sign in (-1, 1):
            add((a + b) / 2 + sign * off * normal, "near_edge")
    # away from the polygon: towards it the query is also within the on-edge band of both edges at vertex 0, where
    # the reference's fp32 row sums to exactly 0
    d = (poly[0] - centre) / np.linalg.norm(poly[0] - centre)
    for off in OFFSETS + [3e-8, 3e-9]:
        add(poly[0] + off * d, "near_vertex")                    # vertex 0 is the origin
    return np.stack(pts).astype(np.float32), np.array(kinds, np.int8)


# ------------------------------------------------------------------------------------------------ recording
def run(mvc, q, p, dtype, grad_of=None):
    qt = torch.tensor(q, dtype=dtype, requires_grad=grad_of is not None)
    pt = torch.tensor(p, dtype=dtype, requires_grad=grad_of is not None)
    phi, w = mvc(qt, pt, verbose=True)
    assert not bool((w.sum(1) == 0).any()), "a row with a zero weight sum: the reference switches its divisor"
    if grad_of is None:
        return phi.detach().numpy(), w.detach().numpy()
    gq, gp = torch.autograd.grad((phi * torch.tensor(grad_of)).sum(), (qt, pt))
    return phi.detach().numpy(), w.detach().numpy(), gq.numpy(), gp.numpy()


def record(mvc, name, q, p, kind, seed):
    """q (B,N,2), p (B,M,2) fp32 -> the channel-first fixture"""
    rng = np.random.default_rng(seed + 2000)
    q, p = np.ascontiguousarray(q.transpose(0, 2, 1)), np.ascontiguousarray(p.transpose(0, 2, 1))
    B, _, N = q.shape
    M = p.shape[2]
    q64, p64 = q.astype(np.float64), p.astype(np.float64)
    G = rng.normal(size=(B, M, N))
    moves = [(np.array(t).reshape(1, 2, 1),) * 2 for t in ([1e-9, -2e-9], [-3e-9, 1e-9], [2e-9, 2e-9])]
    moves += [(rng.normal(scale=1e-11, size=q.shape), 0.0) for _ in range(2)]     # the queries alone, by ~1e-11
    phi64, w64, gq64, _ = run(mvc, q64, p64, torch.float64, G)
    stable = np.ones((B, N), bool)
    for tq, tp in moves:
        phi_t, _, gq_t, _ = run(mvc, q64 + tq, p64 + tp, torch.float64, G)
        row = np.abs(phi_t - phi64).max(1) <= 1e-9
        row &= np.isnan(phi_t).any(1) == np.isnan(phi64).any(1)
        grad = np.abs(gq_t - gq64).max(1) <= 1e-6 * (1 + np.abs(gq64).max(1))
        stable &= row & grad & np.isfinite(gq64).all(1)
    G = G * stable[:, None, :]
    _, _, gq64, gp64 = run(mvc, q64, p64, torch.float64, G)
    gp_stable = np.ones(B, bool)
    for tq, tp in moves:
        gp_t = run(mvc, q64 + tq, p64 + tp, torch.float64, G)[3]
        gp_stable &= (np.abs(gp_t - gp64) <= 1e-6 * (1 + np.abs(gp64).reshape(B, -1).max(1))[:, None, None]
                      ).reshape(B, -1).all(1)
    phi32, w32 = run(mvc, q, p, torch.float32)
    path = os.path.join(OUT, "mvc2d_%s.npz" % name)
    np.savez_compressed(path, points=q, polygon=p, kind=kind, phi64=phi64, w64=w64, phi32=phi32, w32=w32, G=G,
                        gq64=gq64, gp64=gp64, stable=stable, gp_stable=gp_stable)
    print("%-10s B=%d N=%3d M=%2d  unstable rows %d (kinds %s), polygon gradient stable %s, %d bytes" % (
        name, B, N, M, (~stable).sum(), sorted(set(kind[~stable].tolist())), gp_stable.tolist(),
        os.path.getsize(path)))


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    mvc = load_reference(os.path.abspath(sys.argv[1]))
    rng = np.random.default_rng(13)
    cages = [("triangle", triangle()), ("pentagon", pentagon()), ("star12", star12()), ("gon64", gon(64))]
    for seed, (name, poly) in enumerate(cages):
        q, kind = queries(rng, poly)
        record(mvc, name, q[None], poly.astype(np.float32)[None], kind[None], seed)
    # B = 2: two different polygons of equal M
    pa, pb = gon(8, 0.9, 0.3), dented8()
    qa, ka = queries(rng, pa)
    qb, kb = queries(rng, pb)
    record(mvc, "b2", np.stack([qa, qb]), np.stack([pa, pb]).astype(np.float32), np.stack([ka, kb]), 10)


if __name__ == "__main__":
    main()
