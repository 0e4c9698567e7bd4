"""The clouds, measures and pinned fp32 floors shared by test_emd_host.py and test_gpu_emd.py (not a test module).

`python tests/emd_cases.py` measures the floors again on the CPU and prints the table below."""
import functools
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from pytorch_points_amd import emd  # noqa: E402

TILE = 512   # kEmdTile of csrc/emd.hip: the staged points of one LDS tile
OWN = 64     # kEmdOwn: the own points of a workgroup
EPS32 = float(np.finfo(np.float32).eps)

# (B, N, M): the sizes of 1, an odd pair below a workgroup's points, sizes that divide and do not, the tile's edges
# in both directions, more than a workgroup's points and more than one tile in both directions, and one B = 3
SIZES = [(2, 1, 1), (2, 1, 70), (2, 65, 63), (2, 100, 250), (2, 257, 1000), (2, TILE - 1, TILE + 1),
         (2, TILE + 1, TILE - 1), (2, 2 * TILE + OWN + 3, TILE + 2 * OWN + 1), (2, 1024, 1024), (3, 130, 77)]
CLOUDS = ["random", "copy", "squeezed"]
CASES = [(size, cloud) for size in SIZES for cloud in CLOUDS] + [((2, 65, 63), "identical")]


def case_id(case):
    (b, n, m), cloud = case
    return "%dx%dx%d-%s" % (b, n, m, cloud)


@functools.lru_cache(maxsize=None)
def clouds(case):
    """fp32 numpy ``(xyz1 (B,N,3), xyz2 (B,M,3))`` of a case, from a seed of its own"""
    (b, n, m), cloud = case
    rng = np.random.default_rng(1000 * CASES.index(case) + 7)
    x1 = rng.random((b, n, 3), dtype=np.float32)
    if cloud == "random":
        x2 = rng.random((b, m, 3), dtype=np.float32)
    elif cloud == "copy":        # points of xyz1 again: coincident pairs, cost near 0 where N == M
        pick = np.stack([rng.permutation(max(n, m))[:m] % n for _ in range(b)])
        x2 = np.take_along_axis(x1, pick[:, :, None], axis=1)
    elif cloud == "squeezed":    # a 0.01 cube at the centre: every exp underflows at the steep levels
        x2 = (0.495 + 0.01 * rng.random((b, m, 3))).astype(np.float32)
    else:                        # every point of both clouds the same
        x1 = np.broadcast_to(np.float32([0.25, 0.5, 0.75]), (b, n, 3)).copy()
        x2 = np.broadcast_to(np.float32([0.25, 0.5, 0.75]), (b, m, 3)).copy()
    return x1, x2


def diameter(case):
    pts = np.concatenate([c.reshape(-1, 3) for c in clouds(case)]).astype(np.float64)
    return max(float(np.linalg.norm(pts.max(0) - pts.min(0))), 1e-30)


def run(x1, x2, device="cpu", fn=None):
    """``(dense, cost, grad1, grad2)`` of one whole step on tensors made from ``x1, x2``; ``fn(t1, t2) -> (match,
    cost)`` defaults to the composition"""
    t1 = torch.as_tensor(x1, device=device).clone().requires_grad_(True)
    t2 = torch.as_tensor(x2, device=device).clone().requires_grad_(True)
    match, cost = (fn or emd.emd_composition)(t1, t2)
    g1, g2 = torch.autograd.grad(cost.sum(), (t1, t2))
    return match.dense(), cost.detach(), g1, g2


@functools.lru_cache(maxsize=None)
def reference(case, device="cpu"):
    """the fp64 composition of a case, computed once"""
    x1, x2 = clouds(case)
    return tuple(t.cpu() for t in run(x1.astype(np.float64), x2.astype(np.float64), device))


def measures(case, got, want):
    """``(match, cost, grad1, grad2)`` errors of ``got`` against the fp64 ``want``: the largest absolute error of the
    match, ``|dcost| / (max(N,M) diameter)``, and for each gradient the largest absolute error over the largest
    ``|gradient|``"""
    (b, n, m), _ = case
    got = [t.detach().cpu().double() for t in got]
    out = [float((got[0] - want[0]).abs().max()),
           float((got[1] - want[1]).abs().max()) / (max(n, m) * diameter(case))]
    for g, w in zip(got[2:], want[2:]):
        out.append(float((g - w).abs().max()) / max(float(w.abs().max()), 1e-30))
    return tuple(out)


def fp32_floor(case):
    """the fp32 CPU composition against fp64 on the case's own inputs, as given and with the points of both clouds
    permuted twice (another summation order): the largest of each measure"""
    x1, x2 = clouds(case)
    want = reference(case)
    worst = [0.0] * 4
    rng = np.random.default_rng(99)
    for trial in range(3):
        p1 = np.arange(x1.shape[1]) if trial == 0 else rng.permutation(x1.shape[1])
        p2 = np.arange(x2.shape[1]) if trial == 0 else rng.permutation(x2.shape[1])
        dense, cost, g1, g2 = run(x1[:, p1], x2[:, p2])
        back1, back2 = torch.as_tensor(np.argsort(p1)), torch.as_tensor(np.argsort(p2))
        got = (dense[:, back1][:, :, back2], cost, g1[:, back1], g2[:, back2])
        worst = [max(w, e) for w, e in zip(worst, measures(case, got, want))]
    return tuple(worst)


def bounds(case):
    """what HIP must stay within: 4 x the pinned fp32 floor, each lifted to 4 eps32 first (the project's rule)"""
    return tuple(4.0 * max(f, 4.0 * EPS32) for f in FLOORS[case_id(case)])


# fp32 CPU composition against fp64: (match, cost, grad1, grad2) as `measures` defines them, from `fp32_floor`
FLOORS = {
    "2x1x1-random": (5.9e-08, 6.97e-08, 7.71e-08, 7.71e-08),
    "2x1x1-copy": (5.3e-10, 0, 0, 0),
    "2x1x1-squeezed": (5.9e-08, 3.15e-08, 8.06e-08, 8.06e-08),
    "2x1x70-random": (3.69e-06, 5.97e-08, 7e-08, 2.57e-06),
    "2x1x70-copy": (9.95e-10, 0, 0, 0),
    "2x1x70-squeezed": (6.67e-06, 5e-08, 1.22e-07, 6.58e-06),
    "2x65x63-random": (1.49e-05, 1.38e-08, 1.11e-05, 7.56e-06),
    "2x65x63-copy": (2.42e-09, 2.62e-11, 1, 0.289),
    "2x65x63-squeezed": (2.24e-07, 1.96e-08, 2.42e-07, 6.79e-07),
    "2x100x250-random": (1.6e-06, 6.1e-09, 8.26e-07, 2.04e-06),
    "2x100x250-copy": (1.99e-08, 3.39e-11, 0.167, 0.276),
    "2x100x250-squeezed": (6e-08, 2.41e-08, 1.92e-07, 5.92e-07),
    "2x257x1000-random": (9.42e-07, 4.69e-09, 3.56e-07, 5.31e-07),
    "2x257x1000-copy": (1.03e-07, 4.26e-12, 5.44e-07, 5.44e-07),
    "2x257x1000-squeezed": (2.21e-08, 2.04e-08, 2.11e-07, 5.97e-07),
    "2x511x513-random": (5.44e-05, 1.6e-08, 4.77e-05, 3.1e-05),
    "2x511x513-copy": (5.96e-08, 1.99e-10, 5.62e-08, 4.53e-07),
    "2x511x513-squeezed": (6.58e-08, 2.03e-08, 2.36e-07, 3.67e-07),
    "2x513x511-random": (0.000708, 1.19e-08, 0.000531, 0.000297),
    "2x513x511-copy": (5.96e-08, 4.37e-10, 2.17e-06, 4.02e-07),
    "2x513x511-squeezed": (2.01e-08, 1.19e-08, 2.26e-07, 5.19e-07),
    "2x1091x641-random": (0.00106, 6.07e-08, 0.000928, 0.000617),
    "2x1091x641-copy": (1.8e-07, 5.55e-11, 4.78e-07, 3.41e-07),
    "2x1091x641-squeezed": (2.18e-08, 1.29e-08, 2.55e-07, 3.44e-07),
    "2x1024x1024-random": (6.05e-05, 5.7e-09, 7.77e-05, 4.27e-05),
    "2x1024x1024-copy": (1.14e-07, 1.27e-10, 3.83e-07, 3.27e-07),
    "2x1024x1024-squeezed": (3.84e-08, 2.58e-08, 2.44e-07, 3.63e-07),
    "3x130x77-random": (5.08e-05, 3.15e-08, 5.15e-05, 4.63e-05),
    "3x130x77-copy": (6.97e-08, 2.1e-11, 1.36e-07, 1.36e-07),
    "3x130x77-squeezed": (4.96e-08, 1.71e-08, 1.6e-07, 8.76e-07),
    "2x65x63-identical": (9.61e-10, 0, 0, 0),
}


# How far a row sum may fall short of multiL (or a column sum of multiR) where one size divides the other, as a share
# of that multiplicity: every division of the ten levels carries a 1e-9 in its denominator, which leaves that much of
# the mass unassigned.  Over every case of emd_cases the CPU composition's largest shortfall was 1.97e-8 in fp64 and
# 6.68e-6 in fp32, and its largest excess 4.4e-16 and 3.05e-7; pinned at 4 x the shortfalls.
SLACK64 = 8e-8
SLACK32 = 2.7e-5


def check_bounds(case, dense, slack):
    """match >= 0; row sums at most multiL and column sums at most multiR; equal to them where one size divides the
    other.  -> the largest shortfall where equality is asked (0 elsewhere)"""
    (b, n, m), _ = case
    big = max(n, m)
    mult_l, mult_r = big // n, big // m
    dense = dense.double()
    assert dense.shape == (b, n, m)
    assert bool((dense >= 0).all())
    rows, cols = dense.sum(2), dense.sum(1)
    assert float(rows.max()) <= mult_l * (1 + slack) and float(cols.max()) <= mult_r * (1 + slack)
    if big % n == 0 and big % m == 0:
        short = max(float((mult_l - rows).max()) / mult_l, float((mult_r - cols).max()) / mult_r)
        assert short <= slack, short
        return short
    return 0.0


if __name__ == "__main__":
    for c in CASES:
        print('    "%s": (%s),' % (case_id(c), ", ".join("%.3g" % v for v in fp32_floor(c))), flush=True)
