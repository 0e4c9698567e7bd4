#!/usr/bin/env python3
"""Generates tests/golden/range_*.npz: small INPUTS (no expected outputs) at the extremes of the fp32 range, for the
cross-check of the CPU oracle against the reference's kernel bodies (oracle/xcheck/ref_xcheck.py --range ->
ref_xcheck_range.npz; tests/test_oracle_range.py) and for tests/test_gpu_range.py, which builds the same families at
other sizes through `family` below.

Families (finite inputs at any magnitude are in the contract), each in two variants:
  lattice   small integers times a power of two: every difference is exact, so ties are exact and plentiful
  jitter    the same with noise of a fraction of the lattice step, so that ties are broken

  saturated     64 unit-scale clusters 2^20 (about 1e6) apart: squared distances between clusters are far above
                FPS's initial temp of 1e10
  inf_spread    coordinates up to 8 * 2^63 (about 7e19): most squared distances are inf
  inf_outliers  a unit cloud with a few points at about +-1e19
  huge_box      a unit cloud with a few points at about +-3e38: the box extent hi - lo is inf
  tiny_19       extent about 2e-19: squared differences subnormal or small normal
  tiny_21       extent about 3e-21: squared differences subnormal
  tiny_23       extent about 1e-23: squared differences 0 -- every pair ties
  subnormal     the coordinates themselves are subnormal (about 1e-40)

Run from the repo root:  python tests/golden/gen_range.py
"""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

# (lattice step, integer range) of the plain families; the others are built in `family`
_PLAIN = {"inf_spread": (2.0 ** 63, 8), "tiny_19": (2.0 ** -66, 8), "tiny_21": (2.0 ** -72, 8),
          "tiny_23": (2.0 ** -80, 8), "subnormal": (2.0 ** -134, 8)}
FAMILIES = ["saturated", "inf_spread", "inf_outliers", "huge_box", "tiny_19", "tiny_21", "tiny_23", "subnormal"]
UNDERFLOW = ["tiny_19", "tiny_21", "tiny_23", "subnormal"]
VARIANTS = ["lattice", "jitter"]


def family(name, variant, n, seed):
    """(n, 3) float32 points of one family"""
    rng = np.random.default_rng([seed, FAMILIES.index(name), VARIANTS.index(variant)])
    jit = variant == "jitter"
    if name in _PLAIN:
        step, k = _PLAIN[name]
        x = rng.integers(-k, k + 1, (n, 3)).astype(np.float64) * step
        if jit and name == "subnormal":   # random subnormals, down to the smallest
            x = rng.integers(-2 ** 15, 2 ** 15, (n, 3)).astype(np.float64) * 2.0 ** -149
        elif jit:
            x = x + rng.normal(size=(n, 3)) * (step / 4)
    elif name == "saturated":
        g = np.stack(np.meshgrid(*[np.arange(4.0)] * 3, indexing="ij"), -1).reshape(64, 3) * 2.0 ** 20
        x = g[np.arange(n) % 64] + rng.integers(-4, 5, (n, 3)) * 0.25
        if jit:
            x = x + rng.normal(size=(n, 3)) * 0.0625
    else:   # a unit cloud with a few far points
        x = rng.integers(-8, 9, (n, 3)).astype(np.float64) * 0.125
        if jit:
            x = x + rng.normal(size=(n, 3)) * 0.03
        far = 2.0 ** 63 if name == "inf_outliers" else 7.0 * 2.0 ** 125
        k = min(5, n)
        where = rng.choice(n, k, replace=False)
        x[where, rng.integers(0, 3, k)] = far * rng.choice([-1.0, 1.0], k) * (1 if name == "huge_box" else rng.integers(1, 4, k))
    x = x.astype(np.float32)
    assert np.isfinite(x).all()
    return x


def pair(name, variant, n, seed):
    """(2, n, 3): batch element 0 of the family, element 1 a clean unit cloud"""
    rng = np.random.default_rng([seed, 99])
    clean = rng.normal(size=(n, 3))
    clean /= np.linalg.norm(clean, axis=1, keepdims=True)
    return np.stack([family(name, variant, n, seed), clean.astype(np.float32)])


def radii(name):
    """ball_query radii: 0, r^2 subnormal, r^2 == 0 in fp32 (even duplicates outside), r^2 == inf, and the family's
    own scale"""
    own = {"saturated": 1.0, "inf_spread": 2.0 ** 64, "inf_outliers": 0.5, "huge_box": 0.5, "tiny_19": 2.0 ** -64,
           "tiny_21": 2.0 ** -70, "tiny_23": 2.0 ** -78, "subnormal": 2.0 ** -131}[name]
    return [0.0, 2.0 ** -70, 2.0 ** -76, 2.0 ** 65, own]


def labels(n, seed):
    """labels 0..2 such that every cluster of `saturated` holds every label (so no labeled distance reaches 1e10)"""
    return ((np.arange(n) // 64) % 3).astype(np.int32)


def three_nn_sparse(n, m, finite, seed):
    """queries (2, n, 3) of a unit cloud; knowns (2, m, 3) of which only the first `finite` are at a finite distance
    from the queries (the rest at about +-2^126 in every coordinate, where every squared distance is inf)"""
    rng = np.random.default_rng([seed, finite])
    q = (rng.integers(-8, 9, (2, n, 3)) * 0.125).astype(np.float32)
    k = (rng.choice([-1.0, 1.0], (2, m, 3)) * 2.0 ** 126 * rng.integers(1, 4, (2, m, 3))).astype(np.float32)
    k[:, :finite] = (rng.integers(-8, 9, (2, finite, 3)) * 0.125).astype(np.float32)
    return q, k


def fps_nonfinite(n, seed):
    """(2, n, 3) unit clouds; element 0 with one NaN point, one +inf and one -inf point (element 1 clean)"""
    rng = np.random.default_rng([seed, 7])
    x = rng.normal(size=(2, n, 3))
    x /= np.linalg.norm(x, axis=2, keepdims=True)
    x = x.astype(np.float32)
    x[0, n // 3, 1] = np.nan
    x[0, n // 2, 0] = np.inf
    x[0, (2 * n) // 3, 2] = -np.inf
    return x


def main():
    total = 0
    for name in FAMILIES:
        for variant in VARIANTS:   # one batch element of the family (the GPU tests add a clean one beside it)
            arrays = {"xyz1": family(name, variant, 700, 1)[None], "xyz2": family(name, variant, 800, 2)[None],
                      "fps_xyz": family(name, variant, 2500, 3)[None], "fps_npoint": np.int32(96),
                      "new_xyz": family(name, variant, 128, 4)[None], "radii": np.array(radii(name), np.float32),
                      "nsample": np.int32(16)}
            if name == "saturated" or name in UNDERFLOW:
                arrays["label1"] = labels(700, 5)[None]
                arrays["label2"] = labels(800, 6)[None]
            path = os.path.join(HERE, "range_%s_%s.npz" % (name, variant))
            np.savez_compressed(path, **arrays)
            total += os.path.getsize(path)
    q, k = {}, {}
    for f in (1, 2):
        q[f], k[f] = three_nn_sparse(300, 40, f, 8)
    path = os.path.join(HERE, "range_special.npz")
    np.savez_compressed(path, tn_unknown1=q[1], tn_known1=k[1], tn_unknown2=q[2], tn_known2=k[2],
                        fps_xyz=fps_nonfinite(2500, 9), fps_npoint=np.int32(96))
    total += os.path.getsize(path)
    print("wrote %d range fixtures, %.2f MB" % (2 * len(FAMILIES) + 1, total / 1e6))


if __name__ == "__main__":
    main()
