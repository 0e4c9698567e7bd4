"""The CPU oracle against the reference's own kernel bodies (tests/golden/ref_xcheck_range.npz, written by
oracle/xcheck/ref_xcheck.py --range) on the range corpus of tests/golden/gen_range.py: saturated FPS temps, squared
distances that overflow to inf or underflow to subnormals and 0, subnormal coordinates, three_nn queries with fewer
than three knowns at a finite distance, FPS with NaN / inf points.  The GPU tests hold the kernels to the oracle bit
for bit at these magnitudes, so the oracle must read the reference right there too.

Both contraction tags of the cross-check (nocontract, fma: the contraction of the reference's sums is nvcc's choice)
are compared: indices exactly on the lattice-exact families (every difference exact: nothing depends on contraction);
on the jittered ones exactly except where the two tags disagree with each other (a contraction-dependent edge: counted
and capped); distances within 2 ulp, NaN and inf where the reference has them."""
import glob
import os

import numpy as np
import pytest

import oracle

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TAGS = ("nocontract", "fma")
MAX_EDGES = 8   # contraction-dependent indices per array of a jittered family


@pytest.fixture(scope="module")
def ref():
    return np.load(os.path.join(GOLDEN, "ref_xcheck_range.npz"))


def _cases():
    return sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "range_*.npz")))


def _ulps(a, b):
    """distance in units in the last place of finite fp32 arrays (0 where both are the same non-finite value)"""
    a = np.asarray(a, np.float32)
    b = np.asarray(b, np.float32)
    same = (a == b) | (np.isnan(a) & np.isnan(b))
    ia = a.view(np.int32).astype(np.int64)
    ib = b.view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, -(ia & 0x7FFFFFFF), ia)
    ib = np.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    d = np.abs(ia - ib)
    d[same] = 0
    d[~same & ~(np.isfinite(a) & np.isfinite(b))] = 1 << 40   # inf / NaN against anything else
    return d


def _check_idx(ref, key, got, lattice):
    r = [ref["%s/%s" % (t, key)] for t in TAGS]
    for t, e in zip(TAGS, r):
        diff = got != e
        if lattice:
            assert not diff.any(), "%s (%s): %d indices differ" % (key, t, int(diff.sum()))
        else:
            edge = r[0] != r[1]
            assert not (diff & ~edge).any(), "%s (%s): %d indices differ off the edges" % (key, t, int((diff & ~edge).sum()))
            assert int(edge.sum()) <= MAX_EDGES, "%s: %d contraction-dependent indices" % (key, int(edge.sum()))


def _check_dist(ref, key, got, idx_key=None, got_idx=None):
    for t in TAGS:
        e = ref["%s/%s" % (t, key)]
        u = _ulps(got, e)
        if idx_key is not None:   # where the index differs (an edge, checked above) the distance is another point's
            u[got_idx != ref["%s/%s" % (t, idx_key)]] = 0
        assert u.max(initial=0) <= 2, "%s (%s): %d values beyond 2 ulp" % (key, t, int((u > 2).sum()))


@pytest.mark.parametrize("case", _cases())
def test_oracle_matches_reference_bodies_on_range_corpus(ref, case):
    g = dict(np.load(os.path.join(GOLDEN, case + ".npz")))
    if case == "range_special":
        for f in (1, 2):
            d, i = oracle.three_nn(g["tn_unknown%d" % f], g["tn_known%d" % f])
            _check_idx(ref, "%s/tn%d/idx" % (case, f), i, True)
            _check_dist(ref, "%s/tn%d/dist2" % (case, f), d)
            assert np.isinf(d[..., f:]).all() and (i[..., f:] == 0).all()   # the empty slots: (inf, 0)
        i, t = oracle.furthest_sampling(g["fps_xyz"], int(g["fps_npoint"]))
        _check_idx(ref, case + "/fps/idx", i, True)
        _check_dist(ref, case + "/fps/temp", t)
        assert (i[0, 1:] == i[0, 1]).all()   # the first non-finite pick repeats
        return
    lattice = case.endswith("_lattice")
    x1, x2 = g["xyz1"], g["xyz2"]
    d1, i1, d2, i2 = oracle.chamfer_forward(x1, x2)
    _check_idx(ref, case + "/chamfer/idx1", i1, lattice)
    _check_idx(ref, case + "/chamfer/idx2", i2, lattice)
    _check_dist(ref, case + "/chamfer/dist1", d1, case + "/chamfer/idx1", i1)
    _check_dist(ref, case + "/chamfer/dist2", d2, case + "/chamfer/idx2", i2)
    if "label1" in g:
        d1, i1, d2, i2 = oracle.labeled_chamfer_forward(x1, x2, g["label1"], g["label2"])
        assert (d1 < 1e10).all() and (d2 < 1e10).all()   # inside the contract
        _check_idx(ref, case + "/labeled/idx1", i1, lattice)
        _check_idx(ref, case + "/labeled/idx2", i2, lattice)
        _check_dist(ref, case + "/labeled/dist1", d1, case + "/labeled/idx1", i1)
        _check_dist(ref, case + "/labeled/dist2", d2, case + "/labeled/idx2", i2)
    i, t = oracle.furthest_sampling(g["fps_xyz"], int(g["fps_npoint"]))
    _check_idx(ref, case + "/fps/idx", i, lattice)
    if lattice:
        _check_dist(ref, case + "/fps/temp", t)
    for j, r in enumerate(g["radii"]):
        _check_idx(ref, "%s/ball_r%d" % (case, j), oracle.ball_query(g["new_xyz"], x2, float(r), int(g["nsample"])), lattice)
    d, i = oracle.three_nn(g["new_xyz"], x2)
    _check_idx(ref, case + "/three_nn/idx", i, lattice)
    _check_dist(ref, case + "/three_nn/dist2", d, case + "/three_nn/idx", i)


def test_range_corpus_reaches_the_extremes():
    """the corpus does what it is for: saturated FPS temps, inf and subnormal squared distances, inf box extents"""
    sat = np.load(os.path.join(GOLDEN, "range_saturated_lattice.npz"))
    _, t = oracle.furthest_sampling(sat["fps_xyz"][:1], 8)
    assert (t == np.float32(1e10)).any()
    g = np.load(os.path.join(GOLDEN, "range_inf_spread_lattice.npz"))
    with np.errstate(over="ignore", invalid="ignore"):
        pair = ((g["xyz1"][0, :, None] - g["xyz2"][0, None]) ** 2).sum(-1, dtype=np.float32)
    assert np.isinf(pair).mean() > 0.5   # most squared distances overflow
    x = np.load(os.path.join(GOLDEN, "range_huge_box_lattice.npz"))["xyz1"][0]
    with np.errstate(over="ignore"):
        assert np.isinf(x.max(0) - x.min(0)).any()
    for fam in ("tiny_21", "subnormal"):
        d1 = oracle.chamfer_forward(*[np.load(os.path.join(GOLDEN, "range_%s_jitter.npz" % fam))[k] for k in ("xyz1", "xyz2")])[0][0]
        assert ((d1 > 0) & (d1 < np.finfo(np.float32).tiny)).any() or fam == "subnormal"
    assert (d1 == 0).all()   # subnormal coordinates: every squared difference underflows
