"""CPU tests (no GPU) of tests/geometry_fuzz.py, for every family and seed that tests/test_gpu_geometry_fuzz.py uses:
the generators give what they promise (coordinates exact in fp32, indices in range, edges and coordinates inside the
range, exactly zero fp64 area where promised and fp32 zero with it, at most half of a cloud on the surface, ``thin`` and
``far`` closed and oriented outwards), and the fp32 CPU compositions of the operators that do arithmetic per triangle
are measured against fp64 on ill-shaped faces: every figure is printed beside its pinned value in the ``*_MEASURED``
tables below, which the GPU tests bound HIP by.  What the contracts promise outright -- indices in range, weights that
are weights, the residual identity, a partner wherever one is usable, the lowest index among ties, no face without
area drawn, the degenerate rules' exact values and zero gradients -- is asserted of the compositions here as it is of
HIP there."""
import functools

import numpy as np
import pytest
import torch

import geometry_fuzz as G
import topology_fuzz as T
from pytorch_points_amd import mesh_sample, mesh_winding
from test_mesh_distance_host import extent
from test_mesh_sample_host import faces_of
from test_mesh_winding_host import np_winding

F32 = np.float32
EPS32 = 2.0 ** -23
SEEDS = list(G.seeds())
DEFAULT_SEEDS = 8               # the pinned figures are those of the default run


def report(what, family, got, pinned):
    print("%s, %s: %s (pinned %s)" % (family, what, ", ".join("%.3g" % g for g in got), pinned))


def held(got, bound):
    """every figure within its bound; the figures are pinned for the default seeds, a longer run only prints them"""
    return len(SEEDS) != DEFAULT_SEEDS or all(g <= b for g, b in zip(got, bound))


# ------------------------------------------------------------------------------------------------ the generators
def fp32_cross(tri):
    """the cross product (b - a) x (c - a) of (F,3,3) in fp32 with every operation rounded on its own"""
    tri = tri.astype(F32)
    u, v = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    return np.stack([u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1], u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2],
                     u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]], -1)


@pytest.mark.parametrize("family", G.FAMILIES)
def test_generator_keeps_its_promises(family):
    for seed in SEEDS:
        c = G.case(family, seed)
        what = G.describe(c)
        again = G.case.__wrapped__(family, seed)
        assert all(np.array_equal(a, b) for a, b in zip(c[2:], again[2:])), what          # a seed is all there is
        n, f, p = c.vertices.shape[1], c.faces.shape[-2], c.points.shape[1]
        assert c.vertices.shape == (2, n, 3) and c.points.shape == (2, p, 3) and c.faces.dtype == np.int64, what
        assert c.faces.shape in ((f, 3), (2, f, 3)) and (c.faces.ndim == 3) == bool(seed % 2), what
        assert c.faces.min() >= 0 and c.faces.max() < n, what
        for a in (c.vertices, c.points):
            assert np.isfinite(a).all() and np.array_equal(a.astype(F32).astype(np.float64), a), what
            assert np.abs(a).max() <= 2e3, what
        if family in G.SOUPS:
            assert f in G.SOUP_FACES and n == 3 * f, what
        else:
            assert 300 <= f <= 4000, what
        assert p in G.CLOUD_SIZES, what
        assert not np.array_equal(c.vertices[0], c.vertices[1]), what                      # a seed per batch element
        flat = G.flat_faces(c)
        for b in range(2):
            tri = G.triangles(c, b)
            edge = np.linalg.norm(tri[:, [1, 2, 0]] - tri, axis=-1)
            assert (edge[edge > 0] >= 1e-5).all(), (what, edge[edge > 0].min())
            if family not in ("coincident", "lattice", "mixed", "collapsed"):
                assert (edge > 0).all(), what
            zero32 = (fp32_cross(tri) == 0).all(-1)
            assert (zero32[flat[b]]).all(), (what, "a face without fp64 area has an fp32 cross product")
            if family in G.FLAT:
                assert np.array_equal(zero32, flat[b]), what
            kind = (np.arange(f) if c.faces.ndim == 2 or b == 0 else f - 1 - np.arange(f)) % 5   # (listed backwards)
            if family in ("collinear", "coincident"):
                assert flat[b].all(), what
            elif family == "mixed":
                assert flat[b][kind >= 2].all() and not flat[b][kind < 2].any(), what
            elif family == "collapsed":
                assert 0.05 <= flat[b].mean() <= 0.25, what
            elif family != "lattice":
                assert not flat[b].any(), what
        if family == "dyadic":
            assert all(np.array_equal(a, np.round(a / G.GRID) * G.GRID) for a in (c.vertices,)), what
        if family == "offset":
            for b in range(2):
                assert 0.04 <= extent(c.vertices[b]) <= 1.01 and np.abs(c.vertices[b]).min() >= 890, what
        near = [r["near"].mean() for r in G.reference(family, seed)]
        assert max(near) <= 0.5, (what, near)


def test_the_cases_cover_what_they_are_for():
    """over the default run: every face count and cloud size of the soups, both forms of topology in every family, and
    about a third of the points on the surface"""
    if len(SEEDS) < DEFAULT_SEEDS:
        return
    cases = [G.case(family, seed) for family in G.SOUPS for seed in range(DEFAULT_SEEDS)]
    assert {c.faces.shape[-2] for c in cases} == set(G.SOUP_FACES)
    assert {c.points.shape[1] for c in cases} == set(G.CLOUD_SIZES)
    assert {(c.faces.shape[-2], c.faces.ndim) for c in cases} >= {(f, d) for f in (255, 256, 257, 600) for d in (2, 3)}
    for family in G.FAMILIES:
        assert {G.case(family, seed).faces.ndim for seed in range(DEFAULT_SEEDS)} == {2, 3}
        assert {G.case(family, seed).points.shape[1] for seed in range(DEFAULT_SEEDS)} & {257, 1000}
    share = np.mean([r["near"].mean() for c in cases if c.points.shape[1] > 1 for r in G.reference(c.family, c.seed)])
    assert 0.25 <= share <= 0.45, share


@pytest.mark.parametrize("family", G.CLOSED)
def test_closed_families_are_closed_and_oriented_outwards(family):
    """every directed edge once and its reverse once, a positive volume, and the fp64 brute-force winding number
    within 1e-9 of 0 or 1 at every point that is not near; some points are inside"""
    inside = 0
    for seed in SEEDS:
        c = G.case(family, seed)
        for b in range(2):
            faces = faces_of(c.faces, b)
            directed = np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]])
            keys = directed[:, 0] * c.vertices.shape[1] + directed[:, 1]
            back = directed[:, 1] * c.vertices.shape[1] + directed[:, 0]
            assert np.unique(keys).shape == keys.shape and np.array_equal(np.sort(keys), np.sort(back)), G.describe(c)
            assert G.outwards(c.vertices[b], faces) > 0, G.describe(c)
            keep = ~G.reference(family, seed)[b]["near"]
            w = np_winding(c.points[b][keep], G.triangles(c, b))
            assert (np.abs(w - np.round(w)) <= 1e-9).all() and np.isin(np.round(w), (0, 1)).all(), G.describe(c)
            assert np.array_equal(np.round(w) == 1, G.winding(family, seed)[0][b].numpy()[keep] > 0.5)
            inside += int((np.round(w) == 1).sum())
    assert inside >= 50 or len(SEEDS) < DEFAULT_SEEDS


# ------------------------------------------------------------------------------------------------ the distances
# Per family, over the default seeds, of the fp32 CPU composition, as measured (printed again by the test below).  The
# first four: the largest excess of the fp64 distance at the chosen (index, bary) over the fp64 minimum, in units of
# (largest |coordinate difference|)^2 eps32: point -> face and face -> point over the faces with area -- the contract's
# measure; it is 0 where no face has area -- and then over every face, the segments that a face without area is
# included.  The last four: the gradients' errors against the fp64 composition at the same choices in eps32, point ->
# face to the points and the vertices, face -> point to the points and the vertices (not of a soup of one face, see
# geometry_fuzz.gradient_figures).  A figure below 4 stands as 4, as in test_mesh_distance_host.py.  Only the
# well-shaped families are at the five meshes' order of magnitude: slivers, needles and far-off meshes exceed 4 units
# by far although every face has area; a face with two coincident vertices is dropped for most points where it is
# listed as (a,a,c) -- the 0/0 of the ab region -- and served as (a,c,c).
DISTANCE_MEASURED = {
    "well": [0.0423, 0.0317, 0.0423, 0.0317, 0.637, 2.09, 2.93, 2.27],
    "sliver_2": [0.143, 0.0222, 0.143, 0.0222, 0.766, 4.79, 5.68, 4.18],
    "sliver_4": [154, 96.4, 154, 96.4, 0.585, 1.1, 5.64, 3.38],
    "sliver_6": [3.72e+04, 66.8, 3.72e+04, 66.8, 0.766, 2.55, 5.66, 4.84],
    "needle": [23.1, 89.1, 23.1, 89.1, 0.79, 5.67, 9.09, 4.36],
    "collinear": [0, 0, 3.39e+03, 23.2, 0.432, 5.83, 6.24, 6.46],
    "coincident": [0, 0, 1.64e+05, 6.76e+06, 0.761, 2.89, 4.03, 1.08],
    "lattice": [0.236, 0.414, 0.236, 9.25e+04, 1.08, 0.935, 12.6, 3.78],
    "offset": [140, 7.81, 140, 7.81, 734, 252, 9.24e+04, 9.51e+04],
    "mixed_scale": [9.7e-05, 0.00902, 9.7e-05, 0.00902, 0.652, 1.39, 18.4, 15],
    "mixed": [14.1, 7.57, 1.4e+04, 992, 0.734, 9.83, 2.6, 1.14],
    "dyadic": [2.2e+04, 43, 2.2e+04, 43, 0.768, 5.23, 3.71, 2.74],
    "thin": [0.000298, 0.026, 0.000298, 0.026, 0.744, 1.69, 12.4, 14],
    "rows": [0.527, 0.000135, 0.527, 0.000135, 0.655, 2, 23.7, 20.9],
    "collapsed": [0.0299, 0.000435, 0.0299, 3.18e+04, 0.712, 1.26, 16.9, 19.2],
    "far": [51.2, 57, 51.2, 57, 86.9, 37.9, 2.97e+04, 2.71e+04],
}
DISTANCE_LABELS = ["excess point -> face", "excess face -> point", "the same over every face",
                   "the same over every face", "point -> face to points", "to vertices", "face -> point to points",
                   "to vertices"]


def figures_of(pinned, measured):
    """The figures that bound HIP: the pinned ones on the default run; on a longer run (PP_FUZZ_SEEDS) the larger of
    those and the fp32 CPU composition's over the seeds of that run, measured there"""
    return list(pinned) if len(SEEDS) == DEFAULT_SEEDS else [max(a, b) for a, b in zip(pinned, measured())]


def distance_bound(family):
    return [max(f, 4.0) for f in figures_of(DISTANCE_MEASURED[family], lambda: measure_distance(family))]


def host_interpolate(c):
    x, corners = G.tensors(c)[1], G.host_corners(c)
    return lambda face, bary: mesh_sample.mesh_interpolate(x, corners, face, bary)


@functools.lru_cache(maxsize=None)
def measure_distance(family):
    worst = [0.0] * 8
    for seed in SEEDS:
        c = G.case(family, seed)
        pf, fp = G.composed(family, seed)
        G.check_choice(c, pf, fp, host_interpolate(c))
        ref = G.composition_gradients(c, pf, fp, torch.float64)
        got = G.composition_gradients(c, pf, fp, torch.float32)
        figures = G.excess(c, pf, fp) + G.excess(c, pf, fp, True) + G.gradient_figures(c, got, ref)
        worst = [max(a, b) for a, b in zip(worst, figures)]
    return worst


@pytest.mark.parametrize("family", G.FAMILIES)
def test_distance_composition_against_fp64(family):
    """the contract's promises hold of the fp32 CPU composition on every case (``check_choice``; a non-finite gradient
    fails in ``gradient_error``), and its figures are the pinned ones"""
    got = measure_distance(family)
    report("distances: " + "; ".join(DISTANCE_LABELS), family, got, DISTANCE_MEASURED[family])
    assert held(got, distance_bound(family)), got


def test_control_family_is_at_the_five_meshes_order_of_magnitude():
    """test_mesh_distance_host.CPU_MEASURED has 0.0001 to 0.66 units: ``well`` is within one unit too"""
    assert max(DISTANCE_MEASURED["well"][:4]) <= 1.0


def test_the_lowest_index_wins_among_equal_distances_on_the_lattice():
    """against the sequential rule on the composition's own fp32 pair matrix: numpy's argmin is the first minimum"""
    ties = 0
    for seed in SEEDS:
        c = G.case("lattice", seed)
        d = G.pair_matrix32(c)
        pf, fp = G.composed("lattice", seed)
        assert np.array_equal(pf.face.numpy(), np.where(np.isinf(d.min(2)), -1, d.argmin(2))), G.describe(c)
        assert np.array_equal(fp.point.numpy(), np.where(np.isinf(d.min(1)), -1, d.argmin(1))), G.describe(c)
        ties += int(((d == d.min(2, keepdims=True)).sum(2) > 1).sum())
    assert ties >= 100 or len(SEEDS) < DEFAULT_SEEDS                        # there was something to decide


# -------------------------------------------------------------------------------------------------- the winding
# Per family, the largest |w32 - w64| of the fp32 CPU composition against the fp64 one over the points that are not
# near (farther than 1e-4 of the extent from every face), over the default seeds, as measured.  The GPU test bounds HIP
# by 4 x max(figure, 16 eps32), test_mesh_winding_host.fp32_bound's rule; the fp32 CPU composition is held to 2 x that
# maximum here, as there: another CPU's atan2 and sqrt may differ in their last bits.
WINDING_MEASURED = {
    "well": [7.22e-07],
    "sliver_2": [0.000536],
    "sliver_4": [8.84e-06],
    "sliver_6": [0.000257],
    "needle": [0.000368],
    "collinear": [0.000172],
    "coincident": [0.000825],
    "lattice": [1.33e-07],
    "offset": [1.48e-05],
    "mixed_scale": [2.73e-05],
    "mixed": [1.98e-05],
    "dyadic": [0.000199],
    "thin": [3.68e-05],
    "rows": [9.04e-05],
    "collapsed": [3.21e-06],
    "far": [2.09e-06],
}


@functools.lru_cache(maxsize=None)
def measure_winding(family):
    worst = 0.0
    for seed in SEEDS:
        c = G.case(family, seed)
        w64, w32 = G.winding(family, seed)
        keep = torch.from_numpy(G.not_near(family, seed))
        assert bool(torch.isfinite(w32).all()) and bool(torch.isfinite(w64).all()), G.describe(c)
        worst = max(worst, float((w32.double() - w64)[keep].abs().max()) if bool(keep.any()) else 0.0)
        if family in G.CLOSED:
            assert torch.equal((w32 > 0.5)[keep], (w64 > 0.5)[keep]), G.describe(c)
            out = mesh_winding.signed_distance_composition(*G.tensors(c), G.host_corners(c))
            pf = G.composed(family, seed)[0]
            assert all(a.numpy().tobytes() == b.numpy().tobytes() for a, b in zip(out[1:4], pf)), G.describe(c)
            assert torch.equal(out.signed, torch.where(w32 > 0.5, -pf.dist.sqrt(), pf.dist.sqrt())), G.describe(c)
    return [worst]


def winding_bound(family):
    return max(figures_of(WINDING_MEASURED[family], lambda: measure_winding(family))[0], 16 * EPS32)


@pytest.mark.parametrize("family", G.FAMILIES)
def test_winding_composition_against_fp64(family):
    """finite at every point; at the points that are not near, the pinned figure; on the closed families the fp64
    composition's side at those points, and the signed distance is the distance with that sign"""
    worst = measure_winding(family)[0]
    report("winding |w32 - w64| off the surface", family, [worst], WINDING_MEASURED[family])
    assert held([worst], [2 * winding_bound(family)]), worst


# ------------------------------------------------------------------------------------------------- the sampling
@pytest.mark.parametrize("family", G.FAMILIES)
def test_sampling_composition(family):
    """``check_samples`` on the composition: the restatement's faces, no face without area drawn, -1 and NaN where an
    element has no area at all, every sample on its face within 4 units"""
    worst, empty = 0.0, 0
    for seed in SEEDS:
        c = G.case(family, seed)
        out, areas = G.sample_run(c, "cpu")
        worst = max(worst, G.check_samples(c, out, areas))
        empty += int((out.face == -1).all())
    print("%s: a sample is off its face by at most %.3g units" % (family, worst))
    assert empty == (len(SEEDS) if family in ("collinear", "coincident") else 0)


# -------------------------------------------------------------------------------------------------- the normals
# Per family, the errors of the fp32 CPU compositions against the fp64 ones over the default seeds, in the order of
# geometry_fuzz.NORMALS_METRICS and in eps32, as measured: unit normals absolutely, areas over |ab| |ac|, gradients over
# the largest |gradient|.  A figure below 4 stands as 4, as in test_gpu_mesh_normals.py; held to 2 x here (another
# CPU's sqrt).  The area of a 1e-6 sliver is wrong by its own size and its normal by an angle of order 1: the cross
# product's rounding, eps32 |ab| |ac|, is what the area is made of.
NORMALS_MEASURED = {
    "well": [1.06, 0.716, 1.75, 1.26, 2.45, 0.989, 1.4],
    "sliver_2": [33.1, 1.04, 23.4, 44.7, 15.4, 44.7, 15.5],
    "sliver_4": [3.49e+03, 0.829, 2.99e+03, 5.16e+03, 1.29e+03, 5.16e+03, 1.29e+03],
    "sliver_6": [3.26e+05, 1.03, 2.02e+05, 4.22e+05, 7.49e+05, 4.22e+05, 7.49e+05],
    "needle": [6.87e+04, 3.85e+04, 4.17e+04, 8.09e+04, 2.49e+04, 8.09e+04, 2.49e+04],
    "collinear": [0, 0, 0, 0, 0, 0, 0],
    "coincident": [0, 0, 0, 0, 0, 0, 0],
    "lattice": [0.569, 0.228, 1.13, 0.569, 5.51, 0.655, 4.13],
    "offset": [0.961, 0.444, 1.64, 0.961, 1.97, 0.716, 1.19],
    "mixed_scale": [0.977, 0.629, 2.21, 1.07, 1.28, 1.09, 1.18],
    "mixed": [3.16e+03, 0.72, 1.75e+03, 3.16e+03, 1.17e+03, 3.16e+03, 1.17e+03],
    "dyadic": [9.33e+03, 0.454, 1.16e+04, 1.27e+04, 1.09e+04, 1.27e+04, 1.09e+04],
    "thin": [151, 9.27, 213, 148, 156, 219, 295],
    "rows": [1.05, 0.706, 1.64, 1.1, 2.14, 0.976, 1.87],
    "collapsed": [0.902, 0.553, 1.14, 1.05, 1.52, 0.951, 1.57],
    "far": [0.997, 0.447, 1.42, 0.875, 2.13, 1.01, 1.77],
}


@functools.lru_cache(maxsize=None)
def measure_normals(family):
    worst = [0.0] * 7
    for seed in SEEDS:
        c = G.case(family, seed)
        ref, cpu32 = G.mesh_references(family, seed, "normals")
        worst = [max(a, e / EPS32) for a, e in zip(worst, G.normals_errors(c, cpu32, ref))]
        if family in G.FLAT + ["mixed"]:
            G.check_flat_normals(c, cpu32)
            G.check_flat_normals(c, ref)
    return worst


def test_dyadic_slivers_tell_a_recovered_difference_of_products_from_a_plain_one():
    """The kernels' cross product is csrc/mesh_common.h's v3_dop, ``a*b - c*d`` within 1.5 ulp of the exact value; the
    compositions' is the plain difference of two rounded products.  On ``dyadic`` the edge vectors and the cross product
    are exact in fp32 and the products are not, so the first, emulated in numpy with an fp32 fma, gives every area
    within 4 eps32 of itself -- 1.5 ulp a component, three squares and two sums, a root that halves the error, 3 eps32
    in all -- and the second misses that on every case, by a factor of 1e3 on the larger ones.  The bound of 4 eps32 is
    what tests/test_gpu_geometry_fuzz.py holds HIP's areas to on this family."""
    plain_worst = 0.0
    for seed in SEEDS:
        c = G.case("dyadic", seed)
        normals = G.mesh_references("dyadic", seed, "normals")[0][0]

        def area(dop):
            return np.stack([G.np_area32(G.triangles(c, b), dop) for b in range(2)]).astype(np.float64)

        kahan = G.dyadic_errors(c, normals, area(G.np_dop))[0]
        plain = G.dyadic_errors(c, normals, area(lambda a, b, c_, d: a * b - c_ * d))[0]
        print("%s: relative area error %.3g eps32 recovered, %.3g eps32 plain" % (G.describe(c), kahan / EPS32,
                                                                                  plain / EPS32))
        assert kahan <= 4 * EPS32 < plain, G.describe(c)
        plain_worst = max(plain_worst, plain)
    assert plain_worst >= 1000 * EPS32 or len(SEEDS) < DEFAULT_SEEDS


def normals_bound(family):
    return [max(f, 4.0) for f in figures_of(NORMALS_MEASURED[family], lambda: measure_normals(family))]


@pytest.mark.parametrize("family", G.FAMILIES)
def test_normals_compositions_against_fp64(family):
    got = measure_normals(family)
    report("normals: " + "; ".join(G.NORMALS_METRICS), family, got, NORMALS_MEASURED[family])
    assert held(got, [2 * b for b in normals_bound(family)]), got


# ----------------------------------------------------------------------- the dihedral angles and the cotangents
# Per manifold family, topology_fuzz.measure (largest absolute error over largest absolute reference) of the fp32 CPU
# compositions against the fp64 ones over the default seeds, as measured: the dihedral angles and their gradient; the
# cotangent weights, the cot-Laplacian applied with them and its gradient.  test_topology_fuzz_host.within_the_rule
# bounds HIP by 4 x the figure, floor 1e-6; held to 2 x max(figure, 1e-6) here (another CPU's acos and sqrt).
DIHEDRAL_MEASURED = {
    "thin": [3.68e-05, 0.00973],
    "rows": [2.75e-05, 0.00503],
    "collapsed": [1.41e-05, 0.00342],
    "far": [1.39e-05, 0.0795],
}
COT_MEASURED = {
    "thin": [0.0364, 0.0106, 0.0361],
    "rows": [0.23, 0.0065, 0.0581],
    "collapsed": [8.74e-07, 1.02e-06, 3.53e-07],
    "far": [7.78e-07, 5.81e-07, 3.78e-07],
}


def flat_wing(c, table, count, b):
    """(count,) bool: the edges of which a wing triangle has no fp64 area"""
    v, t = c.vertices[b], table[b, :count]
    one = (np.cross(v[t[:, 2]] - v[t[:, 0]], v[t[:, 1]] - v[t[:, 0]]) ** 2).sum(-1) == 0
    two = (np.cross(v[t[:, 3]] - v[t[:, 1]], v[t[:, 0]] - v[t[:, 1]]) ** 2).sum(-1) == 0
    return one | two


def check_degenerate_rules(c, angles, table, counts, weights):
    """``collapsed``: a wing normal of length <= 1e-12 -- exactly 0 here -- contributes zero, so the dot is 0 and the
    angle pi - acos(0) = pi/2 to fp32's rounding of it; a face with two equal vertices has Heron's area exactly 0
    (l1 = l2, l3 = 0: s - l1 = 0) and the cotangents the reference's ``A == 0 -> 0`` mask gives: exactly 0"""
    hit = 0
    for b in range(2):
        wing = flat_wing(c, table, counts[b], b)
        hit += int(wing.sum())
        assert (np.abs(angles[b, :counts[b]][wing] - np.pi / 2) <= 4 * EPS32).all(), G.describe(c)
    flat = G.flat_faces(c)
    assert hit > 0 and flat.any() and (weights[flat] == 0).all(), G.describe(c)


@functools.lru_cache(maxsize=None)
def measure_manifold(family):
    worst = {"dihedral": [0.0] * 2, "cot": [0.0] * 3}
    for seed in SEEDS:
        c = G.case(family, seed)
        for op in worst:
            ref, cpu32 = G.mesh_references(family, seed, op)
            assert all(np.isfinite(a).all() for a in cpu32 + ref), (G.describe(c), op)
            worst[op] = [max(w, T.measure(a, r)) for w, a, r in zip(worst[op], cpu32, ref)]
        if family == "collapsed":
            for dtype, k in ((torch.float64, 0), (torch.float32, 1)):
                out, table, counts = G.dihedral_run(c, "cpu", dtype)
                check_degenerate_rules(c, out[0], table, counts, G.mesh_references(family, seed, "cot")[k][0])
    return worst


def manifold_bound(family, op):
    """test_topology_fuzz_host.within_the_rule's bound over the figures: 4 x the composition's, floor 1e-6"""
    pinned = {"dihedral": DIHEDRAL_MEASURED, "cot": COT_MEASURED}[op][family]
    return [max(4 * f, 1e-6) for f in figures_of(pinned, lambda: measure_manifold(family)[op])]


@pytest.mark.parametrize("family", G.MANIFOLDS)
def test_dihedral_and_cotangent_compositions_against_fp64(family):
    got = measure_manifold(family)
    report("dihedral angles; their gradient", family, got["dihedral"], DIHEDRAL_MEASURED[family])
    report("cotangent weights; cot-Laplacian; its gradient", family, got["cot"], COT_MEASURED[family])
    assert held(got["dihedral"], [2 * max(f, 1e-6) for f in DIHEDRAL_MEASURED[family]]), got
    assert held(got["cot"], [2 * max(f, 1e-6) for f in COT_MEASURED[family]]), got
