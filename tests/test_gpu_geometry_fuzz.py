"""GPU tests of the operators that do arithmetic per triangle on the ill-shaped geometry of tests/geometry_fuzz.py, the
cases that tests/test_geometry_fuzz_host.py pins on the CPU: slivers, needles, collinear and coincident vertices, exact
ties, meshes far from the origin, faces of very different sizes, thin closed meshes, collapsed grid rows.  Where the
contract promises bits -- both directions of the point-to-mesh distance, the fused walk of the signed distance, the
sampling's faces, weights and points -- HIP equals the fp32 CPU composition to the bit, NaN pattern and -1s included;
everything else is bound by the operator's own rule over the figure pinned for the fp32 CPU composition in the host
file (4 x the figure, with the floor of 4 units, 4 eps32, 16 eps32 or 1e-6), never over anything HIP gives.  What the
contracts promise outright is checked of HIP's output on its own, against fp64 alone."""
import numpy as np
import pytest
import torch

import geometry_fuzz as G
import topology_fuzz as T
from pytorch_points_amd import mesh_distance, mesh_normals, mesh_sample, mesh_winding
from test_geometry_fuzz_host import (DISTANCE_LABELS, SEEDS, check_degenerate_rules, distance_bound, manifold_bound,
                                     normals_bound, winding_bound)
from test_gpu_mesh_distance import bits, dev_t, same

pytestmark = pytest.mark.gpu

F32 = np.float32
EPS32 = 2.0 ** -23


def device_case(c, grad=False):
    """(points, vertices, corners) of a case on the device"""
    return (dev_t(c.points.astype(F32), grad), dev_t(c.vertices.astype(F32), grad), G._corners(c, "cuda"))


def to_cpu(out):
    return type(out)(*(t.detach().cpu() for t in out))


def hip_distances(c):
    pts, x, corners = device_case(c)
    return mesh_distance.point_face_distance(pts, x, corners), mesh_distance.face_point_distance(pts, x, corners)


# ------------------------------------------------------------------------------------------------ the distances
@pytest.mark.parametrize("family", G.FAMILIES)
def test_distances_equal_the_composition_to_the_bit_and_keep_the_contract(cuda, family):
    """``dist``, index and ``bary`` of both directions are the fp32 CPU composition's byte for byte, the NaN pattern
    and the -1s with them; HIP's own output keeps what the contract promises (geometry_fuzz.check_choice: decided from
    fp64 and from ``mesh_interpolate`` on the device, not from the composition); and its excess over the fp64 minimum
    is within the figure pinned for the composition"""
    worst = [0.0] * 4
    for seed in SEEDS:
        c = G.case(family, seed)
        pts, x, corners = device_case(c)
        pf, fp = hip_distances(c)
        assert pf.face.dtype == torch.int64 and pf.dist.is_cuda and fp.bary.shape == (2, c.faces.shape[-2], 3)
        G.check_choice(c, to_cpu(pf), to_cpu(fp),
                       lambda face, bary: mesh_sample.mesh_interpolate(x, corners, face.cuda(), bary.cuda()).cpu())
        want = G.composed(family, seed)
        assert same(pf, want[0]), (G.describe(c), "point -> face")
        assert same(fp, want[1]), (G.describe(c), "face -> point")
        worst = [max(a, b) for a, b in zip(worst, G.excess(c, pf, fp) + G.excess(c, pf, fp, True))]
    print("%s: HIP's excess over the fp64 minimum (%s): %s units, bound %s" % (
        family, "; ".join(DISTANCE_LABELS[:4]), ", ".join("%.3g" % w for w in worst), distance_bound(family)[:4]))
    assert all(w <= b for w, b in zip(worst, distance_bound(family)[:4])), worst


@pytest.mark.parametrize("family", G.FAMILIES)
def test_distance_gradients_against_the_fp64_composition(cuda, family):
    """to the points and to the vertices, both directions, with a random incoming gradient: finite everywhere, and
    against the fp64 CPU composition at HIP's own ``(index, bary)`` within 4 x the figure pinned for the fp32 CPU
    composition, itself lifted to 4 eps32 -- test_gpu_mesh_distance.py's bound"""
    worst = [0.0] * 4
    for seed in SEEDS:
        c = G.case(family, seed)
        pts, x, corners = device_case(c, grad=True)
        g1, g2 = (dev_t(g.astype(F32)) for g in G.incoming(family, seed))
        pf = mesh_distance.point_face_distance(pts, x, corners)
        fp = mesh_distance.face_point_distance(pts, x, corners)
        assert "MeshDistance" in type(pf.dist.grad_fn).__name__ and "MeshDistance" in type(fp.dist.grad_fn).__name__
        grads = torch.autograd.grad(pf.dist, (pts, x), g1) + torch.autograd.grad(fp.dist, (pts, x), g2)
        grads = [g.double().cpu().numpy() for g in grads]
        assert all(np.isfinite(g).all() for g in grads), G.describe(c)
        ref = G.composition_gradients(c, pf, fp, torch.float64)
        worst = [max(a, b) for a, b in zip(worst, G.gradient_figures(c, grads, ref))]
    bound = [4 * b for b in distance_bound(family)[4:]]
    print("%s: HIP's gradient errors (%s): %s eps32, bound %s" % (
        family, "; ".join(DISTANCE_LABELS[4:]), ", ".join("%.3g" % w for w in worst), bound))
    assert all(w <= b for w, b in zip(worst, bound)), worst


def test_the_lowest_index_wins_among_equal_distances_on_the_lattice(cuda):
    """against the sequential rule on the composition's own fp32 pair matrix: numpy's argmin is the first minimum.
    Ties fall inside an LDS tile and across tiles (F = 257 and 600, P = 1000 and the face -> point tile of 1024)."""
    ties = 0
    for seed in SEEDS:
        c = G.case("lattice", seed)
        d = G.pair_matrix32(c)
        pf, fp = hip_distances(c)
        assert np.array_equal(pf.face.cpu().numpy(), np.where(np.isinf(d.min(2)), -1, d.argmin(2))), G.describe(c)
        assert np.array_equal(fp.point.cpu().numpy(), np.where(np.isinf(d.min(1)), -1, d.argmin(1))), G.describe(c)
        ties += int(((d == d.min(2, keepdims=True)).sum(2) > 1).sum())
    assert ties >= 100 or len(SEEDS) < 8


# ------------------------------------------------------------------------ the winding number and the signed distance
@pytest.mark.parametrize("family", G.FAMILIES)
def test_winding_and_signed_distance(cuda, family):
    """The fused walk equals the two separate walks to the bit, its ``dist``, ``face`` and ``bary`` are
    ``point_face_distance``'s; the winding number is finite at every point, and at the points that are not near (fp64:
    farther than 1e-4 of the extent from every face) within 4 x max(the figure pinned for the fp32 CPU composition,
    16 eps32) of the fp64 composition; on the closed families ``points_inside_mesh`` is the fp64 composition's at
    those points and ``signed`` is -+sqrt(dist) accordingly"""
    worst = 0.0
    for seed in SEEDS:
        c = G.case(family, seed)
        pts, x, corners = device_case(c)
        fused = mesh_winding.point_mesh_signed_distance(pts, x, corners)
        alone = mesh_winding.mesh_winding_number(pts, x, corners)
        assert same(fused[1:4], mesh_distance.point_face_distance(pts, x, corners)), G.describe(c)
        assert bits(fused.winding) == bits(alone), G.describe(c)
        assert bool(torch.isfinite(alone).all()), G.describe(c)
        inside = mesh_winding.points_inside_mesh(pts, x, corners)
        assert torch.equal(inside, alone > 0.5)
        root = torch.where(fused.face >= 0, fused.dist.sqrt(), torch.full_like(fused.dist, float("nan")))
        assert same([fused.signed], [torch.where(inside, -root, root)]), G.describe(c)
        w64 = G.winding(family, seed)[0]
        keep = torch.from_numpy(G.not_near(family, seed))
        if bool(keep.any()):
            worst = max(worst, float((alone.double().cpu() - w64)[keep].abs().max()))
        if family in G.CLOSED:
            assert torch.equal(inside.cpu()[keep], (w64 > 0.5)[keep]), G.describe(c)
            assert bool((fused.signed.cpu()[keep & (w64 > 0.5)] < 0).all()), G.describe(c)
            assert bool((fused.signed.cpu()[keep & (w64 < 0.5)] > 0).all()), G.describe(c)
    print("%s: |w_hip - w64| off the surface %.3g, bound %.3g" % (family, worst, 4 * winding_bound(family)))
    assert worst <= 4 * winding_bound(family)


# ------------------------------------------------------------------------------------------------- the sampling
@pytest.mark.parametrize("family", G.FAMILIES)
def test_sampling(cuda, family):
    """geometry_fuzz.check_samples on HIP's draw (the restatement's faces on HIP's own areas, no face without area
    drawn, -1 and NaN for an element without area, every sample on its face within 4 units); weights, points and
    normals are the fp32 CPU composition's to the bit, as test_gpu_mesh_sample.py asserts for the five meshes; the CDF
    that the faces are searched in is non-decreasing and ends at the fp64 sum of the areas"""
    worst = 0.0
    for seed in SEEDS:
        c = G.case(family, seed)
        out, areas = G.sample_run(c, "cuda")
        worst = max(worst, G.check_samples(c, out, areas))
        _, x, corners = device_case(c)
        cdf = mesh_sample._cdf(areas.contiguous()).cpu().numpy()
        assert (np.diff(cdf, axis=1) >= 0).all() and (cdf[:, 0] >= 0).all(), G.describe(c)
        total = areas.double().cpu().numpy().sum(1)
        assert (np.abs(cdf[:, -1] - total) <= 2 * cdf.shape[1] * 2.0 ** -53 * total).all(), G.describe(c)
        assert torch.equal(mesh_sample.mesh_sample_faces(areas, dev_t(G.sample_uniforms(c)[..., 0])), out.face)
        bary = mesh_sample.bary_composition(torch.from_numpy(G.sample_uniforms(c)))
        bary = torch.where((out.face.cpu() >= 0)[..., None], bary, torch.full_like(bary, float("nan")))
        want = mesh_sample.sample_composition(G.tensors(c)[1], G.host_corners(c), face=out.face.cpu(), bary=bary)[0]
        assert same([out.bary, out.points], [bary, want]), G.describe(c)
        assert same([mesh_sample.mesh_interpolate(x, corners, out.face, out.bary)], [want]), G.describe(c)
        normals = mesh_normals.mesh_face_normals(x, corners)[0]
        rows = out.face.clamp(min=0) + torch.arange(2, device="cuda")[:, None] * corners.n_faces
        picked = normals.reshape(-1, 3)[rows.reshape(-1)].reshape(out.normals.shape)
        picked = torch.where((out.face >= 0)[..., None], picked, torch.full_like(picked, float("nan")))
        assert same([out.normals], [picked]), G.describe(c)
    print("%s: a sample of HIP's is off its face by at most %.3g units" % (family, worst))


# -------------------------------------------------------------------------------------------------- the normals
@pytest.mark.parametrize("family", G.FAMILIES)
def test_normals_against_the_fp64_composition(cuda, family):
    """test_gpu_mesh_normals.py's rule: every metric of HIP against the fp64 CPU composition is within 4 x the figure
    pinned for the fp32 CPU composition (never below 4 eps32), the areas in units of |ab| |ac| eps32; the degenerate
    rule of DESIGN.md "Mesh normals" holds exactly where a face has no area.  On ``dyadic``, where the composition's
    plain difference of products is wrong by 1e3 eps32 and so bounds nothing, HIP's areas are within 4 eps32 of
    themselves and its normals within 8 eps32 (1.5 ulp a component, the length's 3 eps32, the division):
    test_geometry_fuzz_host.py derives the figure and shows that a plain ``a*b - c*d`` misses it."""
    worst = [0.0] * 7
    for seed in SEEDS:
        c = G.case(family, seed)
        got = G.normals_run(c, "cuda", torch.float32)
        errors = G.normals_errors(c, got, G.mesh_references(family, seed, "normals")[0])
        worst = [max(a, e / EPS32) for a, e in zip(worst, errors)]
        if family in G.FLAT + ["mixed"]:
            G.check_flat_normals(c, got)
        if family == "dyadic":                                # exact edge vectors and cross products: v3_dop's 1.5 ulp
            area_error, normal_error = G.dyadic_errors(c, got[0], got[1])   # a component is 3 eps32 of an area
            print("%s: relative area error %.3g eps32, normals %.3g eps32" % (G.describe(c), area_error / EPS32,
                                                                              normal_error / EPS32))
            assert area_error <= 4 * EPS32 and normal_error <= 8 * EPS32, G.describe(c)
    bound = [4 * b for b in normals_bound(family)]
    print("%s: HIP's errors (%s): %s eps32, bound %s" % (family, "; ".join(G.NORMALS_METRICS),
                                                         ", ".join("%.3g" % w for w in worst), bound))
    assert all(w <= b for w, b in zip(worst, bound)), worst


# ----------------------------------------------------------------------- the dihedral angles and the cotangents
@pytest.mark.parametrize("family", G.MANIFOLDS)
def test_dihedral_angles_and_cotangents_against_the_fp64_compositions(cuda, family):
    """test_topology_fuzz_host.within_the_rule over the pinned figures: topology_fuzz.measure of HIP against the fp64
    CPU composition is within 4 x the fp32 CPU composition's, floor 1e-6, for the angles and their gradient, the
    cotangent weights, the cot-Laplacian applied with them and its gradient; on ``collapsed`` the deliberate
    degenerate rules hold exactly"""
    worst = {"dihedral": [0.0] * 2, "cot": [0.0] * 3}
    for seed in SEEDS:
        c = G.case(family, seed)
        angles, table, counts = G.dihedral_run(c, "cuda", torch.float32)
        got = {"dihedral": angles, "cot": G.cot_run(c, "cuda", torch.float32)}
        for op in worst:
            assert all(np.isfinite(a).all() for a in got[op]), (G.describe(c), op)
            ref = G.mesh_references(family, seed, op)[0]
            worst[op] = [max(w, T.measure(a, r)) for w, a, r in zip(worst[op], got[op], ref)]
        if family == "collapsed":
            check_degenerate_rules(c, angles[0], table, counts, got["cot"][0])
    for op in worst:
        bound = manifold_bound(family, op)
        print("%s, %s: HIP %s, bound %s" % (family, op, ", ".join("%.3g" % w for w in worst[op]), bound))
        assert all(w <= b for w, b in zip(worst[op], bound)), (op, worst[op])
