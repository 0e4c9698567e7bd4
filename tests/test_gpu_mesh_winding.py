"""GPU tests of the mesh winding number and the signed point-to-mesh distance (csrc/mesh_winding.hip through
pytorch_points_amd/mesh_winding.py): the winding number against the fp64 CPU composition within 4 x the pinned error
of the fp32 CPU composition, every point's side, the fused walk against ``point_face_distance`` and the winding-alone
walk to the bit, gradients to the bit, indices out of range handed straight to the entry points, shared and
per-element topology, empty problems, run-to-run identity, graph capture and a side stream, the surface itself, the
geo_operations names and MeshEnclosureLoss."""
import functools

import numpy as np
import pytest
import torch

from pytorch_points_amd import _lib, mesh_distance, mesh_winding
from pytorch_points_amd.mesh_laplacian import MeshCorners
from pytorch_points_amd.network import geo_operations, model_loss
from test_gpu_mesh_distance import bits, deterministic, dev_t, hip_distances, same
from test_mesh_distance_host import SIZES, cloud, repeated_cloud, tie_mesh
from test_mesh_sample_host import MESHES
from test_mesh_winding_host import (NAMES, TILE, fp32_bound, sided_cloud, surface_cloud, winding64,
                                    winding_mesh)

pytestmark = pytest.mark.gpu

F32 = np.float32
EPS32 = 2.0 ** -23


@functools.lru_cache(maxsize=None)
def device_mesh(name):
    v, faces = winding_mesh(name)
    return dev_t(v.astype(F32)), MeshCorners.from_faces(dev_t(faces), v.shape[1])


@functools.lru_cache(maxsize=None)
def hip_signed(name, k):
    """HIP's ``PointMeshSignedDistance`` on ``sided_cloud(name, k)``, computed once"""
    x, corners = device_mesh(name)
    return mesh_winding.point_mesh_signed_distance(dev_t(sided_cloud(name, k)[0].astype(F32)), x, corners)


# ------------------------------------------------------------------------------------------------- 1. accuracy
@pytest.mark.parametrize("name", NAMES + TILE)
def test_winding_against_the_fp64_composition(cuda, name):
    """|w_hip - w64| <= 4 max(the pinned |w32 - w64| of the fp32 CPU composition, 16 eps32) per mesh and cloud: the
    halves are summed in fp64 on both sides, so HIP and the fp32 CPU composition differ in the last bits of atan2f
    alone.  ``inside`` is the fp64 composition's on every point of every sided cloud, the open meshes' included, where
    a winding number comes nearest to 0.5 (7.9e-6 from it on the grid at P = 1000, against an error of 1e-6).
    DESIGN.md "Mesh winding numbers and signed distance" records the measured figures."""
    x, corners = device_mesh(name)
    failed = []
    for k, p in enumerate(SIZES):
        pts = dev_t(sided_cloud(name, k)[0].astype(F32))
        got = mesh_winding.mesh_winding_number(pts, x, corners)
        assert got.shape == (x.shape[0], p) and got.dtype == torch.float32 and got.is_cuda and not got.requires_grad
        want = winding64(name, k)
        error, bound = float((got.double().cpu() - want).abs().max()), 4 * fp32_bound(name, k)
        print("%s, P=%d: |w_hip - w64| %.3g, bound %.3g" % (name, p, error, bound))
        if not error <= bound:
            failed.append((p, error, bound))
        inside = mesh_winding.points_inside_mesh(pts, x, corners)
        margin = float((want - 0.5).abs().min())
        print("%s, P=%d: smallest |w64 - 0.5| %.3g" % (name, p, margin))
        assert inside.dtype == torch.bool and torch.equal(inside.cpu(), want > 0.5), (name, p, margin, error)
        assert bits(hip_signed(name, k).winding) == bits(got)
    assert not failed, failed


# ------------------------------------------------------------------------------------------ 2. exact agreement
def fused_and_separate(pts, x, corners):
    fused = mesh_winding.point_mesh_signed_distance(pts, x, corners)
    assert fused._fields == ("signed", "dist", "face", "bary", "winding") and fused.face.dtype == torch.int64
    return fused, mesh_distance.point_face_distance(pts, x, corners), mesh_winding.mesh_winding_number(pts, x, corners)


@pytest.mark.parametrize("name", NAMES + TILE)
def test_the_fused_walk_equals_the_two_separate_walks_to_the_bit(cuda, name):
    """``dist``, ``face`` and ``bary`` are ``point_face_distance``'s and ``winding`` is the winding-alone entry's, on
    the sided clouds and on the distances' own clouds, which hold points on the surface"""
    x, corners = device_mesh(name)
    for k, p in enumerate(SIZES):
        fused, pf, alone = fused_and_separate(dev_t(sided_cloud(name, k)[0].astype(F32)), x, corners)
        assert same(fused[1:4], pf), (name, p)
        assert bits(fused.winding) == bits(alone), (name, p)
        inside = fused.winding > 0.5
        assert torch.equal(fused.signed, torch.where(inside, -fused.dist.sqrt(), fused.dist.sqrt()))
        if name in MESHES:
            pts = dev_t(cloud(name, k).astype(F32))
            fused = mesh_winding.point_mesh_signed_distance(pts, x, corners)
            assert same(fused[1:4], hip_distances(name, k)[0]), (name, p, "with points on the surface")
            assert bits(fused.winding) == bits(mesh_winding.mesh_winding_number(pts, x, corners))
            assert bool(torch.isfinite(fused.winding).all()) and bool(torch.isfinite(fused.signed).all())


def test_the_fused_walk_decides_ties_as_point_face_distance_does(cuda):
    v, faces = tie_mesh()
    x, corners = dev_t(v.astype(F32)), MeshCorners.from_faces(dev_t(faces), v.shape[1])
    pts = dev_t(cloud("grid_40x130", 2).astype(F32))
    fused, pf, alone = fused_and_separate(pts, x, corners)
    assert same(fused[1:4], pf) and bits(fused.winding) == bits(alone)
    assert bool((fused.face < faces.shape[0] // 2).all())
    for name in ("cage", "two_topologies"):
        x, corners = device_mesh(name)
        fused, pf, alone = fused_and_separate(dev_t(repeated_cloud(name).astype(F32)), x, corners)
        assert same(fused[1:4], pf) and same(fused[1:4], hip_distances(name, "repeated")[0])
        assert bits(fused.winding) == bits(alone)
        assert bits(fused.winding[:, 1000:]) == bits(fused.winding[:, :32])


def signed_gradients(name):
    """``(signed distance, d sum(signed^2) / d (points, vertices))``, and ``point_face_distance``'s gradients of
    ``dist`` with the incoming gradient 1 where ``dist > 0`` and 0 elsewhere, on ``cloud(name, 3)``"""
    x, corners = device_mesh(name)
    x = x.clone().requires_grad_(True)
    p = dev_t(cloud(name, 3).astype(F32), True)
    out = mesh_winding.point_mesh_signed_distance(p, x, corners)
    assert "MeshSignedDistance" in type(out.dist.grad_fn).__name__
    assert not out.face.requires_grad and not out.bary.requires_grad and not out.winding.requires_grad
    got = torch.autograd.grad((out.signed * out.signed).sum(), (p, x))
    pf = mesh_distance.point_face_distance(p, x, corners)
    want = torch.autograd.grad(pf.dist, (p, x), (pf.dist > 0).float())
    return out, got, want


@pytest.mark.parametrize("name", MESHES)
def test_gradients_of_signed_squared_are_point_face_distances_to_the_bit(cuda, name):
    """d signed^2 / d dist = (2 signed) (1 / (2 signed)) = 1 exactly where dist > 0, and 0 where dist == 0, so both
    gradients are the backward of ``point_face_distance`` for that incoming gradient: the same launches"""
    out, got, want = signed_gradients(name)
    off = out.dist > 0
    assert bool(off.any()) and bool((~off).any())                              # the cloud has points on the surface
    assert bool(torch.isfinite(got[0]).all()) and bool(torch.isfinite(got[1]).all())
    assert bits(got[0][off]) == bits(want[0][off]) and bool((got[0][~off] == 0).all())
    assert bits(got[1]) == bits(want[1]) and bool((got[1] != 0).any())


# ------------------------------------------------------------------------------------------------ 3. robustness
def raw_forward(pts, x, faces, shared):
    """the records and the three walks, handed ``faces`` as they are: ``(winding alone, fused (dist, face, bary,
    winding), point -> face (dist, face, bary))``"""
    b, n, _ = x.shape
    p, f = pts.shape[1], faces.shape[1]
    records = torch.empty(b, f, mesh_distance.RECORD, device="cuda")
    alone = torch.empty(b, p, device="cuda")
    triple = lambda: (torch.empty(b, p, device="cuda"), torch.empty(b, p, dtype=torch.int64, device="cuda"),   # noqa: E731
                      torch.empty(b, p, 3, device="cuda"))
    fused, pf = triple() + (torch.empty(b, p, device="cuda"),), triple()
    lib = _lib.lib()
    with _lib.on_device(x.device) as stream:
        _lib.check(lib.pp_mesh_distance_records_f32(_lib.ptr(x), _lib.ptr(faces), _lib.ptr(records), b, n, f, shared,
                                                    stream), "records")
        _lib.check(lib.pp_mesh_winding_forward_f32(_lib.ptr(pts), _lib.ptr(records), _lib.ptr(alone), b, p, f, stream),
                   "winding")
        _lib.check(lib.pp_mesh_signed_distance_forward_f32(_lib.ptr(pts), _lib.ptr(records), *map(_lib.ptr, fused),
                                                           b, p, f, stream), "fused")
        _lib.check(lib.pp_mesh_point_face_forward_f32(_lib.ptr(pts), _lib.ptr(records), *map(_lib.ptr, pf), b, p, f,
                                                      stream), "point -> face")
    return alone, fused, pf


def test_indices_out_of_range_are_skipped_and_the_stream_goes_on(cuda):
    """a faces entry of -1 and one of N go straight to the entries: those two faces add nothing to any point's sum and
    are never chosen, so every item has the bytes of a run on the table without them (the same terms in the same
    order), and the next call is a clean one"""
    v, faces = winding_mesh("cage")
    n, f = v.shape[1], faces.shape[0]
    x, corners = device_mesh("cage")
    pts = dev_t(sided_cloud("cage", 3)[0].astype(F32))
    good = hip_signed("cage", 3)
    alone, fused, pf = raw_forward(pts, x, corners.faces, 1)
    assert bits(alone) == bits(good.winding) and same(fused, good[1:]) and same(pf, good[1:4])
    hit = [int(good.face[0].mode().values), f - 1]
    bad = faces.copy()
    bad[hit[0], 1], bad[hit[1], 2] = -1, n
    alone, fused, pf = raw_forward(pts, x, dev_t(bad)[None], 1)
    rest = np.delete(faces, hit, axis=0)
    want = raw_forward(pts, x, dev_t(rest)[None], 1)
    assert bits(alone) == bits(want[0]) and bits(fused[3]) == bits(want[0])
    assert bool(torch.isfinite(alone).all()) and not bits(alone) == bits(good.winding)
    assert same(fused[:3], pf) and bool((pf[1] >= 0).all())
    assert not bool((pf[1] == hit[0]).any()) and not bool((pf[1] == hit[1]).any())
    kept = torch.from_numpy(np.delete(np.arange(f), hit)).cuda()                # the rows of ``rest`` in ``faces``
    assert torch.equal(fused[1], kept[want[1][1]]) and bits(fused[0]) == bits(want[1][0])
    assert bits(fused[2]) == bits(want[1][2])
    again = mesh_winding.point_mesh_signed_distance(pts, x, corners)           # the next call
    assert same(again, good)


def test_shared_and_per_element_topology_give_the_same_bits(cuda):
    v, faces = winding_mesh("cage")
    assert faces.ndim == 2
    x, tf = dev_t(v.astype(F32)), dev_t(faces)
    shared = MeshCorners.from_faces(tf, 162)
    copies = MeshCorners.from_faces(tf[None].repeat(3, 1, 1), 162)
    assert shared.batch == 1 and copies.batch == 3
    results = []
    for corners in (shared, copies):
        p, y = dev_t(sided_cloud("cage", 3)[0].astype(F32), True), x.clone().requires_grad_(True)
        out = mesh_winding.point_mesh_signed_distance(p, y, corners)
        grads = torch.autograd.grad(out.signed.sum(), (p, y))
        results.append(list(out) + list(grads) + [mesh_winding.mesh_winding_number(p, y, corners)])
    for a, b in zip(*results):
        assert bits(a) == bits(b)
    assert same(results[0][:5], hip_signed("cage", 3))


def test_empty_problems(cuda):
    x, corners = device_mesh("cage")
    pts = dev_t(sided_cloud("cage", 1)[0].astype(F32), True)
    y = x.clone().requires_grad_(True)
    none = torch.zeros(0, 63, 3, device="cuda"), torch.zeros(0, 162, 3, device="cuda")                       # B = 0
    assert mesh_winding.mesh_winding_number(*none, corners).shape == (0, 63)
    out = mesh_winding.point_mesh_signed_distance(*none, corners)
    assert out.signed.shape == (0, 63) and out.bary.shape == (0, 63, 3) and out.face.dtype == torch.int64
    nothing = torch.zeros(3, 0, 3, device="cuda", requires_grad=True)                                        # P = 0
    out = mesh_winding.point_mesh_signed_distance(nothing, y, corners)
    assert out.signed.shape == (3, 0) and out.winding.shape == (3, 0) and out.signed.is_cuda
    g_p, g_x = torch.autograd.grad(out.signed.sum(), (nothing, y))
    assert g_p.shape == (3, 0, 3) and bool((g_x == 0).all())
    assert mesh_winding.points_inside_mesh(nothing, y, corners).shape == (3, 0)
    empty = MeshCorners.from_faces(torch.zeros(0, 3, dtype=torch.int64, device="cuda"), 162)                 # F = 0
    bare = MeshCorners(torch.zeros(1, 0, 3, dtype=torch.int64, device="cuda"),                              # N = 0
                       torch.zeros(1, 1, dtype=torch.int32, device="cuda"),
                       torch.zeros(1, 0, dtype=torch.int32, device="cuda"),
                       torch.zeros(1, 0, 2, dtype=torch.int32, device="cuda"), 0)
    for vertices, topology in ((y, empty), (torch.zeros(3, 0, 3, device="cuda", requires_grad=True), bare)):
        w = mesh_winding.mesh_winding_number(pts, vertices, topology)
        assert w.shape == (3, 63) and w.is_cuda and bool((w == 0).all())
        assert not bool(mesh_winding.points_inside_mesh(pts, vertices, topology).any())
        out = mesh_winding.point_mesh_signed_distance(pts, vertices, topology)
        assert bool((out.winding == 0).all()) and bool((out.face == -1).all())
        assert bool(torch.isnan(out.signed).all()) and bool(torch.isnan(out.dist).all()) and bool(torch.isnan(out.bary).all())
        g_p, g_x = torch.autograd.grad(out.signed.sum(), (pts, vertices))
        assert bool((g_p == 0).all()) and bool((g_x == 0).all())
    lib = _lib.lib()
    assert lib.pp_mesh_winding_forward_f32(*(None,) * 3, 2, 0, 5, None) == 0                # PP_OK, nothing launched
    assert lib.pp_mesh_signed_distance_forward_f32(*(None,) * 6, 2, 5, 0, None) == 0
    assert lib.pp_mesh_winding_forward_f32(*(None,) * 3, 2, -1, 5, None) != 0
    assert lib.pp_mesh_signed_distance_forward_f32(*(None,) * 6, 2, 5, 2 ** 30, None) != 0


@pytest.mark.parametrize("name", ["cage", "two_topologies"])
def test_every_run_gives_the_same_bits(cuda, name):
    def run():
        out, got, _ = signed_gradients(name)
        x, corners = device_mesh(name)
        alone = mesh_winding.mesh_winding_number(dev_t(cloud(name, 3).astype(F32)), x, corners)
        return [bits(t) for t in list(out) + list(got) + [alone]]

    first = run()
    for _ in range(2):
        assert run() == first
    with deterministic():
        assert run() == first


def test_a_nan_point_is_nan_and_outside(cuda):
    x, corners = device_mesh("gc_cube")
    pts = dev_t(np.array([[[0, 0, 0], [np.nan, 0, 0], [3, 0, 0], [0, np.nan, 0]]], F32), True)
    out = mesh_winding.point_mesh_signed_distance(pts, x, corners)
    assert abs(float(out.winding[0, 0]) - 1) <= 16 * EPS32 and abs(float(out.winding[0, 2])) <= 16 * EPS32
    assert bool(torch.isnan(out.winding[0, [1, 3]]).all())
    assert mesh_winding.points_inside_mesh(pts, x, corners).tolist() == [[True, False, False, False]]
    assert out.face[0].tolist()[1::2] == [-1, -1] and out.signed[0, [0, 2]].tolist() == [-1.0, 2.0]
    assert bool(torch.isnan(out.signed[0, [1, 3]]).all())
    g_p, = torch.autograd.grad(out.signed[0, [0, 2]].sum(), pts)
    assert bool(torch.isfinite(g_p).all()) and bool((g_p[0, [1, 3]] == 0).all())


def test_steps_are_capturable_and_stream_safe(cuda):
    _, corners = device_mesh("two_topologies")                                # kept: built outside the capture
    v, _ = winding_mesh("two_topologies")
    first = sided_cloud("two_topologies", 2)[0].astype(F32)
    other = (sided_cloud("two_topologies", 2)[0][::-1] * 0.75).astype(F32)
    x = dev_t(v.astype(F32), True)

    def step(p):
        out = mesh_winding.point_mesh_signed_distance(p, x, corners)
        alone = mesh_winding.mesh_winding_number(p, x, corners)
        return list(out) + [alone] + list(torch.autograd.grad((out.signed * out.signed).sum(), (p, x)))

    p = dev_t(first, True)
    step(p)
    eagers = [[t.detach().clone() for t in step(dev_t(values, True))] for values in (other, first)]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = step(dev_t(other, True))
        step(p)                                                            # and the warm-up of the capture below
    torch.cuda.current_stream().wait_stream(side)
    for a, b in zip(got, eagers[0]):
        assert bits(a) == bits(b)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        held = step(p)
    for values, eager in zip((other, first), eagers):                      # replayed twice, with new point values
        with torch.no_grad():
            p.copy_(dev_t(values))
            for t in held:
                t.fill_(7)
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(held, eager):
            assert bits(a) == bits(b)


@pytest.mark.parametrize("name", NAMES)
def test_the_surface_itself_is_finite(cuda, name):
    x, corners = device_mesh(name)
    pts = dev_t(surface_cloud(name).astype(F32), True)
    out = mesh_winding.point_mesh_signed_distance(pts, x, corners)
    assert bool(torch.isfinite(out.winding).all()) and bool(torch.isfinite(out.signed).all())
    assert bits(out.winding) == bits(mesh_winding.mesh_winding_number(pts, x, corners))
    g_p, = torch.autograd.grad(out.signed.sum(), pts)
    assert bool(torch.isfinite(g_p).all())


# --------------------------------------------------------------------------------------------- 4. the API paths
def test_geo_operations_and_model_loss_names_reach_hip(cuda):
    v, faces = winding_mesh("cage")
    x, _ = device_mesh("cage")
    y = x.clone().requires_grad_(True)
    p = dev_t(sided_cloud("cage", 3)[0].astype(F32), True)
    tf = dev_t(faces)
    good = hip_signed("cage", 3)
    out = geo_operations.point_mesh_signed_distance(p, y, tf)
    assert "MeshSignedDistance" in type(out.dist.grad_fn).__name__ and same(out, good)
    assert bits(geo_operations.mesh_winding_number(p, y, tf)) == bits(good.winding)
    inside = geo_operations.points_inside_mesh(p, y, tf)
    assert torch.equal(inside, good.winding > 0.5) and bool(inside.any()) and bool((~inside).any())
    zero = torch.zeros_like(good.dist)
    for side, wrong in (("inside", ~inside), ("outside", inside)):
        values = []
        for keep in (False, True):
            mod = model_loss.MeshEnclosureLoss(side, consistent_topology=keep)
            loss = mod(p, y, tf)
            assert isinstance(mod.E, MeshCorners) and mod.E.faces.is_cuda
            if keep:
                kept = mod.E
                assert torch.equal(mod(p, y), loss) and mod.E is kept
            # margin = 0: the masked dist mean; sqrt(d)^2 is d within 1.5 eps32, and the two sums round on their own
            want = torch.where(wrong, good.dist, zero).mean()
            value = float(loss.detach())
            assert value > 0 and abs(value - float(want)) <= 16 * EPS32 * float(want)
            g_p, g_x = torch.autograd.grad(loss, (p, y))
            assert bool(torch.isfinite(g_p).all()) and bool((g_p[wrong] != 0).any()) and bool((g_p[~wrong] == 0).all())
            assert bool(torch.isfinite(g_x).all()) and bool((g_x != 0).any())
            values.append((g_p, g_x))
        assert bits(values[0][0]) == bits(values[1][0]) and bits(values[0][1]) == bits(values[1][1])


def test_fp64_cuda_input_takes_the_composition(cuda):
    v, faces = winding_mesh("cage")
    x, p = dev_t(v, True), dev_t(sided_cloud("cage", 2)[0], True)
    corners = MeshCorners.from_faces(dev_t(faces), 162)
    out = mesh_winding.point_mesh_signed_distance(p, x, corners)
    assert out.signed.dtype == torch.float64 and out.winding.dtype == torch.float64 and out.signed.is_cuda
    assert "MeshSignedDistance" not in type(out.dist.grad_fn).__name__
    assert float((out.winding.cpu() - winding64("cage", 2)).abs().max()) <= 1e-12
    assert float((mesh_winding.mesh_winding_number(p, x, corners).cpu() - winding64("cage", 2)).abs().max()) <= 1e-12
    g_p, g_x = torch.autograd.grad(out.signed.sum(), (p, x))
    assert bool(torch.isfinite(g_p).all()) and bool((g_x != 0).any())
