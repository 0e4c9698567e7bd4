"""GPU tests of the mesh normals (csrc/mesh_normals.hip through pytorch_points_amd/mesh_normals.py): forward and
backward of both operators against the fp64 CPU composition within a bound measured on the fp32 CPU composition,
run-to-run identity, faces without area and vertices without faces, a slice longer than a workgroup, indices out of
range handed straight to the entry points, empty problems, graph capture and a side stream, the geo_operations names
and MeshNormalLoss."""
import contextlib
import functools

import numpy as np
import pytest
import torch

from pytorch_points_amd import _lib, mesh_normals, synthetic
from pytorch_points_amd.mesh_laplacian import MeshCorners
from pytorch_points_amd.network import geo_operations, model_loss
from test_mesh_dihedral_host import folded_grid, jittered_cage, two_topologies, zigzag_fan
from test_mesh_edges_host import soup_mesh
from test_mesh_normals_host import WEIGHTINGS, face_shape_quality, np_vertex_normals

pytestmark = pytest.mark.gpu

F32 = np.float32
EPS32 = 2.0 ** -23
CASES = ["cage", "grid_40x130", "fan_300", "two_topologies"]
METRICS = ["face normals", "areas", "face gradient", "vertex normals, area", "vertex gradient, area",
           "vertex normals, uniform", "vertex gradient, uniform"]


def dev_t(a, grad=False):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda").requires_grad_(grad)


@functools.lru_cache(maxsize=None)
def case(name):
    """The inputs of tests/test_gpu_mesh_dihedral.py's cases: (vertices (B,N,3) float64 that are exact in fp32, faces
    (F,3) or (B,F,3), and the incoming gradients g_n (B,F,3), g_a (B,F), g_v (B,N,3), exact in fp32 too)"""
    if name == "cage":
        faces, v = jittered_cage(12, batch=3)
    elif name == "grid_40x130":
        v, faces = folded_grid(40, 130, 13, batch=3)
    elif name == "fan_300":
        v, faces = zigzag_fan(300, 14, batch=3)
    else:
        v, faces = two_topologies()
    v = v.astype(F32).astype(np.float64)
    rng = np.random.default_rng(15)
    b, n, f = v.shape[0], v.shape[1], faces.shape[-2]
    g = [rng.uniform(-1, 1, size=shape).astype(F32).astype(np.float64) for shape in ((b, f, 3), (b, f), (b, n, 3))]
    return v, faces, g


def run(name, device, dtype):
    """every output and gradient of both operators, in the order of METRICS, as float64 numpy"""
    v, faces, g = case(name)
    corners = MeshCorners.from_faces(torch.from_numpy(faces).to(device), v.shape[1])
    g_n, g_a, g_v = (torch.from_numpy(a).to(device=device, dtype=dtype) for a in g)
    x = torch.from_numpy(v).to(device=device, dtype=dtype).requires_grad_(True)
    normals, areas = mesh_normals.mesh_face_normals(x, corners)
    out = [normals, areas, torch.autograd.grad((normals, areas), x, (g_n, g_a))[0]]
    for w in WEIGHTINGS:
        per_vertex = mesh_normals.mesh_vertex_normals(x, corners, w)
        out += [per_vertex, torch.autograd.grad(per_vertex, x, g_v)[0]]
    return [t.detach().double().cpu().numpy() for t in out]


@functools.lru_cache(maxsize=None)
def references(name):
    """the fp64 and the fp32 CPU composition, computed once"""
    return run(name, "cpu", torch.float64), run(name, "cpu", torch.float32)


def errors(got, ref):
    """per metric: the largest absolute error of the unit normals, the largest relative error of the areas, the
    largest gradient error over the largest |gradient| of the reference"""
    out = []
    for what, a, r in zip(METRICS, got, ref):
        assert a.shape == r.shape and np.isfinite(a).all(), what
        if what == "areas":
            out.append(float(np.max(np.abs(a - r) / r)))
        elif "gradient" in what:
            out.append(float(np.abs(a - r).max() / np.abs(r).max()))
        else:
            out.append(float(np.abs(a - r).max()))
    return out


# The errors of the fp32 CPU composition on the inputs of case(), in units of eps32 and in the order of METRICS, as
# measured (printed again by the test below beside HIP's).  A figure below 4 stands as 4: a correctly rounded chain of
# four operations already errs by half of that, and another CPU's torch build may measure less.
CPU_MEASURED = {
    "cage": [0.979, 1.52, 0.95, 0.915, 1.1, 1.09, 1.72],
    "grid_40x130": [0.841, 1.15, 1.08, 0.953, 1.26, 0.996, 1.3],
    "fan_300": [0.909, 1.18, 2.26, 1.36, 8.32, 1.36, 1.28],
    "two_topologies": [1.23, 1.62, 1.11, 0.955, 0.824, 0.754, 1.16],
}
CPU_ERROR = {name: [max(figure, 4.0) for figure in row] for name, row in CPU_MEASURED.items()}


def assert_nothing_is_left_out(name):
    """every face has 2A / (sum of its squared edges) >= 0.05 and every vertex with corners |S| / sum|c| >= 0.2, for
    both weightings: the comparison below covers every face and every vertex"""
    v, faces, _ = case(name)
    worst_face = worst_vertex = np.inf
    for b in range(v.shape[0]):
        fb = faces if faces.ndim == 2 else faces[b]
        worst_face = min(worst_face, face_shape_quality(v[b], fb).min())
        for w in WEIGHTINGS:
            _, length, size = np_vertex_normals(v[b], fb, w)
            used = size > 0
            worst_vertex = min(worst_vertex, (length[used] / size[used]).min())
    print("%s: the worst face 2A/sum e^2 = %.3f, the worst vertex |S|/sum|c| = %.3f" % (name, worst_face, worst_vertex))
    assert worst_face >= 0.05 and worst_vertex >= 0.2


@pytest.mark.parametrize("name", CASES)
def test_forward_and_backward_against_the_fp64_composition(cuda, name):
    """Every metric of HIP against the fp64 CPU composition is within 4 x the pinned error of the fp32 CPU composition
    on the same inputs (never below 4 eps32); DESIGN.md "Mesh normals" records the measured figures."""
    assert_nothing_is_left_out(name)
    ref, cpu32 = references(name)
    e_cpu, e_hip = errors(cpu32, ref), errors(run(name, "cuda", torch.float32), ref)
    failed = []
    for what, c, h, pinned in zip(METRICS, e_cpu, e_hip, CPU_ERROR[name]):
        assert pinned >= 4
        bound = 4 * pinned * EPS32
        print("%s, %s: fp32 CPU composition %.3g eps32 (pinned %.3g), HIP %.3g eps32, bound %.3g eps32"
              % (name, what, c / EPS32, pinned, h / EPS32, bound / EPS32))
        if not h <= bound:
            failed.append((what, h / EPS32, bound / EPS32))
    assert not failed, failed


# ------------------------------------------------------------------------ determinism and the special inputs
@contextlib.contextmanager
def deterministic():
    torch.use_deterministic_algorithms(True)
    try:
        yield
    finally:
        torch.use_deterministic_algorithms(False)


@pytest.mark.parametrize("name", ["fan_300", "two_topologies"])
def test_backwards_are_bit_identical_from_run_to_run(cuda, name):
    v, faces, g = case(name)
    corners = MeshCorners.from_faces(dev_t(faces), v.shape[1])
    g_n, g_a, g_v = (dev_t(a.astype(F32)) for a in g)

    def backwards():
        x = dev_t(v.astype(F32), True)
        normals, areas = mesh_normals.mesh_face_normals(x, corners)
        grads = [torch.autograd.grad((normals, areas), x, (g_n, g_a), retain_graph=True)[0],
                 torch.autograd.grad(normals, x, g_n, retain_graph=True)[0],          # g_a NULL
                 torch.autograd.grad(areas, x, g_a)[0]]                                # g_n NULL
        for w in WEIGHTINGS:
            grads.append(torch.autograd.grad(mesh_normals.mesh_vertex_normals(x, corners, w), x, g_v)[0])
        return [t.cpu().numpy() for t in grads]

    first = backwards()
    assert all((a != 0).any() and np.isfinite(a).all() for a in first)
    np.testing.assert_allclose(first[1] + first[2], first[0], rtol=0, atol=64 * EPS32 * np.abs(first[0]).max())
    for _ in range(2):
        assert [a.tobytes() for a in backwards()] == [a.tobytes() for a in first]
    with deterministic():
        assert [a.tobytes() for a in backwards()] == [a.tobytes() for a in first]


def test_faces_without_area_and_vertices_without_faces(cuda):
    faces, n = soup_mesh(50, 200, 1)
    flat = (faces[:, 0] == faces[:, 1]) | (faces[:, 1] == faces[:, 2]) | (faces[:, 0] == faces[:, 2])
    v = synthetic.unit_sphere(2, 1, n).astype(F32)
    corners = MeshCorners.from_faces(dev_t(faces), n)
    x = dev_t(v, True)
    normals, areas = mesh_normals.mesh_face_normals(x, corners)
    mask = torch.from_numpy(flat).cuda()
    assert bool((areas[0][mask] == 0).all()) and bool((normals[0][mask] == 0).all())
    assert bool((areas[0][~mask] > 0).all())
    grad, = torch.autograd.grad(normals.sum() + areas.sum(), x)
    assert bool(torch.isfinite(grad).all()) and bool((grad != 0).any())
    host = torch.from_numpy(v).requires_grad_(True)                       # the composition's rule is the same one
    hn, ha = mesh_normals.mesh_face_normals(host, MeshCorners.from_faces(torch.from_numpy(faces), n))
    want, = torch.autograd.grad(hn.sum() + ha.sum(), host)
    assert float((grad.cpu() - want).abs().max()) <= 64 * EPS32 * float(want.abs().max())
    for w in WEIGHTINGS:
        y = dev_t(v, True)
        out = mesh_normals.mesh_vertex_normals(y, corners, w)
        grad, = torch.autograd.grad(out.sum(), y)
        assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(grad).all())
    # the 19 vertices of the second topology that no face uses
    v2, faces2, _ = case("two_topologies")
    used = np.zeros(99, bool)
    used[faces2[1].reshape(-1)] = True
    idle = torch.from_numpy(~used).cuda()
    corners = MeshCorners.from_faces(dev_t(faces2), 99)
    for w in WEIGHTINGS:
        x = dev_t(v2.astype(F32), True)
        out = mesh_normals.mesh_vertex_normals(x, corners, w)
        got = out[1][idle].detach().cpu().numpy()
        assert (got == 0).all() and not np.signbit(got).any()
        grad, = torch.autograd.grad(out.sum() + (out * out).sum(), x)
        assert bool((grad[1][idle] == 0).all()) and bool((grad[1][~idle] != 0).any())
    x = dev_t(v2.astype(F32), True)
    normals, areas = mesh_normals.mesh_face_normals(x, corners)
    grad, = torch.autograd.grad(normals.sum() + areas.sum(), x)
    assert bool((grad[1][idle] == 0).all())


def test_a_slice_longer_than_a_workgroup(cuda):
    """zigzag_fan(8000): the apex has 8000 slots, summed by one lane in slot order.  A sequential fp32 sum of n terms
    errs by at most n eps32 sum|c|, so its unit vector by n eps32 sum|c| / |S| (plus the few eps32 of the terms and of
    the division, which n = 8000 covers)."""
    v, faces = zigzag_fan(8000, 14)
    v = v.astype(F32)
    corners = MeshCorners.from_faces(dev_t(faces), v.shape[1])
    assert int(corners.counts()[0, 0]) == 8000
    for w in WEIGHTINGS:
        got = mesh_normals.mesh_vertex_normals(dev_t(v), corners, w).double().cpu().numpy()
        want, length, size = np_vertex_normals(v[0], faces, w)
        bound = 8000 * EPS32 * size / length
        assert bound[0] < 0.05                                   # the apex's sum does not cancel
        assert (np.abs(got[0] - want).max(-1) <= bound).all(), w
    normals, areas = mesh_normals.mesh_face_normals(dev_t(v), corners)
    assert bool(torch.isfinite(normals).all()) and bool((areas > 0).all())


def test_indices_out_of_range_give_nan_and_the_stream_goes_on(cuda):
    """a face index of -1 and one of N go straight to the face forward, a neighbour of -1 and one of N to the vertex
    forward: NaN in those lanes, every other lane as before, and the next call on the stream is correct"""
    v, faces, _ = case("two_topologies")
    n, f = 99, faces.shape[1]
    x = dev_t(v.astype(F32))
    corners = MeshCorners.from_faces(dev_t(faces), n)
    good_n, good_a = mesh_normals.mesh_face_normals(x, corners)
    bad = faces.copy()
    bad[0, 7, 1], bad[1, 11, 2] = -1, n
    tf = dev_t(bad)
    normals = torch.empty(2, f, 3, device="cuda")
    areas = torch.empty(2, f, device="cuda")
    with _lib.on_device(x.device) as stream:
        _lib.check(_lib.lib().pp_mesh_face_normals_forward_f32(_lib.ptr(x), _lib.ptr(tf), _lib.ptr(normals),
                                                               _lib.ptr(areas), 2, n, f, 0, stream), "face forward")
    hit = torch.zeros(2, f, dtype=torch.bool, device="cuda")
    hit[0, 7] = hit[1, 11] = True
    assert bool(torch.isnan(normals[hit]).all()) and bool(torch.isnan(areas[hit]).all())
    assert torch.equal(normals[~hit], good_n[~hit]) and torch.equal(areas[~hit], good_a[~hit])
    for code, w in enumerate(WEIGHTINGS):
        good = mesh_normals.mesh_vertex_normals(x, corners, w)
        nbr = corners.nbr.clone()
        start = corners.start.cpu().numpy()
        rows = (5, 60)                                           # vertices of batch elements 0 and 1 with corners
        nbr[0, int(start[0, rows[0]]), 0] = -1
        nbr[1, int(start[1, rows[1] + 1]) - 1, 1] = n
        out = torch.empty_like(x)
        with _lib.on_device(x.device) as stream:
            _lib.check(_lib.lib().pp_mesh_vertex_normals_forward_f32(
                _lib.ptr(x), _lib.ptr(corners.start), _lib.ptr(nbr), _lib.ptr(out), 2, n, f, code, 0, stream),
                "vertex forward")
        hit = torch.zeros(2, n, dtype=torch.bool, device="cuda")
        hit[0, rows[0]] = hit[1, rows[1]] = True
        assert bool(torch.isnan(out[hit]).all()) and torch.equal(out[~hit], good[~hit])
        assert torch.equal(mesh_normals.mesh_vertex_normals(x, corners, w), good)          # the next call
    again_n, again_a = mesh_normals.mesh_face_normals(x, corners)
    assert torch.equal(again_n, good_n) and torch.equal(again_a, good_a)


def test_empty_problems(cuda):
    faces = dev_t(case("cage")[1])
    corners = MeshCorners.from_faces(faces, 162)
    none = MeshCorners.from_faces(torch.zeros(0, 3, dtype=torch.int64, device="cuda"), 162)
    x0 = torch.zeros(0, 162, 3, device="cuda", requires_grad=True)
    normals, areas = mesh_normals.mesh_face_normals(x0, corners)
    assert normals.shape == (0, 320, 3) and areas.shape == (0, 320) and normals.is_cuda
    out = mesh_normals.mesh_vertex_normals(x0, corners)
    assert out.shape == (0, 162, 3)
    assert torch.autograd.grad(out.sum() + normals.sum() + areas.sum(), x0)[0].shape == (0, 162, 3)
    x = torch.ones(2, 162, 3, device="cuda", requires_grad=True)
    normals, areas = mesh_normals.mesh_face_normals(x, none)
    assert normals.shape == (2, 0, 3) and areas.shape == (2, 0)
    out = mesh_normals.mesh_vertex_normals(x, none, "uniform")
    assert out.shape == (2, 162, 3) and bool((out == 0).all())
    assert bool((torch.autograd.grad(out.sum() + areas.sum(), x)[0] == 0).all())
    for entry, args in (("pp_mesh_face_normals_forward_f32", (None, None, None, None, 0, 5, 5, 0, None)),
                        ("pp_mesh_vertex_normals_forward_f32", (None, None, None, None, 2, 0, 5, 0, 0, None)),
                        ("pp_mesh_vertex_normals_backward_f32", (None,) * 6 + (2, 5, 0, 1, 0, None))):
        assert getattr(_lib.lib(), entry)(*args) == 0                       # PP_OK, nothing launched
    assert _lib.lib().pp_mesh_vertex_normals_forward_f32(None, None, None, None, 2, 5, 5, 2, 0, None) != 0
    assert _lib.lib().pp_mesh_face_normals_forward_f32(None, None, None, None, 2, -1, 5, 0, None) != 0


# ------------------------------------------------------------------------------- capture and a side stream
def test_steps_are_capturable_and_stream_safe(cuda):
    v, faces, g = case("two_topologies")
    other = np.ascontiguousarray(v[::-1]).astype(F32)
    corners = MeshCorners.from_faces(dev_t(faces), 99)                      # kept: built outside the capture
    g_n, g_a, g_v = (dev_t(a.astype(F32)) for a in g)

    def step(a):
        normals, areas = mesh_normals.mesh_face_normals(a, corners)
        out = [normals, areas, torch.autograd.grad((normals, areas), a, (g_n, g_a))[0]]
        for w in WEIGHTINGS:
            per_vertex = mesh_normals.mesh_vertex_normals(a, corners, w)
            out += [per_vertex, torch.autograd.grad(per_vertex, a, g_v)[0]]
        return out

    x = dev_t(v.astype(F32), True)
    step(x)
    eager = [t.detach().clone() for t in step(dev_t(other, True))]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = step(dev_t(other, True))
        step(x)                                                            # and the warm-up of the capture below
    torch.cuda.current_stream().wait_stream(side)
    for a, b in zip(got, eager):
        assert torch.equal(a.detach(), b)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        held = step(x)
    with torch.no_grad():
        x.copy_(dev_t(other))
    for _ in range(2):
        with torch.no_grad():
            for t in held:
                t.fill_(7.0)
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(held, eager):
            assert torch.equal(a.detach(), b)


# --------------------------------------------------------------------------------------------- the API paths
def test_geo_operations_names_and_the_loss_on_cuda_tensors(cuda):
    v, faces, _ = case("two_topologies")
    x1 = dev_t(v.astype(F32), True)
    x2 = dev_t((v + 0.004 * np.random.default_rng(19).uniform(-1, 1, size=v.shape)).astype(F32), True)
    tf = dev_t(faces)
    corners = MeshCorners.from_faces(tf, 99)
    for a, b in zip(geo_operations.mesh_face_normals(x1, tf), geo_operations.mesh_face_normals(x1, corners)):
        assert a.is_cuda and a.dtype == torch.float32 and torch.equal(a, b)         # built every call | kept
    for w in WEIGHTINGS:
        assert torch.equal(geo_operations.mesh_vertex_normals(x1, tf, w),
                           geo_operations.mesh_vertex_normals(x1, corners, w))
    scaled = geo_operations.normalize_to_same_area(x2, corners, x1, tf)
    areas = [geo_operations.mesh_face_normals(t, corners)[1].sum(-1).detach() for t in (scaled, x2)]
    assert float(((areas[0] - areas[1]).abs() / areas[1]).max()) <= 64 * EPS32
    for use_face in (False, True):
        for w in WEIGHTINGS:
            values = []
            for keep in (False, True):
                mod = model_loss.MeshNormalLoss(torch.nn.MSELoss(), use_face, w, consistent_topology=keep)
                loss = mod(x1, x2, tf)
                if keep:
                    kept = mod.E
                    assert torch.equal(mod(x1, x2), loss) and mod.E is kept and kept.faces.is_cuda
                grads = torch.autograd.grad(loss, (x1, x2))
                assert all(bool(torch.isfinite(t).all()) and bool((t != 0).any()) for t in grads)
                values.append([loss.detach()] + list(grads))
            assert all(torch.equal(a, b) for a, b in zip(*values))
            host = model_loss.MeshNormalLoss(torch.nn.MSELoss(), use_face, w)(
                x1.detach().double().cpu(), x2.detach().double().cpu(), torch.from_numpy(faces))
            assert abs(float(values[0][0]) - float(host)) <= 1e-4 * float(host)


def test_fp64_cuda_input_takes_the_composition(cuda):
    v, faces, _ = case("cage")
    corners = MeshCorners.from_faces(dev_t(faces), 162)
    host = MeshCorners.from_faces(torch.from_numpy(faces), 162)
    x = dev_t(v, True)
    normals, areas = mesh_normals.mesh_face_normals(x, corners)
    assert normals.dtype == torch.float64 and normals.is_cuda
    assert "MeshFaceNormals" not in type(normals.grad_fn).__name__
    want_n, want_a = mesh_normals.face_normals_composition(torch.from_numpy(v), host)
    assert float((normals.detach().cpu() - want_n).abs().max()) <= 1e-14
    assert float(((areas.detach().cpu() - want_a).abs() / want_a).max()) <= 1e-14
    out = mesh_normals.mesh_vertex_normals(x, corners, "uniform")
    want = mesh_normals.vertex_normals_composition(torch.from_numpy(v), host, "uniform")
    assert out.dtype == torch.float64 and float((out.detach().cpu() - want).abs().max()) <= 1e-13
    grad, = torch.autograd.grad(out.sum() + areas.sum(), x)
    assert bool(torch.isfinite(grad).all())
