"""GPU tests of the mesh surface sampling (csrc/mesh_sample.hip through pytorch_points_amd/mesh_sample.py): the face
choice against the CPU's fp64 CDF, points and weights against the fp32 CPU composition to the bit, gradients against
the fp64 CPU composition within a bound measured on the fp32 CPU composition, run-to-run identity, a face list far
beyond a workgroup, faces without area and vertices without faces, indices out of range handed straight to the entry
points, empty problems, graph capture and a side stream, the geo_operations names and SampledMeshChamferLoss."""
import contextlib
import functools

import numpy as np
import pytest
import torch

from pytorch_points_amd import _lib, mesh_normals, mesh_sample, synthetic
from pytorch_points_amd.mesh_laplacian import MeshCorners
from pytorch_points_amd.network import geo_operations, model_loss
from test_mesh_sample_host import MESHES, SIZES, brute_nndistance, corners_of, mesh, np_faces, uniforms

pytestmark = pytest.mark.gpu

F32 = np.float32
EPS32 = 2.0 ** -23
KINDS = ["g_points", "g_normals", "both"]


def dev_t(a, grad=False):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda").requires_grad_(grad)


def bits(t):
    return t.detach().cpu().contiguous().numpy().tobytes()


@functools.lru_cache(maxsize=None)
def device_mesh(name):
    v, faces = mesh(name)
    return dev_t(v.astype(F32)), MeshCorners.from_faces(dev_t(faces), v.shape[1])


@functools.lru_cache(maxsize=None)
def hip_samples(name, k):
    """HIP's ``(points, face, bary, normals)`` for SIZES[k] samples of ``mesh(name)``, computed once"""
    x, corners = device_mesh(name)
    u = dev_t(uniforms(100 + k, x.shape[0], SIZES[k]))
    return mesh_sample.sample_points_from_meshes(x, corners, u=u, return_normals=True)


# ------------------------------------------------------------------------------------------------- 1. the faces
@pytest.mark.parametrize("name", MESHES)
def test_face_choice_is_exact(cuda, name):
    """HIP's areas, read back, give the CPU's fp64 CDF; no target lies within 2 F 2^-53 cdf[F-1] of a CDF value (the
    seeds are chosen so), and then the faces are the CPU's on every sample"""
    x, corners = device_mesh(name)
    areas = mesh_normals.mesh_face_normals(x, corners)[1]
    for k, s in enumerate(SIZES):
        u1 = uniforms(100 + k, x.shape[0], s)[..., 0]
        want, clear = np_faces(areas.cpu().numpy(), u1)
        assert clear, (name, s)
        got = hip_samples(name, k).face
        assert got.dtype == torch.int64 and got.shape == (x.shape[0], s)
        assert np.array_equal(got.cpu().numpy(), want), (name, s)
        assert torch.equal(mesh_sample.mesh_sample_faces(areas, dev_t(u1)), got)


# ------------------------------------------------------------------------------ 2. the points and the weights
@pytest.mark.parametrize("name", MESHES)
def test_points_and_weights_equal_the_fp32_cpu_composition_to_the_bit(cuda, name):
    v, faces = mesh(name)
    x, corners = device_mesh(name)
    host_x, host = torch.from_numpy(v.astype(F32)), corners_of(faces, v.shape[1])
    face_normals = mesh_normals.mesh_face_normals(x, corners)[0]
    for k, s in enumerate(SIZES):
        got = hip_samples(name, k)
        face = got.face.cpu()
        bary = mesh_sample.bary_composition(torch.from_numpy(uniforms(100 + k, v.shape[0], s)))
        assert bits(got.bary) == bits(bary), (name, s)
        want = mesh_sample.sample_composition(host_x, host, face=face, bary=bary)[0]
        assert bits(got.points) == bits(want), (name, s)
        again = mesh_sample.mesh_interpolate(x, corners, got.face, got.bary)
        assert again.is_cuda and bits(again) == bits(want), (name, s)
        rows = got.face + torch.arange(v.shape[0], device="cuda")[:, None] * corners.n_faces
        assert bits(got.normals) == bits(face_normals.reshape(-1, 3)[rows.reshape(-1)])


# ---------------------------------------------------------------------------------------------- 3. the gradients
@functools.lru_cache(maxsize=None)
def incoming(name, k):
    """g_points and g_normals (B,S,3), exact in fp32"""
    v, _ = mesh(name)
    rng = np.random.default_rng(15)
    return tuple(rng.uniform(-1, 1, size=(v.shape[0], SIZES[k], 3)).astype(F32).astype(np.float64) for _ in range(2))


def composition_gradients(name, k, face, bary, dtype):
    """the gradients of KINDS from the CPU composition in ``dtype``, on the samples ``(face, bary)``, as float64"""
    v, faces = mesh(name)
    x = torch.from_numpy(v).to(dtype).requires_grad_(True)
    g_p, g_n = (torch.from_numpy(g).to(dtype) for g in incoming(name, k))
    points, _, _, normals = mesh_sample.sample_composition(x, corners_of(faces, v.shape[1]), face=face,
                                                           bary=bary.to(dtype), return_normals=True)
    out = [torch.autograd.grad(points, x, g_p, retain_graph=True)[0],
           torch.autograd.grad(normals, x, g_n, retain_graph=True)[0],
           torch.autograd.grad((points, normals), x, (g_p, g_n))[0]]
    return [t.double().numpy() for t in out]


def hip_gradients(name, k):
    x, corners = device_mesh(name)
    x = x.clone().requires_grad_(True)
    u = dev_t(uniforms(100 + k, x.shape[0], SIZES[k]))
    g_p, g_n = (dev_t(g.astype(F32)) for g in incoming(name, k))
    out = mesh_sample.sample_points_from_meshes(x, corners, u=u, return_normals=True)
    assert "MeshSamplePoints" in type(out.points.grad_fn).__name__
    assert not out.face.requires_grad and not out.bary.requires_grad
    grads = [torch.autograd.grad(out.points, x, g_p, retain_graph=True)[0],
             torch.autograd.grad(out.normals, x, g_n, retain_graph=True)[0],
             torch.autograd.grad((out.points, out.normals), x, (g_p, g_n))[0]]
    return out, grads


def gradient_error(got, ref):
    """the largest absolute error over the largest |gradient| of the reference"""
    assert got.shape == ref.shape and np.isfinite(got).all()
    return float(np.abs(got - ref).max() / np.abs(ref).max())


# The errors of the fp32 CPU composition against the fp64 one at SIZES[-1] samples, in units of eps32 and in the order
# of KINDS, as measured (printed again by the test below beside HIP's).  A figure below 4 stands as 4: a correctly
# rounded chain of four operations already errs by half of that, and another CPU's torch build may measure less.
CPU_MEASURED = {
    "cage": [2.28, 1.7, 1.73],
    "grid_40x130": [0.661, 1.57, 1.77],
    "fan_300": [8.2, 2.79, 5.53],
    "two_topologies": [1.6, 1.29, 1.27],
    "soup": [3.22, 1.52, 1.55],
}
CPU_ERROR = {name: [max(figure, 4.0) for figure in row] for name, row in CPU_MEASURED.items()}


@pytest.mark.parametrize("name", MESHES)
def test_gradients_against_the_fp64_composition(cuda, name):
    """g_points alone, g_normals alone and both: HIP against the fp64 CPU composition on HIP's samples is within 4 x
    the pinned error of the fp32 CPU composition on the same samples (never below 4 eps32); DESIGN.md "Mesh surface
    sampling" records the measured figures."""
    k = len(SIZES) - 1
    out, grads = hip_gradients(name, k)
    face, bary = out.face.cpu(), out.bary.cpu()
    ref = composition_gradients(name, k, face, bary, torch.float64)
    cpu32 = composition_gradients(name, k, face, bary, torch.float32)
    failed = []
    for kind, r, c, h, pinned in zip(KINDS, ref, cpu32, grads, CPU_ERROR[name]):
        assert pinned >= 4
        e_cpu, e_hip = gradient_error(c, r), gradient_error(h.double().cpu().numpy(), r)
        bound = 4 * pinned * EPS32
        print("%s, %s: fp32 CPU composition %.3g eps32 (pinned %.3g), HIP %.3g eps32, bound %.3g eps32"
              % (name, kind, e_cpu / EPS32, pinned, e_hip / EPS32, bound / EPS32))
        if not e_hip <= bound:
            failed.append((kind, e_hip / EPS32, bound / EPS32))
    assert not failed, failed


# ------------------------------------------------------------------------------------------- 4. run to run
@contextlib.contextmanager
def deterministic():
    torch.use_deterministic_algorithms(True)
    try:
        yield
    finally:
        torch.use_deterministic_algorithms(False)


@pytest.mark.parametrize("name", ["fan_300", "two_topologies"])
def test_backwards_are_bit_identical_from_run_to_run(cuda, name):
    k = len(SIZES) - 1
    first = [bits(t) for t in hip_gradients(name, k)[1]]
    for _ in range(2):
        assert [bits(t) for t in hip_gradients(name, k)[1]] == first
    with deterministic():
        assert [bits(t) for t in hip_gradients(name, k)[1]] == first


# ------------------------------------------------------------------------------------------ 5. one long list
def test_a_face_list_far_beyond_a_workgroup(cuda):
    """Two triangles with areas in the ratio 1e6 and 20000 samples: nearly every sample is on face 0, a list that a
    whole workgroup sums.  Any fp32 summation order over S terms stays within S eps32 sum|terms| of the exact sum (a
    term's own rounding, one eps32 of it, included)."""
    s = 20000
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [2, 0, 0], [2.001, 0, 0], [2, 0.001, 0]], F32)
    v = np.stack([v, v[:, [1, 2, 0]] * F32(1.5)])
    faces = np.array([[0, 1, 2], [3, 4, 5]])
    x = dev_t(v, True)
    corners = MeshCorners.from_faces(dev_t(faces), 6)
    areas = mesh_normals.mesh_face_normals(x, corners)[1].detach()
    assert float((areas[:, 0] / areas[:, 1] / 1e6 - 1).abs().max()) < 1e-3
    out = mesh_sample.sample_points_from_meshes(x, corners, u=dev_t(uniforms(21, 2, s)))
    assert int((out.face == 0).sum(1).min()) > s - 20
    g = np.random.default_rng(22).uniform(-1, 1, size=(2, s, 3)).astype(F32)
    grad, = torch.autograd.grad(out.points, x, dev_t(g))
    face, bary = out.face.cpu().numpy(), out.bary.double().cpu().numpy()
    want, size = np.zeros((2, 6, 3)), np.zeros((2, 6, 3))
    for b in range(2):
        for c in range(3):
            term = bary[b][:, c, None] * g[b].astype(np.float64)
            np.add.at(want[b], faces[face[b], c], term)
            np.add.at(size[b], faces[face[b], c], np.abs(term))
    assert (np.abs(grad.double().cpu().numpy() - want) <= s * EPS32 * size).all()
    assert bool((grad[:, :3] != 0).all())
    for _ in range(2):
        again, = torch.autograd.grad(mesh_sample.mesh_interpolate(x, corners, out.face, out.bary), x, dev_t(g))
        assert bits(again) == bits(grad)


# ------------------------------------------------------------- 6. faces without area, vertices without faces
def test_faces_without_area_and_vertices_without_faces(cuda):
    v, faces = mesh("soup")
    flat = (faces[:, 0] == faces[:, 1]) | (faces[:, 1] == faces[:, 2]) | (faces[:, 0] == faces[:, 2])
    x, corners = device_mesh("soup")
    x = x.clone().requires_grad_(True)
    u = uniforms(4, 1, 5000)
    u[0, :3, 0] = (0.0, 1 - 2.0 ** -24, 0.5)
    out = mesh_sample.sample_points_from_meshes(x, corners, u=dev_t(u), return_normals=True)
    drawn = np.bincount(out.face[0].cpu().numpy(), minlength=faces.shape[0])
    assert (drawn[flat] == 0).all() and drawn.sum() == 5000
    only_flat = np.ones(v.shape[1], bool)
    only_flat[faces[~flat].reshape(-1)] = False
    lone = torch.from_numpy(only_flat).cuda()
    for outputs in ((out.points,), (out.normals,), (out.points, out.normals)):
        grad, = torch.autograd.grad([t.sum() for t in outputs], x, retain_graph=True)
        assert bool(torch.isfinite(grad).all()) and bool((grad != 0).any())
        assert bool((grad[0][lone] == 0).all())
    # the 19 vertices of the second topology that no face uses
    v2, faces2 = mesh("two_topologies")
    used = np.zeros(99, bool)
    used[faces2[1].reshape(-1)] = True
    idle = torch.from_numpy(~used).cuda()
    assert int(idle.sum()) == 19
    for kind, grad in zip(KINDS, hip_gradients("two_topologies", 2)[1]):
        got = grad[1][idle].cpu().numpy()
        assert (got == 0).all() and not np.signbit(got).any(), kind
        assert bool((grad[1][~idle] != 0).any())


# ---------------------------------------------------------------------------------------- 7. indices out of range
def test_indices_out_of_range_give_nan_and_the_stream_goes_on(cuda):
    """a faces entry of -1 and one of N go straight to the forward, a face of -1 and one of F to the interpolating
    form: NaN in those samples only; in the backward they add nothing, and the next call on the stream is correct"""
    v, faces = mesh("two_topologies")
    n, f, s = 99, faces.shape[1], SIZES[3]
    x, corners = device_mesh("two_topologies")
    u = dev_t(uniforms(103, 2, s))
    good = hip_samples("two_topologies", 3)
    bad = faces.copy()
    bad[0, 7, 1], bad[1, 11, 2] = -1, n
    tf = dev_t(bad)
    hit = torch.zeros(2, s, dtype=torch.bool, device="cuda")
    hit[0], hit[1] = good.face[0] == 7, good.face[1] == 11
    assert bool(hit[0].any()) and bool(hit[1].any())
    face_normals, areas = mesh_normals.mesh_face_normals(x, corners)
    cdf = mesh_sample._cdf(areas)
    face = torch.empty(2, s, dtype=torch.int64, device="cuda")
    bary, points, normals = (torch.empty(2, s, 3, device="cuda") for _ in range(3))
    lib = _lib.lib()
    with _lib.on_device(x.device) as stream:
        _lib.check(lib.pp_mesh_sample_forward_f32(
            _lib.ptr(x), _lib.ptr(tf), _lib.ptr(cdf), _lib.ptr(u), 3, None, None, _lib.ptr(face_normals),
            _lib.ptr(face), _lib.ptr(bary), _lib.ptr(points), _lib.ptr(normals), 2, n, f, s, 0, stream), "forward")
    assert torch.equal(face, good.face) and torch.equal(bary, good.bary)
    for got, want in ((points, good.points), (normals, good.normals)):
        assert bool(torch.isnan(got[hit]).all()) and torch.equal(got[~hit], want[~hit])
    # the interpolating form, with two faces out of range as well
    picked = good.face.clone()
    picked[0, 3], picked[1, 5] = -1, f
    miss = hit.clone()
    miss[0, 3] = miss[1, 5] = True
    with _lib.on_device(x.device) as stream:
        _lib.check(lib.pp_mesh_sample_forward_f32(
            _lib.ptr(x), _lib.ptr(tf), None, None, 0, _lib.ptr(picked), _lib.ptr(good.bary), None, None, None,
            _lib.ptr(points), None, 2, n, f, s, 0, stream), "interpolate")
    assert bool(torch.isnan(points[miss]).all()) and torch.equal(points[~miss], good.points[~miss])
    # the backward: the lists are those of the faces in range
    g = dev_t(np.random.default_rng(23).uniform(-1, 1, size=(2, s, 3)).astype(F32))
    hand = MeshCorners(tf, corners.start, corners.codes, corners.nbr, n)
    y = x.clone().requires_grad_(True)
    out = mesh_sample.mesh_interpolate(y, hand, picked, good.bary)
    assert bool(torch.isnan(out[miss]).all()) and torch.equal(out[~miss], good.points[~miss])
    grad, = torch.autograd.grad(out, y, g)
    assert bool(torch.isfinite(grad).all()) and bool((grad != 0).any())
    masked = torch.where(miss[..., None], torch.zeros_like(g), g)
    want, = torch.autograd.grad(mesh_sample.mesh_interpolate(y, corners, good.face, good.bary), y, masked)
    assert torch.equal(grad, want)
    again = mesh_sample.sample_points_from_meshes(x, corners, u=u, return_normals=True)          # the next call
    assert all(torch.equal(a, b) for a, b in zip(again, good))


# ------------------------------------------------------------------------------------------------------ 8. empty
def test_empty_problems(cuda):
    x, corners = device_mesh("cage")
    none = MeshCorners.from_faces(torch.zeros(0, 3, dtype=torch.int64, device="cuda"), 162)
    x0 = torch.zeros(0, 162, 3, device="cuda", requires_grad=True)
    out = mesh_sample.sample_points_from_meshes(x0, corners, 7, return_normals=True)
    assert out.points.shape == (0, 7, 3) and out.face.shape == (0, 7) and out.normals.shape == (0, 7, 3)
    assert torch.autograd.grad(out.points.sum() + out.normals.sum(), x0)[0].shape == (0, 162, 3)
    y = x.clone().requires_grad_(True)
    out = mesh_sample.sample_points_from_meshes(y, corners, 0)
    assert out.points.shape == (3, 0, 3) and out.face.shape == (3, 0) and out.bary.shape == (3, 0, 3)
    assert out.points.is_cuda and out.face.dtype == torch.int64
    assert bool((torch.autograd.grad(out.points.sum(), y)[0] == 0).all())
    out = mesh_sample.sample_points_from_meshes(y, none, 5, return_normals=True)
    assert out.points.shape == (3, 5, 3) and bool((out.face == -1).all())
    assert all(bool(torch.isnan(t).all()) for t in (out.points, out.bary, out.normals))
    assert bool((torch.autograd.grad(out.points.sum(), y)[0] == 0).all())
    empty = mesh_sample.mesh_interpolate(y, corners, torch.zeros(3, 0, dtype=torch.int64, device="cuda"),
                                         torch.zeros(3, 0, 3, device="cuda"))
    assert empty.shape == (3, 0, 3)
    assert mesh_sample.mesh_sample_faces(torch.zeros(0, 4, device="cuda"), torch.zeros(0, 9, device="cuda")).shape == (0, 9)
    assert bool((mesh_sample.mesh_sample_faces(torch.zeros(2, 0, device="cuda"), torch.zeros(2, 9, device="cuda")) == -1).all())
    lib = _lib.lib()
    assert lib.pp_mesh_sample_cdf_f32(None, None, 0, 5, None) == 0                      # PP_OK, nothing launched
    for b, n, f, s in ((0, 5, 5, 5), (2, 5, 0, 5), (2, 5, 5, 0)):
        assert lib.pp_mesh_sample_forward_f32(*(None,) * 4, 3, *(None,) * 7, b, n, f, s, 0, None) == 0
        assert lib.pp_mesh_sample_backward_f32(*(None,) * 11, b, n, f, s, 0, None, 0, None) == 0
    assert lib.pp_mesh_sample_cdf_f32(None, None, 2, -1, None) != 0
    assert lib.pp_mesh_sample_forward_f32(*(None,) * 4, 3, *(None,) * 7, 2, 5, 5, -1, 0, None) != 0
    assert lib.pp_mesh_sample_backward_f32(*(None,) * 11, 2, -1, 5, 5, 0, None, 0, None) != 0


# ------------------------------------------------------------------------------- 9. capture and a side stream
def test_steps_are_capturable_and_stream_safe(cuda):
    v, faces = mesh("two_topologies")
    other = np.ascontiguousarray(v[::-1]).astype(F32)
    _, corners = device_mesh("two_topologies")                                # kept: built outside the capture
    u = dev_t(uniforms(102, 2, SIZES[2]))
    g_p, g_n = (dev_t(g.astype(F32)) for g in incoming("two_topologies", 2))

    def step(a):
        out = mesh_sample.sample_points_from_meshes(a, corners, u=u, return_normals=True)
        moved = mesh_sample.mesh_interpolate(a, corners, out.face, out.bary)
        return list(out) + [moved, torch.autograd.grad((out.points, out.normals), a, (g_p, g_n))[0],
                            torch.autograd.grad(moved, a, g_p)[0]]

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
        assert bits(a) == bits(b)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        held = step(x)
    with torch.no_grad():
        x.copy_(dev_t(other))
    for _ in range(2):
        with torch.no_grad():
            for t in held:
                t.fill_(7)
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(held, eager):
            assert bits(a) == bits(b)


# --------------------------------------------------------------------------------------------- 10. the API paths
def test_geo_operations_names_with_faces_and_with_kept_corners(cuda):
    v, faces = mesh("two_topologies")
    x, corners = device_mesh("two_topologies")
    tf = dev_t(faces)
    u = dev_t(uniforms(31, 2, 1000))
    built = geo_operations.sample_points_from_meshes(x, tf, u=u, return_normals=True)
    kept = geo_operations.sample_points_from_meshes(x, corners, 1000, u=u, return_normals=True)
    assert built._fields == ("points", "face", "bary", "normals")
    for a, b in zip(built, kept):
        assert a.is_cuda and bits(a) == bits(b)
    drawn = geo_operations.sample_points_from_meshes(x, tf, 65, generator=torch.Generator("cuda").manual_seed(3))
    same = geo_operations.sample_points_from_meshes(
        x, corners, u=torch.rand((2, 65, 3), device="cuda", generator=torch.Generator("cuda").manual_seed(3)))
    assert drawn._fields == ("points", "face", "bary") and all(bits(a) == bits(b) for a, b in zip(drawn, same))
    shared = MeshCorners.from_faces(tf[0], 99)                                # one topology for the batch
    one = geo_operations.sample_points_from_meshes(x, shared, u=u, return_normals=True)
    assert shared.batch == 1 and all(bits(a[0]) == bits(b[0]) for a, b in zip(one, kept))
    assert bits(geo_operations.mesh_interpolate(x, shared, one.face, one.bary)) == bits(one.points)


def test_fp64_cuda_input_takes_the_composition(cuda):
    v, faces = mesh("cage")
    x = dev_t(v, True)
    corners = MeshCorners.from_faces(dev_t(faces), 162)
    u = uniforms(32, 3, 65)
    out = mesh_sample.sample_points_from_meshes(x, corners, u=dev_t(u), return_normals=True)
    assert out.points.dtype == torch.float64 and out.points.is_cuda
    assert "MeshSamplePoints" not in type(out.points.grad_fn).__name__
    want = mesh_sample.sample_composition(torch.from_numpy(v), corners_of(faces, 162), u=torch.from_numpy(u),
                                          return_normals=True)
    assert torch.equal(out.face.cpu(), want[1])
    assert float((out.points.detach().cpu() - want[0]).abs().max()) <= 1e-14
    assert float((out.normals.detach().cpu() - want[3]).abs().max()) <= 1e-12
    grad, = torch.autograd.grad(out.points.sum() + out.normals.sum(), x)
    assert bool(torch.isfinite(grad).all()) and bool((grad != 0).any())
    moved = mesh_sample.mesh_interpolate(x, corners, out.face, out.bary)
    assert "MeshSamplePoints" not in type(moved.grad_fn).__name__ and torch.equal(moved, out.points)


def test_sampled_mesh_chamfer_loss(cuda):
    v, faces = mesh("two_topologies")
    x = dev_t(v.astype(F32), True)
    tf = dev_t(faces)
    cloud = synthetic.unit_sphere(9, 2, 700)
    target = dev_t(cloud)
    u = uniforms(33, 2, 1000)
    values = []
    for keep in (False, True):
        mod = model_loss.SampledMeshChamferLoss(1000, consistent_topology=keep)
        loss = mod(x, tf, target, u=dev_t(u))
        if keep:
            kept = mod.E
            assert torch.equal(mod(x, None, target, u=dev_t(u)), loss) and mod.E is kept and kept.faces.is_cuda
        grad, = torch.autograd.grad(loss, x)
        assert bool(torch.isfinite(grad).all()) and bool((grad != 0).any())
        values.append((loss.detach(), grad))
    assert torch.equal(values[0][0], values[1][0])
    assert float((values[0][1] - values[1][1]).abs().max()) <= 64 * EPS32 * float(values[1][1].abs().max())
    points = mesh_sample.sample_composition(torch.from_numpy(v), corners_of(faces, 99), u=torch.from_numpy(u))[0]
    d1, d2, _, _ = brute_nndistance(points, torch.from_numpy(cloud).double())
    host = float(d1.mean() + d2.mean())
    assert abs(float(values[0][0]) - host) <= 1e-4 * host
    drawn = model_loss.SampledMeshChamferLoss(63)(x, tf, target)                   # its own random numbers
    assert drawn.shape == () and bool(torch.isfinite(drawn))
