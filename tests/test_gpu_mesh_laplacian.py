"""GPU tests of the mesh Laplacians (the corner, cotangent and apply kernels of csrc/mesh_edges.hip through
pytorch_points_amd/mesh_laplacian.py) and of the modules and losses over them: the corner incidence bit for bit against
numpy, the out-of-range contract, the cotangent kernel against the fp64 composition, both applies, forward and backward,
bit for bit against a sequential numpy fp32 loop over the sorted slices, the operators and losses against the fp64 CPU
compositions, graph capture and a side stream."""
import contextlib
import ctypes
import functools

import numpy as np
import pytest
import torch

from pytorch_points_amd import _lib, mesh_laplacian, synthetic
from pytorch_points_amd.network import geo_operations, model_loss
from test_mesh_edges_host import fan_mesh, grid_mesh, jittered_grid, soup_mesh
from test_mesh_laplacian_host import quad_grid, with_isolated_vertex
from topology_fuzz import np_apply, np_corners

pytestmark = pytest.mark.gpu

F32 = np.float32


def dev_t(a, grad=False):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda").requires_grad_(grad)


@functools.lru_cache(maxsize=None)
def mesh(name):
    """(faces (F,L) int64, n_vertices)"""
    if name.startswith("grid_"):
        rows, cols = (int(x) for x in name[5:].split("x"))
        return grid_mesh(rows, cols)[1], rows * cols
    if name.startswith("fan_"):
        return fan_mesh(int(name[4:]))
    if name == "soup":
        return soup_mesh(257, 3000, 7)
    if name == "quads":
        return quad_grid(9, 31)
    if name == "isolated":
        return with_isolated_vertex()
    raise KeyError(name)


def two_topologies():
    """grid 9x11 and a soup over the same 99 vertices, 160 faces each"""
    fa = grid_mesh(9, 11)[1]
    return np.stack([fa, soup_mesh(99, fa.shape[0], 5)[0]])


def assert_corners(corners, b, faces, n):
    start, codes, nbr = np_corners(faces, n)
    assert corners.start.dtype == corners.codes.dtype == corners.nbr.dtype == torch.int32
    assert np.array_equal(corners.start[b].cpu().numpy(), start)
    assert np.array_equal(corners.codes[b].cpu().numpy(), codes)
    assert np.array_equal(corners.nbr[b].cpu().numpy(), nbr)
    assert corners.faces.dtype == torch.int64 and np.array_equal(corners.faces[b].cpu().numpy(), faces)


def corner_bytes(corners):
    return tuple(t.cpu().numpy().tobytes() for t in (corners.start, corners.codes, corners.nbr))


# --------------------------------------------------------------------------------------- 1. corner incidence
@pytest.mark.parametrize("name", ["grid_3x3", "grid_33x32", "grid_33x63", "fan_255", "fan_256", "fan_257", "fan_700",
                                  "soup", "quads", "isolated"])
def test_corner_incidence_bit_equal(cuda, name):
    faces, n = mesh(name)
    tf = dev_t(faces)
    builds = [mesh_laplacian.MeshCorners.from_faces(tf, n) for _ in range(3)]
    corners = builds[0]
    assert corners.batch == 1 and corners.degree == faces.shape[1]
    assert corners.start.shape == (1, n + 1) and corners.codes.shape == (1, faces.size)
    assert corners.nbr.shape == (1, faces.size, 2)
    assert_corners(corners, 0, faces, n)
    if name.startswith("fan_"):
        assert int(corners.start[0, 1]) == int(name[4:])               # the apex's slice: one corner per triangle
    assert corner_bytes(builds[0]) == corner_bytes(builds[1]) == corner_bytes(builds[2])


def test_corner_incidence_batch_view_and_int32(cuda):
    faces = two_topologies()
    corners = mesh_laplacian.MeshCorners.from_faces(dev_t(faces), 99)
    assert corners.batch == 2
    for b in range(2):
        assert_corners(corners, b, faces[b], 99)
    grid, n = mesh("grid_33x32")
    view = mesh_laplacian.MeshCorners.from_faces(dev_t(grid)[None].expand(4, -1, -1), n)   # builds once
    assert view.batch == 1
    assert_corners(view, 0, grid, n)
    assert_corners(mesh_laplacian.MeshCorners.from_faces(dev_t(grid.astype(np.int32)), n), 0, grid, n)
    assert_corners(mesh_laplacian.MeshCorners.from_faces(dev_t(faces.astype(np.int32)), 99), 1, faces[1], 99)


def test_out_of_range_index_raises_and_the_stream_goes_on(cuda):
    faces = two_topologies()
    for value in (99, -1):
        bad = faces.copy()
        bad[1, 17, 1] = value
        with pytest.raises(IndexError, match="batch element 1"):
            mesh_laplacian.MeshCorners.from_faces(dev_t(bad), 99)
        corners = mesh_laplacian.MeshCorners.from_faces(dev_t(faces), 99)   # the next call on the same stream
        for b in range(2):
            assert_corners(corners, b, faces[b], 99)
        with pytest.raises(IndexError, match="batch element 0"):
            geo_operations.UniformLaplacian()(dev_t(synthetic.unit_sphere(1, 2, 99)), dev_t(bad[::-1]))


def corner_lists(faces, n):
    """pp_mesh_corner_incidence itself on ``faces`` (Bt,F,L) over ``n`` vertices, whatever the flags say: (start, codes,
    nbr, flags) as numpy; the outputs are handed over filled with -7"""
    tf = dev_t(faces)
    bt, f, deg = faces.shape
    out = [torch.full(shape, -7, dtype=torch.int32, device="cuda")
           for shape in ((bt, n + 1), (bt, deg * f), (bt, deg * f, 2), (bt,))]
    nbytes = int(_lib.lib().pp_mesh_edges_workspace_bytes(bt, n, deg * f))
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    with _lib.on_device(tf.device) as stream:
        _lib.check(_lib.lib().pp_mesh_corner_incidence(_lib.ptr(tf), *(_lib.ptr(t) for t in out), bt, f, deg, n,
                                                       _lib.ptr(ws), ctypes.c_size_t(nbytes), stream), "corner lists")
    return tuple(t.cpu().numpy() for t in out)


@pytest.mark.parametrize("deg", [3, 4])
def test_corner_lists_of_the_smallest_batch(cuda, deg):
    """Bt=2, N=5, F=3: the lists byte for byte; then an index N in element 1 only: its flag alone, element 0 intact"""
    faces = np.random.default_rng(60 + deg).integers(0, 5, size=(2, 3, deg)).astype(np.int64)
    start, codes, nbr, flags = corner_lists(faces, 5)
    assert not flags.any()
    for b in range(2):
        for got, want in zip((start[b], codes[b], nbr[b]), np_corners(faces[b], 5)):
            assert got.tobytes() == want.tobytes()
    bad = faces.copy()
    bad[1, 1, 1] = 5
    start, codes, nbr, flags = corner_lists(bad, 5)
    assert flags[0] == 0 and flags[1] != 0
    for got, want in zip((start[0], codes[0], nbr[0]), np_corners(faces[0], 5)):
        assert got.tobytes() == want.tobytes()


def test_corner_lists_without_faces_and_without_vertices(cuda):
    start, _, _, flags = corner_lists(np.zeros((2, 0, 3), np.int64), 5)
    assert start.shape == (2, 6) and not start.any() and not flags.any()
    start, _, _, flags = corner_lists(np.zeros((2, 1, 3), np.int64), 0)          # every corner is out of range
    assert start.shape == (2, 1) and not start.any() and flags.all()


# ----------------------------------------------------------------------------------------------- 2. cotangent
def measure(got, ref):
    """the largest absolute error over the largest absolute reference"""
    return float(np.abs(got - ref).max(initial=0.0)) / max(float(np.abs(ref).max(initial=0.0)), 1e-30)


def test_cotangent_kernel(cuda):
    """against the fp64 CPU composition: at most 4x the figure of the fp32 CPU composition, floor 1e-6 (the rule of
    DESIGN.md "k-NN edge operators").  Heron's formula in fp32 sets the figure, not the kernel."""
    v, faces = jittered_grid(20, 20, 31, batch=2)
    faces = np.concatenate([faces, [[3, 3, 10], [5, 5, 5]]])           # without area: exactly +0
    tf = torch.from_numpy(faces)
    ref = mesh_laplacian.cotangent_composition(torch.from_numpy(v).double(), tf).numpy()
    cpu32 = mesh_laplacian.cotangent_composition(torch.from_numpy(v), tf).numpy()
    got = geo_operations.cotangent(dev_t(v), dev_t(faces)[None].expand(2, -1, -1))
    assert got.dtype == torch.float32 and got.shape == ref.shape and not got.requires_grad
    got = got.cpu().numpy()
    err, base = measure(got, ref), measure(cpu32, ref)
    bound = max(4 * base, 1e-6)
    same = np.array_equal(got, cpu32)
    print("cotangent 20x20: error %.3g, fp32 CPU composition %.3g, bound %.3g, bit-identical to it: %s"
          % (err, base, bound, same))
    assert np.isfinite(got).all() and err <= bound
    assert (got[:, -2:] == 0).all() and not np.signbit(got[:, -2:]).any()
    # under no_grad a vertex tensor that requires a gradient still takes the kernel; with a gradient the composition
    x = dev_t(v, True)
    with torch.no_grad():
        assert np.array_equal(geo_operations.cotangent(x, dev_t(faces)).cpu().numpy(), got)
    with_grad = geo_operations.cotangent(x, dev_t(faces))
    assert with_grad.requires_grad and measure(with_grad.detach().cpu().numpy(), ref) <= bound
    # a face with an index outside [0, N) gives NaN and the stream goes on
    bad = faces.copy()
    bad[7, 2] = 400
    out = geo_operations.cotangent(dev_t(v), dev_t(bad)).cpu().numpy()
    assert np.isnan(out[:, 7]).all() and np.array_equal(np.delete(out, 7, 1), np.delete(got, 7, 1))


# ------------------------------------------------------------------------------------------------ 3. applies
def np_apply_batch(x, faces, n, weights, mode):
    out = []
    for b in range(x.shape[0]):
        start, codes, nbr = np_corners(faces if faces.ndim == 2 else faces[b], n)
        out.append(np_apply(x[b], start, nbr, codes, None if weights is None else weights[b], mode))
    return np.stack(out)


@contextlib.contextmanager
def deterministic():
    torch.use_deterministic_algorithms(True)
    try:
        yield
    finally:
        torch.use_deterministic_algorithms(False)


def check_applies(faces, n, batch, seed, cot=True):
    """forward and backward of both operators, bit for bit, twice, and under deterministic algorithms"""
    rng = np.random.default_rng(seed)
    x = synthetic.unit_sphere(seed, batch, n)
    g = rng.uniform(-1, 1, size=x.shape).astype(F32)
    n_faces = faces.shape[-2]
    weights = rng.uniform(-0.5, 2.0, size=(batch, n_faces, 3)).astype(F32)
    corners = mesh_laplacian.MeshCorners.from_faces(dev_t(faces), n)
    assert corners.batch == (1 if faces.ndim == 2 else faces.shape[0])
    cases = [("uniform", lambda t: mesh_laplacian.mesh_uniform_laplacian(t, corners), None, 0, 1)]
    if cot:
        tw = dev_t(weights)
        cases.append(("cot", lambda t: mesh_laplacian.mesh_cot_laplacian(t, corners, tw), weights, 2, 2))
    for what, op, w, fwd_mode, bwd_mode in cases:
        def run():
            t = dev_t(x, True)
            out = op(t)
            grad, = torch.autograd.grad(out, t, dev_t(g))
            return out.detach().cpu().numpy(), grad.cpu().numpy()

        out, grad = run()
        assert out.dtype == F32 and out.shape == x.shape
        assert np.array_equal(out, np_apply_batch(x, faces, n, w, fwd_mode)), what
        assert np.array_equal(grad, np_apply_batch(g, faces, n, w, bwd_mode)), what
        again = run()
        assert out.tobytes() == again[0].tobytes() and grad.tobytes() == again[1].tobytes()
        with deterministic():
            again = run()
        assert out.tobytes() == again[0].tobytes() and grad.tobytes() == again[1].tobytes()
    return corners


@pytest.mark.parametrize("name", ["fan_700", "soup", "grid_33x32"])
def test_applies_bit_equal_to_the_sequential_loop(cuda, name):
    faces, n = mesh(name)
    check_applies(faces, n, 1, 41)


def test_uniform_apply_on_quads(cuda):
    faces, n = mesh("quads")
    check_applies(faces, n, 2, 42, cot=False)


def test_applies_with_an_isolated_vertex(cuda):
    faces, n = mesh("isolated")
    corners = check_applies(faces, n, 2, 43)
    x = dev_t(synthetic.unit_sphere(43, 2, n), True)
    for out in (mesh_laplacian.mesh_uniform_laplacian(x, corners),
                mesh_laplacian.mesh_cot_laplacian(x, corners, torch.ones(2, 4, 3, device="cuda"))):
        tail = out[:, 4:].detach().cpu().numpy()
        assert (tail == 0).all() and not np.signbit(tail).any()
        grad, = torch.autograd.grad(out.sum(), x)
        assert bool(torch.isfinite(grad).all()) and bool((grad[:, 4:] == 0).all())


def test_applies_share_a_topology_across_the_batch(cuda):
    faces, n = mesh("grid_33x32")
    check_applies(faces, n, 3, 44)


def test_applies_over_a_batch_of_two_topologies(cuda):
    check_applies(two_topologies(), 99, 2, 45)


def test_apply_without_faces(cuda):
    corners = mesh_laplacian.MeshCorners.from_faces(torch.zeros(0, 3, dtype=torch.int64, device="cuda"), 5)
    x = dev_t(synthetic.unit_sphere(46, 2, 5), True)
    out = mesh_laplacian.mesh_uniform_laplacian(x, corners)
    assert bool((out == 0).all()) and bool((torch.autograd.grad(out.sum(), x)[0] == 0).all())
    assert bool((mesh_laplacian.mesh_cot_laplacian(x, corners, torch.zeros(2, 0, 3, device="cuda")) == 0).all())


# ------------------------------------------------------------------------------ 4. operators and losses
@functools.lru_cache(maxsize=None)
def loss_inputs():
    """(vert1, vert2 (3,400,3) float32, faces (3,F,3)): jittered 20x20 grids, lifted off their plane so that the
    Laplacians have three ordinary components"""
    vert1, f = jittered_grid(20, 20, 51, batch=3)
    vert2 = jittered_grid(20, 20, 52, batch=3)[0]
    bump = 0.05 * synthetic.unit_sphere(53, 3, 400)
    return (vert1 + bump).astype(F32), (vert2 - bump).astype(F32), np.stack([f, f, f])


def operator_cases():
    l1, mse = torch.nn.L1Loss, torch.nn.MSELoss
    cases = [("UniformLaplacian", lambda: geo_operations.UniformLaplacian(), 1),
             ("CotLaplacian", lambda: geo_operations.CotLaplacian(), 1),
             ("smoothness", lambda: (lambda v, f: model_loss.UniformLaplacianSmoothnessLoss(400, f, None)(v)), 1)]
    for metric in (l1, mse):
        for use_cot in (False, True):
            for use_norm in (False, True):
                name = "laplacian_loss_%s%s%s" % (metric.__name__, "_cot" if use_cot else "", "_norm" if use_norm else "")
                cases.append((name, lambda m=metric, c=use_cot, u=use_norm: model_loss.MeshLaplacianLoss(m(), c, u), 2))
    cases.append(("laplacian_loss_consistent", lambda: model_loss.MeshLaplacianLoss(l1(), True, False, True), 2))
    cases.append(("laplacian_loss_mean", lambda: model_loss.MeshLaplacianLoss(l1(), True, True), 0))
    return cases


def run_operator(make, nargs, device, dtype):
    vert1, vert2, faces = loss_inputs()
    xs = [torch.from_numpy(a).to(device=device, dtype=dtype).requires_grad_(True) for a in (vert1, vert2)]
    tf = torch.from_numpy(faces).to(device)
    mod = make()
    if nargs == 2:
        out = mod(xs[0], xs[1], tf)
        if getattr(mod, "consistent_topology", False):       # the second call runs on the kept Laplacian
            out = mod(xs[0], xs[1])
    elif nargs == 1:
        out = mod(xs[0], tf)
    else:
        out = mod(xs[0], None, tf)
    used = xs[:max(nargs, 1)]
    weight = torch.from_numpy(synthetic.normal(54, tuple(out.shape) or (1,))).to(device=device, dtype=dtype).reshape(out.shape)
    grads = torch.autograd.grad((out * weight).sum(), used)
    return [out.detach().double().cpu().numpy()] + [g.double().cpu().numpy() for g in grads]


@pytest.mark.parametrize("name,make,nargs", operator_cases(), ids=[c[0] for c in operator_cases()])
def test_operators_against_the_fp64_composition(cuda, name, make, nargs):
    """value and gradients against the fp64 CPU composition; the bound is the standing rule of DESIGN.md "k-NN edge
    operators": 4x the same figure of the fp32 CPU composition, floor 1e-6"""
    ref = run_operator(make, nargs, "cpu", torch.float64)
    cpu32 = run_operator(make, nargs, "cpu", torch.float32)
    assert all(np.isfinite(a).all() for a in ref + cpu32)
    got = run_operator(make, nargs, "cuda", torch.float32)
    for what, g, c, r in zip(("value", "grad vert1", "grad vert2"), got, cpu32, ref):
        assert g.shape == r.shape and np.isfinite(g).all()
        err, base = measure(g, r), measure(c, r)
        bound = max(4 * base, 1e-6)
        print("%s %s: error %.3g, fp32 CPU composition %.3g, bound %.3g" % (name, what, err, base, bound))
        assert err <= bound, (what, err, bound)


def test_cot_laplacian_reuses_the_weights_of_the_building_vertices(cuda):
    vert1, vert2, faces = loss_inputs()
    tf = dev_t(faces)
    lap = geo_operations.CotLaplacian()
    x1 = dev_t(vert1, True)
    first = lap(x1, tf)
    assert first.requires_grad and isinstance(lap.L.corners, mesh_laplacian.MeshCorners)
    weights = geo_operations.cotangent(dev_t(vert1), tf)
    assert torch.equal(lap.L.weights, weights) and not lap.L.weights.requires_grad
    second = lap(dev_t(vert2))
    assert not second.requires_grad
    assert torch.equal(second, mesh_laplacian.mesh_cot_laplacian(dev_t(vert2), lap.L.corners, weights))
    assert not torch.equal(second, geo_operations.CotLaplacian()(dev_t(vert2), tf))
    uni = geo_operations.UniformLaplacian()
    uni(dev_t(vert1[:1]), tf[:1])                                        # a single-mesh L serves the batch
    assert uni.L.batch == 1 and uni.Lii.shape == (400,) and uni.Lii.is_cuda
    assert torch.equal(uni(dev_t(vert1)), mesh_laplacian.mesh_uniform_laplacian(dev_t(vert1), uni.L))


# ------------------------------------------------------------------------------- 5. capture and a side stream
def test_applies_are_capturable_and_stream_safe(cuda):
    vert1, vert2, faces = loss_inputs()
    corners = mesh_laplacian.MeshCorners.from_faces(dev_t(faces[0]), 400)
    weights = geo_operations.cotangent(dev_t(vert1), dev_t(faces[0]))
    g = dev_t(synthetic.normal(55, vert1.shape))

    def step(x):
        u = mesh_laplacian.mesh_uniform_laplacian(x, corners)
        c = mesh_laplacian.mesh_cot_laplacian(x, corners, weights)
        return (u, c) + torch.autograd.grad((u * g).sum() + (c * g).sum(), x)

    x = dev_t(vert1, True)
    step(x)
    eager = [t.detach().clone() for t in step(dev_t(vert2, True))]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = step(dev_t(vert2, True))
        step(x)                                                          # and the warm-up of the capture below
    torch.cuda.current_stream().wait_stream(side)
    for a, b in zip(got, eager):
        assert torch.equal(a.detach(), b)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        held = step(x)
    with torch.no_grad():
        x.copy_(dev_t(vert2))
    for _ in range(2):
        with torch.no_grad():
            for t in held:
                t.fill_(7.0)
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(held, eager):
            assert torch.equal(a.detach(), b)


@pytest.mark.parametrize("use_cot", [False, True], ids=["uniform", "cot"])
def test_a_loss_step_on_a_kept_topology_reads_nothing_back(cuda, use_cot):
    """a device-to-host copy cannot be captured: a step that captures makes none"""
    vert1, vert2, faces = loss_inputs()
    mod = model_loss.MeshLaplacianLoss(torch.nn.L1Loss(), use_cot=use_cot, use_norm=True, consistent_topology=True)

    def step(a, b):
        loss = mod(a, b)
        return (loss,) + torch.autograd.grad(loss, (a, b))

    x1, x2 = dev_t(vert1, True), dev_t(vert2, True)
    mod(x1, x2, dev_t(faces))                                            # the first call builds
    eager = [t.detach().clone() for t in step(x1, x2)]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(x1, x2)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        held = step(x1, x2)
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(held, eager):
        assert torch.equal(a.detach(), b)
