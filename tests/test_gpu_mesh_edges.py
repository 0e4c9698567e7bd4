"""GPU tests of the mesh edge operators (csrc/mesh_edges.hip through pytorch_points_amd/mesh_edges.py) and of the mesh
losses over them: the unique edges bit for bit against numpy, the out-of-range contract, the forward bit for bit against
knn_edge_lengths, the backward bit for bit against a sequential numpy loop, the incidence lists, the losses against
the fp64 CPU composition, graph capture and a side stream, and the reference-API utilities on CUDA tensors."""
import contextlib
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from pytorch_points_amd import _lib, knn_edges, mesh_edges, synthetic
from pytorch_points_amd.network import geo_operations, model_loss
from test_mesh_edges_host import (REDUCTIONS, fan_mesh, grid_mesh, jittered_grid, np_unique_edges, soup_mesh,
                                  tetrahedron)
from topology_fuzz import np_backward

pytestmark = pytest.mark.gpu

F32 = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gc_ico2.npz")


def dev_t(a, grad=False):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda").requires_grad_(grad)


@functools.lru_cache(maxsize=None)
def mesh(name):
    """(faces (F,3) int64, n_vertices, vertices (N,3) float32)"""
    if name.startswith("grid_"):
        rows, cols = (int(x) for x in name[5:].split("x"))
        v, f = jittered_grid(rows, cols, rows * cols)
        return f, rows * cols, v[0]
    if name.startswith("fan_"):
        f, n = fan_mesh(int(name[4:]))
    elif name == "tetrahedron":
        f, n = tetrahedron()
    elif name == "soup":
        f, n = soup_mesh(257, 3000, 7)
    elif name == "cage":
        z = np.load(GOLDEN)
        return z["faces"][0].astype(np.int64), z["vertices"].shape[1], z["vertices"][0].astype(F32)
    else:
        raise KeyError(name)
    return f, n, synthetic.unit_sphere(n, 1, n)[0]


@functools.lru_cache(maxsize=None)
def unique_of(name):
    return np_unique_edges(mesh(name)[0])


def assert_topology(topo, b, want):
    """batch element b of topo: rows, padding and counts, bit for bit"""
    edges = topo.edges[b].cpu().numpy()
    assert topo.counts_host[b] == want.shape[0] and int(topo.counts[b]) == want.shape[0]
    assert edges.dtype == np.int64 and np.array_equal(edges[:want.shape[0]], want)
    assert (edges[want.shape[0]:] == -1).all()


def two_topologies():
    """grid 9x11 and a soup over the same 99 vertices, 160 faces each: different edge counts"""
    fa = grid_mesh(9, 11)[1]
    fd = soup_mesh(99, fa.shape[0], 5)[0]
    assert np_unique_edges(fa).shape[0] != np_unique_edges(fd).shape[0]
    return np.stack([fa, fd])


# ------------------------------------------------------------------------------------------- 1. unique edges
@pytest.mark.parametrize("name", ["grid_3x3", "grid_40x130", "fan_300", "fan_8000", "soup", "tetrahedron", "cage"])
def test_unique_edges_bit_equal(cuda, name):
    faces, n, _ = mesh(name)
    topo = mesh_edges.MeshEdges.from_faces(dev_t(faces), n)
    assert topo.batch == 1 and topo.edges.shape == (1, 3 * faces.shape[0], 2)
    assert_topology(topo, 0, unique_of(name))


def test_unique_edges_batch_of_two_topologies(cuda):
    faces = two_topologies()
    topo = mesh_edges.MeshEdges.from_faces(dev_t(faces), 99)
    assert topo.batch == 2 and topo.counts_host[0] != topo.counts_host[1]
    for b in range(2):
        assert_topology(topo, b, np_unique_edges(faces[b]))
        assert np.array_equal(topo.edge_list(b).cpu().numpy(), np_unique_edges(faces[b]))


def test_unique_edges_of_an_expanded_view_build_once(cuda):
    faces, n, _ = mesh("grid_40x130")
    topo = mesh_edges.MeshEdges.from_faces(dev_t(faces)[None].expand(4, -1, -1), n)
    assert topo.batch == 1 and topo.count(3) == unique_of("grid_40x130").shape[0]
    assert_topology(topo, 0, unique_of("grid_40x130"))
    # int32 faces are accepted
    assert_topology(mesh_edges.MeshEdges.from_faces(dev_t(faces.astype(np.int32)), n), 0, unique_of("grid_40x130"))


def test_unique_edges_do_not_depend_on_atomic_order(cuda):
    faces, n, _ = mesh("soup")
    tf = dev_t(faces)
    runs = []
    for _ in range(3):
        topo = mesh_edges.MeshEdges.from_faces(tf, n)
        inc_start, inc_entries = topo.incidence()
        total = int(inc_start[0, -1])
        runs.append((topo.edges.cpu().numpy().tobytes(), inc_start.cpu().numpy().tobytes(),
                     inc_entries[0, :total].cpu().numpy().tobytes()))
    assert runs[0] == runs[1] == runs[2]
    assert_topology(topo, 0, unique_of("soup"))


# ------------------------------------------------------------------------------------------- 2. out of range
def test_out_of_range_face_index_raises_and_the_stream_goes_on(cuda):
    faces = two_topologies()
    for value in (99, -1):
        bad = faces.copy()
        bad[1, 17, 1] = value
        with pytest.raises(IndexError, match="batch element 1"):
            mesh_edges.MeshEdges.from_faces(dev_t(bad), 99)
        with pytest.raises(IndexError, match="batch element 1"):
            mesh_edges.MeshEdges.from_edges(dev_t(bad[:, :, :2]), 99)
        topo = mesh_edges.MeshEdges.from_faces(dev_t(faces), 99)          # the next call on the same stream
        for b in range(2):
            assert_topology(topo, b, np_unique_edges(faces[b]))


# ------------------------------------------------------------------------------------------------ 3. forward
def owner_graph(edges, n):
    """idx (N,K): row v lists the other end of every edge whose first end is v, padded with v itself"""
    degree = np.bincount(edges[:, 0], minlength=n)
    k = max(int(degree.max()), 1)
    idx = np.repeat(np.arange(n, dtype=np.int64)[:, None], k, 1)
    slot = np.arange(edges.shape[0]) - np.repeat(np.cumsum(degree) - degree, degree)   # edges are sorted by first end
    idx[edges[:, 0], slot] = edges[:, 1]
    return idx, slot


def knn_squared(points, idx):
    """knn_edge_lengths(..., squared=True), its K <= 128 columns at a time"""
    parts = [knn_edges.knn_edge_lengths(points, idx[:, :, c:c + knn_edges.MAX_K].contiguous(), squared=True)
             for c in range(0, idx.shape[2], knn_edges.MAX_K)]
    return torch.cat(parts, dim=2)


@pytest.mark.parametrize("name", ["grid_40x130", "fan_300", "soup", "cage"])
def test_forward_bit_equal_to_knn_edge_lengths(cuda, name):
    faces, n, v = mesh(name)
    edges = unique_of(name)
    verts = np.stack([v, (v * F32(1.5) + F32(0.25)).astype(F32)])                     # B = 2 over one topology
    topo = mesh_edges.MeshEdges.from_faces(dev_t(faces), n)
    out = mesh_edges.mesh_edge_sqrlen(dev_t(verts), topo).cpu().numpy()
    assert out.shape == (2, 3 * faces.shape[0]) and out.dtype == F32
    idx, slot = owner_graph(edges, n)
    knn = knn_squared(dev_t(verts), dev_t(np.stack([idx, idx]))).cpu().numpy()
    assert np.array_equal(out[:, :edges.shape[0]], knn[:, edges[:, 0], slot])
    assert (out[:, edges.shape[0]:] == 0).all() and not np.signbit(out[:, edges.shape[0]:]).any()
    # three subtractions, one product, two fmas, each within half an ulp of fp32: 8 * 2^-24 of the exact value of
    # the same fp32 inputs
    v64 = verts.astype(np.float64)
    t = v64[:, edges[:, 0]] - v64[:, edges[:, 1]]
    exact = np.sum(t * t, axis=-1)
    rel = np.abs(out[:, :edges.shape[0]] - exact) / np.where(exact == 0, 1.0, exact)
    print("%s: largest relative error of the squared lengths %.3g" % (name, rel.max()))
    assert rel.max() <= 8 * 2.0 ** -24


# ----------------------------------------------------------------------------------------------- 4. backward
@contextlib.contextmanager
def deterministic():
    torch.use_deterministic_algorithms(True)
    try:
        yield
    finally:
        torch.use_deterministic_algorithms(False)


def check_backward(topo, verts, edges_of, seed):
    g = np.random.default_rng(seed).uniform(-1, 1, size=(verts.shape[0], topo.capacity)).astype(F32)
    want = np_backward(verts, edges_of, g)

    def run():
        x = dev_t(verts, True)
        grad, = torch.autograd.grad(mesh_edges.mesh_edge_sqrlen(x, topo), x, dev_t(g))
        return grad.cpu().numpy()

    first = run()
    assert np.array_equal(first, want)
    assert first.tobytes() == run().tobytes()
    with deterministic():
        assert first.tobytes() == run().tobytes()


@pytest.mark.parametrize("name", ["grid_40x130", "fan_8000"])
def test_backward_bit_equal_to_the_sequential_loop(cuda, name):
    faces, n, v = mesh(name)
    topo = mesh_edges.MeshEdges.from_faces(dev_t(faces), n)
    if name == "fan_8000":
        inc_start = topo.incidence()[0].cpu().numpy()
        assert inc_start[0, 1] - inc_start[0, 0] == 8001          # the apex's slice: one entry per rim vertex
    check_backward(topo, v[None], lambda b: unique_of(name), 1)


def test_backward_over_a_user_edge_list(cuda):
    """from_edges on a list that is not unique, not sorted and has self-edges"""
    faces, n, v = mesh("soup")
    rng = np.random.default_rng(2)
    edges = faces[:, :2][rng.permutation(faces.shape[0])]
    assert (edges[:, 0] == edges[:, 1]).any() and np.unique(edges, axis=0).shape[0] < edges.shape[0]
    topo = mesh_edges.MeshEdges.from_edges(dev_t(edges), n)
    assert topo.batch == 1 and topo.capacity == edges.shape[0] and topo.counts_host == (edges.shape[0],)
    check_backward(topo, np.stack([v, v[::-1]]), lambda b: edges, 3)


def test_backward_batch_of_two_topologies(cuda):
    faces = two_topologies()
    topo = mesh_edges.MeshEdges.from_faces(dev_t(faces), 99)
    check_backward(topo, synthetic.unit_sphere(4, 2, 99), lambda b: np_unique_edges(faces[b]), 4)


def test_backward_shared_topology(cuda):
    faces, n, _ = mesh("grid_40x130")
    topo = mesh_edges.MeshEdges.from_faces(dev_t(faces)[None].expand(3, -1, -1), n)
    check_backward(topo, jittered_grid(40, 130, 8, batch=3)[0], lambda b: unique_of("grid_40x130"), 5)


# ---------------------------------------------------------------------------------------------- 5. incidence
def test_incidence_of_a_shuffled_duplicated_edge_list(cuda):
    rng = np.random.default_rng(6)
    n, e = 257, 3000
    edges = rng.integers(0, n, size=(e, 2)).astype(np.int64)
    edges[1000:2000] = edges[:1000]                                 # duplicates
    edges[2000:2050, 1] = edges[2000:2050, 0]                       # self-edges
    edges = edges[rng.permutation(e)]
    topo = mesh_edges.MeshEdges.from_edges(dev_t(edges), n)
    inc_start, inc_entries = (t.cpu().numpy() for t in topo.incidence())
    assert inc_start.shape == (1, n + 1) and inc_entries.shape == (1, 2 * e)
    assert inc_start[0, 0] == 0 and inc_start[0, n] == 2 * e
    flat = edges.reshape(-1)
    for v in range(n):
        got = inc_entries[0, inc_start[0, v]:inc_start[0, v + 1]]
        assert np.array_equal(got, np.flatnonzero(flat == v))       # sorted, and the same multiset (codes are distinct)


@pytest.mark.parametrize("counts", [(0, 4), (2, 3)])
def test_incidence_of_counted_rows(cuda, counts):
    """pp_mesh_edge_incidence itself, Ecap = 4: only the rows e < counts[b] are listed"""
    n, ecap = 5, 4
    edges = np.random.default_rng(7).integers(0, n, size=(2, ecap, 2)).astype(np.int64)
    te, tc = dev_t(edges), dev_t(np.asarray(counts, np.int32))
    inc_start = torch.full((2, n + 1), -7, dtype=torch.int32, device="cuda")
    inc_entries = torch.full((2, 2 * ecap), -7, dtype=torch.int32, device="cuda")
    flags = torch.zeros(2, dtype=torch.int32, device="cuda")
    nbytes = int(_lib.lib().pp_mesh_edges_workspace_bytes(2, n, 2 * ecap))
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    with _lib.on_device(te.device) as stream:
        _lib.check(_lib.lib().pp_mesh_edge_incidence(_lib.ptr(te), _lib.ptr(tc), _lib.ptr(inc_start),
                                                     _lib.ptr(inc_entries), _lib.ptr(flags), 2, ecap, n, _lib.ptr(ws),
                                                     ctypes.c_size_t(nbytes), stream), "edge incidence")
    inc_start, inc_entries = inc_start.cpu().numpy(), inc_entries.cpu().numpy()
    assert not flags.cpu().numpy().any()
    for b in range(2):
        flat = edges[b, :counts[b]].reshape(-1)
        assert inc_start[b, 0] == 0 and inc_start[b, n] == 2 * counts[b]
        for v in range(n):
            got = inc_entries[b, inc_start[b, v]:inc_start[b, v + 1]]
            assert np.array_equal(got, np.flatnonzero(flat == v))


# ------------------------------------------------------------------------------------------------- 6. losses
def loss_cases():
    cases = [("edge_length_l1", lambda: model_loss.MeshEdgeLengthLoss(torch.nn.L1Loss()), 2),
             ("edge_length_mse", lambda: model_loss.MeshEdgeLengthLoss(torch.nn.MSELoss()), 2)]
    cases += [("stretch_" + r, (lambda r=r: model_loss.MeshStretchLoss(r)), 2) for r in REDUCTIONS]
    cases += [("repulsion_" + r, (lambda t, r=r: model_loss.SimpleMeshRepulsionLoss(t, None, r)), 1)
              for r in REDUCTIONS]
    return cases


@functools.lru_cache(maxsize=None)
def loss_inputs(batch_name):
    """(vert1, vert2 (B,N,3) float32, faces (B,F,3)): jittered grids, so that every reference edge is far from zero
    length and the fp32 composition stays finite"""
    if batch_name == "grid_20x20_b3":
        vert1, f = jittered_grid(20, 20, 21, batch=3)
        vert2 = jittered_grid(20, 20, 22, batch=3)[0]
        return vert1, vert2, np.stack([f, f, f])
    # the 9x11 grid and a soup over the same 99 vertices; a soup face with a repeated vertex (a zero-length edge) is
    # replaced by one over three consecutive vertices
    vert1, f = jittered_grid(9, 11, 23, batch=2)
    vert2 = jittered_grid(9, 11, 24, batch=2)[0]
    soup = soup_mesh(99, f.shape[0], 5)[0]
    repeated = (soup[:, 0] == soup[:, 1]) | (soup[:, 1] == soup[:, 2]) | (soup[:, 0] == soup[:, 2])
    soup[repeated] = (soup[repeated, :1] + np.arange(3)) % 99
    assert np_unique_edges(soup).shape[0] != np_unique_edges(f).shape[0]
    return vert1, vert2, np.stack([f, soup])


def measure(got, ref):
    """the largest absolute error over the largest absolute reference"""
    return float(np.abs(got - ref).max(initial=0.0)) / max(float(np.abs(ref).max(initial=0.0)), 1e-30)


THRESHOLD = {"grid_20x20_b3": 0.055, "two_topologies": 0.11}   # cuts through the grid's edges (spacing 1/19, 1/10)


def run_loss(make, nargs, batch_name, device, dtype):
    vert1, vert2, faces = loss_inputs(batch_name)
    xs = [torch.from_numpy(a).to(device=device, dtype=dtype).requires_grad_(True) for a in (vert1, vert2)[:nargs]]
    tf = torch.from_numpy(faces).to(device)
    if nargs == 2:
        loss = make()(*xs, tf)
    else:   # the repulsion's shared edge list: the first element's unique edges
        edges = np_unique_edges(faces[0])
        sq = np.sum((vert1[:, edges[:, 0]] - vert1[:, edges[:, 1]]) ** 2, -1)
        assert 0 < int((sq < THRESHOLD[batch_name] ** 2).sum()) < sq.size
        loss = make(THRESHOLD[batch_name])(xs[0], torch.from_numpy(edges).to(device))
    grads = torch.autograd.grad(loss.sum(), xs)
    return [loss.detach().double().cpu().numpy()] + [g.double().cpu().numpy() for g in grads]


@pytest.mark.parametrize("batch_name", ["grid_20x20_b3", "two_topologies"])
@pytest.mark.parametrize("name,make,nargs", loss_cases(), ids=[c[0] for c in loss_cases()])
def test_losses_against_the_fp64_composition(cuda, name, make, nargs, batch_name):
    """value and gradients against the fp64 CPU composition; the bound is the standing rule of DESIGN.md "k-NN edge
    operators": 4x the same figure of the fp32 CPU composition, floor 1e-6"""
    ref = run_loss(make, nargs, batch_name, "cpu", torch.float64)
    cpu32 = run_loss(make, nargs, batch_name, "cpu", torch.float32)
    assert all(np.isfinite(a).all() for a in ref + cpu32)
    for a, b in zip(cpu32, ref):                   # the inputs keep the fp32 composition itself inside the rule
        assert measure(a, b) <= 1e-5
    got = run_loss(make, nargs, batch_name, "cuda", torch.float32)
    for what, g, c, r in zip(("value", "grad vert1", "grad vert2"), got, cpu32, ref):
        assert g.shape == r.shape and np.isfinite(g).all()
        err, base = measure(g, r), measure(c, r)
        bound = max(4 * base, 1e-6)
        print("%s %s %s: error %.3g, fp32 CPU composition %.3g, bound %.3g" % (name, batch_name, what, err, base, bound))
        assert err <= bound, (what, err, bound)


def test_zero_length_reference_edge(cuda):
    """HIP and the composition agree on where inf / NaN appear; nothing else is asserted"""
    vert1, vert2, faces = (a.copy() for a in loss_inputs("grid_20x20_b3"))
    vert1[1, 21] = vert1[1, 20]                     # one reference edge of length zero
    for reduction in REDUCTIONS:
        outs = []
        for device in ("cpu", "cuda"):
            xs = [torch.from_numpy(a).to(device).requires_grad_(True) for a in (vert1, vert2)]
            loss = model_loss.MeshStretchLoss(reduction)(*xs, torch.from_numpy(faces).to(device))
            grads = torch.autograd.grad(loss.sum(), xs)
            outs.append([t.detach().cpu().numpy() for t in (loss,) + grads])
        for a, b in zip(*outs):
            assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.isinf(a), np.isinf(b))
            assert np.array_equal(np.sign(a[np.isinf(a)]), np.sign(b[np.isinf(b)]))
        assert not np.isfinite(outs[1][0]).all()


# ------------------------------------------------------------------------------- 7. capture and a side stream
def test_step_is_capturable_and_stream_safe(cuda):
    vert1, vert2, faces = loss_inputs("two_topologies")
    other1, other2 = (np.ascontiguousarray(a[::-1]) for a in (vert1, vert2))
    tf = dev_t(faces)
    mod = model_loss.MeshEdgeLengthLoss(torch.nn.L1Loss(), consistent_topology=True)

    def step(a, b):
        loss = mod(a, b, tf)
        return (loss,) + torch.autograd.grad(loss, (a, b))

    x1, x2 = dev_t(vert1, True), dev_t(vert2, True)
    step(x1, x2)                                                           # the warm call: builds the topology
    eager = [t.detach().clone() for t in step(dev_t(other1, True), dev_t(other2, True))]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = step(dev_t(other1, True), dev_t(other2, True))
        step(x1, x2)                                                       # and the warm-up of the capture below
    torch.cuda.current_stream().wait_stream(side)
    for a, b in zip(got, eager):
        assert torch.equal(a.detach(), b)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        held = step(x1, x2)
    with torch.no_grad():
        x1.copy_(dev_t(other1))
        x2.copy_(dev_t(other2))
    for _ in range(2):
        with torch.no_grad():
            for t in held:
                t.fill_(7.0)
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(held, eager):
            assert torch.equal(a.detach(), b)


# ------------------------------------------------------------------------------------ 8. reference utilities
def test_geo_operations_on_cuda_tensors(cuda):
    for name in ("grid_40x130", "soup"):
        faces, n, v = mesh(name)
        edges = geo_operations.edge_vertex_indices(dev_t(faces))
        assert edges.dtype == torch.int64 and np.array_equal(edges.cpu().numpy(), unique_of(name))
        x = dev_t(v, True)
        sq = geo_operations.get_edge_lengths(x, edges)
        topo = mesh_edges.MeshEdges.from_faces(dev_t(faces), n)
        want = mesh_edges.mesh_edge_sqrlen(dev_t(v[None]), topo)[0, :edges.shape[0]]
        assert sq.shape == (edges.shape[0],) and torch.equal(sq.detach(), want)
        g = np.random.default_rng(9).uniform(-1, 1, size=(1, edges.shape[0])).astype(F32)
        grad, = torch.autograd.grad(sq, x, dev_t(g[0]))
        assert np.array_equal(grad.cpu().numpy(), np_backward(v[None], lambda b: unique_of(name), g)[0])
    ints = geo_operations.edge_vertex_indices(dev_t(mesh("soup")[0].astype(np.int32)))
    assert ints.dtype == torch.int32 and np.array_equal(ints.cpu().numpy(), unique_of("soup"))
