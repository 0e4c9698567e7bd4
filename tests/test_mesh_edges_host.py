"""CPU tests (no GPU) of the mesh edge utilities and losses (pytorch_points_amd/mesh_edges.py, network/geo_operations.py
edge_vertex_indices / get_edge_lengths, network/model_loss.py MeshEdgeLengthLoss / MeshStretchLoss /
SimpleMeshRepulsionLoss) through their torch compositions, against numpy restatements of reference
geo_operations.py:562-600 and model_loss.py:166-308.  The mesh generators here also serve tests/test_gpu_mesh_edges.py."""
import numpy as np
import pytest
import torch

from pytorch_points_amd import _lib, mesh_edges, synthetic
from pytorch_points_amd.network import geo_operations, model_loss

REDUCTIONS = ["mean", "max", "sum", "none"]


# ------------------------------------------------------------------------------------------------------- meshes
def grid_mesh(rows, cols):
    """A: a triangulated rows x cols vertex grid -> (vertices (N,3) float32 in the unit square, faces (F,3) int64)"""
    r, c = np.meshgrid(np.arange(rows - 1), np.arange(cols - 1), indexing="ij")
    v00 = (r * cols + c).reshape(-1)
    faces = np.concatenate([np.stack([v00, v00 + 1, v00 + cols], -1), np.stack([v00 + 1, v00 + cols + 1, v00 + cols], -1)])
    y, x = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    vertices = np.stack([x / max(cols - 1, 1), y / max(rows - 1, 1), np.zeros_like(x, float)], -1).reshape(-1, 3)
    return vertices.astype(np.float32), faces.astype(np.int64)


def jittered_grid(rows, cols, seed, batch=1, amount=0.2):
    """(vertices (batch,N,3) float32, faces (F,3)): the grid's own coordinates moved by at most ``amount`` of the grid
    spacing in each direction, so that no edge comes near zero length"""
    v, f = grid_mesh(rows, cols)
    step = 1.0 / (max(rows, cols) - 1)
    u = synthetic.uniform01(seed, (batch, v.shape[0], 3)).reshape(batch, -1, 3)
    return (v[None] + amount * step * (2 * u - 1)).astype(np.float32), f


def fan_mesh(t):
    """B: t triangles round apex 0 over the rim vertices 1..t+1 (an open fan): the apex has t+1 edges"""
    k = np.arange(1, t + 1)
    return np.stack([np.zeros_like(k), k, k + 1], -1).astype(np.int64), t + 2


def tetrahedron():
    """C"""
    return np.array([[0, 1, 2], [0, 3, 1], [1, 3, 2], [0, 2, 3]], np.int64), 4


def soup_mesh(n, f, seed):
    """D: random triples in [0,n) with duplicated faces, both orientations of one face, and repeated vertices"""
    rng = np.random.default_rng(seed)
    faces = rng.integers(0, n, size=(f, 3)).astype(np.int64)
    q = f // 8
    faces[q:2 * q] = faces[:q]                       # the same face again
    faces[2 * q:3 * q] = faces[:q][:, ::-1]          # and in the other orientation
    faces[3 * q:4 * q, 1] = faces[3 * q:4 * q, 0]    # a repeated vertex: an (a,a) edge
    faces[4 * q:4 * q + 3] = faces[4 * q:4 * q + 3, :1]   # all three corners equal
    return faces[rng.permutation(f)], n


def np_unique_edges(faces):
    """the reference's edge_vertex_indices (geo_operations.py:562-583) in numpy"""
    pairs = np.sort(np.stack([faces, faces[:, [1, 2, 0]]], axis=-1), axis=-1)
    return np.unique(pairs.reshape(-1, 2), axis=0)


def np_sqrlen(vertices, edges):
    t = vertices[edges[:, 0]] - vertices[edges[:, 1]]
    return np.sum(t * t, axis=-1)


def two_topology_batch(seed=3):
    """two batch elements over 25 vertices with DIFFERENT edge counts: A 5x5 and D -> (vert1, vert2 (2,25,3) float64,
    faces (2,F,3)); the 5x5 grid's face list is padded with repeats of its first face to the soup's length"""
    v, fa = grid_mesh(5, 5)
    fd, _ = soup_mesh(25, 60, seed)
    fa = np.concatenate([fa, np.repeat(fa[:1], 60 - fa.shape[0], 0)])
    vert1 = synthetic.unit_sphere(seed, 2, 25).astype(np.float64)
    vert1[0] = jittered_grid(5, 5, seed)[0][0]
    vert2 = vert1 + 0.05 * synthetic.unit_sphere(seed + 1, 2, 25)
    return vert1, vert2, np.stack([fa, fd])


# ------------------------------------------------------------------------------------- 1. edge_vertex_indices
CASES = {"grid_7x9": lambda: grid_mesh(7, 9)[1], "tetrahedron": lambda: tetrahedron()[0],
         "soup": lambda: soup_mesh(50, 200, 1)[0]}


@pytest.mark.parametrize("name", sorted(CASES))
def test_edge_vertex_indices_composition(name):
    faces = CASES[name]()
    want = np_unique_edges(faces)
    got = geo_operations.edge_vertex_indices(torch.from_numpy(faces))
    assert isinstance(got, torch.Tensor) and got.dtype == torch.int64
    assert np.array_equal(got.numpy(), want)
    as_numpy = geo_operations.edge_vertex_indices(faces)
    assert isinstance(as_numpy, np.ndarray) and np.array_equal(as_numpy, want)
    topo = mesh_edges.MeshEdges.from_faces(torch.from_numpy(faces), int(faces.max()) + 1)
    assert topo.batch == 1 and topo.capacity == 3 * faces.shape[0] and topo.counts_host == (want.shape[0],)
    assert topo.counts.tolist() == [want.shape[0]]
    assert np.array_equal(topo.edge_list(0).numpy(), want)
    assert bool((topo.edges[0, want.shape[0]:] == -1).all())


def test_soup_keeps_self_edges():
    faces, _ = soup_mesh(50, 200, 1)
    edges = geo_operations.edge_vertex_indices(torch.from_numpy(faces)).numpy()
    assert (edges[:, 0] == edges[:, 1]).any() and (edges[:, 0] <= edges[:, 1]).all()


# ----------------------------------------------------------------------------------------- 2. get_edge_lengths
def test_get_edge_lengths_returns_squares():
    v = synthetic.unit_sphere(2, 1, 63)[0].astype(np.float64)
    edges = np_unique_edges(grid_mesh(7, 9)[1])
    got = geo_operations.get_edge_lengths(torch.from_numpy(v), torch.from_numpy(edges))
    assert got.dtype == torch.float64 and got.shape == (edges.shape[0],)
    np.testing.assert_allclose(got.numpy(), np_sqrlen(v, edges), rtol=1e-14, atol=0)
    # two vertices 0.5 apart: 0.25, not 0.5
    pair = torch.tensor([[0.0, 0.0, 0.0], [0.5, 0.0, 0.0]], dtype=torch.float64)
    assert geo_operations.get_edge_lengths(pair, torch.tensor([[0, 1]])).tolist() == [0.25]
    # columns beyond the first two are ignored (the reference's (E,4) edge_points)
    wide = torch.from_numpy(np.concatenate([edges, edges[::-1]], 1))
    assert torch.equal(geo_operations.get_edge_lengths(torch.from_numpy(v), wide), got)


def test_sqrlen_composition_masks_padding_and_shares_a_topology():
    vert1, _, faces = two_topology_batch()
    topo = mesh_edges.MeshEdges.from_faces(torch.from_numpy(faces), 25)
    out = mesh_edges.mesh_edge_sqrlen(torch.from_numpy(vert1), topo)
    assert out.shape == (2, 180) and len(set(topo.counts_host)) == 2
    for b in range(2):
        edges = np_unique_edges(faces[b])
        assert topo.count(b) == edges.shape[0]
        np.testing.assert_allclose(out[b, :topo.count(b)].numpy(), np_sqrlen(vert1[b], edges), rtol=1e-14, atol=0)
        assert bool((out[b, topo.count(b):] == 0).all())
    shared = mesh_edges.MeshEdges.from_faces(torch.from_numpy(faces[:1]).expand(2, -1, -1), 25)
    assert shared.batch == 1
    both = mesh_edges.mesh_edge_sqrlen(torch.from_numpy(vert1), shared)
    assert torch.equal(both[0], out[0])
    np.testing.assert_allclose(both[1, :shared.count(1)].numpy(), np_sqrlen(vert1[1], np_unique_edges(faces[0])),
                               rtol=1e-14, atol=0)
    # the padding passes no gradient, and no NaN
    x = torch.from_numpy(vert1).requires_grad_(True)
    g, = torch.autograd.grad(mesh_edges.mesh_edge_sqrlen(x, topo).sum(), x)
    assert bool(torch.isfinite(g).all())


# --------------------------------------------------------------------------------------------------- 3. losses
def ref_edge_length_loss(metric, vert1, vert2, faces):
    """model_loss.py:186-209, one batch element at a time"""
    loss = []
    for b in range(vert1.shape[0]):
        edges = torch.from_numpy(np_unique_edges(faces[b]))
        loss.append(metric(geo_operations.get_edge_lengths(vert1[b], edges),
                           geo_operations.get_edge_lengths(vert2[b], edges)))
    return torch.mean(torch.stack(loss))


def ref_reduce(per_element, reduction):
    """model_loss.py:253-264 and :294-306"""
    loss = []
    for x in per_element:
        if reduction in ("mean", "none"):
            loss.append(x.mean())
        elif reduction == "max":
            loss.append(x.max())
        elif reduction == "sum":
            loss.append(x.sum())
        else:
            raise NotImplementedError
    loss = torch.stack(loss)
    return loss if reduction == "none" else loss.mean()


def ref_stretch_loss(reduction, vert1, vert2, faces):
    per = []
    for b in range(vert1.shape[0]):
        edges = torch.from_numpy(np_unique_edges(faces[b]))
        sq1 = geo_operations.get_edge_lengths(vert1[b], edges)
        sq2 = geo_operations.get_edge_lengths(vert2[b], edges)
        per.append(torch.max(sq2 / sq1 - 1, torch.zeros_like(sq1)))
    return ref_reduce(per, reduction)


def ref_repulsion_loss(threshold, reduction, verts, edges):
    per = []
    for b in range(verts.shape[0]):
        sq = geo_operations.get_edge_lengths(verts[b], edges)
        tmp = 1 / (sq + 1e-6)
        per.append(torch.where(sq < threshold * threshold, tmp, torch.zeros_like(tmp)))
    return ref_reduce(per, reduction)


def clean_two_topology_batch():
    """the two-topology batch without (a,a) edges in the reference mesh's soup (their zero length would put inf / NaN
    into the stretch): the soup's repeated-vertex faces are replaced by ordinary ones"""
    vert1, vert2, faces = two_topology_batch()
    soup = faces[1]
    rng = np.random.default_rng(9)
    for f in range(soup.shape[0]):
        while len(set(soup[f])) < 3:
            soup[f] = rng.integers(0, 25, 3)
    return vert1, vert2, faces


def _assert_loss_and_grads(got_fn, ref_fn, tensors):
    xs = [torch.from_numpy(t).requires_grad_(True) for t in tensors]
    ys = [torch.from_numpy(t).requires_grad_(True) for t in tensors]
    got, want = got_fn(*xs), ref_fn(*ys)
    assert got.shape == want.shape
    torch.testing.assert_close(got, want, rtol=1e-12, atol=1e-12)
    for a, b in zip(torch.autograd.grad(got.sum(), xs), torch.autograd.grad(want.sum(), ys)):
        torch.testing.assert_close(a, b, rtol=1e-10, atol=1e-12)


@pytest.mark.parametrize("metric", [torch.nn.L1Loss(), torch.nn.MSELoss()], ids=["l1", "mse"])
def test_mesh_edge_length_loss(metric):
    vert1, vert2, faces = two_topology_batch()
    tf = torch.from_numpy(faces)
    _assert_loss_and_grads(lambda a, b: model_loss.MeshEdgeLengthLoss(metric)(a, b, tf),
                           lambda a, b: ref_edge_length_loss(metric, a, b, faces), (vert1, vert2))
    ev = model_loss.MeshEdgeLengthLoss.getEV(tf, 25)
    assert len(ev) == 2 and all(e.dtype == torch.int64 for e in ev)
    for b in range(2):
        assert np.array_equal(ev[b].numpy(), np_unique_edges(faces[b]))


@pytest.mark.parametrize("reduction", REDUCTIONS)
def test_mesh_stretch_loss(reduction):
    vert1, vert2, faces = clean_two_topology_batch()
    tf = torch.from_numpy(faces)
    mod = model_loss.MeshStretchLoss(reduction)
    _assert_loss_and_grads(lambda a, b: mod(a, b, tf), lambda a, b: ref_stretch_loss(reduction, a, b, faces),
                           (vert1, vert2))
    out = mod(torch.from_numpy(vert1), torch.from_numpy(vert2), tf)
    assert out.shape == ((2,) if reduction == "none" else ())
    assert float(out.sum()) > 0


@pytest.mark.parametrize("reduction", REDUCTIONS)
def test_simple_mesh_repulsion_loss(reduction):
    vert1, _, faces = two_topology_batch()
    edges = torch.from_numpy(np.concatenate([np_unique_edges(faces[0]), np_unique_edges(faces[1])])[::-1].copy())
    threshold = 0.9
    sq = np_sqrlen(vert1[1], edges.numpy())
    assert 0 < int((sq < threshold ** 2).sum()) < sq.shape[0]        # the threshold cuts through the edges
    mod = model_loss.SimpleMeshRepulsionLoss(threshold, edges, reduction)
    _assert_loss_and_grads(lambda a: mod(a), lambda a: ref_repulsion_loss(threshold, reduction, a, edges), (vert1,))
    assert mod(torch.from_numpy(vert1)).shape == ((2,) if reduction == "none" else ())


def test_unknown_reduction_raises():
    vert1, vert2, faces = two_topology_batch()
    a, b, tf = torch.from_numpy(vert1), torch.from_numpy(vert2), torch.from_numpy(faces)
    with pytest.raises(NotImplementedError):
        model_loss.MeshStretchLoss("median")(a, b, tf)
    with pytest.raises(NotImplementedError):
        model_loss.SimpleMeshRepulsionLoss(0.5, torch.tensor([[0, 1]]), "median")(a)


def test_repulsion_compares_the_squared_length_with_the_squared_threshold():
    """an edge of length 0.5 and threshold 0.6: counted through its squared length, 0.25 < 0.36, as 1 / (0.25 + 1e-6);
    with threshold 0.4 it is not (0.25 >= 0.16), although 0.25 < 0.4"""
    verts = torch.tensor([[[0.0, 0.0, 0.0], [0.5, 0.0, 0.0]]], dtype=torch.float64)
    edges = torch.tensor([[0, 1]])
    got = model_loss.SimpleMeshRepulsionLoss(0.6, edges, "sum")(verts)
    assert float(got) == 1 / (0.25 + 1e-6)
    assert float(model_loss.SimpleMeshRepulsionLoss(0.4, edges, "sum")(verts)) == 0.0


def test_stretch_uses_squared_lengths_without_epsilon():
    v1 = torch.tensor([[[0.0, 0, 0], [1.0, 0, 0], [0.0, 1, 0]]], dtype=torch.float64)
    v2 = v1 * 2
    face = torch.tensor([[[0, 1, 2]]])
    # every edge doubles: squared ratio 4, stretch 3
    assert float(model_loss.MeshStretchLoss("max")(v1, v2, face)) == 3.0
    # a zero-length reference edge is not masked: the division's inf comes through
    flat = v1.clone()
    flat[0, 1] = flat[0, 0]
    assert float(model_loss.MeshStretchLoss("max")(flat, v2, face)) == float("inf")


def test_consistent_topology_keeps_the_first_faces():
    vert1, vert2, faces = clean_two_topology_batch()
    a, b = torch.from_numpy(vert1), torch.from_numpy(vert2)
    tf = torch.from_numpy(faces)
    other = torch.from_numpy(np.ascontiguousarray(faces[::-1]))
    for make in (lambda keep: model_loss.MeshEdgeLengthLoss(torch.nn.L1Loss(), consistent_topology=keep),
                 lambda keep: model_loss.MeshStretchLoss("sum", consistent_topology=keep)):
        kept, fresh = make(True), make(False)
        first = kept(a, b, tf)
        assert torch.equal(first, fresh(a, b, tf))
        topo = kept.E
        assert torch.equal(kept(a, b, other), first) and kept.E is topo         # the other faces are not looked at
        assert torch.equal(kept(a, b), first)                                   # nor are faces needed any more
        assert not torch.equal(fresh(a, b, other), first)
    with pytest.raises(AssertionError, match="Face is required"):
        model_loss.MeshStretchLoss()(a, b)


def test_repulsion_forward_edges_override_and_cache():
    vert1, _, faces = two_topology_batch()
    x = torch.from_numpy(vert1)
    e0 = torch.from_numpy(np_unique_edges(faces[0]))
    e1 = torch.from_numpy(np_unique_edges(faces[1]))
    mod = model_loss.SimpleMeshRepulsionLoss(10.0, e0, "sum")
    base = mod(x)
    torch.testing.assert_close(base, ref_repulsion_loss(10.0, "sum", x, e0), rtol=1e-12, atol=0)
    over = mod(x, e1)
    torch.testing.assert_close(over, ref_repulsion_loss(10.0, "sum", x, e1), rtol=1e-12, atol=0)
    assert not torch.equal(base, over)
    topo = mod._built[3]
    mod(x, e1)
    assert mod._built[3] is topo                      # the same tensor, unmodified: the topology is reused
    e1[0, 1] = e1[1, 1]                               # modified in place: rebuilt
    torch.testing.assert_close(mod(x, e1), ref_repulsion_loss(10.0, "sum", x, e1), rtol=1e-12, atol=0)
    assert mod._built[3] is not topo
    with pytest.raises(AssertionError):
        model_loss.SimpleMeshRepulsionLoss(1.0)(x)


# --------------------------------------------------------------------------------------------------- 4. errors
def test_shape_and_dtype_errors():
    vert1, vert2, faces = two_topology_batch()
    a, b, tf = torch.from_numpy(vert1), torch.from_numpy(vert2), torch.from_numpy(faces)
    quads = torch.zeros(2, 4, 4, dtype=torch.int64)
    with pytest.raises(NotImplementedError):
        mesh_edges.MeshEdges.from_faces(quads, 25)
    with pytest.raises(NotImplementedError):
        model_loss.MeshEdgeLengthLoss(torch.nn.L1Loss())(a, b, quads)
    with pytest.raises(NotImplementedError):
        geo_operations.edge_vertex_indices(quads[0])
    with pytest.raises(TypeError):
        mesh_edges.MeshEdges.from_faces(tf.double(), 25)
    with pytest.raises(TypeError):
        model_loss.MeshStretchLoss()(a, b, tf.float())
    with pytest.raises(TypeError):
        geo_operations.edge_vertex_indices(tf[0].float())
    with pytest.raises(TypeError):
        mesh_edges.MeshEdges.from_edges(torch.zeros(4, 2), 25)
    with pytest.raises(AssertionError):
        model_loss.MeshEdgeLengthLoss(torch.nn.L1Loss())(a, b[:, :20], tf)
    with pytest.raises(AssertionError):
        model_loss.MeshStretchLoss()(a, b[:1], tf)
    with pytest.raises(ValueError):
        mesh_edges.mesh_edge_sqrlen(a[:, :20], mesh_edges.MeshEdges.from_faces(tf, 25))
    with pytest.raises(ValueError):
        mesh_edges.mesh_edge_sqrlen(a[0], mesh_edges.MeshEdges.from_faces(tf, 25))
    bad = tf.clone()
    bad[1, 3, 2] = -1
    with pytest.raises(IndexError, match="batch element 1"):
        mesh_edges.MeshEdges.from_faces(bad, 25)
    with pytest.raises(IndexError, match="batch element 0"):
        mesh_edges.MeshEdges.from_edges(torch.tensor([[0, 25]]), 25)


# ------------------------------------------------------------------------------------------------ 5. workspace
def bucket_scratch_bytes(b, n, items, owner):
    """csrc/bucket_lists.h's layout restated (also serves tests/test_knn_edges_host.py): 256-byte-aligned regions, a
    counter slot, cursor and start of one word per vertex, the long list, the entries and, on request, their owners"""
    def align(x):
        return (x + 255) // 256 * 256
    words = [b * n, b * n, b * items // 256 + 1, b * items] + ([b * items] if owner else [])
    return 256 + sum(align(4 * w) for w in words)


def test_workspace_bytes_follow_the_layout():
    """pure host arithmetic, callable without a GPU"""
    size = _lib.lib().pp_mesh_edges_workspace_bytes
    assert bucket_scratch_bytes(1, 257, 9000, True) == 75264
    # B*N a multiple of 64 and not, items on both sides of a multiple of 256, several batch elements
    for b, n, items in [(1, 257, 9000), (1, 64, 256), (3, 70, 255), (2, 4, 12), (5, 1, 3), (4, 5000, 30000)]:
        assert size(b, n, items) == bucket_scratch_bytes(b, n, items, True), (b, n, items)
    for b, n, items in [(0, 10, 30), (2, 0, 30), (2, 10, 0), (-1, 10, 30), (2, -1, 30), (2, 10, -3),
                        (2, 10, 1 << 30), (3, 1 << 30, 30)]:       # B*items or B*N beyond 2^31 - 1
        assert size(b, n, items) == 0, (b, n, items)
    assert size(1, 10, (1 << 31) - 1) == bucket_scratch_bytes(1, 10, (1 << 31) - 1, True)


def test_drop_in_names_resolve():
    import pytorch_points_amd
    pytorch_points_amd.install_as_pytorch_points()
    from pytorch_points.network.geo_operations import edge_vertex_indices, get_edge_lengths  # noqa: F401
    from pytorch_points.network.model_loss import MeshEdgeLengthLoss, MeshStretchLoss, SimpleMeshRepulsionLoss  # noqa: F401
    assert MeshStretchLoss is model_loss.MeshStretchLoss
