"""CPU tests (no GPU) of the mesh Laplacians (pytorch_points_amd/mesh_laplacian.py, network/geo_operations.py
UniformLaplacian / CotLaplacian / cotangent, network/model_loss.py UniformLaplacianSmoothnessLoss / MeshLaplacianLoss)
through their torch compositions, against dense fp64 restatements of the matrices of reference
geo_operations.py:155-346 and of the control flow of model_loss.py:8-71.  The restatements here also serve
tests/test_gpu_mesh_laplacian.py."""
import itertools

import numpy as np
import pytest
import torch

from pytorch_points_amd import mesh_laplacian, synthetic
from pytorch_points_amd.network import geo_operations, model_loss
from test_mesh_edges_host import grid_mesh, jittered_grid, soup_mesh, tetrahedron, two_topology_batch


# ------------------------------------------------------------------------------------------------------- meshes
def quad_grid(rows, cols):
    """faces (F,4) int64 of a rows x cols vertex grid of quadrilaterals, and its vertex count"""
    r, c = np.meshgrid(np.arange(rows - 1), np.arange(cols - 1), indexing="ij")
    v00 = (r * cols + c).reshape(-1)
    return np.stack([v00, v00 + 1, v00 + cols + 1, v00 + cols], -1).astype(np.int64), rows * cols


def with_isolated_vertex():
    """the tetrahedron over 6 vertices: vertices 4 and 5 belong to no face"""
    return tetrahedron()[0], 6


MESHES = {"grid_7x9": lambda: (grid_mesh(7, 9)[1], 63), "soup": lambda: soup_mesh(50, 200, 1),
          "tetrahedron": tetrahedron, "quads_5x6": lambda: quad_grid(5, 6), "isolated": with_isolated_vertex,
          "no_faces": lambda: (np.zeros((0, 3), np.int64), 7)}


def random_vertices(seed, batch, n, dtype=np.float64):
    return synthetic.unit_sphere(seed, batch, n).astype(dtype)


# ------------------------------------------------------------------------------- the reference's matrices, dense
def dense_uniform(faces, n):
    """computeLaplacian of reference :165-185 for one mesh, dense fp64: -(A + A^T) over the half-edges with
    multiplicity (np.add.at), plus the diagonal Lii of its negated row sums -> (L (n,n), Lii (n,))"""
    deg = faces.shape[1]
    row = faces[:, list(range(deg))].reshape(-1)
    col = faces[:, list(range(1, deg)) + [0]].reshape(-1)
    a = np.zeros((n, n))
    np.add.at(a, (row, col), -1.0)
    lap = a.T + a
    lii = -lap.sum(1)
    return lap + np.diag(lii), lii


def np_uniform(vertices, faces, n):
    """reference :196-205: L v / (Lii + 1e-12); vertices (B,n,D), faces (F,L) shared or (B,F,L)"""
    out = []
    for b in range(vertices.shape[0]):
        lap, lii = dense_uniform(faces if faces.ndim == 2 else faces[b], n)
        out.append(lap @ vertices[b] / (lii[:, None] + 1e-12))
    return np.stack(out)


def np_cotangent(vertices, faces):
    """reference :306-346 in numpy, in the dtype of ``vertices`` (B,n,3); faces (F,3) shared or (B,F,3) -> (B,F,3)"""
    out = []
    for b in range(vertices.shape[0]):
        f = faces if faces.ndim == 2 else faces[b]
        v1, v2, v3 = (vertices[b][f[:, c]] for c in range(3))
        l1 = np.sqrt(((v2 - v3) ** 2).sum(1))
        l2 = np.sqrt(((v3 - v1) ** 2).sum(1))
        l3 = np.sqrt(((v1 - v2) ** 2).sum(1))
        sp = (l1 + l2 + l3) * 0.5
        inside = sp * (sp - l1) * (sp - l2) * (sp - l3)
        inside[inside < 0] = 0
        area = 2 * np.sqrt(inside)
        c = np.stack([l2 ** 2 + l3 ** 2 - l1 ** 2, l1 ** 2 + l3 ** 2 - l2 ** 2, l1 ** 2 + l2 ** 2 - l3 ** 2], 1)
        c = c / (area[:, None] + 1e-10) / 4
        c[area == 0] = 0.0
        out.append(c)
    return np.stack(out)


def dense_cot(faces, cot, n):
    """computeLaplacian of reference :227-253 for one mesh, dense fp64: cot (F,3) summed at (rows, cols) =
    (F[:, [1,2,0]], F[:, [2,0,1]]), symmetrised, minus the diagonal of the row sums"""
    lap = np.zeros((n, n))
    np.add.at(lap, (faces[:, [1, 2, 0]].reshape(-1), faces[:, [2, 0, 1]].reshape(-1)), cot.reshape(-1))
    lap = lap + lap.T
    return lap - np.diag(lap.sum(1))


def np_cot(vertices, faces, cot, n):
    """L v with the dense cotangent matrix of every batch element; cot (B,F,3)"""
    return np.stack([dense_cot(faces if faces.ndim == 2 else faces[b], cot[b], n) @ vertices[b]
                     for b in range(vertices.shape[0])])


def assert_close_to_dense(got, want):
    """rtol 1e-12, with an absolute term of 1e-12 of the largest reference value: a vertex whose terms cancel has no
    relative accuracy of its own in either implementation"""
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-12 * max(float(np.abs(want).max(initial=0.0)), 1e-300))


# ------------------------------------------------------------------------------------------------ 1. topology
@pytest.mark.parametrize("name", sorted(MESHES))
def test_corner_lists_are_sorted_and_complete(name):
    faces, n = MESHES[name]()
    corners = mesh_laplacian.MeshCorners.from_faces(torch.from_numpy(faces), n)
    deg = faces.shape[1]
    assert corners.batch == 1 and corners.degree == deg and corners.n_faces == faces.shape[0]
    assert corners.start.dtype == torch.int32 and corners.start.shape == (1, n + 1)
    assert corners.codes.shape == (1, faces.size) and corners.nbr.shape == (1, faces.size, 2)
    start, codes, nbr = corners.start[0].numpy(), corners.codes[0].numpy(), corners.nbr[0].numpy()
    flat = faces.reshape(-1)
    assert start[0] == 0 and start[n] == flat.size
    for v in range(n):
        mine = codes[start[v]:start[v + 1]]
        assert np.array_equal(mine, np.flatnonzero(flat == v))          # ascending, and every corner once
        f, c = mine // deg, mine % deg
        assert np.array_equal(nbr[start[v]:start[v + 1], 0], faces[f, (c + 1) % deg])
        assert np.array_equal(nbr[start[v]:start[v + 1], 1], faces[f, (c - 1) % deg])
    assert np.array_equal(corners.lii(torch.float64).numpy(), 2.0 * np.bincount(flat, minlength=n))


def test_a_shared_topology_has_one_batch_element():
    faces, n = MESHES["grid_7x9"]()
    tf = torch.from_numpy(faces)
    assert mesh_laplacian.MeshCorners.from_faces(tf[None], n).batch == 1
    assert mesh_laplacian.MeshCorners.from_faces(tf[None].expand(4, -1, -1), n).batch == 1
    assert mesh_laplacian.MeshCorners.from_faces(tf[None].repeat(2, 1, 1).int(), n).batch == 2


# ------------------------------------------------------------------------------------------ 2. compositions
@pytest.mark.parametrize("name", sorted(MESHES))
def test_uniform_composition_against_the_dense_matrix(name):
    faces, n = MESHES[name]()
    v = random_vertices(11, 3, n)
    corners = mesh_laplacian.MeshCorners.from_faces(torch.from_numpy(faces), n)
    got = mesh_laplacian.mesh_uniform_laplacian(torch.from_numpy(v), corners).numpy()
    assert got.shape == v.shape and np.isfinite(got).all()
    assert_close_to_dense(got, np_uniform(v, faces, n))
    if name == "isolated":
        assert (got[:, 4:] == 0).all() and not np.signbit(got[:, 4:]).any()
    if name == "no_faces":
        assert (got == 0).all()
    # any D, and fp32 stays within fp32 of it
    wide = np.concatenate([v, v[..., :2] * 3], -1)
    assert_close_to_dense(mesh_laplacian.mesh_uniform_laplacian(torch.from_numpy(wide), corners).numpy(),
                          np_uniform(wide, faces, n))
    low = mesh_laplacian.mesh_uniform_laplacian(torch.from_numpy(v.astype(np.float32)), corners)
    assert low.dtype == torch.float32
    np.testing.assert_allclose(low.numpy(), got, rtol=0, atol=2e-5)


@pytest.mark.parametrize("name", ["grid_7x9", "soup", "tetrahedron", "isolated", "no_faces"])
def test_cot_composition_against_the_dense_matrix(name):
    faces, n = MESHES[name]()
    v = random_vertices(12, 2, n)
    weights = np_cotangent(random_vertices(13, 2, n), faces)            # any constant weights, per batch element
    corners = mesh_laplacian.MeshCorners.from_faces(torch.from_numpy(faces), n)
    got = mesh_laplacian.mesh_cot_laplacian(torch.from_numpy(v), corners, torch.from_numpy(weights)).numpy()
    assert got.shape == v.shape and np.isfinite(got).all()
    assert_close_to_dense(got, np_cot(v, faces, weights, n))
    if name == "isolated":
        assert (got[:, 4:] == 0).all()


def test_compositions_over_two_topologies_in_one_batch():
    vert1, _, faces = two_topology_batch()
    corners = mesh_laplacian.MeshCorners.from_faces(torch.from_numpy(faces), 25)
    assert corners.batch == 2
    assert_close_to_dense(mesh_laplacian.mesh_uniform_laplacian(torch.from_numpy(vert1), corners).numpy(),
                          np_uniform(vert1, faces, 25))
    weights = np_cotangent(vert1, faces)
    assert np.isfinite(weights).all()
    got = mesh_laplacian.mesh_cot_laplacian(torch.from_numpy(vert1), corners, torch.from_numpy(weights))
    assert_close_to_dense(got.numpy(), np_cot(vert1, faces, weights, 25))


def test_cotangent_composition_against_numpy():
    v, faces = jittered_grid(7, 9, 5, batch=2)
    v = v.astype(np.float64)
    faces = np.concatenate([faces, [[3, 3, 10], [5, 5, 5], [0, 1, 2]]])   # without area: a repeated vertex, a point,
    v[:, 2] = 2 * v[:, 1] - v[:, 0]                                      # and three vertices on a line
    want = np_cotangent(v, faces)
    got = mesh_laplacian.cotangent_composition(torch.from_numpy(v), torch.from_numpy(faces))
    assert_close_to_dense(got.numpy(), want)     # (numpy and torch sum the three squares in different orders)
    assert (got[:, -3:-1] == 0).all() and not np.signbit(got[:, -3:-1].numpy()).any()
    assert np.isfinite(got.numpy()).all()
    assert torch.equal(geo_operations.cotangent(torch.from_numpy(v), torch.from_numpy(faces)[None].expand(2, -1, -1)), got)
    # a right isosceles triangle: cot 90 = 0 at vertex 0 (edge 23), cot 45 = 1 at the others, times 1/2
    tri = torch.tensor([[[0.0, 0, 0], [1.0, 0, 0], [0.0, 1, 0]]], dtype=torch.float64)
    np.testing.assert_allclose(geo_operations.cotangent(tri, torch.tensor([[[0, 1, 2]]])).numpy(),
                               [[[0.0, 0.5, 0.5]]], rtol=0, atol=1e-9)


def test_gradcheck_of_both_compositions():
    faces, n = soup_mesh(12, 30, 2)
    corners = mesh_laplacian.MeshCorners.from_faces(torch.from_numpy(faces), n)
    x = torch.from_numpy(random_vertices(14, 2, n)).requires_grad_(True)
    weights = torch.from_numpy(np_cotangent(random_vertices(15, 2, n), faces))
    assert torch.autograd.gradcheck(lambda t: mesh_laplacian.mesh_uniform_laplacian(t, corners), (x,))
    assert torch.autograd.gradcheck(lambda t: mesh_laplacian.mesh_cot_laplacian(t, corners, weights), (x,))
    quads, nq = quad_grid(3, 4)
    cq = mesh_laplacian.MeshCorners.from_faces(torch.from_numpy(quads), nq)
    xq = torch.from_numpy(random_vertices(16, 1, nq)).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda t: mesh_laplacian.mesh_uniform_laplacian(t, cq), (xq,))


# ------------------------------------------------------------------------------------------ 3. the modules
def test_uniform_laplacian_module():
    faces, n = MESHES["grid_7x9"]()
    v = random_vertices(17, 3, n)
    tf = torch.from_numpy(faces)[None]
    lap = geo_operations.UniformLaplacian()
    assert lap.L is None
    with pytest.raises(AssertionError):
        lap(torch.from_numpy(v))                                        # the first call needs faces
    out = lap(torch.from_numpy(v[:1]), tf)                              # built from a single mesh ...
    assert isinstance(lap.L, mesh_laplacian.MeshCorners) and lap.L.batch == 1
    assert_close_to_dense(out.numpy(), np_uniform(v[:1], faces, n))
    assert lap.Lii.shape == (n,) and np.array_equal(lap.Lii.numpy(), dense_uniform(faces, n)[1])
    kept = lap.L
    assert_close_to_dense(lap(torch.from_numpy(v)).numpy(), np_uniform(v, faces, n))   # ... it serves a batch
    assert lap.L is kept
    lap.L = None                                                        # reset from outside
    other = soup_mesh(n, 100, 4)[0]
    assert_close_to_dense(lap(torch.from_numpy(v), torch.from_numpy(other)[None].expand(3, -1, -1)).numpy(),
                          np_uniform(v, other, n))
    quads, nq = quad_grid(5, 6)
    vq = random_vertices(18, 2, nq)
    assert_close_to_dense(geo_operations.UniformLaplacian()(torch.from_numpy(vq), torch.from_numpy(quads)[None]).numpy(),
                          np_uniform(vq, quads, nq))


def test_cot_laplacian_module_keeps_the_weights_of_the_building_call(capsys):
    v, faces = jittered_grid(7, 9, 6, batch=2)
    v = v.astype(np.float64)
    w = v + 0.02 * random_vertices(19, 2, 63)
    tf = torch.from_numpy(faces)[None].expand(2, -1, -1)
    lap = geo_operations.CotLaplacian()
    with pytest.raises(AssertionError):
        lap(torch.from_numpy(v))
    x = torch.from_numpy(v).requires_grad_(True)
    out = lap(x, tf)
    assert capsys.readouterr().out == ""                                # it does not print
    assert out.requires_grad and not lap.L.weights.requires_grad
    cot_v = np_cotangent(v, faces)
    np.testing.assert_allclose(lap.L.weights.numpy(), cot_v, rtol=1e-12, atol=0)
    assert_close_to_dense(out.detach().numpy(), np_cot(v, faces, cot_v, 63))
    # the operator is a constant: the gradient is L g, and another V meets the first V's cotangents
    g = random_vertices(20, 2, 63)
    grad, = torch.autograd.grad(out, x, torch.from_numpy(g))
    assert_close_to_dense(grad.numpy(), np_cot(g, faces, cot_v, 63))
    second = lap(torch.from_numpy(w))
    assert not second.requires_grad
    assert_close_to_dense(second.numpy(), np_cot(w, faces, cot_v, 63))
    lap.L = None
    assert_close_to_dense(lap(torch.from_numpy(w), tf).numpy(), np_cot(w, faces, np_cotangent(w, faces), 63))


def test_cot_laplacian_rejects_a_non_finite_cotangent():
    v, faces = jittered_grid(5, 5, 7)
    v = v.astype(np.float64)
    v[0, 3, 1] = np.inf
    with pytest.raises(ValueError, match="finite"):
        geo_operations.CotLaplacian()(torch.from_numpy(v), torch.from_numpy(faces)[None])


# ------------------------------------------------------------------------------------------------ 4. losses
class DenseLaplacian(object):
    """either Laplacian module of the reference as dense fp64 torch matrices, one per batch element: ``L`` is built by
    the call that finds it None -- the cotangents from that call's vertices, detached -- and kept"""

    def __init__(self, use_cot):
        self.use_cot = use_cot
        self.L = None

    def __call__(self, verts, faces=None):
        n = verts.shape[1]
        if self.L is None:
            assert faces is not None
            faces = faces.numpy()
            if self.use_cot:
                cot = np_cotangent(verts.detach().numpy(), faces)
                self.L = [(torch.from_numpy(dense_cot(faces[b], cot[b], n)), None) for b in range(faces.shape[0])]
            else:
                self.L = [tuple(torch.from_numpy(a) for a in dense_uniform(faces[b], n)) for b in range(faces.shape[0])]
        out = []
        for b in range(verts.shape[0]):
            lap, lii = self.L[b if len(self.L) > 1 else 0]
            x = lap @ verts[b]
            out.append(x if lii is None else x / (lii.unsqueeze(-1) + 1e-12))
        return torch.stack(out)


class RefMeshLaplacianLoss(object):
    """the control flow of reference model_loss.py:29-71 over DenseLaplacian"""

    def __init__(self, metric, use_cot, use_norm, consistent_topology, precompute_L):
        self.laplacian = DenseLaplacian(use_cot)
        self.metric, self.use_norm = metric, use_norm
        self.consistent_topology, self.precompute_L = consistent_topology, precompute_L
        self.L = None

    def __call__(self, vert1, vert2=None, face=None):
        if not self.consistent_topology:
            self.laplacian.L = None
        if self.L is None or (not self.precompute_L):
            lap1 = self.laplacian(vert1, face)
            if self.use_norm:
                lap1 = torch.norm(lap1, dim=-1, p=2)
            if self.precompute_L:
                self.L = lap1
        else:
            lap1 = self.L
        if vert2 is not None:
            lap2 = self.laplacian(vert2, face)
            if self.use_norm:
                lap2 = torch.norm(lap2, dim=-1, p=2)
            return self.metric(lap1, lap2)
        return lap1.mean()


def laplacian_loss_batch():
    """(vert1, vert2, vert3 (2,25,3) float64, faces (2,F,3)): two different topologies in one batch; the soup's faces
    without area are replaced, so that every cotangent is an ordinary number"""
    vert1, vert2, faces = two_topology_batch()
    rng = np.random.default_rng(9)
    for f in range(faces.shape[1]):
        while len(set(faces[1, f])) < 3:
            faces[1, f] = rng.integers(0, 25, 3)
    return vert1, vert2, vert1 + 0.03 * random_vertices(21, 2, 25), faces


FLAGS = list(itertools.product([False, True], repeat=4))   # use_cot, use_norm, consistent_topology, precompute_L


@pytest.mark.parametrize("use_cot,use_norm,consistent,precompute", FLAGS,
                         ids=["".join(n for n, on in zip(("cot_", "norm_", "consistent_", "precompute_"), f) if on) or "plain"
                              for f in FLAGS])
def test_mesh_laplacian_loss_against_the_restated_control_flow(use_cot, use_norm, consistent, precompute):
    """three calls in a row on one module and one restatement: the state that the flags keep between calls (the
    Laplacian, the kept lap1) shows from the second call on.  The third call swaps the arguments, so that with a
    kept lap1 and a rebuilt Laplacian the cotangents come from ITS vert2."""
    vert1, vert2, vert3, faces = laplacian_loss_batch()
    tf = torch.from_numpy(faces)
    for metric in (torch.nn.L1Loss(), torch.nn.MSELoss()):
        mod = model_loss.MeshLaplacianLoss(metric, use_cot, use_norm, consistent, precompute)
        ref = RefMeshLaplacianLoss(metric, use_cot, use_norm, consistent, precompute)
        for a, b in ((vert1, vert2), (vert3, vert2), (vert2, vert3), (vert3, None)):
            xs = [torch.from_numpy(t).requires_grad_(True) for t in (a, b) if t is not None]
            ys = [torch.from_numpy(t).requires_grad_(True) for t in (a, b) if t is not None]
            got, want = mod(*(xs + [None] * (2 - len(xs))), tf), ref(*(ys + [None] * (2 - len(ys))), tf)
            assert got.shape == want.shape == ()
            torch.testing.assert_close(got, want, rtol=1e-11, atol=1e-12)
            if got.requires_grad:
                # (a kept lap1 holds the graph of the call that made it: only this call's inputs are asked)
                ga = torch.autograd.grad(got, xs, allow_unused=True, retain_graph=True)
                gb = torch.autograd.grad(want, ys, allow_unused=True, retain_graph=True)
                for p, q in zip(ga, gb):
                    assert (p is None) == (q is None)
                    if p is not None:
                        torch.testing.assert_close(p, q, rtol=1e-9, atol=1e-11)


def test_mesh_laplacian_loss_quirks():
    vert1, vert2, vert3, faces = laplacian_loss_batch()
    a, b, c, tf = (torch.from_numpy(t) for t in (vert1, vert2, vert3, faces))
    l1 = torch.nn.L1Loss()
    cot1, cot3 = np_cotangent(vert1, faces), np_cotangent(vert3, faces)
    # a call's cotangents come from vert1 and serve vert2 as well
    got = model_loss.MeshLaplacianLoss(l1, use_cot=True)(a, b, tf)
    want = np.abs(np_cot(vert1, faces, cot1, 25) - np_cot(vert2, faces, cot1, 25)).mean()
    np.testing.assert_allclose(float(got), want, rtol=1e-11)
    # with a kept lap1 and a Laplacian rebuilt on every call they come from vert2
    mod = model_loss.MeshLaplacianLoss(l1, use_cot=True, precompute_L=True)
    mod(a, b, tf)
    kept = np_cot(vert1, faces, cot1, 25)
    np.testing.assert_allclose(mod.L.numpy(), kept, rtol=1e-11, atol=1e-12)
    got = mod(b, c, tf)                                                 # vert1 = b is not looked at
    np.testing.assert_allclose(float(got), np.abs(kept - np_cot(vert3, faces, cot3, 25)).mean(), rtol=1e-11)
    # consistent_topology keeps the first Laplacian: later faces are not looked at, nor needed
    mod = model_loss.MeshLaplacianLoss(l1, use_cot=True, consistent_topology=True)
    first = mod(a, b, tf)
    held = mod.laplacian.L
    other = torch.from_numpy(np.ascontiguousarray(faces[::-1]))
    assert torch.equal(mod(a, b, other), first) and torch.equal(mod(a, b), first) and mod.laplacian.L is held
    np.testing.assert_allclose(float(mod(c, b)), np.abs(np_cot(vert3, faces, cot1, 25) - np_cot(vert2, faces, cot1, 25)).mean(),
                               rtol=1e-11)
    # vert2 = None returns lap1.mean(), and the reference's assert(~precompute_L) never fires
    for precompute in (False, True):
        got = model_loss.MeshLaplacianLoss(l1, use_norm=True, precompute_L=precompute)(a, None, tf)
        np.testing.assert_allclose(float(got), np.linalg.norm(np_uniform(vert1, faces, 25), axis=-1).mean(), rtol=1e-11)
    with pytest.raises(AssertionError):
        model_loss.MeshLaplacianLoss(l1)(a, b)                          # no face to build from


def test_uniform_laplacian_smoothness_loss():
    vert1, vert2, _, faces = laplacian_loss_batch()
    a, b, tf = (torch.from_numpy(t) for t in (vert1, vert2, faces))
    mod = model_loss.UniformLaplacianSmoothnessLoss(25, tf, torch.nn.L1Loss())
    curve = np.linalg.norm(np_uniform(vert1, faces, 25), axis=-1)
    x = a.clone().requires_grad_(True)
    out = mod(x)
    assert out.shape == (2, 25)
    np.testing.assert_allclose(out.detach().numpy(), curve, rtol=1e-11, atol=1e-13)
    y = a.clone().requires_grad_(True)
    ref = torch.norm(DenseLaplacian(False)(y, tf), p=2, dim=-1)
    torch.testing.assert_close(torch.autograd.grad(out.sum(), x)[0], torch.autograd.grad(ref.sum(), y)[0],
                               rtol=1e-9, atol=1e-11)
    # with vert_ref the reference curvature is computed from vert again: metric(curve, curve)
    assert float(mod(a, b)) == 0.0
    assert float(model_loss.UniformLaplacianSmoothnessLoss(25, tf, torch.nn.MSELoss())(b, a)) == 0.0
    # quads, and the topology is kept
    quads, nq = quad_grid(5, 6)
    vq = random_vertices(22, 2, nq)
    modq = model_loss.UniformLaplacianSmoothnessLoss(nq, torch.from_numpy(quads)[None], None)
    np.testing.assert_allclose(modq(torch.from_numpy(vq)).numpy(), np.linalg.norm(np_uniform(vq, quads, nq), axis=-1),
                               rtol=1e-11, atol=1e-13)
    held = modq.laplacian.L
    modq(torch.from_numpy(vq))
    assert modq.laplacian.L is held


# ------------------------------------------------------------------------------------------------ 5. errors
def test_errors():
    vert1, _, _, faces = laplacian_loss_batch()
    a, tf = torch.from_numpy(vert1), torch.from_numpy(faces)
    for value in (25, -1):
        bad = tf.clone()
        bad[1, 3, 2] = value
        with pytest.raises(IndexError, match="batch element 1"):
            mesh_laplacian.MeshCorners.from_faces(bad, 25)
        with pytest.raises(IndexError, match="batch element 1"):
            geo_operations.UniformLaplacian()(a, bad)
        with pytest.raises(IndexError, match="batch element 1"):
            model_loss.MeshLaplacianLoss(torch.nn.L1Loss(), use_cot=True)(a, a, bad)
    with pytest.raises(TypeError):
        mesh_laplacian.MeshCorners.from_faces(tf.double(), 25)
    with pytest.raises(TypeError):
        geo_operations.UniformLaplacian()(a, tf.float())
    with pytest.raises(TypeError):
        mesh_laplacian.MeshCorners.from_faces(faces, 25)
    quads = torch.from_numpy(quad_grid(5, 5)[0])[None]
    with pytest.raises(NotImplementedError):
        geo_operations.CotLaplacian()(a, quads)
    with pytest.raises(NotImplementedError):
        model_loss.MeshLaplacianLoss(torch.nn.L1Loss(), use_cot=True)(a, a, quads)
    with pytest.raises(NotImplementedError):
        geo_operations.cotangent(a, quads)
    cq = mesh_laplacian.MeshCorners.from_faces(quads, 25)
    with pytest.raises(NotImplementedError):
        mesh_laplacian.mesh_cot_laplacian(a, cq, torch.zeros(2, quads.shape[1], 3, dtype=torch.float64))
    with pytest.raises(ValueError):
        mesh_laplacian.MeshCorners.from_faces(tf[:, :, :2], 25)
    corners = mesh_laplacian.MeshCorners.from_faces(tf, 25)
    with pytest.raises(ValueError):
        mesh_laplacian.mesh_uniform_laplacian(a[:, :20], corners)
    with pytest.raises(ValueError):
        mesh_laplacian.mesh_uniform_laplacian(torch.cat([a, a, a]), corners)   # 2 topologies do not serve 6 sets
    with pytest.raises(ValueError):
        mesh_laplacian.mesh_cot_laplacian(a, corners, torch.zeros(2, 5, 3, dtype=torch.float64))
    with pytest.raises(TypeError):
        mesh_laplacian.mesh_uniform_laplacian(a, faces)


def test_drop_in_names_resolve():
    import pytorch_points_amd
    pytorch_points_amd.install_as_pytorch_points()
    from pytorch_points.network.geo_operations import CotLaplacian, UniformLaplacian, cotangent  # noqa: F401
    from pytorch_points.network.model_loss import MeshLaplacianLoss, UniformLaplacianSmoothnessLoss  # noqa: F401
    assert MeshLaplacianLoss is model_loss.MeshLaplacianLoss and UniformLaplacian is geo_operations.UniformLaplacian
