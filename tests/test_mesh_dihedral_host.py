"""CPU tests (no GPU) of the mesh dihedral angles (pytorch_points_amd/mesh_dihedral.py, network/geo_operations.py
get_edge_points / get_normals / dihedral_angle, network/model_loss.py MeshDihedralAngleLoss) through their torch
compositions, against numpy restatements of reference geo_operations.py:603-619, :775-789 and an independent build of
the (E,4) table.  The mesh generators here also serve tests/test_gpu_mesh_dihedral.py."""
import functools
import os

import numpy as np
import pytest
import torch

from pytorch_points_amd import mesh_dihedral, mesh_edges, synthetic
from pytorch_points_amd.network import geo_operations, model_loss
from test_mesh_edges_host import REDUCTIONS, fan_mesh, grid_mesh, np_unique_edges, tetrahedron

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LO, HI = -1 + 1e-6, 1 - 1e-6
FLAT = np.pi - np.arccos(HI)          # a flat interior edge
BOUNDARY = np.pi - np.arccos(LO)      # a boundary edge: its one face on both sides


# ------------------------------------------------------------------------------------------------------- meshes
def cage():
    """the ico cage of tests/golden/gc_ico2.npz: (faces (320,3) int64, vertices (162,3) float64), closed"""
    z = np.load(os.path.join(GOLDEN_DIR, "gc_ico2.npz"))
    return z["faces"][0].astype(np.int64), z["vertices"][0].astype(np.float64)


def jittered_cage(seed, batch=1, amount=0.003):
    faces, v = cage()
    return faces, v[None] + amount * (2 * synthetic.uniform01(seed, (batch, v.shape[0], 3)).reshape(batch, -1, 3) - 1)


def folded_grid(rows, cols, seed, batch=1):
    """(vertices (batch,N,3) float64, faces): the grid with heights that repeat with period 2 in both directions,
    t = [[0, 1], [2, 5]] * 0.15 of the spacing, and a jitter of 0.03 of it.  Across a row edge the four heights miss
    a plane by (2 + 5 - 1) units, across a column edge by (1 + 5 - 2), across a diagonal by (5 - 1 - 2): no pair of
    neighbouring faces is near flat."""
    v, f = grid_mesh(rows, cols)
    step = 1.0 / (max(rows, cols) - 1)
    r, c = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    height = np.array([[0.0, 1.0], [2.0, 5.0]])[r % 2, c % 2].reshape(-1)
    out = np.repeat(v[None].astype(np.float64), batch, 0)
    out[:, :, 2] = 0.15 * step * height
    return out + 0.03 * step * (2 * synthetic.uniform01(seed, (batch, v.shape[0], 3)).reshape(batch, -1, 3) - 1), f


def zigzag_fan(t, seed, batch=1):
    """(vertices (batch,t+2,3) float64, faces): fan_mesh(t) with the apex at the origin and the rim on a slowly
    widening spiral of 0.25 rad a step whose height alternates between +0.3 and -0.3"""
    faces, n = fan_mesh(t)
    k = np.arange(n - 1)
    radius = 1 + 0.01 * k
    rim = np.stack([radius * np.cos(0.25 * k), radius * np.sin(0.25 * k), 0.3 * (-1.0) ** k], -1)
    v = np.concatenate([np.zeros((1, 3)), rim])
    return v[None] + 0.01 * (2 * synthetic.uniform01(seed, (batch, n, 3)).reshape(batch, -1, 3) - 1), faces


def torus_mesh(rows, cols):
    """a closed rows x cols torus (both even): (vertices (rows*cols,3) float64, faces (2*rows*cols,3)).  The minor
    radius follows folded_grid's period-2 pattern, 0.4 - 0.02 * [[0, 1], [2, 5]]: a plain torus' quads are planar and
    their diagonals flat edges."""
    r, c = (a.reshape(-1) for a in np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij"))
    at = lambda i, j: (i % rows) * cols + (j % cols)   # noqa: E731
    faces = np.concatenate([np.stack([at(r, c), at(r, c + 1), at(r + 1, c)], -1),
                            np.stack([at(r, c + 1), at(r + 1, c + 1), at(r + 1, c)], -1)]).astype(np.int64)
    u, w = 2 * np.pi * r / rows, 2 * np.pi * c / cols
    minor = 0.4 - 0.02 * np.array([[0.0, 1.0], [2.0, 5.0]])[r % 2, c % 2]
    v = np.stack([(1 + minor * np.cos(u)) * np.cos(w), (1 + minor * np.cos(u)) * np.sin(w), minor * np.sin(u)], -1)
    return v, faces


def two_topologies(seed=31):
    """(vertices (2,99,3) float64, faces (2,160,3)): the folded 9x11 grid (258 edges) and an 8x10 torus (240 edges)
    over the first 80 of the same 99 vertices"""
    vg, fg = folded_grid(9, 11, seed)
    vt, ft = torus_mesh(8, 10)
    verts = np.stack([vg[0], np.concatenate([vt, vg[0, 80:] + 3.0])])
    verts[1] += 0.002 * (2 * synthetic.uniform01(seed + 1, (99, 3)).reshape(99, 3) - 1)
    assert fg.shape == ft.shape and np_unique_edges(fg).shape[0] != np_unique_edges(ft).shape[0]
    return verts, np.stack([fg, ft])


# --------------------------------------------------------------------------------------------- numpy references
def dict_edge_points(faces):
    """the contract of the table, built another way: a dict from the sorted pair to the list of (half-edge number,
    opposite corner) in face order; rows by ascending pair, wings of the first and the last entry"""
    found = {}
    for f, face in enumerate(faces.tolist()):
        for j in range(3):
            key = tuple(sorted((face[j], face[(j + 1) % 3])))
            found.setdefault(key, []).append((3 * f + j, face[(j + 2) % 3]))
    rows = []
    for key in sorted(found):
        entries = sorted(found[key])
        assert len(entries) <= 2
        rows.append([key[0], key[1], entries[0][1], entries[-1][1]])
    return np.array(rows, np.int64).reshape(-1, 4), {k: len(v) for k, v in found.items()}


def np_unclamped_dot(v, table):
    """the reference's formula edge by edge in the dtype of ``v``: the dot of the two unit normals before the clamp"""
    d = np.zeros(table.shape[0], v.dtype)
    eps = v.dtype.type(1e-12)
    for e, (i0, i1, i2, i3) in enumerate(table.tolist()):
        na = np.cross(v[i2] - v[i0], v[i1] - v[i0])
        nb = np.cross(v[i3] - v[i1], v[i0] - v[i1])
        na = na / max(np.sqrt(np.sum(na * na)), eps)
        nb = nb / max(np.sqrt(np.sum(nb * nb)), eps)
        d[e] = np.sum(na * nb)
    return d


def np_angles(v, table):
    return np.pi - np.arccos(np.clip(np_unclamped_dot(v, table), LO, HI))


def assert_clear_of_the_clamp(v64, table):
    """every interior edge's unclamped fp64 |d| < 0.999 and every boundary edge's at -1: no edge sits where fp32 and
    fp64 could take different sides of the clamp.  No edge is left out."""
    d = np_unclamped_dot(v64, table)
    boundary = table[:, 2] == table[:, 3]
    assert (np.abs(d[~boundary]) < 0.999).all(), float(np.abs(d[~boundary]).max())
    assert (np.abs(d[boundary] + 1) < 1e-9).all()
    return d


@functools.lru_cache(maxsize=None)
def table_of(name):
    """(faces, n_vertices) by name -> the independent table"""
    faces, n = named_faces(name)
    return dict_edge_points(faces)[0]


def named_faces(name):
    if name == "tetrahedron":
        return tetrahedron()
    if name == "cage":
        return cage()[0], 162
    if name.startswith("grid_"):
        rows, cols = (int(x) for x in name[5:].split("x"))
        return grid_mesh(rows, cols)[1], rows * cols
    if name.startswith("fan_"):
        return fan_mesh(int(name[4:]))
    raise KeyError(name)


# ------------------------------------------------------------------------------------------------- 1. the table
@pytest.mark.parametrize("name", ["tetrahedron", "grid_3x3", "fan_8", "cage"])
def test_edge_points_composition_against_the_dict_build(name):
    faces, n = named_faces(name)
    want, incident = dict_edge_points(faces)
    got = mesh_dihedral.edge_points_composition(torch.from_numpy(faces))
    assert got.dtype == torch.int64 and np.array_equal(got.numpy(), want)
    assert np.array_equal(want[:, :2], np_unique_edges(faces))
    for row in want.tolist():
        boundary = incident[(row[0], row[1])] == 1
        assert (row[2] == row[3]) == boundary                     # w1 == w0 exactly on the boundary edges ...
        # ... and the wing rule: each wing closes a face of the mesh with the edge
        for w in row[2:]:
            assert any(sorted(f) == sorted((row[0], row[1], w)) for f in faces.tolist())
    if name in ("tetrahedron", "cage"):
        assert (want[:, 2] != want[:, 3]).all()
    topo = mesh_dihedral.MeshEdgePoints.from_faces(torch.from_numpy(faces), n)
    assert topo.batch == 1 and topo.capacity == 3 * faces.shape[0] and topo.counts_host == (want.shape[0],)
    assert np.array_equal(topo.table(0).numpy(), want) and bool((topo.edge_points[0, want.shape[0]:] == -1).all())
    edges = mesh_edges.MeshEdges.from_faces(torch.from_numpy(faces), n)
    assert torch.equal(topo.edge_points[..., :2], edges.edges)          # the edge numbering is shared
    for as_input in (faces, torch.from_numpy(faces)):
        out = geo_operations.get_edge_points(as_input)
        assert isinstance(out, type(as_input)) and np.array_equal(np.asarray(out), want)


def test_get_edge_points_of_a_mesh_object():
    class Mesh(object):
        pass
    mesh = Mesh()
    mesh.fs, mesh.vs = cage()
    assert np.array_equal(geo_operations.get_edge_points(mesh), table_of("cage"))


def test_batch_of_two_topologies_pads_with_minus_one():
    _, faces = two_topologies()
    topo = mesh_dihedral.MeshEdgePoints.from_faces(torch.from_numpy(faces), 99)
    assert topo.counts_host == (258, 240) and topo.edge_points.shape == (2, 480, 4)
    for b in range(2):
        assert np.array_equal(topo.table(b).numpy(), dict_edge_points(faces[b])[0])
        assert bool((topo.edge_points[b, topo.count(b):] == -1).all())


# ------------------------------------------------------------------------------------------------- 2. the angles
def composition(v, table, dtype=torch.float64):
    return geo_operations.dihedral_angle(torch.from_numpy(v).to(dtype), torch.from_numpy(table))


@pytest.mark.parametrize("name", ["cage", "grid_7x9", "fan_30", "tetrahedron"])
def test_composition_against_the_per_edge_loop(name):
    if name == "cage":
        faces, v = jittered_cage(1)
    elif name == "grid_7x9":
        v, faces = folded_grid(7, 9, 2)
    elif name == "fan_30":
        v, faces = zigzag_fan(30, 3)
    else:
        faces, v = tetrahedron()[0], synthetic.unit_sphere(4, 1, 4).astype(np.float64)
    table = dict_edge_points(faces)[0]
    got = composition(v[0], table)
    assert got.dtype == torch.float64 and got.shape == (table.shape[0],)
    np.testing.assert_allclose(got.numpy(), np_angles(v[0], table), rtol=0, atol=1e-12)


def test_closed_forms():
    # A regular tetrahedron.  The normals of two faces make the angle pi - acos(1/3), their dot is -1/3, and the
    # reference's formula returns pi - acos(-1/3) = acos(1/3): the interior angle between the faces.
    v = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], np.float64)
    got = composition(v, table_of("tetrahedron")).numpy()
    np.testing.assert_allclose(got, np.pi - np.arccos(-1.0 / 3.0), rtol=0, atol=1e-14)
    np.testing.assert_allclose(got, np.arccos(1.0 / 3.0), rtol=0, atol=1e-14)
    # a flat grid: the two constants, and no gradient anywhere (boundary edges are clamped from below, flat ones from
    # above)
    vg, _ = grid_mesh(5, 6)
    table = table_of("grid_5x6")
    boundary = table[:, 2] == table[:, 3]
    assert 0 < boundary.sum() < boundary.size
    x = torch.from_numpy(vg).double().requires_grad_(True)
    out = geo_operations.dihedral_angle(x, torch.from_numpy(table))
    assert np.array_equal(out.detach().numpy()[~boundary], np.full((~boundary).sum(), FLAT))
    assert np.array_equal(out.detach().numpy()[boundary], np.full(boundary.sum(), BOUNDARY))
    grad, = torch.autograd.grad(out.sum(), x)
    assert bool((grad == 0).all())


def test_boundary_edges_pass_no_gradient():
    v, faces = folded_grid(5, 6, 5)
    table = table_of("grid_5x6")
    boundary = torch.from_numpy(table[:, 2] == table[:, 3])
    x = torch.from_numpy(v[0]).requires_grad_(True)
    out = geo_operations.dihedral_angle(x, torch.from_numpy(table))
    np.testing.assert_allclose(out.detach().numpy()[boundary.numpy()], BOUNDARY, rtol=0, atol=0)
    grad, = torch.autograd.grad(out[boundary].sum(), x, retain_graph=True)
    assert bool((grad == 0).all())
    grad, = torch.autograd.grad(out[~boundary].sum(), x)
    assert bool((grad != 0).any())


def swapped(table, columns):
    out = table.copy()
    out[:, list(columns)] = table[:, list(columns)[::-1]]
    return out


@pytest.mark.parametrize("name", ["cage", "grid_7x9"])
def test_column_swaps_are_bit_invariant_in_fp32(name):
    """swapping columns 0 and 1 flips both normals, swapping 2 and 3 trades them: the same angle, and (the rows are
    evaluated in canonical order) the same fp32 bits"""
    if name == "cage":
        faces, v = jittered_cage(6)
    else:
        v, faces = folded_grid(7, 9, 7)
    table = dict_edge_points(faces)[0]
    base = composition(v[0], table, torch.float32)
    assert base.dtype == torch.float32
    rng = np.random.default_rng(8)
    some = rng.random(table.shape[0]) < 0.5
    for columns in ((0, 1), (2, 3)):
        other = swapped(table, columns)
        assert torch.equal(composition(v[0], other, torch.float32), base)
        mixed = np.where(some[:, None], other, table)               # some rows one way, some the other
        assert torch.equal(composition(v[0], mixed, torch.float32), base)
    assert torch.equal(composition(v[0], swapped(swapped(table, (0, 1)), (2, 3)), torch.float32), base)
    # and the plain formula agrees with the canonical evaluation to rounding
    np.testing.assert_allclose(base.numpy(), np_angles(v[0], swapped(table, (0, 1))), rtol=0, atol=2e-5)


def test_reference_table_gives_the_same_edges_and_the_same_bits():
    """tests/golden/dihedral_edge_points.npz: the (E,4) table the reference's build_gemm / get_edge_points make for
    the ico cage (data only).  Per edge it holds the same ends and the same wings as ours, in the reference's
    traversal order, and the angles from either table are bit-equal."""
    z = np.load(os.path.join(GOLDEN_DIR, "dihedral_edge_points.npz"))
    faces, ref = z["faces"], z["edge_points"]
    assert np.array_equal(faces, cage()[0]) and ref.shape == (480, 4)
    ours = table_of("cage")
    order = np.lexsort((np.sort(ref[:, :2], 1)[:, 1], np.sort(ref[:, :2], 1)[:, 0]))
    ref = ref[order]
    assert np.array_equal(np.sort(ref[:, :2], 1), ours[:, :2])
    assert np.array_equal(np.sort(ref[:, 2:], 1), np.sort(ours[:, 2:], 1))
    assert not np.array_equal(ref, ours)                              # (the column orders do differ)
    _, v = jittered_cage(9)
    for dtype in (torch.float32, torch.float64):
        assert torch.equal(composition(v[0], ref, dtype), composition(v[0], ours, dtype))


# ----------------------------------------------------------------------------------------------- 3. the gradient
def test_gradcheck_on_a_jittered_cage():
    faces, v = jittered_cage(10)
    table = table_of("cage")
    d = assert_clear_of_the_clamp(v[0], table)
    assert d.shape == (480,) and not (table[:, 2] == table[:, 3]).any()      # closed: every edge is interior
    topo = mesh_dihedral.MeshEdgePoints.from_faces(torch.from_numpy(faces), 162)
    x = torch.from_numpy(v).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda t: mesh_dihedral.mesh_dihedral_angle(t, topo)[:, :480], (x,),
                                    eps=1e-6, atol=1e-6, rtol=1e-6)


def test_gradcheck_with_boundary_edges_and_two_topologies():
    verts, faces = two_topologies()
    for b in range(2):
        assert_clear_of_the_clamp(verts[b], dict_edge_points(faces[b])[0])
    topo = mesh_dihedral.MeshEdgePoints.from_faces(torch.from_numpy(faces), 99)
    x = torch.from_numpy(verts).requires_grad_(True)
    out = mesh_dihedral.mesh_dihedral_angle(x, topo)
    assert out.shape == (2, 480) and bool((out[0, 258:] == 0).all()) and bool((out[1, 240:] == 0).all())
    assert torch.autograd.gradcheck(lambda t: mesh_dihedral.mesh_dihedral_angle(t, topo), (x,), eps=1e-6, atol=1e-6,
                                    rtol=1e-6)


def test_degenerate_face():
    """a face without area: the reference's forward value (its unit normal is 0, so d = 0 and the angle pi / 2), no
    gradient from that edge -- F.normalize's backward would give about 1e12 -- and everything finite"""
    v = np.array([[0, 0, 0], [1, 0, 0], [0.3, 1, 0.2], [2, 0, 0]], np.float64)   # 0, 1, 3 in a line
    faces = np.array([[0, 1, 2], [1, 0, 3]], np.int64)
    table = dict_edge_points(faces)[0]
    for dtype in (torch.float64, torch.float32):
        x = torch.from_numpy(v).to(dtype).requires_grad_(True)
        out = geo_operations.dihedral_angle(x, torch.from_numpy(table))
        row = int(np.flatnonzero((table[:, 0] == 0) & (table[:, 1] == 1))[0])
        assert float(out[row].detach()) == pytest.approx(np.pi / 2, abs=1e-6) and bool(torch.isfinite(out).all())
        grad, = torch.autograd.grad(out[row], x, retain_graph=True)
        assert bool((grad == 0).all())
        grad, = torch.autograd.grad(out.sum(), x)
        assert bool(torch.isfinite(grad).all())


# --------------------------------------------------------------------------------------------------- 4. errors
def test_errors():
    faces, n = tetrahedron()
    tf = torch.from_numpy(faces)
    fan, fan_n = fan_mesh(4)
    three_on_an_edge = np.array([[0, 1, 2], [1, 0, 3], [0, 1, 4]], np.int64)
    for bad, count in ((three_on_an_edge, 5), (np.concatenate([fan, fan[:1]]), fan_n)):
        with pytest.raises(ValueError, match="more than two"):
            mesh_dihedral.edge_points_composition(torch.from_numpy(bad))
        with pytest.raises(ValueError, match="batch element 0"):
            mesh_dihedral.MeshEdgePoints.from_faces(torch.from_numpy(bad), count)
        with pytest.raises(ValueError):
            geo_operations.get_edge_points(bad)
    stacked = torch.from_numpy(np.stack([fan, np.concatenate([fan[:3], fan[:1]])]))
    with pytest.raises(ValueError, match="batch element 1"):
        mesh_dihedral.MeshEdgePoints.from_faces(stacked, fan_n)
    for value in (4, -1):
        out_of_range = faces.copy()
        out_of_range[2, 1] = value
        with pytest.raises(IndexError, match="batch element 0"):
            mesh_dihedral.MeshEdgePoints.from_faces(torch.from_numpy(out_of_range), n)
        with pytest.raises(IndexError):
            mesh_dihedral.MeshEdgePoints.from_edge_points(torch.from_numpy(out_of_range[:, [0, 1, 2, 2]]), n)
    with pytest.raises(TypeError):
        mesh_dihedral.MeshEdgePoints.from_faces(tf.float(), n)
    with pytest.raises(TypeError):
        mesh_dihedral.MeshEdgePoints.from_faces(faces, n)
    with pytest.raises(NotImplementedError):
        mesh_dihedral.MeshEdgePoints.from_faces(torch.zeros(2, 4, dtype=torch.int64), n)
    with pytest.raises(ValueError):
        mesh_dihedral.MeshEdgePoints.from_faces(torch.zeros(3, dtype=torch.int64), n)
    with pytest.raises(ValueError):
        mesh_dihedral.MeshEdgePoints.from_edge_points(torch.zeros(5, 2, dtype=torch.int64), n)
    with pytest.raises(TypeError):
        mesh_dihedral.MeshEdgePoints.from_edge_points(torch.zeros(5, 4), n)
    topo = mesh_dihedral.MeshEdgePoints.from_faces(tf, n)
    with pytest.raises(TypeError):
        mesh_dihedral.mesh_dihedral_angle(torch.zeros(1, 4, 3), mesh_edges.MeshEdges.from_faces(tf, n))
    with pytest.raises(ValueError):
        mesh_dihedral.mesh_dihedral_angle(torch.zeros(1, 5, 3), topo)
    with pytest.raises(ValueError):
        mesh_dihedral.mesh_dihedral_angle(torch.zeros(1, 4, 2), topo)
    with pytest.raises(RuntimeError):
        mesh_dihedral.mesh_dihedral_angle(torch.zeros(1, 4, 3, dtype=torch.int64), topo)
    with pytest.raises(ValueError):
        geo_operations.dihedral_angle(torch.zeros(4, 3), torch.zeros(6, 2, dtype=torch.int64))
    with pytest.raises(TypeError):
        geo_operations.dihedral_angle(torch.zeros(4, 3), torch.zeros(6, 4))


# ---------------------------------------------------------------------------------------------------- 5. the rest
def loop_loss(angle1, angle2, counts, threshold, reduction):
    """MeshDihedralAngleLoss element by element"""
    per = []
    for b, count in enumerate(counts):
        if angle2 is not None:
            values = [(angle1[b][e] - angle2[b][e]) ** 2 for e in range(count)]
        else:
            values = [max(threshold - angle1[b][e], 0.0) ** 2 for e in range(count)]
        per.append({"max": max(values), "sum": sum(values)}.get(reduction, sum(values) / count))
    return np.array(per) if reduction == "none" else sum(per) / len(per)


@pytest.mark.parametrize("reduction", REDUCTIONS)
@pytest.mark.parametrize("mode", ["pair", "threshold"])
def test_loss_against_a_per_element_loop(mode, reduction):
    verts, faces = two_topologies()
    other = verts + 0.02 * (2 * synthetic.uniform01(40, verts.shape).reshape(verts.shape) - 1)
    tables = [dict_edge_points(faces[b])[0] for b in range(2)]
    a1 = [np_angles(verts[b], tables[b]) for b in range(2)]
    a2 = [np_angles(other[b], tables[b]) for b in range(2)]
    threshold = 2.4                                     # cuts through the interior angles of both meshes
    assert all(0 < (a < threshold).sum() < a.size for a in a1)
    mod = model_loss.MeshDihedralAngleLoss(threshold if mode == "threshold" else None, reduction)
    x1, x2 = (torch.from_numpy(a).requires_grad_(True) for a in (verts, other))
    got = mod(x1, x2 if mode == "pair" else None, torch.from_numpy(faces))
    want = loop_loss(a1, a2 if mode == "pair" else None, [258, 240], threshold, reduction)
    np.testing.assert_allclose(got.detach().numpy(), want, rtol=1e-11, atol=0)
    grads = torch.autograd.grad(got.sum(), (x1, x2) if mode == "pair" else (x1,))
    assert all(bool(torch.isfinite(g).all()) and bool((g != 0).any()) for g in grads)


def test_loss_keeps_its_topology():
    verts, faces = two_topologies()
    mod = model_loss.MeshDihedralAngleLoss(2.4, consistent_topology=True)
    first = mod(torch.from_numpy(verts), face=torch.from_numpy(faces))
    kept = mod.E
    assert isinstance(kept, mesh_dihedral.MeshEdgePoints)
    assert torch.equal(mod(torch.from_numpy(verts)), first) and mod.E is kept
    with pytest.raises(AssertionError):
        model_loss.MeshDihedralAngleLoss(2.4)(torch.from_numpy(verts))
    with pytest.raises(NotImplementedError):
        model_loss.MeshDihedralAngleLoss(2.4, "median")(torch.from_numpy(verts), face=torch.from_numpy(faces))


def test_drop_in_names_and_get_normals():
    for name in ("get_edge_points", "get_normals", "dihedral_angle"):
        assert callable(getattr(geo_operations, name))
    assert issubclass(model_loss.MeshDihedralAngleLoss, torch.nn.Module)
    faces, v = jittered_cage(11)
    table = torch.from_numpy(table_of("cage"))
    x = torch.from_numpy(v[0])
    na, nb = geo_operations.get_normals(x, table, 0), geo_operations.get_normals(x, table, 3)
    assert na.shape == (480, 3) and torch.allclose(na.norm(dim=-1), torch.ones(480, dtype=torch.float64))
    np.testing.assert_allclose(np.pi - np.arccos(np.clip((na * nb).sum(-1).numpy(), LO, HI)),
                               geo_operations.dihedral_angle(x, table).numpy(), rtol=0, atol=1e-12)
    assert torch.equal(geo_operations.get_normals(x, table, 1), na)      # sides 0, 1 and 2, 3 name the same face
    assert torch.equal(geo_operations.get_normals(x, table, 2), nb)
