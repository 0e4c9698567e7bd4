"""CPU tests (no GPU) of what the five mesh topology constructors share (pytorch_points_amd/_mesh_topology.py): the
normalising of the caller's index tensor, the one-topology-for-the-batch rule and the errors.  The smallest inputs that
can go wrong -- one triangle, and two triangles that share the edge (1,2), over 4 vertices -- against tables written
out here."""
import pytest
import torch

from pytorch_points_amd import mesh_dihedral, mesh_edges, mesh_laplacian

N = 4
FACES = {"one": [[0, 1, 2]], "two": [[0, 1, 2], [2, 1, 3]]}
EDGES = {"one": [[0, 1], [0, 2], [1, 2]], "two": [[0, 1], [0, 2], [1, 2], [1, 3], [2, 3]]}
# [a, c, w0, w1]: the wings are the corners opposite the edge's lowest / highest half-edge, the same on a boundary edge
EDGE_POINTS = {"one": [[0, 1, 2, 2], [0, 2, 1, 1], [1, 2, 0, 0]],
               "two": [[0, 1, 2, 2], [0, 2, 1, 1], [1, 2, 0, 3], [1, 3, 2, 2], [2, 3, 1, 1]]}


def padded(rows, capacity):
    return rows + [[-1] * len(rows[0])] * (capacity - len(rows))


# name -> (constructor, its argument's name, the attribute that holds the table, input of a mesh, table of a mesh,
#          a wrong number of columns and the error it raises)
CONSTRUCTORS = {
    "MeshEdges.from_faces": (mesh_edges.MeshEdges.from_faces, "edges", FACES,
                             lambda m: padded(EDGES[m], 3 * len(FACES[m])), 4, NotImplementedError),
    "MeshEdges.from_edges": (mesh_edges.MeshEdges.from_edges, "edges", EDGES, lambda m: EDGES[m], 1, ValueError),
    "MeshEdgePoints.from_faces": (mesh_dihedral.MeshEdgePoints.from_faces, "edge_points", FACES,
                                  lambda m: padded(EDGE_POINTS[m], 3 * len(FACES[m])), 4, NotImplementedError),
    "MeshEdgePoints.from_edge_points": (mesh_dihedral.MeshEdgePoints.from_edge_points, "edge_points", EDGE_POINTS,
                                        lambda m: EDGE_POINTS[m], 3, ValueError),
    "MeshCorners.from_faces": (mesh_laplacian.MeshCorners.from_faces, "faces", FACES, lambda m: FACES[m], 2,
                               ValueError),
}
CASES = [(name, m) for name in CONSTRUCTORS for m in ("one", "two")]


def table_of(name, topo):
    return getattr(topo, CONSTRUCTORS[name][1])


@pytest.mark.parametrize("name,m", CASES)
def test_int32_and_int64_give_the_same_int64_table(name, m):
    build, _, inputs, want, _, _ = CONSTRUCTORS[name]
    for dtype in (torch.int32, torch.int64):
        topo = build(torch.tensor(inputs[m], dtype=dtype), N)
        table = table_of(name, topo)
        assert table.dtype == torch.int64 and table.is_contiguous()
        assert table.tolist() == [want(m)]
        assert topo.n_vertices == N


@pytest.mark.parametrize("name,m", CASES)
def test_one_topology_serves_the_batch(name, m):
    build, _, inputs, want, _, _ = CONSTRUCTORS[name]
    rows = torch.tensor(inputs[m])
    for shared in (rows, rows[None].expand(3, -1, -1)):
        topo = build(shared, N)
        assert topo.batch == 1 and table_of(name, topo).tolist() == [want(m)]
    topo = build(torch.stack([rows, rows]), N)
    assert topo.batch == 2 and table_of(name, topo).tolist() == [want(m), want(m)]


@pytest.mark.parametrize("name", CONSTRUCTORS)
def test_a_float_tensor_and_a_list_are_type_errors(name):
    build, _, inputs, _, _, _ = CONSTRUCTORS[name]
    for bad in (torch.tensor(inputs["one"], dtype=torch.float32), inputs["one"]):
        with pytest.raises(TypeError, match=name.replace(".", r"\.")):
            build(bad, N)


@pytest.mark.parametrize("name,m", CASES)
def test_an_index_out_of_range_names_its_batch_element(name, m):
    build, _, inputs, _, _, _ = CONSTRUCTORS[name]
    rows = torch.tensor(inputs[m])
    bad = rows.clone()
    bad[-1, -1] = N
    with pytest.raises(IndexError, match="%s: batch element 1 " % name.replace(".", r"\.")):
        build(torch.stack([rows, bad]), N)
    build(torch.stack([rows, rows]), N)


@pytest.mark.parametrize("name", CONSTRUCTORS)
def test_the_wrong_last_dimension(name):
    build, _, _, _, cols, error = CONSTRUCTORS[name]
    with pytest.raises(error, match=name.replace(".", r"\.")):
        build(torch.zeros(2, cols, dtype=torch.int64), N)
    with pytest.raises(error, match=name.replace(".", r"\.")):
        build(torch.zeros(2, 2, cols, dtype=torch.int64), N)
