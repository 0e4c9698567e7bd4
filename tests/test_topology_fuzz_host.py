"""CPU tests (no GPU) of tests/topology_fuzz.py, for every seed and directed case that tests/test_gpu_topology_fuzz.py
uses: the generators give what they promise (indices in range, manifold meshes, more than 256 long buckets, the chunk
seams, at most 2 % of a mesh's edges at the dihedral clamp), and every numpy reference agrees with the project's CPU
composition on the same input -- integer tables bit for bit, floats by the suite's measure within 4x the fp32 CPU
composition's own error against the fp64 composition (floor 1e-6; ``within_the_rule`` says what a sequential sum over
a hub gets on top), and the sequential references that run in fp64 agree with the fp64 composition to 1e-11 when fed
fp64 inputs.  So the references are pinned before a GPU is involved."""
import functools

import numpy as np
import pytest
import torch

import topology_fuzz as T
from pytorch_points_amd import edge_features, knn_edges, mesh_dihedral, mesh_edges, mesh_laplacian
from test_mesh_dihedral_host import BOUNDARY, FLAT, HI, LO, dict_edge_points
from test_mesh_edges_host import np_unique_edges

F32 = np.float32
DEFAULT_SEEDS = range(40)       # the coverage statements below are about the default run


def within_the_rule(what, got, cpu32, ref, longest=0):
    """The standing rule of DESIGN.md "k-NN edge operators": 4x the fp32 CPU composition's error, floor 1e-6.  A
    reference that adds a list of ``longest`` terms one after the other -- the ordered kernels' contract -- also gets
    longest * 2^-24: torch's CPU reductions add pairwise, so at a hub of thousands of terms the composition is far more
    accurate than any sequential sum and 4x its error bounds nothing.  Sequential rounding errors of size u = 2^-24
    relative to partial sums of about sqrt(m) terms accumulate like sqrt(m) * u against the hub's own sum, which the
    measure's denominator is at least; m * u leaves a factor sqrt(m) of room.  This checks the rounding only: the
    formula and the index logic are pinned exactly by running the same numpy code in fp64 (``exactly`` below)."""
    err, base = T.measure(got, ref), T.measure(cpu32, ref)
    assert np.isfinite(got).all() and err <= max(4 * base, 1e-6, longest * 2.0 ** -24), (what, err, base, longest)


def exactly(what, got64, ref, tol=1e-11):
    """the numpy reference run on fp64 inputs against the fp64 composition: sums of at most 2e5 terms in other orders"""
    assert got64.dtype == np.float64 and T.measure(got64, ref) <= tol, (what, T.measure(got64, ref))


def grads(fn, arrays, w, dtype):
    xs = [torch.from_numpy(a).to(dtype).requires_grad_(True) for a in arrays]
    out = fn(*xs)
    got = torch.autograd.grad(out, xs, torch.from_numpy(w).to(dtype))
    return out.detach().numpy(), [g.numpy() for g in got]


# ------------------------------------------------------------------------------------------------------ graphs
@pytest.mark.parametrize("name", T.graph_names())
def test_graph_generator(name):
    for query in (None, False):
        points, idx, q = T.graph_case(name, query)
        again = T.graph_case(name, query)
        assert all(a is None and b is None or np.array_equal(a, b) for a, b in zip((points, idx, q), again))
        b, n, d = points.shape
        assert points.dtype == F32 and idx.dtype == np.int64 and idx.shape[0] == b and np.isfinite(points).all()
        assert idx.min() >= 0 and idx.max() < n
        assert idx.shape[1] * idx.shape[2] <= 200000
        if q is None:
            assert idx.shape[1] == n
        else:
            assert q.shape == (b, idx.shape[1], d) and idx.shape[1] != n and query is None
    if isinstance(name, int):
        points, idx, q, profiles = T.random_graph(name, describe=True)
        n, k = points.shape[1], idx.shape[2]
        for e, profile in enumerate(profiles):
            if profile == "permutation" and q is None:
                assert (T.in_degrees(idx[e:e + 1], n) == k).all()


def test_graph_family_covers_what_it_is_for():
    long_lists = big = queries = mixed = empties = loops = dupes = 0
    profiles_seen = set()
    for seed in DEFAULT_SEEDS:
        points, idx, q, profiles = T.random_graph(seed, describe=True)
        deg = T.in_degrees(idx, points.shape[1])
        profiles_seen.update(profiles)
        long_lists += int((deg > T.LONG).sum())
        big += int((deg > 2 * T.CHUNK).sum())
        queries += q is not None
        mixed += len(set(profiles)) > 1
        empties += int(((deg == 0).any(1) & (deg > T.LONG).any(1)).sum())      # empty buckets among full ones
        if q is None:
            loops += int((idx == np.arange(idx.shape[1])[None, :, None]).sum())
        if idx.shape[2] > 1:
            dupes += int((np.diff(np.sort(idx, -1), axis=-1) == 0).sum())
    assert profiles_seen == set(T.PROFILES)
    assert long_lists > 100 and big >= 3 and queries >= 5 and mixed >= 10 and empties >= 5 and loops and dupes


def test_directed_graphs():
    _, idx, _ = T.many_long_graph()
    deg = T.in_degrees(idx, 3000)[0]
    assert idx.shape[0] == 1 and int((deg > T.LONG).sum()) == 300 > T.LONG_BLOCKS and deg.max() <= 400
    _, idx, _ = T.ladder_graph()
    for e in range(2):
        deg = T.in_degrees(idx, 1500)[e]
        assert sorted(deg[deg >= 256].tolist()) == list(T.LADDER)


def np_graph_backward(op, p, idx, w):
    """the sequential reference in the dtype of p and w"""
    if op == "laplacian":
        return T.np_lap_backward(idx, w)
    squared = op == "squared"
    if p.dtype == F32:
        sq = T.np_edge_sqrlen(p, idx)
    else:
        t = p[np.arange(p.shape[0])[:, None, None], idx] - p[:, :, None, :]
        sq = np.sum(t * t, -1)
    return T.np_len_backward(p, idx, sq if squared else np.sqrt(sq), w, squared, op == "detached")


GRAPH_OPS = {"lengths": lambda x, i: knn_edges.edge_lengths_composition(x, i),
             "squared": lambda x, i: knn_edges.edge_lengths_composition(x, i, squared=True),
             "detached": lambda x, i: knn_edges.edge_lengths_composition(x, i, detach_neighbors=True),
             "laplacian": knn_edges.laplacian_composition}


@pytest.mark.parametrize("name", T.graph_names())
def test_knn_edge_references_against_the_compositions(name):
    p, idx, _ = T.graph_case(name, query=False)
    ti = torch.from_numpy(idx)
    rng = np.random.default_rng(3)
    longest = int(T.in_degrees(idx, p.shape[1]).max()) + idx.shape[2]
    for op, comp in GRAPH_OPS.items():
        w = rng.uniform(-1, 1, size=p.shape if op == "laplacian" else idx.shape).astype(F32)
        fn = lambda x: comp(x, ti)   # noqa: E731
        out64, (ref,) = grads(fn, [p], w, torch.float64)
        out32, (cpu32,) = grads(fn, [p], w, torch.float32)
        if op == "laplacian":
            forward = T.np_laplacian(p, idx)
        else:
            forward = T.np_edge_sqrlen(p, idx)
            forward = forward if op == "squared" else np.sqrt(forward)
        assert forward.dtype == F32
        within_the_rule((op, "forward"), forward, out32, out64)
        within_the_rule((op, "backward"), np_graph_backward(op, p, idx, w), cpu32, ref, longest)
        # (np_len_backward rounds the unsquared form's coefficient g / length to fp32 whatever the inputs: one 2^-24)
        exactly((op, "backward"), np_graph_backward(op, p.astype(np.float64), idx, w.astype(np.float64)), ref,
                1e-11 if op in ("squared", "laplacian") else 2.0 ** -23)


@pytest.mark.parametrize("name", T.graph_names())
def test_edge_feature_references_against_the_composition(name):
    p, idx, q = T.graph_case(name)
    x = np.ascontiguousarray(p.transpose(0, 2, 1))
    qq = None if q is None else np.ascontiguousarray(q.transpose(0, 2, 1))
    ti = torch.from_numpy(idx)
    c = x.shape[1]
    w = np.random.default_rng(4).uniform(-1, 1, size=(x.shape[0], 2 * c) + idx.shape[1:]).astype(F32)
    for dtype in (torch.float32, torch.bfloat16):
        xr, qr, wr = T.round_to(x, dtype), None if qq is None else T.round_to(qq, dtype), T.round_to(w, dtype)
        args = [torch.from_numpy(xr).to(dtype)] + ([] if qr is None else [torch.from_numpy(qr).to(dtype)])
        out = edge_features.composition(args[0], ti, *args[1:]).float().numpy()
        want = T.np_ef_forward(xr, idx, xr if qr is None else qr, dtype)
        assert np.array_equal(out.view(np.uint32), np.ascontiguousarray(want).view(np.uint32))
    fn = lambda *a: edge_features.composition(a[0], ti, *a[1:])   # noqa: E731
    arrays = [x] + ([] if qq is None else [qq])
    _, ref = grads(fn, arrays, w, torch.float64)
    _, cpu32 = grads(fn, arrays, w, torch.float32)
    got = T.np_ef_backward(w, idx, x.shape[2], qq is None, torch.float32)
    longest = int(T.in_degrees(idx, x.shape[2]).max()) + idx.shape[2]
    for what, g, c32, r in zip(("grad_x", "grad_query"), got, cpu32, ref):
        within_the_rule(what, g, c32, r, longest)


@pytest.mark.parametrize("name", T.graph_names())
def test_poisoned_graphs(name):
    _, idx, q = T.graph_case(name)
    n = T.graph_case(name)[0].shape[1]
    bad, quiet, rows = T.poison_graph(idx, n, 0)
    differs = bad != idx
    assert differs.any() and not differs[rows].any() and set(bad[differs].tolist()) <= {-1, n, 2 ** 31 - 1}
    assert quiet.min() >= 0 and quiet.max() < n and np.array_equal(quiet[rows], idx[rows])
    assert np.array_equal(differs.any(-1), ~rows) and (differs.sum(-1) <= 1).all()


# ------------------------------------------------------------------------------------------------------- soups
@pytest.mark.parametrize("name", T.soup_names())
def test_soup_generator(name):
    faces, n = T.soup_case(name)
    assert np.array_equal(faces, T.soup_case(name)[0])
    assert faces.dtype == np.int64 and faces.ndim == 3 and faces.shape[2] == 3
    assert faces.min() >= 0 and faces.max() < n and 3 * faces.shape[1] <= 250000


def test_soup_family_covers_what_it_is_for():
    over_long = over_chunk = isolated = duplicated = repeated = both = 0
    sizes = set()
    for seed in DEFAULT_SEEDS:
        faces, n = T.random_soup(seed)
        sizes.add((n, 3 * faces.shape[1]))
        for f in faces:
            half, corners = T.bucket_sizes_of_faces(f, n)
            over_long += int((corners > T.LONG).sum() + (half > T.LONG).sum())
            over_chunk += int((corners > T.CHUNK).sum() + (half > T.CHUNK).sum())
            isolated += int((corners == 0).sum())
            keys = np.sort(f, 1)
            duplicated += f.shape[0] - np.unique(f, axis=0).shape[0]
            both += np.unique(f, axis=0).shape[0] - np.unique(keys, axis=0).shape[0]
            repeated += int((f[:, 0] == f[:, 1]).sum())
            assert (corners == 0).any()
    assert over_long > 100 and over_chunk >= 10 and isolated and duplicated and both > 0 and repeated
    assert {n % T.CHUNK for n, _ in sizes} >= {0, 1, T.CHUNK - 1}
    assert {t % T.CHUNK for _, t in sizes} >= {0, 1, T.CHUNK - 1}


def test_directed_soups():
    faces, n = T.many_long_faces()
    half, corners = T.bucket_sizes_of_faces(faces[0], n)
    assert faces.shape[0] == 1 and int((half > T.LONG).sum()) == 300 > T.LONG_BLOCKS
    assert int((corners > T.LONG).sum()) == 300 and corners.max() <= 400
    edges, n = T.many_long_edges()
    ends = np.bincount(edges.reshape(-1), minlength=n)
    assert int((ends > T.LONG).sum()) == 300 > T.LONG_BLOCKS and ends.max() <= 400 and 2 * edges.shape[0] <= 200000
    totals = set()
    for name, (f, nv) in T.SEAMS.items():
        faces, n = T.seam_faces(name)
        assert faces.shape == (1, f, 3) and n == nv and n in (1024, 1025, 2048)
        totals.add(3 * f % T.CHUNK)
        seams, across = T.seams_straddled(faces[0])
        assert across.all() and seams.size == 3 * f // T.CHUNK - (3 * f % T.CHUNK == 0)
        pairs = T.sorted_half_edges(faces[0])
        for s in seams:                                    # stated again without the helper
            assert s % 1024 == 0 and tuple(pairs[s - 1]) == tuple(pairs[s])
    assert totals == {T.CHUNK - 1, 0, 1}
    assert sum(T.seams_straddled(T.seam_faces(name)[0][0])[0].size for name in T.SEAMS) >= 4


@pytest.mark.parametrize("name", T.soup_names())
def test_soup_references_against_the_compositions(name):
    faces, n = T.soup_case(name)
    b = faces.shape[0]
    tf = torch.from_numpy(faces)
    rng = np.random.default_rng(5)
    # integer tables, bit for bit
    topo = mesh_edges.MeshEdges.from_faces(tf, n)
    corners = mesh_laplacian.MeshCorners.from_faces(tf, n)
    for e in range(b):
        want = np_unique_edges(faces[e])
        assert np.array_equal(mesh_edges.unique_edges_composition(tf[e]).numpy(), want)
        assert np.array_equal(topo.edge_list(e).numpy(), want)
        for got, ref in zip((corners.start[e], corners.codes[e], corners.nbr[e]), T.np_corners(faces[e], n)):
            assert got.dtype == torch.int32 and np.array_equal(got.numpy(), ref)
    # the squared lengths' backward
    v = rng.standard_normal((b, n, 3)).astype(F32)
    g = rng.uniform(-1, 1, size=(b, topo.capacity)).astype(F32)
    fn = lambda x: mesh_edges.sqrlen_composition(x, topo)   # noqa: E731
    _, (ref,) = grads(fn, [v], g, torch.float64)
    _, (cpu32,) = grads(fn, [v], g, torch.float32)
    edges_of = lambda e: np_unique_edges(faces[e])   # noqa: E731
    longest = max(int(np.bincount(edges_of(e).reshape(-1), minlength=n).max()) for e in range(b))
    within_the_rule("sqrlen backward", T.np_backward(v, edges_of, g), cpu32, ref, longest)
    exactly("sqrlen backward", T.np_backward(v.astype(np.float64), edges_of, g.astype(np.float64)), ref)
    # the applies
    weights = rng.uniform(-0.5, 2.0, size=(b, faces.shape[1], 3)).astype(F32)
    tables = [T.np_corners(faces[e], n) for e in range(b)]

    def apply(x, mode):
        return np.stack([T.np_apply(x[e], tables[e][0], tables[e][2], tables[e][1],
                                    weights[e] if mode == 2 else None, mode) for e in range(b)])

    longest = 2 * max(int(np.diff(t[0]).max()) for t in tables)
    uni = lambda x: mesh_laplacian.uniform_laplacian_composition(x, corners)   # noqa: E731
    out64, (ref,) = grads(uni, [v], v, torch.float64)
    out32, (cpu32,) = grads(uni, [v], v, torch.float32)
    within_the_rule("uniform forward", apply(v, 0), out32, out64, longest)
    within_the_rule("uniform backward", apply(v, 1), cpu32, ref, longest)
    out64 = mesh_laplacian.cot_laplacian_composition(torch.from_numpy(v).double(), corners,
                                                     torch.from_numpy(weights).double()).numpy()
    out32 = mesh_laplacian.cot_laplacian_composition(torch.from_numpy(v), corners, torch.from_numpy(weights)).numpy()
    within_the_rule("cotangent apply", apply(v, 2), out32, out64, longest)


def test_edge_list_references_against_the_composition():
    edges, n = T.many_long_edges()
    topo = mesh_edges.MeshEdges.from_edges(torch.from_numpy(edges), n)
    rng = np.random.default_rng(6)
    v = rng.standard_normal((2, n, 3)).astype(F32)
    g = rng.uniform(-1, 1, size=(2, topo.capacity)).astype(F32)
    fn = lambda x: mesh_edges.sqrlen_composition(x, topo)   # noqa: E731
    _, (ref,) = grads(fn, [v], g, torch.float64)
    _, (cpu32,) = grads(fn, [v], g, torch.float32)
    within_the_rule("sqrlen backward", T.np_backward(v, lambda e: edges, g), cpu32, ref, 400)
    exactly("sqrlen backward", T.np_backward(v.astype(np.float64), lambda e: edges, g.astype(np.float64)), ref)
    start, entries = T.incidence_of(edges, n)
    flat = edges.reshape(-1)
    for vertex in (int(np.argmax(np.diff(start))), 0, n - 1):
        assert np.array_equal(entries[start[vertex]:start[vertex + 1]], np.flatnonzero(flat == vertex))


# ---------------------------------------------------------------------------------------------------- manifold
@functools.lru_cache(maxsize=None)
def manifold(seed):
    v, faces = T.random_manifold(seed)
    return v, faces, [dict_edge_points(f)[0] for f in faces]      # (the dict build asserts <= 2 faces on an edge)


@pytest.mark.parametrize("seed", T.manifold_names())
def test_manifold_generator(seed):
    v, faces, tables = manifold(seed)
    again = T.random_manifold(seed)
    assert np.array_equal(v, again[0]) and np.array_equal(faces, again[1])
    b, n, _ = v.shape
    assert v.dtype == F32 and faces.dtype == np.int64 and faces.shape[0] == b and np.isfinite(v).all()
    assert faces.min() >= 0 and faces.max() < n and 12 * faces.shape[1] <= 200000
    for e in range(b):
        f = faces[e]
        assert (f[:, 0] != f[:, 1]).all() and (f[:, 1] != f[:, 2]).all() and (f[:, 0] != f[:, 2]).all()
        assert np.bincount(f.reshape(-1), minlength=n).min() == 0                 # isolated vertices
        table = tables[e]
        assert (table[:, 2] == table[:, 3]).any()                                 # boundary edges
        assert np.array_equal(mesh_dihedral.edge_points_composition(torch.from_numpy(f)).numpy(), table)
        assert np.array_equal(table[:, :2], np_unique_edges(f))
        start, entries = T.incidence_of(table, n)
        hub = int(np.argmax(np.diff(start)))
        assert np.array_equal(entries[start[hub]:start[hub + 1]], np.flatnonzero(table.reshape(-1) == hub))


@pytest.mark.parametrize("seed", T.manifold_names())
def test_dihedral_cap_with_the_fp64_composition_alone(seed):
    """at most 2 % of a mesh's edges sit at the clamp, and at_the_clamp names exactly the interior edges at which the
    fp64 composition returns one of the clamp's two constants"""
    v, faces, tables = manifold(seed)
    topo = mesh_dihedral.MeshEdgePoints.from_faces(torch.from_numpy(faces), v.shape[1])
    angle = mesh_dihedral.dihedral_composition(torch.from_numpy(v).double(), topo).numpy()
    for e, table in enumerate(tables):
        left_out = T.at_the_clamp(v[e], table)
        assert left_out.mean() <= 0.02, (e, int(left_out.sum()), table.shape[0])
        count = table.shape[0]
        assert topo.count(e) == count and (angle[e, count:] == 0).all()
        interior = table[:, 2] != table[:, 3]
        clamped = (angle[e, :count] == FLAT) | (angle[e, :count] == BOUNDARY)
        assert np.array_equal(clamped & interior, left_out)
        assert (angle[e, :count][~interior] == BOUNDARY).all()
        d = np.clip(T.unclamped_dot64(v[e], table), LO, HI)
        np.testing.assert_allclose(angle[e, :count], np.pi - np.arccos(d), rtol=0, atol=1e-9)


def test_manifold_family_covers_what_it_is_for():
    longest = 0
    lists_over_long = deleted = 0
    for seed in DEFAULT_SEEDS:
        v, faces, tables = manifold(seed)
        for table in tables:
            sizes = np.diff(T.incidence_of(table, v.shape[1])[0])
            longest = max(longest, int(sizes.max()))
            lists_over_long += int((sizes > T.LONG).sum())
        deleted += faces.shape[1] not in T.MANIFOLD_F
    assert longest > 4 * T.CHUNK and lists_over_long >= 20 and deleted >= 10
