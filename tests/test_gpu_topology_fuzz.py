"""Every operator that stands on csrc/bucket_lists.h's count / scan / fill / sort chain -- knn_edge_lengths,
knn_laplacian, knn_edge_features, the mesh unique edges, edge and corner incidence with the Laplacian applies, the edge
points and dihedral angles -- on the seeded random topologies and directed cases of tests/topology_fuzz.py: random
in-degree profiles (uniform, Zipf, permutations, all-to-one, hubs), query graphs with P != N, soups with hubs, duplicated
faces and isolated vertices, manifold meshes of grids, cones, tori, tetrahedra and fans; more than 256 long buckets, a
ladder of list lengths round the sort's thresholds, and sizes on the scans' chunk seams.  The contracts are exact --
integer tables bit-equal to numpy, ordered backwards bit-equal to a sequential loop -- so a single wrong bit fails;
default-mode backwards and the dihedral angles are measured against the fp64 CPU composition with bounds taken from
the fp32 CPU composition on the same input at run time.  tests/test_topology_fuzz_host.py pins the generators and the
references without a GPU.  PP_FUZZ_SEEDS scales the seed count as in test_gpu_fuzz.py (40 a family by default)."""
import contextlib

import numpy as np
import pytest
import torch

import topology_fuzz as T
from pytorch_points_amd import edge_features, knn_edges, mesh_dihedral, mesh_edges, mesh_laplacian
from test_mesh_dihedral_host import HI, LO
from test_mesh_edges_host import np_unique_edges

pytestmark = pytest.mark.gpu

F32 = np.float32
EPS32 = 2.0 ** -23
ROUNDING = {torch.float32: 0.0, torch.bfloat16: 2.0 ** -8}        # test_gpu_edge_features.py's
BAD_VALUES = (-1, None, 2 ** 31 - 1)                               # None: the vertex count


def dev_t(a, dtype=None, grad=False):
    t = torch.from_numpy(np.ascontiguousarray(a)).to("cuda")
    if dtype is not None:
        t = t.to(dtype)
    return t.requires_grad_(grad)


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


@contextlib.contextmanager
def deterministic():
    torch.use_deterministic_algorithms(True)
    try:
        yield
    finally:
        torch.use_deterministic_algorithms(False)


def grad_of(fn, p, idx, w, device, dtype):
    x = torch.from_numpy(p).to(device=device, dtype=dtype).requires_grad_(True)
    out = fn(x, torch.from_numpy(idx).to(device))
    g, = torch.autograd.grad(out, x, torch.from_numpy(w).to(device=device, dtype=dtype))
    return g.cpu().numpy()


def assert_within_the_rule(what, got, cpu32, ref, extra=0.0):
    """test_gpu_knn_edges.py's bound: max(4 x the fp32 CPU composition's error by the same measure on the same input,
    1e-6), computed here, at run time, from the two CPU compositions alone"""
    err, base = T.measure(got, ref), T.measure(cpu32, ref)
    bound = extra + max(4 * base, 1e-6)
    print("%s: error %.3g, fp32 CPU composition %.3g, bound %.3g" % (what, err, base, bound))
    assert np.isfinite(got).all() and err <= bound, (what, err, bound)


# ------------------------------------------------------------------------------------------------------ graphs
KNN_OPS = [("lengths", lambda x, i: knn_edges.knn_edge_lengths(x, i), knn_edges.edge_lengths_composition, "k"),
           ("squared", lambda x, i: knn_edges.knn_edge_lengths(x, i, squared=True),
            lambda x, i: knn_edges.edge_lengths_composition(x, i, squared=True), "k"),
           ("detached", lambda x, i: knn_edges.knn_edge_lengths(x, i, detach_neighbors=True),
            lambda x, i: knn_edges.edge_lengths_composition(x, i, detach_neighbors=True), "k"),
           ("laplacian", knn_edges.knn_laplacian, knn_edges.laplacian_composition, "d")]


@pytest.mark.parametrize("name", T.graph_names())
def test_fuzz_knn_edges(cuda, name):
    p, idx, _ = T.graph_case(name, query=False)
    tp, ti = dev_t(p), dev_t(idx)
    sq = T.np_edge_sqrlen(p, idx)
    # forwards, bit for bit
    for indices in (ti, ti.int()):
        assert np.array_equal(bits(knn_edges.knn_edge_lengths(tp, indices, squared=True).cpu().numpy()), bits(sq))
        assert np.array_equal(bits(knn_edges.knn_edge_lengths(tp, indices).cpu().numpy()), bits(np.sqrt(sq)))
        assert np.array_equal(bits(knn_edges.knn_laplacian(tp, indices).cpu().numpy()), bits(T.np_laplacian(p, idx)))
    assert np.array_equal(bits(knn_edges.knn_edge_lengths(tp, ti, detach_neighbors=True).cpu().numpy()), bits(np.sqrt(sq)))
    # ordered backwards: the sequential loop's bits, twice
    rng = np.random.default_rng(4)
    wk = rng.uniform(-1, 1, size=idx.shape).astype(F32)
    wd = rng.uniform(-1, 1, size=p.shape).astype(F32)
    with deterministic():
        for squared in (False, True):
            out = sq if squared else np.sqrt(sq)
            for detach in (False, True):
                fn = lambda x, i: knn_edges.knn_edge_lengths(x, i, squared=squared, detach_neighbors=detach)  # noqa: E731
                a = grad_of(fn, p, idx, wk, "cuda", torch.float32)
                assert np.array_equal(bits(a), bits(grad_of(fn, p, idx, wk, "cuda", torch.float32))), (squared, detach)
                assert np.array_equal(bits(a), bits(T.np_len_backward(p, idx, out, wk, squared, detach))), (squared, detach)
        a = grad_of(knn_edges.knn_laplacian, p, idx, wd, "cuda", torch.float32)
        assert np.array_equal(bits(a), bits(grad_of(knn_edges.knn_laplacian, p, idx, wd, "cuda", torch.float32)))
        assert np.array_equal(bits(a), bits(T.np_lap_backward(idx, wd)))
    # default-mode backwards against the fp64 composition
    rng = np.random.default_rng(3)
    for op, hip, comp, wshape in KNN_OPS:
        w = rng.uniform(-1, 1, size=idx.shape if wshape == "k" else p.shape).astype(F32)
        ref = grad_of(comp, p, idx, w, "cpu", torch.float64)
        cpu32 = grad_of(comp, p, idx, w, "cpu", torch.float32)
        assert_within_the_rule("%s %s" % (name, op), grad_of(hip, p, idx, w, "cuda", torch.float32), cpu32, ref)


def ef_grads(x, idx, q, w, dtype, device, fn, index_dtype=torch.int64):
    """[grad_x, grad_query | None] as numpy in the dtype's values"""
    tx = torch.from_numpy(x).to(device=device, dtype=dtype).requires_grad_(True)
    tq = None if q is None else torch.from_numpy(q).to(device=device, dtype=dtype).requires_grad_(True)
    out = fn(tx, torch.from_numpy(idx).to(device=device, dtype=index_dtype), tq)
    got = torch.autograd.grad(out, (tx,) if q is None else (tx, tq), torch.from_numpy(w).to(device=device, dtype=dtype))
    wide = torch.float64 if dtype is torch.float64 else torch.float32
    return [t.to(wide).cpu().numpy() for t in got] + ([None] if q is None else [])


def ef_inputs(name, dtype):
    p, idx, q = T.graph_case(name)
    x = T.round_to(np.ascontiguousarray(p.transpose(0, 2, 1)), dtype)
    qq = None if q is None else T.round_to(np.ascontiguousarray(q.transpose(0, 2, 1)), dtype)
    return x, idx, qq


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("name", T.graph_names())
def test_fuzz_edge_features(cuda, name, dtype):
    x, idx, q = ef_inputs(name, dtype)
    c, (p, k) = x.shape[1], idx.shape[1:]
    tx, tq = dev_t(x, dtype), None if q is None else dev_t(q, dtype)
    want = T.np_ef_forward(x, idx, x if q is None else q, dtype)
    composed = edge_features.composition(tx, dev_t(idx), tq)
    w = T.round_to(np.random.default_rng(4).uniform(-1, 1, size=(x.shape[0], 2 * c, p, k)), dtype)
    ordered = T.np_ef_backward(w, idx, x.shape[2], q is None, dtype)
    for index_dtype in (torch.int64, torch.int32):
        out = edge_features.knn_edge_features(tx, dev_t(idx).to(index_dtype), tq)
        assert out.dtype == dtype and torch.equal(out, composed)
        assert np.array_equal(bits(out.float().cpu().numpy()), bits(want))
        with deterministic():
            a = ef_grads(x, idx, q, w, dtype, "cuda", edge_features.knn_edge_features, index_dtype)
            again = ef_grads(x, idx, q, w, dtype, "cuda", edge_features.knn_edge_features, index_dtype)
        for g, g2, e in zip(a, again, ordered):
            if g is not None:
                assert np.array_equal(bits(g), bits(g2)) and np.array_equal(bits(g), bits(e))
    # default mode: test_gpu_edge_features.py's bound, one rounding of the reference to a 16-bit type on top
    w = T.round_to(np.random.default_rng(3).uniform(-1, 1, size=w.shape), dtype)
    ref = ef_grads(x, idx, q, w, torch.float64, "cpu", edge_features.composition)
    cpu32 = ef_grads(x, idx, q, w, torch.float32, "cpu", edge_features.composition)
    got = ef_grads(x, idx, q, w, dtype, "cuda", edge_features.knn_edge_features)
    for what, g, r, c32 in zip(("grad_x", "grad_query"), got, ref, cpu32):
        if g is not None:
            assert_within_the_rule("%s %s %s" % (name, dtype, what), g, c32, r, ROUNDING[dtype])


def by_row(a):
    """(B,C,P[,K]) -> (B,P[,K],C): a (B,P) mask then picks rows"""
    return np.moveaxis(a, 1, -1)


@pytest.mark.parametrize("name", T.graph_names())
def test_fuzz_graphs_with_indices_out_of_range(cuda, name):
    """-1, N and 2^31 - 1 in rows that point into the longest list: NaN exactly where DESIGN.md section 4 says, the bits
    of the clean run everywhere else.  The kernels only compare such an index."""
    p, idx, _ = T.graph_case(name, query=False)
    n = p.shape[1]
    bad, quiet, rows = T.poison_graph(idx, n, 1)
    isnan = bad != idx
    tp = dev_t(p)
    rng = np.random.default_rng(6)
    wk = rng.uniform(-1, 1, size=idx.shape).astype(F32)
    wd = rng.uniform(-1, 1, size=p.shape).astype(F32)
    with deterministic():
        for squared in (False, True):
            fn = lambda x, i: knn_edges.knn_edge_lengths(x, i, squared=squared)   # noqa: E731
            out = fn(tp, dev_t(bad)).cpu().numpy()
            clean = fn(tp, dev_t(idx)).cpu().numpy()
            assert np.array_equal(np.isnan(out), isnan) and np.array_equal(bits(out[~isnan]), bits(clean[~isnan]))
            g = grad_of(fn, p, bad, wk, "cuda", torch.float32)
            gq = grad_of(fn, p, quiet, wk * rows[..., None], "cuda", torch.float32)
            assert np.isnan(g[~rows]).all() and np.array_equal(bits(g[rows]), bits(gq[rows]))
        lap = knn_edges.knn_laplacian(tp, dev_t(bad)).cpu().numpy()
        clean = knn_edges.knn_laplacian(tp, dev_t(idx)).cpu().numpy()
        assert np.array_equal(np.isnan(lap), np.broadcast_to(~rows[..., None], lap.shape))
        assert np.array_equal(bits(lap[rows]), bits(clean[rows]))
        g = grad_of(knn_edges.knn_laplacian, p, bad, wd, "cuda", torch.float32)
        gq = grad_of(knn_edges.knn_laplacian, p, quiet, wd * rows[..., None], "cuda", torch.float32)
        assert np.isnan(g[~rows]).all() and np.array_equal(bits(g[rows]), bits(gq[rows]))
    # the edge features over the drawn form of the same case (with its query, where it has one), int32 indices
    x, idx, q = ef_inputs(name, torch.float32)
    n, c = x.shape[2], x.shape[1]
    bad, quiet, rows = T.poison_graph(idx, n, 2)
    isnan = np.zeros((x.shape[0], 2 * c) + idx.shape[1:], bool)
    isnan[:, c:] = (bad != idx)[:, None]
    tx, tq = dev_t(x), None if q is None else dev_t(q)
    out = edge_features.knn_edge_features(tx, dev_t(bad).int(), tq).cpu().numpy()
    clean = edge_features.knn_edge_features(tx, dev_t(idx).int(), tq).cpu().numpy()
    assert np.array_equal(np.isnan(out), isnan) and np.array_equal(bits(out[~isnan]), bits(clean[~isnan]))
    w = rng.uniform(-1, 1, size=out.shape).astype(F32)
    wq = w.copy()
    wq[:, c:] = np.where(rows[:, None, :, None], wq[:, c:], 0)
    with deterministic():
        g = ef_grads(x, bad, q, w, torch.float32, "cuda", edge_features.knn_edge_features, torch.int32)
        gr = ef_grads(x, quiet, q, wq, torch.float32, "cuda", edge_features.knn_edge_features, torch.int32)
    if q is None:
        assert np.isnan(by_row(g[0])[~rows]).all()
        assert np.array_equal(bits(by_row(g[0])[rows]), bits(by_row(gr[0])[rows]))
    else:
        assert np.array_equal(bits(g[0]), bits(gr[0]))
        assert np.isnan(by_row(g[1])[~rows]).all()
        assert np.array_equal(bits(by_row(g[1])[rows]), bits(by_row(gr[1])[rows]))


# ------------------------------------------------------------------------------------------------------- soups
def assert_topology(topo, b, want):
    """batch element b of topo: rows, padding and counts, bit for bit"""
    edges = topo.edges[b].cpu().numpy()
    assert topo.counts_host[b] == want.shape[0] and int(topo.counts[b]) == want.shape[0]
    assert edges.dtype == np.int64 and np.array_equal(edges[:want.shape[0]], want)
    assert (edges[want.shape[0]:] == -1).all()


def assert_incidence(start, entries, b, table, n):
    """the vertex lists of batch element b over its table (E,COLS): exactly the ascending codes"""
    want_start, want = T.incidence_of(table, n)
    assert np.array_equal(start[b], want_start)
    assert np.array_equal(entries[b, :want.size], want)


def assert_sqrlen(topo, edges_of, n, batch, seed):
    """mesh_edge_sqrlen over topo: the forward's bits, and the backward's bits of the sequential loop, on every run"""
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((batch, n, 3)).astype(F32)
    g = rng.uniform(-1, 1, size=(batch, topo.capacity)).astype(F32)
    want = T.np_backward(v, edges_of, g)

    def run():
        x = dev_t(v, grad=True)
        out = mesh_edges.mesh_edge_sqrlen(x, topo)
        grad, = torch.autograd.grad(out, x, dev_t(g))
        return out.detach().cpu().numpy(), grad.cpu().numpy()

    out, first = run()
    for b in range(batch):
        e = edges_of(b)
        assert np.array_equal(bits(out[b, :e.shape[0]]), bits(T.np_sqdist(v[b, e[:, 0]] - v[b, e[:, 1]])))
        assert (out[b, e.shape[0]:] == 0).all() and not np.signbit(out[b, e.shape[0]:]).any()
    assert np.array_equal(bits(first), bits(want))
    assert first.tobytes() == run()[1].tobytes()
    with deterministic():
        assert first.tobytes() == run()[1].tobytes()


@pytest.mark.parametrize("name", T.soup_names())
def test_fuzz_soup_edges(cuda, name):
    faces, n = T.soup_case(name)
    batch = faces.shape[0]
    tf = dev_t(faces)
    unique = [np_unique_edges(f) for f in faces]
    runs = []
    for _ in range(3):
        topo = mesh_edges.MeshEdges.from_faces(tf, n)
        start, entries = (t.cpu().numpy() for t in topo.incidence())
        runs.append((topo.edges.cpu().numpy().tobytes(), start.tobytes())
                    + tuple(entries[b, :2 * unique[b].shape[0]].tobytes() for b in range(batch)))
    assert runs[0] == runs[1] == runs[2]
    assert topo.batch == batch and topo.edges.shape == (batch, 3 * faces.shape[1], 2)
    assert start.shape == (batch, n + 1) and entries.shape == (batch, 6 * faces.shape[1])
    for b in range(batch):
        assert_topology(topo, b, unique[b])
        assert_incidence(start, entries, b, unique[b], n)
    assert_sqrlen(topo, lambda b: unique[b], n, batch, 7)


@pytest.mark.parametrize("name", T.soup_names())
def test_fuzz_soup_corners_and_applies(cuda, name):
    faces, n = T.soup_case(name)
    batch = faces.shape[0]
    tf = dev_t(faces)
    builds = [mesh_laplacian.MeshCorners.from_faces(tf, n) for _ in range(3)]
    corners = builds[0]
    tables = [T.np_corners(f, n) for f in faces]
    for b in range(batch):
        for got, want in zip((corners.start[b], corners.codes[b], corners.nbr[b]), tables[b]):
            assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want)
    as_bytes = [tuple(t.cpu().numpy().tobytes() for t in (c.start, c.codes, c.nbr)) for c in builds]
    assert as_bytes[0] == as_bytes[1] == as_bytes[2]
    rng = np.random.default_rng(8)
    x = rng.standard_normal((batch, n, 3)).astype(F32)
    g = rng.uniform(-1, 1, size=x.shape).astype(F32)
    weights = rng.uniform(-0.5, 2.0, size=(batch, faces.shape[1], 3)).astype(F32)     # random finite weights
    tw = dev_t(weights)

    def reference(values, mode):
        return np.stack([T.np_apply(values[b], tables[b][0], tables[b][2], tables[b][1],
                                    weights[b] if mode == 2 else None, mode) for b in range(batch)])

    for what, op, fwd_mode, bwd_mode in (("uniform", lambda t: mesh_laplacian.mesh_uniform_laplacian(t, corners), 0, 1),
                                         ("cot", lambda t: mesh_laplacian.mesh_cot_laplacian(t, corners, tw), 2, 2)):
        def run():
            t = dev_t(x, grad=True)
            out = op(t)
            grad, = torch.autograd.grad(out, t, dev_t(g))
            return out.detach().cpu().numpy(), grad.cpu().numpy()

        out, grad = run()
        assert np.array_equal(bits(out), bits(reference(x, fwd_mode))), what
        assert np.array_equal(bits(grad), bits(reference(g, bwd_mode))), what
        with deterministic():
            again = run()
        assert out.tobytes() == again[0].tobytes() and grad.tobytes() == again[1].tobytes()


def test_many_long_lists_in_an_edge_list(cuda):
    edges, n = T.many_long_edges()
    topo = mesh_edges.MeshEdges.from_edges(dev_t(edges), n)
    start, entries = (t.cpu().numpy() for t in topo.incidence())
    assert topo.batch == 1 and topo.counts_host == (edges.shape[0],)
    assert_incidence(start, entries, 0, edges, n)
    assert_sqrlen(topo, lambda b: edges, n, 2, 9)


def first_face_at_the_longest_list(faces, n):
    """(batch element, face, corner) of the first corner of the last batch element's busiest vertex"""
    b = faces.shape[0] - 1
    hub = int(np.argmax(np.bincount(faces[b].reshape(-1), minlength=n)))
    f, c = np.argwhere(faces[b] == hub)[0]
    return b, int(f), int(c)


@pytest.mark.parametrize("name", [0, 1, 2, "many_long"] + sorted(T.SEAMS))
def test_fuzz_soups_with_an_index_out_of_range(cuda, name):
    """the builds raise as documented -- the bad entry in the longest list, and in a seam case in the duplicated face
    that lies across the seam -- and the next call on the same stream is right"""
    faces, n = T.soup_case(name)
    spots = [first_face_at_the_longest_list(faces, n)]
    if name in T.SEAMS and 3 * faces.shape[1] > T.CHUNK:                 # (1023 half-edges have no seam between them)
        pairs = T.sorted_half_edges(faces[0])
        seam = pairs[T.seams_straddled(faces[0])[0][0]]
        f = int(np.flatnonzero((faces[0] == seam[0]).any(1) & (faces[0] == seam[1]).any(1))[0])
        spots.append((0, f, int(np.flatnonzero(faces[0, f] == seam[0])[0])))
    for i, (b, f, c) in enumerate(spots):
        for value in BAD_VALUES:
            bad = faces.copy()
            bad[b, f, c] = n if value is None else value
            with pytest.raises(IndexError, match="batch element %d" % b):
                mesh_edges.MeshEdges.from_faces(dev_t(bad), n)
            with pytest.raises(IndexError, match="batch element %d" % b):
                mesh_edges.MeshEdges.from_edges(dev_t(bad[:, :, [c, (c + 1) % 3]]), n)
            with pytest.raises(IndexError, match="batch element %d" % b):
                mesh_laplacian.MeshCorners.from_faces(dev_t(bad), n)
            topo = mesh_edges.MeshEdges.from_faces(dev_t(faces), n)
            corners = mesh_laplacian.MeshCorners.from_faces(dev_t(faces), n)
            for e in range(faces.shape[0]):
                assert_topology(topo, e, np_unique_edges(faces[e]))
                assert np.array_equal(corners.codes[e].cpu().numpy(), T.np_corners(faces[e], n)[1])


# ---------------------------------------------------------------------------------------------------- manifold
def cpu_table(faces):
    return mesh_dihedral.edge_points_composition(torch.from_numpy(faces)).numpy()


def forward_ratio(got, ref, d):
    """test_gpu_mesh_dihedral.py's: the largest K for which |got - ref| <= K eps32 / sqrt(1 - d^2) + 4 eps32 pi is
    tight, over the edges"""
    return float(np.max((np.abs(got - ref) - 4 * EPS32 * np.pi) * np.sqrt(1 - d * d) / EPS32, initial=0.0))


def dihedral(v, faces, g, device, dtype):
    """(angles (B,Ecap), gradient (B,N,3)) as float64 numpy"""
    topo = mesh_dihedral.MeshEdgePoints.from_faces(torch.from_numpy(faces).to(device), v.shape[1])
    x = torch.from_numpy(v).to(device=device, dtype=dtype).requires_grad_(True)
    out = mesh_dihedral.mesh_dihedral_angle(x, topo)
    grad, = torch.autograd.grad(out, x, torch.from_numpy(g).to(device=device, dtype=dtype))
    return out.detach().double().cpu().numpy(), grad.double().cpu().numpy()


@pytest.mark.parametrize("seed", T.manifold_names())
def test_fuzz_manifold_tables_and_dihedral_angles(cuda, seed):
    """The table and its vertex lists bit for bit; then the measure of
    test_forward_and_backward_against_the_fp64_composition with K = 4 x the fp32 CPU composition's K and a gradient
    bound of 4 x its error, both computed here on the same input.  An interior edge whose fp64 dot the clamp replaces
    (topology_fuzz.at_the_clamp; at most 2 % of a mesh's edges) is left out of the value comparison only."""
    v, faces = T.random_manifold(seed)
    batch, n, _ = v.shape
    tf = dev_t(faces)
    tables = [cpu_table(f) for f in faces]
    runs = []
    for _ in range(2):
        topo = mesh_dihedral.MeshEdgePoints.from_faces(tf, n)
        start, entries = (t.cpu().numpy() for t in topo.incidence())
        runs.append((topo.edge_points.cpu().numpy().tobytes(), start.tobytes())
                    + tuple(entries[b, :4 * tables[b].shape[0]].tobytes() for b in range(batch)))
    assert runs[0] == runs[1]
    assert topo.batch == batch and topo.edge_points.shape == (batch, 3 * faces.shape[1], 4)
    for b in range(batch):
        table = topo.edge_points[b].cpu().numpy()
        count = tables[b].shape[0]
        assert topo.counts_host[b] == count and int(topo.counts[b]) == count
        assert np.array_equal(table[:count], tables[b]) and (table[count:] == -1).all()
        assert_incidence(start, entries, b, tables[b], n)
    # the angles
    g = np.random.default_rng(15).uniform(-1, 1, size=(batch, topo.capacity)).astype(F32)
    ref, gref = dihedral(v, faces, g, "cpu", torch.float64)
    c32, g32 = dihedral(v, faces, g, "cpu", torch.float32)
    got, ggot = dihedral(v, faces, g, "cuda", torch.float32)
    assert got.shape == ref.shape and ggot.shape == gref.shape and np.isfinite(got).all() and np.isfinite(ggot).all()
    k_cpu = k_hip = 0.0
    for b in range(batch):
        count = tables[b].shape[0]
        left_out = T.at_the_clamp(v[b], tables[b])
        assert left_out.mean() <= 0.02
        keep = ~left_out
        d = np.clip(T.unclamped_dot64(v[b], tables[b]), LO, HI)[keep]
        k_cpu = max(k_cpu, forward_ratio(c32[b, :count][keep], ref[b, :count][keep], d))
        k_hip = max(k_hip, forward_ratio(got[b, :count][keep], ref[b, :count][keep], d))
        assert (got[b, count:] == 0).all() and not np.signbit(got[b, count:]).any()          # padding rows: +0
    scale = np.abs(gref).max()
    e_cpu, e_hip = np.abs(g32 - gref).max() / scale, np.abs(ggot - gref).max() / scale
    print("seed %d: forward K fp32 CPU composition %.3g, HIP %.3g, bound %.3g; gradient error fp32 CPU composition "
          "%.3g, HIP %.3g, bound %.3g" % (seed, k_cpu, k_hip, 4 * k_cpu, e_cpu, e_hip, 4 * e_cpu))
    assert k_hip <= 4 * k_cpu
    assert e_hip <= 4 * e_cpu
    # the same bits on every run, also of the edges left out
    for _ in range(2):
        again = dihedral(v, faces, g, "cuda", torch.float32)
        assert again[0].tobytes() == got.tobytes() and again[1].tobytes() == ggot.tobytes()
    with deterministic():
        again = dihedral(v, faces, g, "cuda", torch.float32)
        assert again[0].tobytes() == got.tobytes() and again[1].tobytes() == ggot.tobytes()


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_fuzz_manifolds_with_an_index_out_of_range(cuda, seed):
    v, faces = T.random_manifold(seed)
    n = v.shape[1]
    b, f, c = first_face_at_the_longest_list(faces, n)
    for value in BAD_VALUES:
        bad = faces.copy()
        bad[b, f, c] = n if value is None else value
        with pytest.raises(IndexError, match="batch element %d" % b):
            mesh_dihedral.MeshEdgePoints.from_faces(dev_t(bad), n)
        topo = mesh_dihedral.MeshEdgePoints.from_faces(dev_t(faces), n)             # the next call on the stream
        for e in range(faces.shape[0]):
            want = cpu_table(faces[e])
            assert np.array_equal(topo.edge_points[e, :want.shape[0]].cpu().numpy(), want)
