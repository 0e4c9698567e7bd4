"""Seeded random topologies and the numpy references for the operators that stand on csrc/bucket_lists.h's count / scan /
fill / sort chain: the k-NN edge lengths and Laplacian, the EdgeConv backward, the mesh unique edges, edge incidence
and corner incidence with the Laplacian applies, the edge points and dihedral angles.  A helper module, not a test
file: tests/test_topology_fuzz_host.py pins the generators and the references on the CPU and
tests/test_gpu_topology_fuzz.py runs the kernels on them.  Every generator takes a seed, returns numpy arrays and is
deterministic; the largest case has about 2e5 list entries per batch element.

The references np_laplacian, np_len_backward, np_lap_backward (tests/test_gpu_knn_edges.py), np_backward (test_gpu_mesh_edges.py),
np_corners, np_apply (test_gpu_mesh_laplacian.py), round_to, np_ef_forward and np_ef_backward
(test_gpu_edge_features.py's np_forward / np_backward) live here, bodies unchanged, and those files import them."""
import os

import numpy as np

from test_mesh_dihedral_host import HI, folded_grid, torus_mesh, zigzag_fan
from test_mesh_edges_host import soup_mesh

F32 = np.float32
LONG = 256          # csrc/bucket_lists.h kBucketLong: a longer bucket is sorted by a whole workgroup
LONG_BLOCKS = 256   # kBucketSortBlocks: the workgroups that share the long buckets
CHUNK = 1024        # kBucketScanThreads: the scans' chunk


def seed_count():
    """test_gpu_fuzz.py's convention: PP_FUZZ_SEEDS (default 100) scales every family; 40 seeds a family by default"""
    return int(os.environ.get("PP_FUZZ_SEEDS", "100")) * 2 // 5


# ------------------------------------------------------------------------------------------ moved references
def np_laplacian(p, idx):
    b = np.arange(p.shape[0])[:, None]
    total = p[b, idx[:, :, 0]]
    for k in range(1, idx.shape[2]):
        total = total + p[b, idx[:, :, k]]
    return -(total / F32(idx.shape[2])) + p


def np_len_backward(p, idx, out, g, squared, detach=False):
    """every point's own edges in ascending k, then the incoming edges in ascending (n, k): fp32, one rounding per
    operation (np.subtract.at applies its operands one after the other, in index order)"""
    bb = np.arange(p.shape[0])[:, None, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        coef = F32(2) * g if squared else np.where(out == 0, F32(0), g / out).astype(F32)
    term = coef[..., None] * (p[:, :, None, :] - p[bb, idx])
    grad = np.zeros_like(p)
    for k in range(idx.shape[2]):
        grad = grad + term[:, :, k]
    if not detach:
        for b in range(p.shape[0]):
            np.subtract.at(grad[b], idx[b].reshape(-1), term[b].reshape(-1, p.shape[2]))
    return grad


def np_lap_backward(idx, g):
    grad = g.copy()
    k = idx.shape[2]
    for b in range(g.shape[0]):
        np.subtract.at(grad[b], idx[b].reshape(-1), np.repeat(g[b] / F32(k), k, axis=0))
    return grad


def np_backward(verts, edges_of, g):
    """the sequential fp32 loop `for e: grad[a] += t_e; grad[b] -= t_e`, t_e = (2 g_e) (v_a - v_b): np.add.at applies
    its operands one after the other, in index order"""
    grad = np.zeros_like(verts)
    for b in range(verts.shape[0]):
        e = edges_of(b)
        t = (F32(2) * g[b, :e.shape[0]])[:, None] * (verts[b, e[:, 0]] - verts[b, e[:, 1]])
        np.add.at(grad[b], e.reshape(-1), np.stack([t, -t], 1).reshape(-1, 3))
    return grad


def np_corners(faces, n):
    """(start (n+1,) int32, codes (L*F,) int32, nbr (L*F,2) int32) of one mesh: a stable sort of the corner keys"""
    deg = faces.shape[1]
    flat = faces.reshape(-1)
    codes = np.argsort(flat, kind="stable")
    start = np.concatenate([[0], np.cumsum(np.bincount(flat, minlength=n))])
    f, c = codes // deg, codes % deg
    nbr = np.stack([faces[f, (c + 1) % deg], faces[f, (c - 1) % deg]], -1)
    return start.astype(np.int32), codes.astype(np.int32), nbr.astype(np.int32)


def np_apply(x, start, nbr, codes, weights, mode):
    """The sequential fp32 loop of one batch element: every vertex's slice in ascending slot order from +0, slot k of
    every vertex at once (numpy's fp32 operations are the kernel's: IEEE, one rounding each).  mode 0: uniform
    forward; 1: uniform backward on the gradient x; 2: cotangent with weights (F,3)."""
    count = (start[1:] - start[:-1]).astype(np.int64)
    div = ((2 * count).astype(F32) + F32(1e-12))[:, None]
    h = (x / div).astype(F32) if mode == 1 else x
    acc = np.zeros_like(x)
    for k in range(int(count.max(initial=0))):
        vs = np.flatnonzero(count > k)
        q = start[vs] + k
        for side in (0, 1):
            other = h[nbr[q, side]]
            if mode == 2:
                f, c = codes[q] // 3, codes[q] % 3
                w = weights[f, (c + 2) % 3 if side == 0 else (c + 1) % 3][:, None]
                acc[vs] = acc[vs] + w * (other - h[vs])
            else:
                acc[vs] = acc[vs] + (h[vs] - other)
    assert acc.dtype == F32
    return (acc / div).astype(F32) if mode == 0 else acc


def round_to(a, dtype):
    """fp32 array -> the nearest values of ``dtype`` (ties to even), held in fp32"""
    import torch
    a = np.ascontiguousarray(a, dtype=F32)
    if dtype is torch.float32:
        return a
    if dtype is torch.float16:
        with np.errstate(over="ignore"):
            return a.astype(np.float16).astype(F32)
    u = a.view(np.uint32).astype(np.uint64)
    u = ((u + 0x7fff + ((u >> 16) & 1)) >> 16) << 16
    return u.astype(np.uint32).view(F32).reshape(a.shape)


def np_ef_forward(x, idx, q, dtype):
    b = np.arange(x.shape[0])[:, None, None, None]
    c = np.arange(x.shape[1])[None, :, None, None]
    centre = np.broadcast_to(q[..., None], q.shape + (idx.shape[2],))
    return np.concatenate([centre, round_to(x[b, c, idx[:, None]] - centre, dtype)], axis=1)


def np_ef_backward(g, idx, n, self_graph, dtype):
    """(grad_x, grad_query) of the ordered form: the centre sums in ascending k from the k = 0 term; grad_x from +0.0
    (the self graph: from the centre sum) with the incoming terms in ascending (p, k), as np.add.at applies them; fp32
    throughout, one rounding to ``dtype`` at the end"""
    c = g.shape[1] // 2
    gc, gd = g[:, :c], g[:, c:]
    t = gc - gd
    gq = t[..., 0]
    for k in range(1, g.shape[3]):
        gq = gq + t[..., k]
    gx = gq.transpose(0, 2, 1).copy() if self_graph else np.zeros((g.shape[0], n, c), F32)
    for b in range(g.shape[0]):
        np.add.at(gx[b], idx[b].reshape(-1), gd[b].reshape(c, -1).T)
    return round_to(gx.transpose(0, 2, 1), dtype), round_to(gq, dtype)


def measure(got, ref):
    """the suite's measure: the largest absolute error over the largest absolute reference"""
    return float(np.abs(got - ref).max(initial=0.0)) / max(float(np.abs(ref).max(initial=0.0)), 1e-30)


# ------------------------------------------------------------------------------------------------- small tools
def fma32(a, b, c):
    """fp32 fused multiply-add in numpy: the product is exact in fp64, the sum is rounded to odd there (TwoSum gives
    the rounding's sign), and 53 bits rounded to odd round to fp32 as the exact value does"""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64)
    s = p + c
    v = s - p
    err = (p - (s - v)) + (c - v)
    even = (np.ascontiguousarray(s).view(np.int64) & 1) == 0
    s = np.where((err != 0) & even, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
    return s.astype(F32)


def np_sqdist(t):
    """the kernels' squared length of the fp32 differences t (...,D): one product, then an fma per further dimension"""
    d2 = t[..., 0] * t[..., 0]
    for c in range(1, t.shape[-1]):
        d2 = fma32(t[..., c], t[..., c], d2)
    return d2


def np_edge_sqrlen(p, idx):
    """knn_edge_lengths(..., squared=True) of in-range indices: (B,N,K) fp32"""
    bb = np.arange(p.shape[0])[:, None, None]
    return np_sqdist(p[bb, idx] - p[:, :, None, :])


def _rotate(faces, shift):
    """every face (row) rotated cyclically by its own shift: orientation kept"""
    return faces[np.arange(faces.shape[0])[:, None], (np.arange(3)[None, :] + shift[:, None]) % 3]


def in_degrees(idx, n):
    """(B,n) in-degree of every vertex of a graph idx (B,P,K)"""
    return np.stack([np.bincount(idx[b].reshape(-1), minlength=n) for b in range(idx.shape[0])])


def sorted_half_edges(faces):
    """the (min,max) pairs of one mesh's 3F half-edges in ascending order: what me_compact_kernel scans"""
    pairs = np.sort(np.stack([faces, faces[:, [1, 2, 0]]], axis=-1), axis=-1).reshape(-1, 2)
    return pairs[np.lexsort((pairs[:, 1], pairs[:, 0]))]


def seams_straddled(faces):
    """the interior positions 1024 j of the sorted half-edges, and at which of them a run of equal pairs lies across"""
    pairs = sorted_half_edges(faces)
    seams = np.arange(CHUNK, pairs.shape[0], CHUNK)
    return seams, np.array([bool((pairs[s - 1] == pairs[s]).all()) for s in seams], bool)


def bucket_sizes_of_faces(faces, n):
    """(half-edge buckets by min-vertex, corner buckets) of one mesh: the two list builds that read faces"""
    pairs = sorted_half_edges(faces)
    return np.bincount(pairs[:, 0], minlength=n), np.bincount(faces.reshape(-1), minlength=n)


def incidence_of(table, n):
    """(start (n+1,), entries) of the vertex lists of a table (E,COLS): ascending COLS*e + slot within a vertex"""
    flat = table.reshape(-1)
    order = np.argsort(flat, kind="stable")
    return np.searchsorted(flat[order], np.arange(n + 1)), order


def unclamped_dot64(v, table):
    """test_mesh_dihedral_host.np_unclamped_dot for every edge at once, fp64: the dot of the two unit normals"""
    v = v.astype(np.float64)
    p = [v[table[:, k]] for k in range(4)]
    na = np.cross(p[2] - p[0], p[1] - p[0])
    nb = np.cross(p[3] - p[1], p[0] - p[1])
    na = na / np.maximum(np.sqrt(np.sum(na * na, -1, keepdims=True)), 1e-12)
    nb = nb / np.maximum(np.sqrt(np.sum(nb * nb, -1, keepdims=True)), 1e-12)
    return np.sum(na * nb, -1)


def at_the_clamp(v, table):
    """the interior edges whose fp64 dot the clamp replaces (|d| >= 1 - 1e-6: two faces within 1.4e-3 rad of flat or
    folded shut).  There fp32 and fp64 may take different sides of the clamp, and the measure's 1 / sqrt(1 - d^2) says
    nothing about an unclamped neighbour: such an edge is left out of the value comparison, only.  A boundary edge --
    one face on both sides, d = -1 whatever the geometry -- is clamped in both precisions by construction and stays
    in, as in test_gpu_mesh_dihedral.py."""
    interior = table[:, 2] != table[:, 3]
    return interior & (np.abs(unclamped_dot64(v, table)) >= HI)


# ------------------------------------------------------------------------------------------------------ graphs
PROFILES = ("uniform", "zipf", "permutation", "one", "hubs1", "hubs3", "hubs300")
GRAPH_N = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2049, 3000)
GRAPH_K = (1, 2, 3, 8, 16, 33)


def _hub_targets(rng, n, size, counts):
    """`size` targets in [0,n): hub i (distinct random vertices) receives counts[i], the rest go anywhere else"""
    counts = list(counts)
    while counts and (sum(counts) > size or len(counts) > n):
        counts.pop()
    verts = rng.permutation(n)
    hubs, others = verts[:len(counts)], verts[len(counts):]
    flat = np.repeat(hubs, counts)
    rest = size - flat.size
    pool = others if others.size else verts
    flat = np.concatenate([flat, pool[rng.integers(0, pool.size, rest)]])
    return flat[rng.permutation(size)].astype(np.int64)


def _targets(rng, profile, n, p, k):
    size = p * k
    if profile == "uniform":
        return rng.integers(0, n, size)
    if profile == "zipf":
        return rng.permutation(n)[(rng.zipf(float(rng.choice([1.2, 1.6, 2.0])), size) - 1) % n]
    if profile == "permutation":     # column k is a permutation: with P == N every in-degree is exactly K
        cols = [np.resize(rng.permutation(n), p) for _ in range(k)]
        return np.stack(cols, 1).reshape(-1)
    if profile == "one":
        return np.full(size, int(rng.integers(0, n)))
    h = int(profile[4:])
    return _hub_targets(rng, n, size, (LONG + 1 + rng.integers(0, 144, h)).tolist())


def random_graph(seed, query=None, describe=False):
    """(points (B,N,D) f32, idx (B,P,K) int64, query (B,P,D) f32 or None).  P == N without a query; ``query``: None
    draws the form from the seed, True / False force it (knn_edges has the self form only).  Every batch element draws
    its own in-degree profile; self-loops and duplicates within a row are sprinkled in (not into a permutation, whose
    in-degrees stay exactly K).  ``describe``: the profiles of the batch elements as a fourth value."""
    rng = np.random.default_rng(41000 + seed)
    b = int(rng.integers(1, 4))
    d = int(rng.choice([3, 5]))
    n = int(rng.choice(GRAPH_N))
    k = int(rng.choice(GRAPH_K))
    with_query = bool(rng.random() < 0.4)
    p_query = int(rng.choice([v for v in (1, 40, 257, 1025, 1500) if v != n]))
    first = int(rng.integers(0, len(PROFILES)))
    if query is not None:
        with_query = bool(query)
    p = p_query if with_query else n
    idx = np.empty((b, p, k), np.int64)
    profiles = []
    for e in range(b):
        profile = PROFILES[(first + e * int(rng.integers(1, len(PROFILES)))) % len(PROFILES)]
        profiles.append(profile)
        idx[e] = np.asarray(_targets(rng, profile, n, p, k), np.int64).reshape(p, k)
        if profile != "permutation":
            rows = np.flatnonzero(rng.random(p) < 0.03)
            for r in rows.tolist():
                if r < n and rng.random() < 0.5:
                    idx[e, r, int(rng.integers(0, k))] = r                       # a self-loop
                else:
                    idx[e, r, int(rng.integers(0, k))] = idx[e, r, 0]            # a duplicate within the row
    points = rng.standard_normal((b, n, d)).astype(F32)
    q = rng.standard_normal((b, p, d)).astype(F32) if with_query else None
    return (points, idx, q, profiles) if describe else (points, idx, q)


def many_long_graph():
    """300 buckets of 257 .. 400 entries in one batch element: more long lists than bucket_sort_long_kernel has
    workgroups, so that its loop makes a second trip"""
    rng = np.random.default_rng(42001)
    n, k = 3000, 33
    idx = _hub_targets(rng, n, n * k, (LONG + 1 + rng.integers(0, 144, 300)).tolist()).reshape(1, n, k)
    return rng.standard_normal((1, n, 3)).astype(F32), idx, None


LADDER = (256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 5000)


def ladder_graph():
    """one graph whose hubs have the in-degrees of LADDER: on both sides of the lane sort's limit, of the in-place
    bitonic network's powers of two and of its thread count; two batch elements, the second the reverse assignment"""
    rng = np.random.default_rng(42002)
    n, k = 1500, 10
    idx = np.stack([_hub_targets(rng, n, n * k, order).reshape(n, k) for order in (LADDER, LADDER[::-1])])
    return rng.standard_normal((2, n, 5)).astype(F32), idx, None


def poison_graph(idx, n, seed):
    """(bad, quiet, rows (B,P) bool): a few entries -1, N and 2^31 - 1 in rows that point into the longest list of
    their batch element, where there is one; ``quiet`` has those rows as loops on one in-range point, which with no
    upstream gradient contribute nothing; ``rows`` is False for them"""
    rng = np.random.default_rng(43000 + seed)
    bad, quiet = idx.copy(), idx.copy()
    rows = np.ones(idx.shape[:2], bool)
    b, p, k = idx.shape
    values = [-1, n, 2 ** 31 - 1]
    for e in range(b):
        hub = int(np.argmax(np.bincount(idx[e].reshape(-1), minlength=n)))
        into = np.flatnonzero((idx[e] == hub).any(1))
        chosen = into[rng.permutation(into.size)[:2]].tolist() + [int(rng.integers(0, p))]
        for i, r in enumerate(sorted(set(chosen))):
            bad[e, r, int(rng.integers(0, k))] = values[(e + i) % 3]
            quiet[e, r] = r % n
            rows[e, r] = False
    return bad, quiet, rows


# ------------------------------------------------------------------------------------------------------- soups
SOUP_N = (300, 1023, 1024, 1025, 2047, 2048, 2049)
SOUP_F = (341, 342, 682, 683, 1023, 1024, 1025, 2048, 2049, 3072)     # 3F on and beside multiples of 1024


def random_soup(seed):
    """(faces (B,F,3) int64, n): vertices by Zipf over a random ranking (hubs beyond 256 and 1024 corners) or uniform,
    with soup_mesh's duplicated faces, both orientations of a face and faces with repeated vertices; the last
    vertices of the ranking belong to no face; n and 3F sit on and beside multiples of 1024"""
    rng = np.random.default_rng(51000 + seed)
    n = int(rng.choice(SOUP_N))
    f = int(rng.choice(SOUP_F))
    b = int(rng.integers(1, 4)) if f <= 2049 else int(rng.integers(1, 3))
    faces = np.empty((b, f, 3), np.int64)
    for e in range(b):
        used = n - int(rng.integers(1, max(2, n // 10)))         # at least one isolated vertex
        rank = rng.permutation(n)[:used]
        a = float(rng.choice([0.0, 1.2, 1.5, 1.8]))
        if a == 0.0:
            tri = rng.integers(0, used, (f, 3))
        else:
            tri = (rng.zipf(a, (f, 3)) - 1) % used
        tri = rank[tri]
        q = f // 8
        tri[q:2 * q] = tri[:q]
        tri[2 * q:3 * q] = tri[:q][:, ::-1]
        tri[3 * q:4 * q, 1] = tri[3 * q:4 * q, 0]
        tri[4 * q:4 * q + 3] = tri[4 * q:4 * q + 3, :1]
        faces[e] = tri[rng.permutation(f)]
    return faces, n


def many_long_edges():
    """(edges (E,2), n): an edge list in which 300 vertices have 257 .. 400 ends each, for the edge incidence"""
    rng = np.random.default_rng(52001)
    n = 3000
    counts = LONG + 1 + rng.integers(0, 144, 300)
    hubs = rng.permutation(n)[:300]
    others = np.setdiff1d(np.arange(n), hubs)
    a = np.repeat(hubs, counts)
    c = others[rng.integers(0, others.size, a.size)]
    flip = rng.random(a.size) < 0.5
    edges = np.where(flip[:, None], np.stack([c, a], 1), np.stack([a, c], 1))
    return edges[rng.permutation(a.size)].astype(np.int64), n


def many_long_faces():
    """(faces (1,F,3), n): every face joins one of 300 hubs -- the lowest vertices, so the min-vertex of two of its
    half-edges -- to two others: 300 corner buckets of 257 .. 290 and 300 half-edge buckets of twice that"""
    rng = np.random.default_rng(52002)
    n = 3000
    counts = LONG + 1 + rng.integers(0, 34, 300)
    hub = np.repeat(np.arange(300), counts)
    tri = np.stack([hub, rng.integers(300, n, hub.size), rng.integers(300, n, hub.size)], 1)
    tri = _rotate(tri, rng.integers(0, 3, hub.size))
    return tri[rng.permutation(hub.size)][None].astype(np.int64), n


SEAMS = {"T1023_n1024": (341, 1024), "T3072_n1025": (1024, 1025), "T2049_n2048": (683, 2048)}


def seam_faces(name):
    """(faces (1,F,3), n): 3F = 1024 j - 1, 1024 j or 1024 j + 1 valid half-edges over n in {1024, 1025, 2048}
    vertices; the first soup (soup_mesh's duplicated faces make the runs) in which a run of equal pairs lies across
    EVERY interior position 1024 j of the sorted half-edges"""
    f, n = SEAMS[name]
    for trial in range(2000):
        faces = soup_mesh(n, f, 53000 + trial)[0]
        if seams_straddled(faces)[1].all():
            return faces[None], n
    raise AssertionError(name)


# ---------------------------------------------------------------------------------------------------- manifold
def _grid_part(rng, faces_wanted):
    # near square: grid_mesh spans the unit square whatever the counts, and folded_grid's heights are set against
    # the finer spacing only, so a long thin grid is flat across its coarse direction
    rows = max(3, int(np.sqrt(faces_wanted / 2.0) * rng.uniform(0.7, 1.4)) + 1)
    cols = max(3, faces_wanted // (2 * (rows - 1)) + 1)
    v, _ = folded_grid(rows, cols, int(rng.integers(1 << 30)))
    r, c = (a.reshape(-1) for a in np.meshgrid(np.arange(rows - 1), np.arange(cols - 1), indexing="ij"))
    v00 = r * cols + c
    one = np.stack([np.stack([v00, v00 + 1, v00 + cols], -1), np.stack([v00 + 1, v00 + cols + 1, v00 + cols], -1)], 1)
    other = np.stack([np.stack([v00, v00 + 1, v00 + cols + 1], -1), np.stack([v00, v00 + cols + 1, v00 + cols], -1)], 1)
    faces = np.where((rng.random(v00.size) < 0.5)[:, None, None], one, other).reshape(-1, 3)   # a diagonal per quad
    return v[0], faces


def _cone_part(rng, t):
    """a closed cone: t (even) triangles round apex 0 over a rim circle whose height alternates by 1.2 chords"""
    t = max(4, t - t % 2)
    k = np.arange(t)
    chord = 2 * np.pi / t
    rim = np.stack([np.cos(chord * k), np.sin(chord * k), 1.2 * chord * (-1.0) ** k], -1)
    v = np.concatenate([np.zeros((1, 3)), rim]) + 0.03 * chord * (2 * rng.random((t + 1, 3)) - 1)
    return v, np.stack([np.zeros_like(k), 1 + k, 1 + (k + 1) % t], -1)


def _tetrahedra_part(rng, count):
    base = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], np.float64)
    tet = np.array([[0, 1, 2], [0, 3, 1], [1, 3, 2], [0, 2, 3]])
    v = np.concatenate([base + 3.0 * i + 0.05 * (2 * rng.random((4, 3)) - 1) for i in range(count)])
    return v, np.concatenate([tet + 4 * i for i in range(count)])


MANIFOLD_F = (40, 341, 1024, 2730, 6000)


def _manifold_element(rng, budget):
    """(vertices (n,3) f64, faces (budget,3)): components over disjoint vertex ranges until the face budget is met;
    the last one is an open fan of exactly the triangles still missing, so every element has boundary edges"""
    parts, have = [], 0
    for _ in range(50):
        if budget - have <= 8 or len(parts) == 4:
            break
        room = budget - have
        kind = int(rng.integers(0, 4))
        want = int(rng.integers(8, room + 1)) if rng.random() < 0.7 else room
        if kind == 0:
            v, f = _grid_part(rng, want)
        elif kind == 1:
            v, f = _cone_part(rng, min(want, 3000))
        elif kind == 2:
            rows = 2 * int(rng.integers(2, 6))
            cols = 2 * max(2, min(want // (4 * rows), 20))     # (a longer torus folds its thin quads shut)
            v, f = torus_mesh(rows, cols)
            v = v + 0.002 * (2 * rng.random(v.shape) - 1)
        else:
            v, f = _tetrahedra_part(rng, max(1, min(want // 4, 50)))
        if f.shape[0] > room - 1:
            continue
        parts.append((v, f))
        have += f.shape[0]
    v, f = zigzag_fan(budget - have, int(rng.integers(1 << 30)))
    parts.append((v[0], f))
    verts, faces, base = [], [], 0
    for i, (v, f) in enumerate(parts):
        verts.append(v + np.array([40.0 * i, 0.0, 0.0]))
        faces.append(f + base)
        base += v.shape[0]
    return np.concatenate(verts), np.concatenate(faces).astype(np.int64)


def random_manifold(seed):
    """(vertices (B,N,3) f32, faces (B,F,3) int64), edge-manifold by construction: per batch element a grid with a
    random diagonal per quad, closed cones, tori, tetrahedra and an open fan over disjoint vertex ranges; then the same
    share of up to 30 % of the faces deleted at random (boundary edges), one vertex permutation that also places the
    isolated vertices, a random face order and a random cyclic rotation of every face (orientation kept).  Geometry is
    each component's own embedding with its jitter, as folded_grid and zigzag_fan make it.  Every element ends in an
    open fan, so none is closed: on a closed mesh the fp32 CPU composition can meet K = 0 and 4 x 0 bounds nothing."""
    rng = np.random.default_rng(61000 + seed)
    b = int(rng.integers(1, 4))
    budget = int(rng.choice(MANIFOLD_F))
    keep = budget - int(budget * rng.choice([0.0, 0.05, 0.3]) * rng.random())
    elements = [_manifold_element(rng, budget) for _ in range(b)]
    n = max(v.shape[0] for v, _ in elements) + int(rng.integers(1, 40))
    vertices = np.zeros((b, n, 3), np.float64)
    faces = np.empty((b, keep, 3), np.int64)
    for e, (v, f) in enumerate(elements):
        perm = rng.permutation(n)
        vertices[e] = 5.0 * rng.random((n, 3))                    # the isolated vertices: anywhere
        vertices[e, perm[:v.shape[0]]] = v
        f = perm[f[rng.permutation(f.shape[0])[:keep]]]
        faces[e] = _rotate(f, rng.integers(0, 3, keep))
    return vertices.astype(F32), faces


# ------------------------------------------------------------------------------------------------ case names
def graph_names():
    return list(range(seed_count())) + ["many_long", "ladder"]


def graph_case(name, query=None):
    if isinstance(name, int):
        return random_graph(name, query)
    return {"many_long": many_long_graph, "ladder": ladder_graph}[name]()


def soup_names():
    return list(range(seed_count())) + ["many_long"] + sorted(SEAMS)


def soup_case(name):
    if isinstance(name, int):
        return random_soup(name)
    return many_long_faces() if name == "many_long" else seam_faces(name)


def manifold_names():
    return list(range(seed_count()))
