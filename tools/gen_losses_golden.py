"""Writes tests/golden/ref_losses_*.npz: what the reference's own ``network.geo_operations`` and ``network.model_loss``
return, on CPU torch, for the mesh Laplacians, the mesh and point-cloud losses and the face, edge and dihedral helpers.
CPU machine only.

    python tools/gen_losses_golden.py <reference checkout>

The reference package is read from the checkout at run time through ``gen_mvc_golden.load_reference`` (nothing of it is
stored here).  Its compiled ``_ext`` stays stubbed; the real ``scipy.sparse``, which its ``CotLaplacian`` needs, is
imported first and put back after the stubbing; the stubbed ``pytorch3d.ops`` gets the ``knn_points`` below (fp64
squared distances, a stable sort, the lowest index first among equals).

A fixture is one family of inputs and every CASE that applies to it (CASES below: a name, the inputs it differentiates,
and a function of ``(api, T)`` that makes the calls; ``api.geo`` / ``api.loss`` are the two modules, ``T`` the inputs
as tensors).  The tests make the same calls on this project's modules through ``run_case``, so the table is written
once.  Every coordinate is generated in fp32 and upcast: the reference's fp64 run and an fp32 kernel see the same
points.  A fixture holds arrays and lists of names only (``allow_pickle=False`` loads it); ``load_fixture`` gives them
under these keys:

    in/<input>                 the inputs; floats fp32, indices int64
    cases                      names of the recorded cases
    raises                     "<case>:<exception class>" where the reference raised instead of returning
    <case>/out64/<output>      the reference on fp64 inputs (integer outputs as they are)
    <case>/out32/<output>      the same call on fp32 inputs, float outputs only
    <case>/cot/<output>        the cotangent G of that output, fp32 values
    <case>/grad64/<input>      the reference's fp64 autograd gradient of sum_outputs sum(G * output), NaN kept
    <case>/graderr32/<input>   max |grad32 - grad64| over the entries finite in both, grad32 the same gradient of the
                               reference's fp32 run: a scalar, all that a bound needs of it

For the point clouds the tool asserts a condition on the INPUT: among every point's first ``nn_size + 2`` neighbours,
consecutive fp64 squared distances differ by at least 2**-15 relative -- far above the few eps32 of an fp32 squared
distance, so fp32 and fp64 searches choose the same neighbours.  A seed that does not meet it is refused.  Two more
conditions of that kind: every interior edge of the dihedral families keeps the dot of its two unit normals below CLEAR
in magnitude (``largest_interior_dot``), and a repulsion threshold sits in a gap of the squared lengths it is compared
with (``clear_threshold``).

The archive is written with fixed time stamps: a second run gives the same bytes."""
import collections
import contextlib
import importlib
import importlib.util
import io
import os
import sys
import types
import zipfile
import zlib

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden")
REDUCTIONS = ["mean", "max", "sum", "none"]
NN_SIZES = [3, 5, 10]
GAP = 2.0 ** -15
CLEAR = 0.999      # every interior edge's |dot of its two unit normals| in the dihedral families is below this
POINT_SEED = 123   # of the seeds 0-199, the one with the widest smallest gap (7.0e-5)

Api = collections.namedtuple("Api", ["geo", "loss"])
Case = collections.namedtuple("Case", ["name", "wrt", "fn"])
KNN = collections.namedtuple("KNN", ["dists", "idx", "knn"])


def knn_points(p1, p2, lengths1=None, lengths2=None, K=1, version=-1, return_nn=False, return_sorted=True):
    """pytorch3d.ops.knn_points for the reference: ``(dists (B,N,K), idx (B,N,K), nn (B,N,K,D) or None)``, the squared
    distances in fp64 whatever the dtype of the clouds, a stable sort, so equal distances keep the lowest index first"""
    d = ((p1.detach().double()[:, :, None] - p2.detach().double()[:, None]) ** 2).sum(-1)
    idx = torch.sort(d, dim=-1, stable=True)[1][:, :, :K]
    nn = torch.gather(p2.unsqueeze(1).expand(-1, p1.shape[1], -1, -1), 2, idx.unsqueeze(-1).expand(-1, -1, -1, p2.shape[-1]))
    dists = ((nn - p1.unsqueeze(2)) ** 2).sum(-1)
    return KNN(dists, idx, nn if return_nn else None)


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def load_reference_api(checkout):
    """the reference's (geo_operations, model_loss, geometry_utils) with the stand-ins described above"""
    import scipy
    import scipy.sparse                                        # the real one, before load_reference stubs the name
    mvc_tool = _load("gen_mvc_golden", os.path.join(ROOT, "tools", "gen_mvc_golden.py"))
    sys.modules["gen_mvc_golden"] = mvc_tool
    mvc_tool.load_reference(checkout)
    # load_reference left empty modules under the names scipy and scipy.sparse, and the reference's modules bound
    # the empty ``sparse``: the real one goes back into sys.modules and into them
    sys.modules.update({"scipy": scipy, "scipy.sparse": scipy.sparse})
    sys.modules["pytorch3d.ops"].knn_points = knn_points
    for name in ("openmesh", "matplotlib", "matplotlib.cm"):              # geometry_utils imports them, unused here
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["matplotlib"].cm = sys.modules["matplotlib.cm"]
    geo = importlib.import_module("pytorch_points.network.geo_operations")
    operations = importlib.import_module("pytorch_points.network.operations")
    geo.sparse = operations.sparse = scipy.sparse
    loss = importlib.import_module("pytorch_points.network.model_loss")
    utils = importlib.import_module("pytorch_points.utils.geometry_utils")
    return Api(geo, loss), utils


# ------------------------------------------------------------------------------------------------ the calls
def _l1():
    return torch.nn.L1Loss()


def _mse():
    return torch.nn.MSELoss()


def _metric(use_cot):
    """the sequences' metric: squares on the uniform Laplacian; on the cotangent one, which the reference rounds to
    fp32, a metric with Lipschitz constant 1, so that the rounding's reach into the loss has a bound"""
    return _l1() if use_cot else _mse()


def _edges_of(api, faces):
    return [api.geo.edge_vertex_indices(faces[b]) for b in range(faces.shape[0])]


def _uniform(api, T):
    return {"lap": api.geo.UniformLaplacian()(T["v1"], T["faces"])}


def _uniform_shared(api, T):
    lap = api.geo.UniformLaplacian()
    return {"single": lap(T["v1"][:1], T["faces"][:1]), "batch": lap(T["v1"])}


def _uniform_kept(api, T):
    lap = api.geo.UniformLaplacian()
    return {"call0": lap(T["v1"], T["faces"]), "call1": lap(T["v2"], T["faces_alt"])}


def _cot(api, T):
    lap = api.geo.CotLaplacian()
    lap(T["v1"].detach(), T["faces"])                # the reference cannot build from vertices that require grad
    return {"lap": lap(T["v1"])}


def _cot_built_with_grad(api, T):
    return {"lap": api.geo.CotLaplacian()(T["v1"], T["faces"])}


def _cot_kept(api, T):
    lap = api.geo.CotLaplacian()
    return {"call0": lap(T["v1"], T["faces"]), "call1": lap(T["v2"], T["faces_alt"])}


def _cotangent(api, T):
    return {"cot": api.geo.cotangent(T["v1"], T["faces"])}


def _face_normals(which):
    def fn(api, T):
        normals, areas = api.geo.compute_face_normals_and_areas(T["v1"], T["faces"])
        return {name: value for name, value in (("normals", normals), ("areas", areas)) if name in which}
    return fn


def _edge_indices(api, T):
    return {"edges%d" % b: e for b, e in enumerate(_edges_of(api, T["faces"]))}


def _edge_lengths(api, T):
    return {"sq%d" % b: api.geo.get_edge_lengths(T["v1"][b], e) for b, e in enumerate(_edges_of(api, T["faces"]))}


def _smoothness(with_ref):
    def fn(api, T):
        mod = api.loss.UniformLaplacianSmoothnessLoss(T["v1"].shape[1], T["faces"], _l1())
        return {"loss": mod(T["v1"], T["v2"]) if with_ref else mod(T["v1"])}
    return fn


def _laplacian_loss(use_cot, use_norm, with_vert2):
    def fn(api, T):
        mod = api.loss.MeshLaplacianLoss(_l1(), use_cot=use_cot, use_norm=use_norm)
        return {"loss": mod(T["v1"], T["v2"] if with_vert2 else None, T["faces"])}
    return fn


def _laplacian_loss_topology(use_cot, consistent):
    def fn(api, T):
        mod = api.loss.MeshLaplacianLoss(_metric(use_cot), use_cot=use_cot, consistent_topology=consistent)
        return {"call0": mod(T["v1"], T["v2"], T["faces"]), "call1": mod(T["v3"], T["v2"], T["faces_alt"])}
    return fn


def _laplacian_loss_precompute(use_cot, consistent):
    def fn(api, T):
        mod = api.loss.MeshLaplacianLoss(_metric(use_cot), use_cot=use_cot, consistent_topology=consistent,
                                         precompute_L=True)
        return {"call0": mod(T["v1"], T["v2"], T["faces"]), "call1": mod(T["v3"], T["v2"], T["faces"]),
                "call2": mod(T["v3"], None, T["faces"])}
    return fn


def _two_calls(make, with_face=True):
    def fn(api, T):
        mod = make(api)
        second = (T["v3"], T["v2"], T["faces_alt"]) if with_face else (T["v3"], T["v2"])
        return {"call0": mod(T["v1"], T["v2"], T["faces"]), "call1": mod(*second)}
    return fn


def _edge_length_loss(api, T):
    return {"loss": api.loss.MeshEdgeLengthLoss(_l1())(T["v1"], T["v2"], T["faces"])}


def _stretch(reduction):
    def fn(api, T):
        return {"loss": api.loss.MeshStretchLoss(reduction)(T["v1"], T["v2"], T["faces"])}
    return fn


def _mesh_repulsion(reduction, at_call):
    def fn(api, T):
        edges = _edges_of(api, T["faces"])[0]
        threshold = float(T["threshold"])
        if at_call:
            return {"loss": api.loss.SimpleMeshRepulsionLoss(threshold, reduction=reduction)(T["v1"], edges)}
        return {"loss": api.loss.SimpleMeshRepulsionLoss(threshold, edges, reduction)(T["v1"])}
    return fn


def mesh_cases(triangles=True):
    cases = [Case("uniform_laplacian", ["v1"], _uniform), Case("uniform_laplacian_shared", ["v1"], _uniform_shared),
             Case("uniform_laplacian_kept", ["v1", "v2"], _uniform_kept)]
    if not triangles:
        return cases
    cases += [Case("cot_laplacian", ["v1"], _cot), Case("cot_laplacian_built_with_grad", ["v1"], _cot_built_with_grad),
              Case("cot_laplacian_kept", ["v2"], _cot_kept), Case("cotangent", ["v1"], _cotangent),
              Case("face_normals_and_areas", [], _face_normals(("normals", "areas"))),
              Case("face_normals_grad", ["v1"], _face_normals(("normals",))),
              Case("face_areas_grad", ["v1"], _face_normals(("areas",))),
              Case("edge_vertex_indices", [], _edge_indices), Case("get_edge_lengths", ["v1"], _edge_lengths),
              Case("smoothness_loss", ["v1"], _smoothness(False)),
              Case("smoothness_loss_vert_ref", ["v1", "v2"], _smoothness(True))]
    for use_cot in (False, True):
        kind = "cot" if use_cot else "uniform"
        # the reference's CotLaplacian cannot be built from vertices that require grad: vert1 and v3 are constants there
        wrt = ["v1", "v2", "v3"]
        for use_norm in (False, True):
            name = "laplacian_loss_%s%s" % (kind, "_norm" if use_norm else "")
            cases.append(Case(name, wrt[1:2] if use_cot else wrt[:2], _laplacian_loss(use_cot, use_norm, True)))
            cases.append(Case(name + "_vert2_none", [] if use_cot else wrt[:1], _laplacian_loss(use_cot, use_norm, False)))
        for consistent in (False, True):
            cases.append(Case("laplacian_loss_%s_consistent_%s" % (kind, "on" if consistent else "off"),
                              wrt[1:2] if use_cot else wrt, _laplacian_loss_topology(use_cot, consistent)))
        cases.append(Case("laplacian_loss_%s_precompute" % kind, wrt[1:2] if use_cot else wrt,
                          _laplacian_loss_precompute(use_cot, False)))
        cases.append(Case("laplacian_loss_%s_precompute_consistent" % kind, wrt[1:2] if use_cot else wrt,
                          _laplacian_loss_precompute(use_cot, True)))
    cases.append(Case("edge_length_loss", ["v1", "v2"], _edge_length_loss))
    for consistent in (False, True):
        tag = "on" if consistent else "off"
        cases.append(Case("edge_length_loss_consistent_" + tag, ["v1", "v2", "v3"], _two_calls(
            lambda api, c=consistent: api.loss.MeshEdgeLengthLoss(_mse(), consistent_topology=c))))
        cases.append(Case("stretch_consistent_" + tag, ["v1", "v2", "v3"], _two_calls(
            lambda api, c=consistent: api.loss.MeshStretchLoss("mean", consistent_topology=c))))
    cases.append(Case("edge_length_loss_kept_without_face", ["v1", "v2", "v3"], _two_calls(
        lambda api: api.loss.MeshEdgeLengthLoss(_mse(), consistent_topology=True), with_face=False)))
    cases.append(Case("stretch_kept_without_face", ["v1", "v2", "v3"], _two_calls(
        lambda api: api.loss.MeshStretchLoss("mean", consistent_topology=True), with_face=False)))
    for reduction in REDUCTIONS:
        cases.append(Case("stretch_" + reduction, ["v1", "v2"], _stretch(reduction)))
        cases.append(Case("mesh_repulsion_" + reduction, ["v1"], _mesh_repulsion(reduction, False)))
    cases.append(Case("mesh_repulsion_edges_at_call", ["v1"], _mesh_repulsion("mean", True)))
    return cases


def dihedral_cases():
    def normals(side):
        return lambda api, T: {"normals": api.geo.get_normals(T["v"], T["table"], side)}
    cases = [Case("get_normals_side%d" % side, ["v"], normals(side)) for side in range(4)]
    cases.append(Case("dihedral_angle", ["v"], lambda api, T: {"angle": api.geo.dihedral_angle(T["v"], T["table"])}))
    return cases


def _point_laplacian(k, given):
    def fn(api, T):
        if given:
            lap, idx = api.geo.pointUniformLaplacian(T["p2"], knn_idx=T["knn%d" % k])
        else:
            lap, idx = api.geo.pointUniformLaplacian(T["p1"], nn_size=k)
        return {"lap": lap, "knn_idx": idx}
    return fn


def _point_laplacian_loss(k, use_norm, with_idx12):
    def fn(api, T):
        mod = api.loss.PointLaplacianLoss(k, _l1(), use_norm=use_norm)
        return {"loss": mod(T["p1"], T["p2"], T["idx12"]) if with_idx12 else mod(T["p1"], T["p2"])}
    return fn


def _point_repulsion(k, reduction, given):
    def fn(api, T):
        mod = api.loss.SimplePointRepulsionLoss(k, float(T["radius%d" % k]), reduction)
        return {"loss": mod(T["p1"], T["knn%d" % k]) if given else mod(T["p1"])}
    return fn


def point_cases():
    cases = [Case("smape", ["p1", "p2"], lambda api, T: {"loss": api.loss.SmapeLoss()(T["p1"], T["p2"])})]
    # every flag at nn_size 5; the other two sizes change the search alone, and the fixtures have a size limit: they
    # get the Laplacian (with its k-NN table) and one loss of each kind that searches
    for k in NN_SIZES:
        cases.append(Case("point_laplacian_k%d" % k, ["p1"], _point_laplacian(k, False)))
        if k != 5:
            cases.append(Case("point_edge_length_loss_k%d" % k, ["p1", "p2"], lambda api, T, k=k: {
                "loss": api.loss.PointEdgeLengthLoss(k, _l1())(T["p1"], T["p2"])}))
            cases.append(Case("point_stretch_k%d_mean" % k, ["p1", "p2"], lambda api, T, k=k: {
                "loss": api.loss.PointStretchLoss(k, "mean")(T["p1"], T["p2"])}))
            cases.append(Case("point_repulsion_k%d_mean" % k, ["p1"], _point_repulsion(k, "mean", False)))
            continue
        cases.append(Case("point_laplacian_given_k%d" % k, ["p2"], _point_laplacian(k, True)))
        for use_norm in (False, True):
            for with_idx12 in (False, True):
                name = "point_laplacian_loss_k%d%s%s" % (k, "_norm" if use_norm else "", "_idx12" if with_idx12 else "")
                cases.append(Case(name, ["p1", "p2"], _point_laplacian_loss(k, use_norm, with_idx12)))
        cases.append(Case("point_edge_length_loss_k%d" % k, ["p1", "p2"], lambda api, T, k=k: {
            "loss": api.loss.PointEdgeLengthLoss(k, _l1())(T["p1"], T["p2"])}))
        for reduction in REDUCTIONS:
            cases.append(Case("point_stretch_k%d_%s" % (k, reduction), ["p1", "p2"], lambda api, T, k=k, r=reduction: {
                "loss": api.loss.PointStretchLoss(k, r)(T["p1"], T["p2"])}))
            for given in (False, True):
                name = "point_repulsion_k%d_%s%s" % (k, reduction, "_given" if given else "")
                cases.append(Case(name, ["p1"], _point_repulsion(k, reduction, given)))
    return cases


FAMILIES = collections.OrderedDict([
    ("closed", mesh_cases), ("open", mesh_cases), ("two_topologies", mesh_cases),
    ("quads", lambda: mesh_cases(triangles=False)), ("degenerate_coincident", mesh_cases),
    ("degenerate_duplicate", mesh_cases), ("degenerate_isolated", mesh_cases), ("dihedral_ico2", dihedral_cases),
    ("dihedral_open", dihedral_cases), ("points", point_cases)])


def cases_of(family):
    return FAMILIES[family]()


def run_case(case, api, inputs, dtype, device="cpu", cot=None, requires_grad=True):
    """Makes the calls of ``case`` on ``api`` with ``inputs`` (name -> array) as ``dtype`` tensors on ``device`` ->
    ``(outputs, grads)``: the outputs by name, detached, and, given the cotangents ``cot`` (name -> array), the gradient
    of ``sum_outputs sum(cot * output)`` for every input in ``case.wrt`` (zeros where autograd reports none).  Without
    ``requires_grad`` no input asks for a gradient."""
    T = {}
    for name, a in inputs.items():
        t = torch.from_numpy(np.array(a))
        T[name] = (t.to(dtype) if t.is_floating_point() else t).to(device)
    for name in case.wrt if requires_grad else []:
        T[name].requires_grad_(True)
    out = case.fn(api, T)
    grads = {}
    if cot is not None and case.wrt:
        total = None
        for name, value in out.items():
            if value.is_floating_point() and value.requires_grad:
                term = (value * torch.from_numpy(np.array(cot[name])).to(dtype).to(device)).sum()
                total = term if total is None else total + term
        leaves = [T[name] for name in case.wrt]
        got = [None] * len(leaves) if total is None else torch.autograd.grad(total, leaves, allow_unused=True)
        grads = {name: (torch.zeros_like(leaf) if g is None else g).detach()
                 for name, leaf, g in zip(case.wrt, leaves, got)}
    return {name: value.detach() for name, value in out.items()}, grads


# ------------------------------------------------------------------------------------------------ the inputs
def f32(a):
    return np.asarray(a, np.float64).astype(np.float32)


def grid_faces(rows, cols, other_diagonal=False):
    faces = []
    for r in range(rows - 1):
        for c in range(cols - 1):
            a, b, d, e = r * cols + c, r * cols + c + 1, (r + 1) * cols + c, (r + 1) * cols + c + 1
            faces += [[a, b, d], [b, e, d]] if not other_diagonal else [[a, b, e], [a, e, d]]
    return np.array(faces, np.int64)


def grid_quads(rows, cols):
    return np.array([[r * cols + c, r * cols + c + 1, (r + 1) * cols + c + 1, (r + 1) * cols + c]
                     for r in range(rows - 1) for c in range(cols - 1)], np.int64)


def grid_vertices(rng, rows, cols, batch):
    xy = np.stack(np.meshgrid(np.arange(cols, dtype=np.float64), np.arange(rows, dtype=np.float64)), -1).reshape(-1, 2)
    v = np.concatenate([xy, np.zeros((rows * cols, 1))], 1)[None].repeat(batch, 0)
    return v + rng.normal(scale=[0.12, 0.12, 0.35], size=v.shape)


def mesh_inputs(rng, v1, faces, faces_alt=None):
    """v1 (B,N,3), faces (B,F,L) -> the inputs of a mesh family: a deformed copy v2, a third set v3, the faces of the
    second call of a sequence (default: the first half of the faces), and the repulsion threshold, about the median edge length"""
    v1 = f32(v1)
    v2 = f32(v1 + rng.normal(scale=0.05, size=v1.shape))
    v3 = f32(v1 * [1.1, 0.9, 1.05] + rng.normal(scale=0.03, size=v1.shape))
    if faces_alt is None:
        faces_alt = faces[:, :faces.shape[1] // 2].copy()
    ends = v1.astype(np.float64)[:, faces[0]]                 # the repulsion loss takes the edges of faces[0] for every b
    squares = ((ends - np.roll(ends, -1, axis=2)) ** 2).sum(-1)
    return collections.OrderedDict([("v1", v1), ("v2", v2), ("v3", v3), ("faces", faces), ("faces_alt", faces_alt),
                                    ("threshold", clear_threshold(squares))])


def clear_threshold(squares):
    """An fp32 length whose square cuts the squared lengths ``squares`` about their median and stays clear of all of
    them: it lies in a gap of at least 2**-10 relative and at least 2**-15 from either side, so the fp32 and the fp64
    comparison ``square < threshold ** 2`` agree on every edge.  A condition on the input."""
    d = np.unique(np.asarray(squares, np.float64).reshape(-1))
    d = d[d > 0]
    m = len(d) // 2
    while d[m] - d[m - 1] < 2.0 ** -10 * d[m]:
        m += 1
    threshold = f32(np.sqrt((d[m - 1] + d[m]) / 2))
    assert d[m - 1] * (1 + 2.0 ** -15) < float(threshold) ** 2 < d[m] * (1 - 2.0 ** -15)
    return threshold


def point_inputs(seed):
    rng = np.random.default_rng(seed)
    batch, n = 2, 200
    p1 = f32(rng.normal(size=(batch, n, 3)))
    p2 = f32(p1 + rng.normal(scale=0.04, size=p1.shape))
    idx12 = np.stack([rng.permutation(n) for _ in range(batch)]).astype(np.int64)
    inputs = collections.OrderedDict([("p1", p1), ("p2", p2), ("idx12", idx12)])
    gathered = np.take_along_axis(p2, idx12[:, :, None], 1)
    smallest = min(smallest_gap(cloud, max(NN_SIZES) + 2) for cloud in (p1, p2, gathered))
    if smallest < GAP:
        raise SystemExit("point seed %d: consecutive neighbour distances %.3g apart (relative), below 2**-15: refused"
                         % (seed, smallest))
    for k in NN_SIZES:
        t = torch.from_numpy(p1)
        found = knn_points(t, t, K=k + 1)
        inputs["knn%d" % k] = found.idx[:, :, 1:].numpy().copy()
        inputs["radius%d" % k] = clear_threshold(found.dists[:, :, 1:].double().numpy())       # cuts through the edges
    return inputs, smallest


def smallest_gap(cloud, k):
    """the smallest relative difference of consecutive fp64 squared distances among every point's first k neighbours
    (itself included)"""
    p = cloud.astype(np.float64)
    d = np.sort(((p[:, :, None] - p[:, None]) ** 2).sum(-1), axis=-1)[:, :, :k + 1]
    return float(((d[..., 1:] - d[..., :-1]) / d[..., 1:]).min())


def largest_interior_dot(v, table):
    """A condition on the INPUT of the dihedral families, as tests/test_gpu_mesh_dihedral.py asks of its own: the largest
    |na . nb| in fp64 over the interior edges of ``table`` (E,4) over ``v`` (N,3) stays below CLEAR, so that no edge
    sits where 1 / sqrt(1 - d^2) turns an fp32 rounding of d into a gradient of another size, or where fp32 and fp64
    take different sides of the clamp.  Boundary edges (both wings the same vertex) are at -1 and clamped in both."""
    v = np.asarray(v, np.float64)
    p = [v[table[:, k]] for k in range(4)]
    na, nb = np.cross(p[2] - p[0], p[1] - p[0]), np.cross(p[3] - p[1], p[0] - p[1])
    d = (na * nb).sum(-1) / np.sqrt((na * na).sum(-1) * (nb * nb).sum(-1))
    return float(np.abs(d[table[:, 2] != table[:, 3]]).max())


def first_clear(make, table):
    """``make(rng)`` of the first seed from 1000 on whose vertices keep every interior edge of ``table`` clear"""
    for seed in range(1000, 1100):
        v = make(np.random.default_rng(seed))
        if largest_interior_dot(v, table) < CLEAR:
            return v
    raise SystemExit("no seed keeps every interior edge clear of the clamp")


def build_inputs(utils):
    mvc_tool = sys.modules["gen_mvc_golden"]
    rng = np.random.default_rng(11)
    families = collections.OrderedDict()
    v, f = mvc_tool.icosphere(1)
    v = np.stack([v * [1.3, 0.8, 1.0], v * [0.9, 1.2, 1.1]]) + rng.normal(scale=0.04, size=(2,) + v.shape)
    families["closed"] = mesh_inputs(rng, v, np.stack([f, f]))
    families["open"] = mesh_inputs(rng, grid_vertices(rng, 5, 5, 2), np.stack([grid_faces(5, 5)] * 2))
    two = np.stack([grid_faces(5, 5), np.roll(grid_faces(5, 5, other_diagonal=True)[::-1], 1, axis=1)])
    families["two_topologies"] = mesh_inputs(rng, grid_vertices(rng, 5, 5, 2), two, faces_alt=two[::-1].copy())
    families["quads"] = mesh_inputs(rng, grid_vertices(rng, 5, 5, 2), np.stack([grid_quads(5, 5)] * 2))
    # the degenerate families have one batch element: what the reference does there does not depend on B
    # one face with two coincident vertices: vertex 12 moved onto vertex 13, so the edge (12,13) has no length and
    # the faces that hold both no area
    d = mesh_inputs(rng, grid_vertices(rng, 5, 5, 1), grid_faces(5, 5)[None])
    for name in ("v1", "v2", "v3"):
        d[name][:, 12] = d[name][:, 13]
    families["degenerate_coincident"] = d
    # one duplicated face: face 9 stands a second time at the end of the list
    dup = np.concatenate([grid_faces(5, 5), grid_faces(5, 5)[9:10]])
    families["degenerate_duplicate"] = mesh_inputs(rng, grid_vertices(rng, 5, 5, 1), dup[None])
    # one vertex that no face uses: the corner 24, whose cell loses its two faces
    iso = grid_faces(5, 5)[:-2]
    assert not (iso == 24).any() and set(iso.reshape(-1)) == set(range(24))
    families["degenerate_isolated"] = mesh_inputs(rng, grid_vertices(rng, 5, 5, 1), iso[None], faces_alt=iso[None, 4:])
    # the recorded (E,4) table of the level-2 icosphere, and one the reference builds for the open patch
    z = np.load(os.path.join(OUT, "dihedral_edge_points.npz"))
    v, f = mvc_tool.icosphere(2)
    assert np.array_equal(f, z["faces"])
    # stretched, and jittered by little: the sphere's flattest edges are at 0.995 already
    jittered = first_clear(lambda r: f32(v * [1.2, 0.9, 1.0] + r.normal(scale=0.002, size=v.shape)), z["edge_points"])
    families["dihedral_ico2"] = collections.OrderedDict([("v", jittered), ("table", z["edge_points"].astype(np.int64))])
    patch = families["open"]
    mesh = types.SimpleNamespace(vs=patch["v1"][0])
    utils.build_gemm(mesh, patch["faces"][0])
    table = utils.get_edge_points(mesh).astype(np.int64)
    # (the patch's own vertices leave two edges within a degree of flat)
    folded = first_clear(lambda r: f32(grid_vertices(r, 5, 5, 1)[0] * [1.0, 1.0, 2.0]), table)
    families["dihedral_open"] = collections.OrderedDict([("v", folded), ("table", table)])
    families["points"], gap = point_inputs(POINT_SEED)
    print("points: smallest relative gap among the first %d neighbours %.3g" % (max(NN_SIZES) + 2, gap))
    return families


# ------------------------------------------------------------------------------------------------ recording
def cotangent_for(family, case, output, shape):
    rng = np.random.default_rng(zlib.crc32(("%s/%s/%s" % (family, case, output)).encode()))
    return f32(rng.integers(-16, 17, size=shape) / 8.0)          # multiples of 1/8 in [-2, 2]: they compress


def record(api, family, inputs):
    arrays = collections.OrderedDict(("in/" + name, a) for name, a in inputs.items())
    names, raises = [], []
    for case in cases_of(family):
        try:
            with contextlib.redirect_stdout(io.StringIO()):
                out64, _ = run_case(case, api, inputs, torch.float64)
                cot = {name: cotangent_for(family, case.name, name, tuple(value.shape))
                       for name, value in out64.items() if value.is_floating_point()}
                out64, grad64 = run_case(case, api, inputs, torch.float64, cot=cot)
                out32, grad32 = run_case(case, api, inputs, torch.float32, cot=cot)
        except Exception as err:  # noqa: BLE001 -- what the reference raises is what is recorded
            raises.append("%s:%s" % (case.name, type(err).__name__))
            continue
        names.append(case.name)
        for name, value in out64.items():
            arrays["%s/out64/%s" % (case.name, name)] = value.numpy()
            if value.is_floating_point():
                assert out32[name].dtype == torch.float32, (case.name, name, out32[name].dtype)
                arrays["%s/out32/%s" % (case.name, name)] = out32[name].numpy()
                arrays["%s/cot/%s" % (case.name, name)] = cot[name]
        for name, value in grad64.items():
            arrays["%s/grad64/%s" % (case.name, name)] = value.numpy()
            both = torch.isfinite(value) & torch.isfinite(grad32[name])
            diff = (grad32[name].double() - value)[both].abs().numpy()
            arrays["%s/graderr32/%s" % (case.name, name)] = np.float64(diff.max(initial=0.0))
    arrays["cases"] = np.array(names)
    arrays["raises"] = np.array(raises, dtype="U") if raises else np.zeros(0, "U1")
    path = os.path.join(OUT, "ref_losses_%s.npz" % family)
    write_npz(path, arrays)
    print("%-22s %3d cases, %d raised %s, %d bytes" % (family, len(names), len(raises), raises, os.path.getsize(path)))


_POOLS = collections.OrderedDict([("f64", np.float64), ("f32", np.float32), ("i64", np.int64)])


def write_npz(path, arrays):
    """The arrays by name as ONE archive of a few members -- a member per array costs more than most of these arrays
    hold: ``names``, and per name its ``pool`` (index into f64 / f32 / i64), ``offset`` into that pool's flat array
    and ``shape`` (padded with -1 to four dimensions); ``cases`` and ``raises`` as they are.  Every member is stamped
    1980-01-01, so the same arrays give the same bytes.  ``load_fixture`` undoes it."""
    members = collections.OrderedDict((key, arrays.pop(key)) for key in ("cases", "raises"))
    pools = {key: [] for key in _POOLS}
    sizes = {key: 0 for key in _POOLS}
    names, pool, offset, shape = [], [], [], []
    for name, a in arrays.items():
        a = np.asarray(a)
        key = [k for k, dtype in _POOLS.items() if a.dtype == dtype]
        assert key and a.ndim <= 4, (name, a.dtype, a.shape)
        names.append(name)
        pool.append(list(_POOLS).index(key[0]))
        offset.append(sizes[key[0]])
        shape.append(list(a.shape) + [-1] * (4 - a.ndim))
        pools[key[0]].append(a.reshape(-1))
        sizes[key[0]] += a.size
    members.update(names=np.array(names), pool=np.array(pool, np.int8), offset=np.array(offset, np.int64),
                   shape=np.array(shape, np.int64).reshape(-1, 4))
    for key, dtype in _POOLS.items():
        members[key] = np.concatenate(pools[key] + [np.zeros(0, dtype)])
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as archive:
        for name, a in members.items():
            a = np.ascontiguousarray(a)
            assert a.dtype != object, name
            buf = io.BytesIO()
            np.lib.format.write_array(buf, a, allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            archive.writestr(info, buf.getvalue(), compresslevel=9)


def load_fixture(path):
    """a fixture as ``{name: array}`` with the keys of this file's docstring"""
    with np.load(path, allow_pickle=False) as z:
        pools = [z[key] for key in _POOLS]
        out = {"cases": [str(c) for c in z["cases"]], "raises": [str(r) for r in z["raises"]]}
        for name, pool, offset, shape in zip(z["names"], z["pool"], z["offset"], z["shape"]):
            shape = tuple(int(n) for n in shape if n >= 0)
            size = int(np.prod(shape, dtype=np.int64))
            out[str(name)] = pools[pool][offset:offset + size].reshape(shape)
    return out


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    torch.set_num_threads(1)
    api, utils = load_reference_api(os.path.abspath(sys.argv[1]))
    for family, inputs in build_inputs(utils).items():
        record(api, family, inputs)


if __name__ == "__main__":
    main()
