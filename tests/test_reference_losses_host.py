"""CPU tests (no GPU) that hold the Python layer above the kernels -- the mesh Laplacians, the mesh and point-cloud
losses, the face, edge and dihedral helpers -- to what the REFERENCE's own functions returned, recorded in
tests/golden/ref_losses_*.npz by tools/gen_losses_golden.py (which documents the fixtures and owns the table of calls:
the same ``Case`` functions run here on this project's modules, on CPU fp64).

* Integer outputs are equal; NaN and inf stand at the same places; values and gradients lie within 1e-12 of the largest
  recorded magnitude of their array; ``CotLaplacian`` gets 2**-24 * |value| on top, because the reference rounds that
  operator's result to fp32 (``torch.Tensor(...)``), and what is built on it that rounding carried through (``on_cot``).
* Where the reference raised (the fixtures' ``raises`` lists) the project raises as well or returns what DEVIATIONS
  says; the one place where the project knowingly differs in value is PI_GAP.  DESIGN.md "Pinned to the reference's
  Python" has one line for each.
* The numpy and dense restatements of the four operator test files are imported and held to the same recordings: from
  here on they are pinned, not trusted.

The k-NN search of this project runs on the GPU only.  On the CPU ``test_knn_edges_host.topk_knn`` stands in for it,
after it has itself been held to the recorded k-NN tables; the search itself is left to
tests/test_gpu_reference_losses.py, for the cases in SEARCHED."""
import functools
import glob
import importlib.util
import math
import os
import types

import numpy as np
import pytest
import torch

from pytorch_points_amd import ops
from pytorch_points_amd.network import geo_operations, model_loss
import test_knn_edges_host as knn_host
import test_mesh_dihedral_host as dihedral_host
import test_mesh_edges_host as edges_host
import test_mesh_laplacian_host as laplacian_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _tool():
    spec = importlib.util.spec_from_file_location("gen_losses_golden", os.path.join(ROOT, "tools", "gen_losses_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


tool = _tool()
API = tool.Api(geo_operations, model_loss)
MESH_FAMILIES = ["closed", "open", "two_topologies", "degenerate_coincident", "degenerate_duplicate", "degenerate_isolated"]
# the reference's PI is the seven-digit constant: in fp64 this project's dihedral angles are lower by 4.64e-8
PI_GAP = math.pi - 3.1415927


@functools.lru_cache(maxsize=None)
def fixture(family):
    return tool.load_fixture(os.path.join(GOLDEN, "ref_losses_%s.npz" % family))


def inputs_of(family):
    return {k[3:]: v for k, v in fixture(family).items() if k.startswith("in/")}


def recorded(family, case, kind):
    prefix = "%s/%s/" % (case, kind)
    return {k[len(prefix):]: v for k, v in fixture(family).items() if k.startswith(prefix)}


def case_of(family, name):
    return {c.name: c for c in tool.cases_of(family)}[name]


def on_cot(family, case):
    """The term that the reference's rounding of its cotangent Laplacian to fp32 adds to the bound, as a function of the
    recorded array: None for a case that does not touch that operator.

    * The operator's own output, and its backward (the same rounded product): 2**-24 * |value|, element by element.
    * A loss built on it is a function of the rounded entries, each off by at most 2**-24 * M, M the largest recorded
      magnitude of the family's cotangent Laplacians.  The metrics of these cases are L1 (Lipschitz constant 1 per
      entry) of two such operands, or of their norms (sqrt(3) more): at most 2 * sqrt(3) * 2**-24 * M < 4 * 2**-24 * M.
      2**-24 * |value| of the loss itself cannot serve there: ``lap1.mean()`` over a mesh is zero in exact arithmetic
      (the operator's rows sum to zero), so the recorded value IS that rounding noise.  Their gradients are rounded
      products of the operator with a cotangent that the forward rounding moves: 4 * 2**-24 of the array's largest
      magnitude."""
    if "cot_laplacian" in case:
        return lambda want: 2.0 ** -24 * np.abs(want)
    if "laplacian_loss_cot" in case:
        laps = recorded(family, "cot_laplacian_kept", "out64")
        m = max(float(np.abs(a[np.isfinite(a)]).max(initial=0.0)) for a in laps.values())
        return lambda want: 4 * 2.0 ** -24 * max(m, float(np.abs(want).max(initial=0.0)))
    return None


# cases whose k-NN graph is searched inside the call: the GPU test runs them through the HIP search
SEARCHED = [c for c in fixture("points")["cases"] + [r.split(":")[0] for r in fixture("points")["raises"]]
            if c != "smape" and "given" not in c]

# Where this project, on purpose, does not do what the reference does.  Per case name (every family): what the
# reference does, and what is asserted here instead.
DEVIATIONS = {
    # the reference's CotLaplacian calls .numpy() on cotangents that require grad: RuntimeError.  Here the operator is
    # built from detached vertices (documented on the class), and the call returns what "cot_laplacian" returns.
    "cot_laplacian_built_with_grad": ("returns", "cot_laplacian"),
    # without consistent_topology the second call rebuilds the cotangent operator from ITS vert2, which requires grad:
    # the same RuntimeError.  Here: the restated control flow (DenseLaplacian detaches).
    "laplacian_loss_cot_precompute": ("restatement", None),
    # the reference halves the areas in place after the sqrt that autograd saved: its backward raises RuntimeError.
    # Here the areas are differentiable; the gradient is held to the one of |cross| / 2 written out below.
    "face_areas_grad": ("areas", None),
    # forward reads face.shape before it looks at self.E: AttributeError with face=None, whatever is kept.  Here the
    # kept topology serves the call, as the constructor's consistent_topology promises.
    "edge_length_loss_kept_without_face": ("kept", "edge_length_loss_consistent_on"),
    "stretch_kept_without_face": ("kept", "stretch_consistent_on"),
    # loss.mean(torch.sum(loss, dim=-1)) is a TypeError.  Here: torch.sum(loss, dim=-1).mean(), as in PointStretchLoss.
    "point_repulsion_k5_sum": ("sum_of_none", "point_repulsion_k5_none"),
    "point_repulsion_k5_sum_given": ("sum_of_none", "point_repulsion_k5_none_given"),
}


# ------------------------------------------------------------------------------------------------ comparison
def assert_matches(got, want, label, fp32_rounded=None, shift=0.0):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (label, got.shape, want.shape)
    if want.dtype.kind in "iub":
        assert got.dtype.kind in "iub" and np.array_equal(got, want), label
        return
    assert np.array_equal(np.isnan(got), np.isnan(want)), (label, "NaN at", np.argwhere(np.isnan(got) != np.isnan(want))[:4])
    for inf in (np.inf, -np.inf):
        assert np.array_equal(got == inf, want == inf), (label, "inf at", np.argwhere((got == inf) != (want == inf))[:4])
    finite = np.isfinite(want)
    if not finite.any():
        return
    want_f = want[finite]
    tol = 1e-12 * np.abs(want_f).max() + (fp32_rounded(want_f) if fp32_rounded else 0.0)
    err = np.abs(got[finite] - shift - want_f)
    worst = int(np.argmax(err - tol))
    assert (err <= tol).all(), (label, "error %.3g" % err[worst], "bound %.3g" % np.broadcast_to(tol, err.shape)[worst])


def run(family, case, api=API):
    fx = fixture(family)
    cot = recorded(family, case.name, "cot") if case.name in fx["cases"] else None
    return tool.run_case(case, api, inputs_of(family), torch.float64, cot=cot)


@pytest.fixture
def cpu_graphs(monkeypatch):
    monkeypatch.setattr(ops, "knn_points", knn_host.topk_knn)


def all_cases():
    out = []
    for path in sorted(glob.glob(os.path.join(GOLDEN, "ref_losses_*.npz"))):
        family = os.path.basename(path)[len("ref_losses_"):-len(".npz")]
        out += [(family, name) for name in fixture(family)["cases"]]
    return out


def all_raises():
    out = []
    for family in tool.FAMILIES:
        out += [(family,) + tuple(r.split(":")) for r in fixture(family)["raises"]]
    return out


# ------------------------------------------------------------------------------------------------ 0. the fixtures
def test_fixtures_are_small_complete_and_hold_no_objects():
    paths = sorted(glob.glob(os.path.join(GOLDEN, "ref_losses_*.npz")))
    assert [os.path.basename(p) for p in paths] == sorted("ref_losses_%s.npz" % f for f in tool.FAMILIES)
    assert sum(os.path.getsize(p) for p in paths) < 1024 * 1024
    for p in paths:
        with np.load(p, allow_pickle=False) as z:
            for key in z.files:
                assert z[key].dtype.kind in "fiuU", (p, key, z[key].dtype)
    for family in tool.FAMILIES:
        fx = fixture(family)
        names = [c.name for c in tool.cases_of(family)]
        assert sorted(fx["cases"] + [r.split(":")[0] for r in fx["raises"]]) == sorted(names), family
        for case in tool.cases_of(family):
            if case.name in fx["cases"]:
                assert sorted(recorded(family, case.name, "grad64")) == sorted(case.wrt), (family, case.name)
                floats = [k for k, v in recorded(family, case.name, "out64").items() if v.dtype.kind == "f"]
                assert sorted(recorded(family, case.name, "out32")) == sorted(recorded(family, case.name, "cot")) == sorted(floats)
    assert len(all_cases()) > 250 and {r[1] for r in all_raises()} == set(DEVIATIONS)


def test_the_inputs_are_what_the_families_promise():
    closed, opened, two = inputs_of("closed"), inputs_of("open"), inputs_of("two_topologies")
    assert closed["v1"].shape == (2, 42, 3) and closed["faces"].shape == (2, 80, 3)
    counts = lambda faces: np.unique(np.sort(np.stack([faces, np.roll(faces, -1, 1)], -1).reshape(-1, 2), -1), axis=0, return_counts=True)[1]  # noqa: E731
    assert (counts(closed["faces"][0]) == 2).all()                       # closed: every edge has two wings
    assert (counts(opened["faces"][0]) == 1).sum() == 16                 # open: the 16 boundary edges of a 5x5 patch
    assert two["faces"].shape == (2, 32, 3) and not np.array_equal(two["faces"][0], two["faces"][1])
    assert inputs_of("quads")["faces"].shape[-1] == 4
    d = inputs_of("degenerate_coincident")
    assert np.array_equal(d["v1"][:, 12], d["v1"][:, 13]) and (d["faces"][0] == 12).any(1)[(d["faces"][0] == 13).any(1)].any()
    d = inputs_of("degenerate_duplicate")["faces"][0]
    assert np.array_equal(d[-1], d[9]) and set(d.reshape(-1)) == set(range(25))
    d = inputs_of("degenerate_isolated")
    assert d["v1"].shape[1] == 25 and not (d["faces"] == 24).any()
    pts = inputs_of("points")
    assert pts["p1"].shape == (2, 200, 3) and pts["p1"].dtype == np.float32
    for cloud in (pts["p1"], pts["p2"], np.take_along_axis(pts["p2"], pts["idx12"][:, :, None], 1)):
        assert tool.smallest_gap(cloud, max(tool.NN_SIZES) + 2) >= tool.GAP
    for family in ("dihedral_ico2", "dihedral_open"):
        d = inputs_of(family)
        assert tool.largest_interior_dot(d["v"], d["table"]) < tool.CLEAR
    # the degenerate inputs reach the non-finite values they are there for
    assert np.isinf(recorded("degenerate_coincident", "stretch_none", "out64")["loss"]).any() or \
        np.isnan(recorded("degenerate_coincident", "stretch_none", "out64")["loss"]).any()
    assert (recorded("degenerate_isolated", "uniform_laplacian", "out64")["lap"][:, 24] == 0).all()


# ------------------------------------------------------------------------------------------------ 1. every call
@pytest.mark.parametrize("family,name", all_cases(), ids=["%s-%s" % c for c in all_cases()])
def test_recorded_call(cpu_graphs, family, name):
    case = case_of(family, name)
    out, grads = run(family, case)
    want = recorded(family, name, "out64")
    assert sorted(out) == sorted(want)
    shift = PI_GAP if name == "dihedral_angle" else 0.0
    for key in want:
        assert_matches(out[key].numpy(), want[key], (family, name, key), on_cot(family, name), shift)
    want = recorded(family, name, "grad64")
    for key in case.wrt:
        assert_matches(grads[key].numpy(), want[key], (family, name, "d/d" + key), on_cot(family, name))


@pytest.mark.parametrize("family,name,error", all_raises(), ids=["%s-%s" % r[:2] for r in all_raises()])
def test_where_the_reference_raises(cpu_graphs, family, name, error):
    how, other = DEVIATIONS[name]
    case = case_of(family, name)
    out, _ = run(family, case)
    if how == "returns":
        want = recorded(family, other, "out64")
        for key in want:
            assert_matches(out[key].numpy(), want[key], (family, name, key), on_cot(family, name))
    elif how == "restatement":
        # both sides are fp64 here; call2, a mean of the operator's output, is zero in exact arithmetic: 1e-12 of the
        # Laplacians' magnitude, not of its own
        m = max(float(np.abs(a).max()) for a in recorded(family, "cot_laplacian_kept", "out64").values())
        want, _ = run(family, case, RESTATED)
        for key in want:
            assert_matches(out[key].numpy(), want[key].numpy(), (family, name, key), lambda w: 1e-12 * m)
    elif how == "areas":
        T = inputs_of(family)
        v = torch.from_numpy(T["v1"]).double().requires_grad_(True)
        corners = v[torch.arange(v.shape[0])[:, None, None], torch.from_numpy(T["faces"])]
        cross = torch.cross(corners[:, :, 1] - corners[:, :, 0], corners[:, :, 2] - corners[:, :, 1], dim=-1)
        areas = torch.sqrt((cross ** 2).sum(-1)) / 2
        assert_matches(out["areas"].numpy(), areas.detach().numpy(), (family, name))
        assert_matches(out["areas"].numpy(), recorded(family, "face_normals_and_areas", "out64")["areas"], (family, name))
        G = torch.from_numpy(tool.cotangent_for(family, name, "areas", tuple(areas.shape))).double()
        want, = torch.autograd.grad((areas * G).sum(), v)
        _, grads = tool.run_case(case, API, T, torch.float64, cot={"areas": G.numpy()})
        assert_matches(grads["v1"].numpy(), want.numpy(), (family, name, "d/dv1"))
    elif how == "kept":
        want = recorded(family, other, "out64")           # call0 alike; call1 on the kept topology, not on faces_alt
        assert_matches(out["call0"].numpy(), want["call0"], (family, name, "call0"))
        T = {k: torch.from_numpy(v) for k, v in inputs_of(family).items()}
        fresh = model_loss.MeshEdgeLengthLoss(torch.nn.MSELoss()) if "edge_length" in name else model_loss.MeshStretchLoss("mean")
        direct = fresh(T["v3"].double(), T["v2"].double(), T["faces"])
        assert_matches(out["call1"].numpy(), direct.numpy(), (family, name, "call1"))
    elif how == "sum_of_none":
        per_edge = recorded(family, other, "out64")["loss"]
        assert_matches(out["loss"].numpy(), per_edge.sum(-1).mean(), (family, name))
    else:
        raise AssertionError(how)


def test_documented_reference_defects_are_recorded_as_they_are():
    """two defects the project keeps, as the recordings show them: ``assert(~self.precompute_L)`` never
    fires -- the vert2=None call of a precompute_L module returned -- and UniformLaplacianSmoothnessLoss compares the
    curvature of ``vert`` with itself"""
    for family in MESH_FAMILIES:
        fx = fixture(family)
        assert "laplacian_loss_uniform_precompute/out64/call2" in fx
        loss = fx["smoothness_loss_vert_ref/out64/loss"]
        assert loss.shape == () and (loss == 0 or np.isnan(loss))
        assert not np.nan_to_num(fx["smoothness_loss_vert_ref/grad64/v2"]).any()


# ------------------------------------------------------------------------------------------------ 2. restatements
class _RestatedLaplacianLoss(laplacian_host.RefMeshLaplacianLoss):
    def __init__(self, metric, use_cot=False, use_norm=False, consistent_topology=False, precompute_L=False):
        super().__init__(metric, use_cot, use_norm, consistent_topology, precompute_L)


def _restated_edge_loss(kind):
    """the one-call restatements of test_mesh_edges_host.py behind the reference's constructor and call signatures"""
    class Loss(object):
        def __init__(self, *args, **kwargs):
            self.args = args

        def __call__(self, vert1, vert2=None, face=None):
            if kind == "edge_length":
                return edges_host.ref_edge_length_loss(self.args[0], vert1, vert2, face.numpy())
            if kind == "stretch":
                return edges_host.ref_stretch_loss(self.args[0], vert1, vert2, face.numpy())
            threshold, edges, reduction = self.args
            return edges_host.ref_repulsion_loss(threshold, reduction, vert1, edges)
    return Loss


RESTATED = tool.Api(
    types.SimpleNamespace(edge_vertex_indices=lambda f: torch.from_numpy(edges_host.np_unique_edges(f.numpy()))),
    types.SimpleNamespace(MeshLaplacianLoss=_RestatedLaplacianLoss, MeshEdgeLengthLoss=_restated_edge_loss("edge_length"),
                          MeshStretchLoss=_restated_edge_loss("stretch"),
                          SimpleMeshRepulsionLoss=_restated_edge_loss("repulsion")))
RESTATED_CASES = ["laplacian_loss_%s%s" % (kind, tail) for kind in ("uniform", "cot")
                  for tail in ("", "_norm", "_vert2_none", "_norm_vert2_none", "_consistent_off", "_consistent_on",
                               "_precompute_consistent")]
RESTATED_CASES += ["laplacian_loss_uniform_precompute", "edge_length_loss"]
RESTATED_CASES += ["stretch_" + r for r in tool.REDUCTIONS] + ["mesh_repulsion_" + r for r in tool.REDUCTIONS]


@pytest.mark.parametrize("name", RESTATED_CASES)
@pytest.mark.parametrize("family", MESH_FAMILIES)
def test_restated_losses_against_the_recordings(family, name):
    """RefMeshLaplacianLoss over DenseLaplacian (test_mesh_laplacian_host.py) and ref_edge_length_loss, ref_stretch_loss,
    ref_repulsion_loss (test_mesh_edges_host.py), through the recorded calls, values and gradients"""
    case = case_of(family, name)
    out, grads = run(family, case, RESTATED)
    for key, want in recorded(family, name, "out64").items():
        assert_matches(out[key].numpy(), want, (family, name, key), on_cot(family, name))
    for key, want in recorded(family, name, "grad64").items():
        assert_matches(grads[key].numpy(), want, (family, name, "d/d" + key), on_cot(family, name))


@pytest.mark.parametrize("family", MESH_FAMILIES + ["quads"])
def test_restated_laplacians_and_edges_against_the_recordings(family):
    """np_uniform, np_cotangent, np_cot / dense_cot (test_mesh_laplacian_host.py), np_unique_edges and np_sqrlen
    (test_mesh_edges_host.py)"""
    T = inputs_of(family)
    v1, faces = T["v1"].astype(np.float64), T["faces"]
    n = v1.shape[1]
    assert_matches(laplacian_host.np_uniform(v1, faces, n), recorded(family, "uniform_laplacian", "out64")["lap"],
                   (family, "np_uniform"))
    if family == "quads":
        return
    cot = laplacian_host.np_cotangent(v1, faces)
    assert_matches(cot, recorded(family, "cotangent", "out64")["cot"], (family, "np_cotangent"))
    assert_matches(laplacian_host.np_cot(v1, faces, cot, n), recorded(family, "cot_laplacian", "out64")["lap"],
                   (family, "np_cot"), on_cot(family, "cot_laplacian"))
    for b in range(faces.shape[0]):
        edges = edges_host.np_unique_edges(faces[b])
        assert_matches(edges, recorded(family, "edge_vertex_indices", "out64")["edges%d" % b], (family, "np_unique_edges"))
        assert_matches(edges_host.np_sqrlen(v1[b], edges), recorded(family, "get_edge_lengths", "out64")["sq%d" % b],
                       (family, "np_sqrlen"))


def test_restated_knn_helpers_against_the_recordings():
    """topk_knn, np_laplacian, gathered and _ref_lengths (test_knn_edges_host.py): the stand-in search finds the recorded
    tables, and the restated Laplacian and edge lengths give the recorded values"""
    T = inputs_of("points")
    p1, p2 = torch.from_numpy(T["p1"]).double(), torch.from_numpy(T["p2"]).double()
    for k in tool.NN_SIZES:
        table = recorded("points", "point_laplacian_k%d" % k, "out64")["knn_idx"]
        assert np.array_equal(T["knn%d" % k], table)
        for dtype in (torch.float64, torch.float32):
            assert np.array_equal(knn_host.topk_knn(p1.to(dtype), p1.to(dtype), K=k + 1).idx[:, :, 1:].numpy(), table)
        assert_matches(knn_host.np_laplacian(p1.numpy(), table), recorded("points", "point_laplacian_k%d" % k, "out64")["lap"],
                       ("points", "np_laplacian", k))
        dist_ref, dist = knn_host._ref_lengths(p1, p2, k)
        assert_matches(torch.nn.functional.l1_loss(dist_ref, dist).numpy(),
                       recorded("points", "point_edge_length_loss_k%d" % k, "out64")["loss"], ("points", "_ref_lengths", k))
    lap = -torch.sum(knn_host.gathered(p2, torch.from_numpy(T["knn5"])), dim=2) / 5 + p2
    assert_matches(lap.numpy(), recorded("points", "point_laplacian_given_k5", "out64")["lap"], ("points", "gathered"))


@pytest.mark.parametrize("family", ["dihedral_ico2", "dihedral_open"])
def test_restated_dihedral_helpers_against_the_recordings(family):
    """np_unclamped_dot / np_angles and dict_edge_points (test_mesh_dihedral_host.py).  np_angles subtracts from np.pi,
    the reference from its PI = 3.1415927: the recorded angles are higher by 4.64e-8."""
    T = inputs_of(family)
    v, table = T["v"].astype(np.float64), T["table"]
    assert_matches(dihedral_host.np_angles(v, table), recorded(family, "dihedral_angle", "out64")["angle"],
                   (family, "np_angles"), shift=PI_GAP)
    if family == "dihedral_open":
        faces = inputs_of("open")["faces"][0]
        own, counts = dihedral_host.dict_edge_points(faces)
        # the same edges; per edge the same pair of wings (the reference's column order follows its face traversal)
        key = lambda t: sorted((min(a, c), max(a, c), min(w0, w1), max(w0, w1)) for a, c, w0, w1 in t.tolist())  # noqa: E731
        assert key(own) == key(table)
        boundary = table[:, 2] == table[:, 3]
        assert boundary.sum() == 16 == sum(1 for c in counts.values() if c == 1)
        got = geo_operations.get_edge_points(torch.from_numpy(faces)).numpy()
        assert np.array_equal(got, own)
