"""GPU tests: the calls recorded from the REFERENCE's own Python in tests/golden/ref_losses_*.npz
(tools/gen_losses_golden.py, tests/test_reference_losses_host.py) made on CUDA fp32, through the HIP kernels.

* The HIP route is asserted by counting the C entry points a call reaches (ROUTES).
* Index outputs -- the k-NN tables, ``edge_vertex_indices`` -- equal the recording.
* NaN and inf stand where the reference's fp32 run has them (its fp64 gradient's, for a gradient).
* Values and gradients: ``|got - ref64|_inf <= max(4 |ref32 - ref64|_inf, 16 * 2**-23 * |ref64|_inf)`` per array, ref32
  and ref64 the two recordings (for a gradient, the recorded ``graderr32`` is |ref32 - ref64|_inf).  The bound is
  measured on the reference, never on the code under test; the factor 4 and the floor of 16 eps32 are DESIGN.md's
  convention for a kernel against an fp64 composition.  The dihedral angle uses its per-edge form: every error is
  weighted by sqrt(1 - d^2), d the clamped fp64 dot, as in tests/test_gpu_mesh_dihedral.py.
* Every measured error over its bound is printed; DESIGN.md "Pinned to the reference's Python" keeps the largest per
  function."""
import collections

import numpy as np
import pytest
import torch

from pytorch_points_amd import _lib
from test_reference_losses_host import (API, DEVIATIONS, MESH_FAMILIES, SEARCHED, all_cases, all_raises, case_of, inputs_of,
                                        recorded, tool)

pytestmark = pytest.mark.gpu
EPS32 = 2.0 ** -23
REF_PI = 3.1415927

APPLY, COT = "pp_mesh_laplacian_apply_f32", "pp_mesh_cotangent_f32"
SQRLEN = ("pp_mesh_edge_sqrlen_forward_f32", "pp_mesh_edge_sqrlen_backward_f32")
KNN_LENGTHS = ("pp_knn_edge_lengths_forward_f32", "pp_knn_edge_lengths_backward_f32")
KNN_LAPLACIAN = ("pp_knn_laplacian_forward_f32", "pp_knn_laplacian_backward_f32")
# the entry points a case has to reach, by the start of its name (the first match); () for the helpers that are torch
# operations on every device.  A case that asks for no gradient is spared the backward entries.
ROUTES = [("uniform_laplacian", (APPLY,)), ("smoothness_loss", (APPLY,)), ("laplacian_loss_uniform", (APPLY,)),
          ("cot_laplacian", (APPLY, COT)), ("laplacian_loss_cot", (APPLY, COT)),
          ("cotangent", ()),                                   # with a gradient: torch operations; without: see below
          ("face_", ()), ("get_normals", ()), ("smape", ()),
          ("edge_vertex_indices", ("pp_mesh_unique_edges",)),
          ("get_edge_lengths", SQRLEN + ("pp_mesh_unique_edges",)), ("edge_length_loss", SQRLEN + ("pp_mesh_unique_edges",)),
          ("stretch", SQRLEN + ("pp_mesh_unique_edges",)), ("mesh_repulsion", SQRLEN),
          ("dihedral_angle", ("pp_mesh_dihedral_forward_f32", "pp_mesh_dihedral_backward_f32")),
          ("point_laplacian", KNN_LAPLACIAN), ("point_edge_length", KNN_LENGTHS), ("point_stretch", KNN_LENGTHS),
          ("point_repulsion", KNN_LENGTHS)]


def route_of(name, wrt):
    entries = next(e for prefix, e in ROUTES if name.startswith(prefix))
    if not wrt:
        entries = tuple(e for e in entries if "backward" not in e)
    return entries + (("pp_knn_ws_f32",) if name in SEARCHED else ())


class CountingLibrary(object):
    """the loaded HIP library, counting every ``pp_*`` entry point that is fetched from it"""

    def __init__(self, real):
        self._real, self.counts = real, collections.Counter()

    def __getattr__(self, name):
        if name.startswith("pp_"):
            self.counts[name] += 1
        return getattr(self._real, name)


@pytest.fixture
def entries(cuda, monkeypatch):
    counting = CountingLibrary(_lib.lib())
    monkeypatch.setattr(_lib, "lib", lambda: counting)
    return counting.counts


def bound_of(ref64, err32):
    return max(4 * err32, 16 * EPS32 * float(np.abs(ref64).max(initial=0.0)))


def check(got, ref64, ref32, label, nonfinite_as, weight=None, err32=None):
    """``got`` against the recordings; ``nonfinite_as``: the recording whose NaN and inf places ``got`` has to show;
    ``weight``: per-element weights of the error; ``err32``: |ref32 - ref64|_inf where ref32 itself is not recorded"""
    got = np.asarray(got, np.float64)
    assert got.shape == ref64.shape, (label, got.shape, ref64.shape)
    assert np.array_equal(np.isnan(got), np.isnan(nonfinite_as)), (label, "NaN")
    for inf in (np.inf, -np.inf):
        assert np.array_equal(got == inf, nonfinite_as == inf), (label, "inf")
    finite = np.isfinite(ref64) & np.isfinite(got)
    if ref32 is not None:
        finite &= np.isfinite(ref32)
    w = np.ones_like(ref64) if weight is None else weight
    if err32 is None:
        err32 = float((np.abs(ref32.astype(np.float64) - ref64) * w)[finite].max(initial=0.0))
    bound = bound_of(ref64[finite], err32)
    err = float((np.abs(got - ref64) * w)[finite].max(initial=0.0))
    ratio = err / bound if bound > 0 else 0.0
    print("RATIO %-60s error %.3g  bound %.3g  ratio %.3g" % (" ".join(label), err, bound, ratio))
    assert err <= bound, (label, err, bound)


def dihedral_weight(angle64):
    d = np.cos(REF_PI - angle64)                        # the reference's clamped fp64 dot, back from its angle
    return np.sqrt(np.maximum(1 - d * d, 0.0))


@pytest.mark.parametrize("family,name", all_cases(), ids=["%s-%s" % c for c in all_cases()])
def test_recorded_call_on_hip(cuda, entries, family, name):
    case = case_of(family, name)
    out, grads = tool.run_case(case, API, inputs_of(family), torch.float32, "cuda", cot=recorded(family, name, "cot"))
    reached = {e for e in entries}
    missing = [e for e in route_of(name, case.wrt) if e not in reached]
    assert not missing, (family, name, "never reached", missing, sorted(reached))
    ref64, ref32 = recorded(family, name, "out64"), recorded(family, name, "out32")
    assert sorted(out) == sorted(ref64)
    for key, want in ref64.items():
        got = out[key].cpu().numpy()
        if want.dtype.kind in "iu":
            assert np.array_equal(got, want), (family, name, key)
            continue
        assert out[key].dtype == torch.float32 and out[key].is_cuda
        weight = dihedral_weight(want) if name == "dihedral_angle" else None
        check(got, want, ref32[key], (family, name, key), ref32[key], weight)
    grad64, graderr32 = recorded(family, name, "grad64"), recorded(family, name, "graderr32")
    for key in case.wrt:
        check(grads[key].cpu().numpy(), grad64[key], None, (family, name, "d/d" + key), grad64[key],
              err32=float(graderr32[key]))


@pytest.mark.parametrize("family", MESH_FAMILIES)
def test_cotangent_kernel(cuda, entries, family):
    """``cotangent`` without a gradient to the vertices is the HIP kernel (with one, torch operations: the case above)"""
    case = case_of(family, "cotangent")
    out, _ = tool.run_case(case, API, inputs_of(family), torch.float32, "cuda", requires_grad=False)
    assert entries[COT] == 1
    ref64, ref32 = recorded(family, "cotangent", "out64")["cot"], recorded(family, "cotangent", "out32")["cot"]
    check(out["cot"].cpu().numpy(), ref64, ref32, (family, "cotangent kernel", "cot"), ref32)


@pytest.mark.parametrize("family,name,error", all_raises(), ids=["%s-%s" % r[:2] for r in all_raises()])
def test_where_the_reference_raises_on_hip(cuda, entries, family, name, error):
    """the deviations of tests/test_reference_losses_host.py DEVIATIONS, on the HIP route: the call returns, reaches
    its kernels, and gives finite values wherever the fp32 recording it is documented to follow does"""
    how, other = DEVIATIONS[name]
    case = case_of(family, name)
    out, _ = tool.run_case(case, API, inputs_of(family), torch.float32, "cuda")
    missing = [e for e in route_of(name, []) if e not in entries]
    assert not missing, (family, name, "never reached", missing)
    if how == "returns":
        ref64, ref32 = recorded(family, other, "out64"), recorded(family, other, "out32")
        for key in ref64:
            check(out[key].cpu().numpy(), ref64[key], ref32[key], (family, name, key), ref32[key])
    elif how == "sum_of_none":
        ref64, ref32 = (recorded(family, other, kind)["loss"].astype(np.float64).sum(-1).mean() for kind in ("out64", "out32"))
        check(out["loss"].cpu().numpy(), np.asarray(ref64), np.asarray(ref32), (family, name, "loss"), np.asarray(ref32))
    elif how == "kept":
        ref64, ref32 = recorded(family, other, "out64")["call0"], recorded(family, other, "out32")["call0"]
        check(out["call0"].cpu().numpy(), ref64, ref32, (family, name, "call0"), ref32)
    elif how == "areas":
        ref64, ref32 = (recorded(family, "face_normals_and_areas", kind)["areas"] for kind in ("out64", "out32"))
        check(out["areas"].cpu().numpy(), ref64, ref32, (family, name, "areas"), ref32)
    else:
        assert how == "restatement" and all(v.is_cuda for v in out.values())
