"""GPU tests of the earth mover's distance kernels (csrc/emd.hip) against the fp64 composition, on every size and cloud
of emd_cases: the sizes of 1, the tile's edges in both directions, more than a workgroup's points, several tiles."""
import contextlib
import ctypes

import numpy as np
import pytest
import torch

import emd_cases as C
from pytorch_points_amd import _lib, emd
from pytorch_points_amd.network import model_loss

pytestmark = pytest.mark.gpu


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy().tobytes()


def hip_step(t1, t2):
    match = emd.approx_match(t1, t2)
    return match, emd.match_cost(t1, t2, match)


_STEPS = {}


def hip_run(case):
    """``(dense, cost, grad1, grad2)`` of the kernels on a case, computed once"""
    if case not in _STEPS:
        _STEPS[case] = tuple(t.cpu() for t in C.run(*C.clouds(case), device="cuda", fn=hip_step))
    return _STEPS[case]


# ------------------------------------------------------------------------------------------------ 1. accuracy
@pytest.mark.parametrize("case", C.CASES, ids=C.case_id)
def test_match_cost_and_gradients_against_the_fp64_composition(cuda, case):
    """The gradients of both sides use their own match, so they are compared as functions of the inputs.  Bound: 4 x
    the fp32 CPU composition's own error on these inputs (emd_cases.FLOORS, lifted to 4 eps32).

    Measured on an MI355X: see DESIGN.md "Earth mover's distance" for the figures of every case."""
    got = C.measures(case, hip_run(case), C.reference(case, "cuda"))
    bound = C.bounds(case)
    print("%s: HIP match %.3g cost %.3g grad1 %.3g grad2 %.3g | fp32 CPU %s | bound %s"
          % (C.case_id(case), *got, " ".join("%.3g" % f for f in C.FLOORS[C.case_id(case)]),
             " ".join("%.3g" % f for f in bound)))
    for name, g, b in zip(("match", "cost", "grad_xyz1", "grad_xyz2"), got, bound):
        assert g <= b, (name, g, b)


@pytest.mark.parametrize("case", C.CASES, ids=C.case_id)
def test_dense_match_is_within_its_row_and_column_bounds(cuda, case):
    C.check_bounds(case, hip_run(case)[0], C.SLACK32)


# ------------------------------------------------------------------------------------------- 2. the same bytes
@contextlib.contextmanager
def deterministic():
    torch.use_deterministic_algorithms(True)
    try:
        yield
    finally:
        torch.use_deterministic_algorithms(False)


def step_bits(case):
    t1, t2 = (torch.from_numpy(c).cuda().requires_grad_(True) for c in C.clouds(case))
    match, cost = hip_step(t1, t2)
    g1, g2 = torch.autograd.grad(cost.sum(), (t1, t2))
    return [bits(t) for t in (match.a, match.b, cost, g1, g2)]


@pytest.mark.parametrize("case", [((2, 65, 63), "random"), ((2, C.TILE + 1, C.TILE - 1), "copy"),
                                  ((2, 1024, 1024), "random")], ids=C.case_id)
def test_three_runs_and_a_deterministic_one_give_the_same_bytes(cuda, case):
    first = step_bits(case)
    for _ in range(2):
        assert step_bits(case) == first
    with deterministic():
        assert step_bits(case) == first


# ------------------------------------------------------------------------------------------------ 3. the API
def test_a_sliced_input_is_made_contiguous(cuda):
    case = ((2, 100, 250), "random")
    x1, x2 = C.clouds(case)
    wide1 = torch.from_numpy(np.concatenate([x1, x1], axis=2)).cuda()
    t1 = wide1[:, :, 1:4].detach().requires_grad_(True)                  # strided rows
    t2 = torch.from_numpy(x2).cuda()[:, ::2].requires_grad_(True)        # every second point
    assert not t1.is_contiguous() and not t2.is_contiguous()
    c1, c2 = (t.detach().contiguous().requires_grad_(True) for t in (t1, t2))
    outs = []
    for u, v in ((t1, t2), (c1, c2)):
        match, cost = hip_step(u, v)
        outs.append([match.a, match.b, match.dense(), cost, *torch.autograd.grad(cost.sum(), (u, v))])
    for a, b in zip(*outs):
        assert a.shape == b.shape and bits(a) == bits(b)


def test_only_the_gradient_asked_for_is_computed(cuda, monkeypatch):
    case = ((2, 100, 250), "random")
    x1, x2 = (torch.from_numpy(c).cuda() for c in C.clouds(case))
    full = hip_run(case)
    seen = []
    real = _lib.lib().pp_emd_cost_backward_f32

    def spy(*args):
        seen.append((args[5] is not None, args[6] is not None))
        return real(*args)

    lib = _lib.lib()
    monkeypatch.setattr(lib, "pp_emd_cost_backward_f32", spy, raising=False)
    t1 = x1.clone().requires_grad_(True)
    cost = emd.emd_distance(t1, x2)
    cost.sum().backward()
    assert seen == [(True, False)] and bits(t1.grad) == bits(full[2])
    t2 = x2.clone().requires_grad_(True)
    g2, = torch.autograd.grad(emd.emd_distance(x1, t2).sum(), (t2,))
    assert seen[1:] == [(False, True)] and bits(g2) == bits(full[3])
    assert emd.emd_distance(x1, x2).grad_fn is None and len(seen) == 2


class Counting(object):
    """the library with its calls counted by name"""

    def __init__(self, lib):
        self._lib, self.calls = lib, {}

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def counted(*args):
            self.calls[name] = self.calls.get(name, 0) + 1
            return fn(*args)

        return counted


def test_emd_distance_and_the_loss_reach_the_kernels(cuda, monkeypatch):
    case = ((2, 100, 250), "random")
    t1, t2 = (torch.from_numpy(c).cuda().requires_grad_(True) for c in C.clouds(case))
    counting = Counting(_lib.lib())
    monkeypatch.setattr(_lib, "lib", lambda: counting)
    cost = emd.emd_distance(t1, t2)
    assert "MatchCost" in type(cost.grad_fn).__name__
    assert counting.calls == {"pp_emd_workspace_bytes": 2, "pp_emd_match_f32": 1, "pp_emd_cost_f32": 1}
    assert bits(cost) == bits(hip_run(case)[1])
    for reduction, reduce in (("mean", lambda c: c.mean()), ("sum", lambda c: c.sum()), ("none", lambda c: c)):
        counting.calls.clear()
        loss = model_loss.EarthMoverLoss(reduction)(t1, t2)
        assert counting.calls.get("pp_emd_match_f32") == 1 and counting.calls.get("pp_emd_cost_f32") == 1
        assert torch.equal(loss, reduce(cost / 250))
    counting.calls.clear()
    g1, g2 = torch.autograd.grad(model_loss.EarthMoverLoss("sum")(t1, t2), (t1, t2))
    assert counting.calls.get("pp_emd_cost_backward_f32") == 1
    w1, w2 = torch.autograd.grad((cost / 250).sum(), (t1, t2))
    assert bits(g1) == bits(w1) and bits(g2) == bits(w2) and bool((g1 != 0).any()) and bool((g2 != 0).any())


def test_fp64_cuda_input_takes_the_composition(cuda, monkeypatch):
    case = ((2, 65, 63), "random")
    monkeypatch.setattr(_lib, "lib", lambda: pytest.fail("an fp64 tensor reached the HIP library"))
    t1, t2 = (torch.from_numpy(c.astype(np.float64)).cuda().requires_grad_(True) for c in C.clouds(case))
    match = emd.approx_match(t1, t2)
    cost = emd.match_cost(t1, t2, match)
    assert not match.hip and cost.dtype == torch.float64 and cost.is_cuda
    g1, g2 = torch.autograd.grad(cost.sum(), (t1, t2))
    want = C.reference(case)
    for got, ref in zip((match.dense(), cost, g1, g2), want):
        assert float((got.detach().cpu() - ref).abs().max()) <= 1e-10 * max(1.0, float(ref.abs().max()))


def test_sizes_beyond_the_limit_take_the_composition(cuda, monkeypatch):
    case = ((2, 65, 63), "random")
    monkeypatch.setattr(emd, "LIMIT", 100)
    t1, t2 = (torch.from_numpy(c).cuda() for c in C.clouds(case))
    match = emd.approx_match(t1, t2)
    assert not match.hip and match.a.dtype == torch.float32
    assert "MatchCost" in type(emd.match_cost(t1.requires_grad_(True), t2, match).grad_fn).__name__


# ------------------------------------------------------------------------------- 4. graphs and streams
def test_a_captured_step_replays_with_the_eager_bytes_and_two_streams_run_side_by_side(cuda):
    first, other = C.clouds(((2, C.TILE + 1, C.TILE - 1), "random")), C.clouds(((2, C.TILE + 1, C.TILE - 1), "squeezed"))

    def step(p, q):
        match, cost = hip_step(p, q)
        return [match.a, match.b, cost, *torch.autograd.grad(cost.sum(), (p, q))]

    def inputs(values):
        return [torch.from_numpy(v).cuda().requires_grad_(True) for v in values]

    p, q = inputs(first)
    step(p, q)
    eagers = [[t.detach().clone() for t in step(*inputs(values))] for values in (other, first)]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side = step(*inputs(other))
        step(p, q)                                                         # the warm-up of the capture below
    on_main = step(*inputs(first))                                         # beside it on the current stream
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for a, b in zip(on_side, eagers[0]):
        assert bits(a) == bits(b)
    for a, b in zip(on_main, eagers[1]):
        assert bits(a) == bits(b)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        held = step(p, q)
    for values, eager in zip((other, first), eagers):                      # replayed twice, with new clouds
        with torch.no_grad():
            p.copy_(torch.from_numpy(values[0]))
            q.copy_(torch.from_numpy(values[1]))
            for t in held:
                t.fill_(7)
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(held, eager):
            assert bits(a) == bits(b)


# ----------------------------------------------------------------------------------------------- 5. the C ABI
def test_empty_problems_and_refused_sizes_return_before_any_launch(cuda):
    """null pointers throughout: a launch would be refused by the pointer check, so PP_OK shows that none was made"""
    lib = _lib.lib()
    none, stream = ctypes.c_void_p(None), ctypes.c_void_p(None)
    for b, n, m in ((0, 4, 5), (2, 0, 5), (2, 4, 0)):
        assert lib.pp_emd_match_f32(none, none, none, none, b, n, m, none, 0, stream) == 0
        assert lib.pp_emd_dense_f32(none, none, none, none, none, b, n, m, stream) == 0
        assert lib.pp_emd_cost_f32(none, none, none, none, none, b, n, m, none, 0, stream) == 0
        assert lib.pp_emd_cost_backward_f32(none, none, none, none, none, none, none, b, n, m, stream) == 0
    for b, n, m in ((-1, 4, 5), (2, -4, 5), (2, 4, -5), (2, 2 ** 30, 5), (4, 5, 2 ** 29), (2, 4, 5)):
        assert lib.pp_emd_match_f32(none, none, none, none, b, n, m, none, 0, stream) == 1
        assert lib.pp_emd_dense_f32(none, none, none, none, none, b, n, m, stream) == 1
        assert lib.pp_emd_cost_f32(none, none, none, none, none, b, n, m, none, 0, stream) == 1
        assert lib.pp_emd_cost_backward_f32(none, none, none, none, none, none, none, b, n, m, stream) == 1
    assert lib.pp_emd_workspace_bytes(2, 4, 5) == 4 * (8 + 10)
    assert lib.pp_emd_workspace_bytes(2, 2 ** 30, 5) == 0 and lib.pp_emd_workspace_bytes(-1, 4, 5) == 0
    assert torch.cuda.is_available() and torch.zeros(1, device="cuda").item() == 0   # and no error is left behind
    for shape in ((0, 4, 5), (2, 0, 5), (2, 4, 0)):
        t1 = torch.zeros(shape[0], shape[1], 3, device="cuda", requires_grad=True)
        t2 = torch.zeros(shape[0], shape[2], 3, device="cuda", requires_grad=True)
        match = emd.approx_match(t1, t2)
        cost = emd.match_cost(t1, t2, match)
        assert match.hip and match.dense().shape == shape and cost.shape == shape[:1] and not bool(cost.any())
        g1, g2 = torch.autograd.grad(cost.sum(), (t1, t2))
        assert g1.shape == t1.shape and not bool(g1.any()) and not bool(g2.any())
