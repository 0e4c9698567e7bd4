"""CPU tests of the earth mover's distance: `emd.emd_composition` in fp64 (the contract of csrc/emd.hip's kernels),
the argument checks, empty problems and the `EarthMoverLoss` reductions."""
import numpy as np
import pytest
import torch

import emd_cases as C
from pytorch_points_amd import emd
from pytorch_points_amd.network import model_loss

@pytest.mark.parametrize("case", C.CASES, ids=C.case_id)
def test_match_is_within_its_row_and_column_bounds(case):
    C.check_bounds(case, C.reference(case)[0], C.SLACK64)


def test_fp32_composition_is_within_the_fp32_slack():
    for case in C.CASES[:12]:
        x1, x2 = C.clouds(case)
        C.check_bounds(case, emd.emd_composition(torch.from_numpy(x1), torch.from_numpy(x2))[0].dense(), C.SLACK32)


def dense_by_levels(x1, x2):
    """the dense (B,N,M) accumulation level by level, written without the module's helpers"""
    b, n, m = x1.shape[0], x1.shape[1], x2.shape[1]
    diff = x1[:, :, None, :] - x2[:, None, :, :]
    d = (diff[..., 0] * diff[..., 0] + diff[..., 1] * diff[..., 1]) + diff[..., 2] * diff[..., 2]
    big = max(n, m)
    remain_l = torch.full((b, n), float(big // n), dtype=x1.dtype)
    remain_r = torch.full((b, m), float(big // m), dtype=x1.dtype)
    match = torch.zeros(b, n, m, dtype=x1.dtype)
    for j in range(7, -3, -1):
        level = -(4.0 ** j) if j >= -1 else 0.0
        e = torch.exp(level * d)
        ratio_l = remain_l / (1e-9 + (e * remain_r[:, None, :]).sum(2))
        s = (e * ratio_l[:, :, None]).sum(1) * remain_r
        ratio_r = torch.clamp(remain_r / (s + 1e-9), max=1.0) * remain_r
        remain_r = torch.clamp(remain_r - s, min=0.0)
        match = match + (e * ratio_l[:, :, None]) * ratio_r[:, None, :]
        remain_l = torch.clamp(remain_l - ratio_l * (e * ratio_r[:, None, :]).sum(2), min=0.0)
    return match, (match * torch.sqrt(d)).sum((1, 2))


@pytest.mark.parametrize("case", [c for c in C.CASES if c[0][1] * c[0][2] <= 300000], ids=C.case_id)
def test_factored_match_equals_the_dense_accumulation(case):
    x1, x2 = (torch.from_numpy(c.astype(np.float64)) for c in C.clouds(case))
    match, cost = dense_by_levels(x1, x2)
    dense, got_cost = C.reference(case)[:2]
    assert torch.equal(dense, match)   # the same sum in the same order
    assert float((got_cost - cost).abs().max()) <= 1e-12 * max(1.0, float(cost.abs().max()))


def test_blocked_composition_equals_the_whole_matrix(monkeypatch):
    case = ((2, 100, 250), "random")
    monkeypatch.setattr(emd, "CHUNK_PAIRS", 5000)   # 10 rows of xyz1 per block
    x1, x2 = C.clouds(case)
    got = C.run(x1.astype(np.float64), x2.astype(np.float64))
    for g, w in zip(got, C.reference(case)):
        assert float((g - w).abs().max()) <= 1e-12 * max(1.0, float(w.abs().max()))


def optimum(x1, x2):
    scipy_optimize = pytest.importorskip("scipy.optimize")
    dist = np.linalg.norm(x1[:, None, :] - x2[None, :, :], axis=-1)
    rows, cols = scipy_optimize.linear_sum_assignment(dist)
    return float(dist[rows, cols].sum())


@pytest.mark.parametrize("n", [64, 128])
def test_cost_is_not_below_the_exact_assignment(n):
    """the match is a feasible (sub-)transport plan and a doubly stochastic matrix is a mixture of permutations
    (Birkhoff), so its cost is at least the optimum's times the mass it moves; the rows leave up to 1e-8 each"""
    rng = np.random.default_rng(n)
    x1, x2 = rng.random((2, n, 3)), rng.random((2, n, 3))
    match, cost = emd.emd_composition(torch.from_numpy(x1), torch.from_numpy(x2))
    assert float((1.0 - match.dense().sum(2)).max()) <= 1e-7
    for b in range(2):
        assert float(cost[b]) >= optimum(x1[b], x2[b]) * (1.0 - 1e-7)


def test_cost_of_a_noisy_shuffled_copy_is_near_the_optimum():
    """N = 128, xyz2 a shuffled copy of xyz1 with 1e-3 noise.  Measured on this cloud: 0.20760 against the optimum's
    0.20734, an excess of 0.125 %; pinned at 4 x that, a factor 1.005"""
    rng = np.random.default_rng(5)
    x1 = rng.random((1, 128, 3))
    x2 = x1[:, rng.permutation(128)] + 1e-3 * rng.standard_normal((1, 128, 3))
    cost = float(emd.emd_composition(torch.from_numpy(x1), torch.from_numpy(x2))[1])
    best = optimum(x1[0], x2[0])
    print("approximate %.5f optimum %.5f" % (cost, best))
    assert best * (1.0 - 1e-7) <= cost <= 1.005 * best


def test_gradients_with_the_match_held_fixed():
    """`match_cost`'s backward against autograd through `sum(match0 * sqrt(d))` with a constant dense `match0`, which
    `gradcheck` holds against finite differences"""
    torch.manual_seed(3)
    x1 = torch.rand(2, 5, 3, dtype=torch.float64, requires_grad=True)
    x2 = torch.rand(2, 7, 3, dtype=torch.float64, requires_grad=True)
    match = emd.approx_match(x1, x2)
    match0 = match.dense()
    weights = torch.tensor([0.75, -1.5], dtype=torch.float64)

    def fixed(u, v):
        diff = u[:, :, None, :] - v[:, None, :, :]
        d = (diff[..., 0] * diff[..., 0] + diff[..., 1] * diff[..., 1]) + diff[..., 2] * diff[..., 2]
        return (match0 * torch.sqrt(d)).sum((1, 2))

    assert torch.autograd.gradcheck(fixed, (x1, x2))
    want = torch.autograd.grad((fixed(x1, x2) * weights).sum(), (x1, x2))
    cost = emd.match_cost(x1, x2, match)
    assert float((cost - fixed(x1, x2)).detach().abs().max()) <= 1e-13
    got = torch.autograd.grad((cost * weights).sum(), (x1, x2))
    for g, w in zip(got, want):
        assert float((g - w).abs().max()) <= 1e-12
    only2 = torch.autograd.grad(emd.match_cost(x1.detach(), x2, match).sum(), x2)[0]
    assert float((only2 - torch.autograd.grad(fixed(x1, x2).sum(), x2)[0]).abs().max()) <= 1e-12
    assert not match.a.requires_grad and not match0.requires_grad


def test_coincident_points_give_a_zero_vector():
    case = ((2, 65, 63), "identical")
    dense, cost, g1, g2 = C.reference(case)
    assert bool((cost == 0).all()) and bool((g1 == 0).all()) and bool((g2 == 0).all())
    assert bool(torch.isfinite(dense).all())


def test_argument_errors():
    x = torch.zeros(2, 4, 3)
    for fn in (emd.approx_match, emd.emd_distance, emd.emd_composition, model_loss.EarthMoverLoss()):
        with pytest.raises(TypeError, match="xyz1"):
            fn(x.int(), x)
        with pytest.raises(TypeError, match="xyz2"):
            fn(x, x.double())
        with pytest.raises(TypeError, match="xyz2"):
            fn(x, [1.0])
        with pytest.raises(ValueError, match="xyz1"):
            fn(torch.zeros(2, 4, 2), x)
        with pytest.raises(ValueError, match="xyz2"):
            fn(x, torch.zeros(3, 4, 3))
        with pytest.raises(ValueError, match="xyz2"):
            fn(x, torch.zeros(2, 12))
        with pytest.raises(RuntimeError, match="xyz2"):
            fn(x, x.to("meta"))
    match = emd.approx_match(x, x)
    with pytest.raises(TypeError, match="match"):
        emd.match_cost(x, x, match.dense())
    with pytest.raises(ValueError, match="match"):
        emd.match_cost(x, torch.zeros(2, 5, 3), match)
    with pytest.raises(TypeError, match="match"):
        emd.match_cost(x.double(), x.double(), match)
    with pytest.raises(ValueError, match="reduction"):
        model_loss.EarthMoverLoss("max")


@pytest.mark.parametrize("shape", [(0, 4, 5), (2, 0, 5), (2, 4, 0), (2, 0, 0)])
def test_empty_problems(shape):
    b, n, m = shape
    x1 = torch.zeros(b, n, 3, requires_grad=True)
    x2 = torch.zeros(b, m, 3, requires_grad=True)
    match = emd.approx_match(x1, x2)
    assert match.a.shape == (b, 10, n) and match.b.shape == (b, 10, m) and match.dense().shape == (b, n, m)
    cost = emd.emd_distance(x1, x2)
    assert cost.shape == (b,) and bool((cost == 0).all())
    g1, g2 = torch.autograd.grad(cost.sum(), (x1, x2))
    assert g1.shape == x1.shape and g2.shape == x2.shape and not bool(g1.any()) and not bool(g2.any())


def test_earth_mover_loss_reductions():
    case = ((2, 100, 250), "random")
    x1, x2 = (torch.from_numpy(c.astype(np.float64)) for c in C.clouds(case))
    per_cloud = C.reference(case)[1] / 250
    assert torch.allclose(model_loss.EarthMoverLoss("none")(x1, x2), per_cloud, rtol=1e-12, atol=0)
    assert torch.allclose(model_loss.EarthMoverLoss("sum")(x1, x2), per_cloud.sum(), rtol=1e-12, atol=0)
    assert torch.allclose(model_loss.EarthMoverLoss()(x1, x2), per_cloud.mean(), rtol=1e-12, atol=0)
    x1.requires_grad_(True)
    model_loss.EarthMoverLoss()(x1, x2).backward()
    assert float((x1.grad - C.reference(case)[2] / 500).abs().max()) <= 1e-12


def test_cpu_fp32_takes_the_composition_and_never_the_library(monkeypatch):
    from pytorch_points_amd import _lib
    monkeypatch.setattr(_lib, "lib", lambda: pytest.fail("a CPU tensor reached the HIP library"))
    x1, x2 = (torch.from_numpy(c) for c in C.clouds(((2, 65, 63), "random")))
    match = emd.approx_match(x1, x2)
    assert not match.hip and match.dense().dtype == torch.float32
    assert emd.emd_distance(x1, x2).shape == (2,)
