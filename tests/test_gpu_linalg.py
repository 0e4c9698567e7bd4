"""GPU tests of the batched SVD (csrc/linalg.hip, pp_batch_svd_f32) and of its operators batch_svd and
batch_normals, against fp64 NumPy / torch on the CPU.

Accuracy contract, tau = 8 max(m, n) 2^-23, against numpy.linalg.svd of the same fp32 input in fp64:
|s - s64| <= tau s64[0] with s descending; U^T U and V^T V within tau of I (full and thin forms);
|A - U_k diag(s) V_k^T| <= tau s64[0]; singular vectors whose sigma is separated from its neighbours by a gap of
1e-2 s64[0] or more agree with the fp64 ones up to sign, |<u, u64>| >= 1 - 1e-4."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 32), (32, 1), (2, 2), (3, 3), (20, 3), (3, 20), (5, 7), (7, 5), (16, 16), (31, 17), (17, 31),
          (32, 32)]
BATCHES = [1, 63, 64, 65, 1000]


def _linalg():
    from pytorch_points_amd._ext import linalg
    return linalg


def svd(cuda, a, full=True, sort=True, max_sweeps=100):
    u, s, v, info = _linalg().batch_svd_forward(torch.from_numpy(np.ascontiguousarray(a)).to(cuda), sort, 1e-7,
                                                max_sweeps, return_info=True, full=full)
    return u.cpu().numpy(), s.cpu().numpy(), v.cpu().numpy(), info.cpu().numpy()


def tau(m, n):
    return 8 * max(m, n) * 2.0 ** -23


def check_contract(a, u, s, v, full, vectors=True, scale=1.0, ref=None):
    """every check of the accuracy contract; ``scale`` multiplies the input and s before comparing (range tests);
    ``ref`` is ``np.linalg.svd`` of that scaled fp64 input when the caller has it already"""
    b, m, n = a.shape
    k = min(m, n)
    t = tau(m, n)
    a64 = a.astype(np.float64) * scale
    u64, s64, vt64 = np.linalg.svd(a64) if ref is None else ref
    s = s.astype(np.float64) * scale
    assert u.shape == (b, m, m if full else k) and v.shape == (b, n, n if full else k) and s.shape == (b, k)
    assert np.isfinite(u).all() and np.isfinite(v).all() and np.isfinite(s).all()
    top = s64[:, :1]
    assert (s >= 0).all() and (np.diff(s, axis=1) <= 0).all()
    assert (np.abs(s - s64) <= t * top).all(), np.abs(s - s64).max()
    for f in (u.astype(np.float64), v.astype(np.float64)):
        g = np.swapaxes(f, 1, 2) @ f
        assert np.abs(g - np.eye(f.shape[2])).max() <= t, np.abs(g - np.eye(f.shape[2])).max()
    uk, vk = u[:, :, :k].astype(np.float64), v[:, :, :k].astype(np.float64)
    rec = (uk * s[:, None, :]) @ np.swapaxes(vk, 1, 2)
    assert (np.abs(rec - a64).max(axis=(1, 2)) <= t * top[:, 0]).all()
    if not vectors:
        return
    pad = np.concatenate([s64, np.zeros((b, 1))], axis=1) if m != n else s64   # a zero neighbour beyond k when m != n
    for j in range(k):
        gap = np.full(b, np.inf)
        if j > 0:
            gap = np.minimum(gap, pad[:, j - 1] - pad[:, j])
        if j + 1 < pad.shape[1]:
            gap = np.minimum(gap, pad[:, j] - pad[:, j + 1])
        sep = gap >= 1e-2 * top[:, 0]
        cu = np.abs(np.einsum("bi,bi->b", uk[:, :, j], u64[:, :, j]))
        cv = np.abs(np.einsum("bi,bi->b", vk[:, :, j], vt64[:, j, :]))
        assert (cu[sep] >= 1 - 1e-4).all() and (cv[sep] >= 1 - 1e-4).all()


def orthogonal(rng, b, d):
    q, r = np.linalg.qr(rng.standard_normal((b, d, d)))
    return q * np.sign(np.diagonal(r, axis1=1, axis2=2))[:, None, :]


def graded(rng, b, m, n, low=1e-6):
    k = min(m, n)
    spec = np.logspace(0, np.log10(low), k) if k > 1 else np.ones(1)
    return ((orthogonal(rng, b, m)[:, :, :k] * spec) @ np.swapaxes(orthogonal(rng, b, n)[:, :, :k], 1, 2)).astype(np.float32)


def gaussian(rng, b, m, n):
    return rng.standard_normal((b, m, n)).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------ shapes
@pytest.mark.parametrize("full", [True, False], ids=["full", "thin"])
@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("m,n", SHAPES)
def test_gaussian_meets_the_contract(cuda, m, n, batch, full):
    a = gaussian(np.random.default_rng(1000 * m + n + batch), batch, m, n)
    u, s, v, info = svd(cuda, a, full)
    check_contract(a, u, s, v, full)
    assert ((info >= 1) & (info <= 100)).all()


@pytest.mark.parametrize("full", [True, False], ids=["full", "thin"])
@pytest.mark.parametrize("m,n", SHAPES)
def test_graded_spectrum_meets_the_contract(cuda, m, n, full):
    a = graded(np.random.default_rng(7 * m + n), 65, m, n)
    u, s, v, info = svd(cuda, a, full)
    check_contract(a, u, s, v, full)
    assert ((info >= 1) & (info <= 100)).all()


def repeated(m, n, kind, rng):
    b, k = 20, min(m, n)
    if kind == "scaled_identity":
        return (np.eye(m, n)[None] * rng.uniform(0.5, 2.0, (b, 1, 1))).astype(np.float32)
    if kind == "rank1":
        return (rng.standard_normal((b, m, 1)) @ rng.standard_normal((b, 1, n))).astype(np.float32)
    if kind == "rank_deficient":
        r = max(1, k // 2)
        return (rng.standard_normal((b, m, r)) @ rng.standard_normal((b, r, n))).astype(np.float32)
    return np.zeros((b, m, n), np.float32)


@pytest.mark.parametrize("full", [True, False], ids=["full", "thin"])
@pytest.mark.parametrize("kind", ["scaled_identity", "rank1", "rank_deficient", "zero"])
@pytest.mark.parametrize("m,n", SHAPES)
def test_repeated_singular_values(cuda, m, n, kind, full):
    a = repeated(m, n, kind, np.random.default_rng(m * 33 + n))
    u, s, v, info = svd(cuda, a, full)
    check_contract(a, u, s, v, full, vectors=False)
    assert (info != -2).all()
    if kind == "zero":
        assert (s == 0).all()


def planar_patches(rng, b, noise=1e-3):
    normal = rng.standard_normal((b, 3))
    normal /= np.linalg.norm(normal, axis=1, keepdims=True)
    e1 = np.cross(normal, rng.standard_normal((b, 3)))
    e1 /= np.linalg.norm(e1, axis=1, keepdims=True)
    e2 = np.cross(normal, e1)
    c = rng.uniform(-1, 1, (b, 20, 2))
    p = c[..., :1] * e1[:, None] + c[..., 1:] * e2[:, None] + noise * rng.standard_normal((b, 20, 1)) * normal[:, None]
    return (p - p.mean(axis=1, keepdims=True)).astype(np.float32)


@pytest.mark.parametrize("full", [True, False], ids=["full", "thin"])
def test_near_planar_patches(cuda, full):
    a = planar_patches(np.random.default_rng(5), 1000)
    u, s, v, info = svd(cuda, a, full)
    check_contract(a, u, s, v, full)
    assert ((info >= 1) & (info <= 100)).all()


def test_normals_size_batch_in_full(cuda):
    """(524288, 20, 3): the batch of batch_normals at B=32, N=16384; thin form, as batch_svd calls it"""
    rng = np.random.default_rng(11)
    a = np.concatenate([gaussian(rng, 262144, 20, 3), planar_patches(rng, 262144)])
    u, s, v, info = svd(cuda, a, full=False)
    check_contract(a, u, s, v, False)
    assert ((info >= 1) & (info <= 100)).all()


# ------------------------------------------------------------------------------------------- every layout, every mode
# pp_batch_svd_f32 picks one of 38 instantiations by (R, K) = (max(m, n), min(m, n)): svd_lane_kernel<RM, K> for
# K <= 4 (RM = R rounded up to a multiple of 4: 32 of them) and svd_cols_kernel<RM, G> above ((8,8), (16,8), (32,8),
# (16,16), (32,16), (32,32)).  Every (m, n) runs; the batch of 67 leaves the last group of every column layout (8, 16
# or 32 matrices a block) and the last wave of the lane layout partial.
SWEEP_SCALES = (1.0, 1e-3, 1e3, 1e-30, 1e30)
SWEEP_GAUSSIAN = 12 * len(SWEEP_SCALES)       # rows 0..59 Gaussian, 60 graded: the full contract
SWEEP_STRUCTURED = 4                          # rank 1, rank k - 1, zero, c I: no singular-vector check (ties)
SWEEP_BATCH = SWEEP_GAUSSIAN + 1 + SWEEP_STRUCTURED + 2   # then one NaN and one +inf matrix


def sweep_batch(m, n, rng):
    k = min(m, n)
    parts = [gaussian(rng, 12, m, n) * np.float32(c) for c in SWEEP_SCALES]
    parts.append(graded(rng, 1, m, n))
    parts.append((rng.standard_normal((1, m, 1)) @ rng.standard_normal((1, 1, n))).astype(np.float32))
    parts.append((rng.standard_normal((1, m, k - 1)) @ rng.standard_normal((1, k - 1, n))).astype(np.float32))
    parts.append(np.zeros((1, m, n), np.float32))
    parts.append((np.eye(m, n) * rng.uniform(0.5, 2.0))[None].astype(np.float32))
    bad = gaussian(rng, 2, m, n)
    bad[0, rng.integers(m), rng.integers(n)] = np.nan
    bad[1, rng.integers(m), rng.integers(n)] = np.inf
    parts.append(bad)
    a = np.concatenate(parts)
    assert a.shape[0] == SWEEP_BATCH
    return a


def bits(x):
    return np.ascontiguousarray(x).view(np.int32)


def permute_columns(x, perm):
    """columns 0..k-1 of every matrix of x (b, r, c) reordered by perm (b, k); columns k.. stay in place"""
    out = x.copy()
    out[:, :, :perm.shape[1]] = np.take_along_axis(x[:, :, :perm.shape[1]], perm[:, None, :], axis=2)
    return out


@pytest.mark.parametrize("n", range(1, 33))
@pytest.mark.parametrize("m", range(1, 33))
def test_every_shape_sorted_unsorted_full_and_thin(cuda, m, n):
    a = sweep_batch(m, n, np.random.default_rng(3000 + 40 * m + n))
    k = min(m, n)
    nv = SWEEP_GAUSSIAN + 1
    fin = np.arange(SWEEP_BATCH) < nv + SWEEP_STRUCTURED
    ref = np.linalg.svd(a[fin].astype(np.float64))
    ref_v = tuple(x[:nv] for x in ref)
    ref_s = tuple(x[nv:] for x in ref)

    def contract(u, s, v, full):
        check_contract(a[:nv], u[:nv], s[:nv], v[:nv], full, ref=ref_v)
        check_contract(a[nv:fin.sum()], u[nv:fin.sum()], s[nv:fin.sum()], v[nv:fin.sum()], full, vectors=False,
                       ref=ref_s)

    res = {}
    for full in (True, False):
        for sort in (True, False):
            res[full, sort] = svd(cuda, a, full, sort)
        u, s, v, info = res[full, True]
        contract(u, s, v, full)
        assert (((info >= 1) & (info <= 100)) | (info == -1))[fin].all(), info
        assert np.isnan(u[~fin]).all() and np.isnan(s[~fin]).all() and np.isnan(v[~fin]).all()
        assert (info[~fin] == -2).all()

        # unsorted: the same columns, placed by original column; the kernel ranks ties lower column first
        uu, su, vu, iu = res[full, False]
        perm = np.argsort(-su, axis=1, kind="stable")
        assert np.array_equal(bits(np.take_along_axis(su, perm, axis=1)), bits(s))
        assert np.array_equal(iu, info)
        up, vp = permute_columns(uu, perm), permute_columns(vu, perm)
        (ys, zs), (yp, zp) = ((u, v), (up, vp)) if m >= n else ((v, u), (vp, up))
        assert np.array_equal(bits(zp), bits(zs))
        # Y columns with sigma > 0 are w_j / sigma_j in either order; the others are completions built against the
        # columns already in place, so they differ: the contract holds for them after the permutation
        keep = np.concatenate([s > 0, np.zeros((SWEEP_BATCH, ys.shape[2] - k), bool)], axis=1)
        keep[~fin] = True
        assert np.array_equal(np.where(keep[:, None, :], bits(yp), 0), np.where(keep[:, None, :], bits(ys), 0))
        contract(up, np.take_along_axis(su, perm, axis=1), vp, full)

    # thin = the first k columns of full, bit for bit: the rotations do not depend on the form, and the completion of
    # a column j < k sees only the columns before k in either
    for sort in (True, False):
        fu, fs, fv, fi = res[True, sort]
        tu, ts, tv, ti = res[False, sort]
        assert np.array_equal(bits(ts), bits(fs)) and np.array_equal(ti, fi)
        assert np.array_equal(bits(tu), bits(fu[:, :, :k])) and np.array_equal(bits(tv), bits(fv[:, :, :k]))


# ------------------------------------------------------------------------------------------------------ determinism
@pytest.mark.parametrize("m,n", [(20, 3), (3, 20), (7, 5), (17, 31), (32, 32)])
def test_bitwise_reproducible_and_independent_of_the_batch(cuda, m, n):
    a = gaussian(np.random.default_rng(m + 40 * n), 1000, m, n)
    first = svd(cuda, a)
    second = svd(cuda, a)
    for x, y in zip(first, second):
        assert np.array_equal(x, y)
    for i in (0, 1, 63, 64, 517, 999):
        alone = svd(cuda, a[i:i + 1])
        for x, y in zip(alone, first):
            assert np.array_equal(x[0], y[i])


def test_max_sweeps_reports_non_convergence(cuda):
    a = graded(np.random.default_rng(2), 64, 32, 32)
    _, _, _, info = svd(cuda, a, max_sweeps=1)
    assert (info == -1).any()
    assert ((info == -1) | (info == 1)).all()
    _, _, _, info = svd(cuda, a)
    assert ((info >= 2) & (info <= 100)).all()


@pytest.mark.parametrize("m,n,batch", [(3, 3, 1 << 20), (32, 32, 65536)])
def test_matrices_that_exhaust_max_sweeps_still_meet_the_contract(cuda, m, n, batch):
    """With tol = 1e-7, below the fp32 rounding of the dot products, a few Gaussian matrices in a million end in a
    cycle of rounding-level rotations and report -1; their factors are still as accurate as the others'."""
    a = gaussian(np.random.default_rng(77), batch, m, n)
    u, s, v, info = svd(cuda, a, full=True)
    assert (info != -2).all()
    stuck = info == -1
    if stuck.any():
        check_contract(a[stuck], u[stuck], s[stuck], v[stuck], True)
    some = np.flatnonzero(~stuck)[:2000]
    check_contract(a[some], u[some], s[some], v[some], True)


# ------------------------------------------------------------------------------------------------------ large batches
def tiled_pattern(rng, m, n):
    """40 distinct matrices, one of them with a NaN"""
    p = np.concatenate([gaussian(rng, 36, m, n), graded(rng, 1, m, n), np.zeros((1, m, n), np.float32),
                        (np.eye(m, n) * 1.5)[None].astype(np.float32), gaussian(rng, 1, m, n)])
    p[-1, m // 2, n // 2] = np.nan
    return p


@pytest.mark.parametrize("m,n,full,batch", [(9, 1, False, (1 << 28) + 37), (17, 17, True, (1 << 23) + 37)],
                         ids=["lane", "cols"])
def test_batch_past_the_block_cap_and_2_31_elements(cuda, m, n, full, batch):
    """The launches cap the grid at 1 << 20 blocks and loop (64-bit offsets, a grid-stride loop for
    any batch).  lane: 2^20 blocks of 256 matrices, 37 matrices in a second iteration, i m n up to 2.4e9.  cols
    (G = 32, 8 matrices a block): 37 matrices in a second iteration of partial blocks, 2.4e9 elements.  Every matrix
    of a batch tiled from 40 must equal that matrix's solo result bit for bit."""
    k = min(m, n)
    words = m * n + m * (m if full else k) + n * (n if full else k) + k + 1
    need = batch * words * 4
    torch.cuda.empty_cache()
    free = torch.cuda.mem_get_info(cuda)[0]
    if free < 1.5 * need:
        pytest.skip("needs 1.5 x %.1f GB of free device memory, %.1f GB free" % (need / 1e9, free / 1e9))
    pattern = torch.from_numpy(tiled_pattern(np.random.default_rng(m * 100 + n), m, n)).to(cuda)
    period = pattern.shape[0]
    solo = _linalg().batch_svd_forward(pattern, True, 1e-7, 100, return_info=True, full=full)
    reps = batch // period
    a = got = x = c = None
    try:
        a = torch.empty(batch, m, n, device=cuda)
        a[:reps * period].view(reps, period, m, n).copy_(pattern)
        a[reps * period:].copy_(pattern[:batch - reps * period])
        got = _linalg().batch_svd_forward(a, True, 1e-7, 100, return_info=True, full=full)
        del a
        for x, y in zip(got, solo):
            x = x.view(torch.int32).view(batch, -1)
            y = y.view(torch.int32).view(period, -1)
            rows = period * max(1, (1 << 28) // (period * x.shape[1]))     # rows per comparison, whole periods
            for lo in range(0, batch, rows):
                c = x[lo:lo + rows]
                whole = c.shape[0] // period
                assert bool((c[:whole * period].view(whole, period, -1) == y).all()), lo
                assert bool((c[whole * period:] == y[:c.shape[0] - whole * period]).all()), lo
    finally:
        a = got = x = c = None          # nothing of this test's 20-30 GB outlives it, a failure's traceback included
        torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------------------ range
@pytest.mark.parametrize("k", [100, -100])
@pytest.mark.parametrize("m,n", [(20, 3), (3, 3), (7, 5), (32, 32)])
def test_power_of_two_scaling_is_exact(cuda, m, n, k):
    rng = np.random.default_rng(m * n)
    a = (rng.choice([-1.0, 1.0], (100, m, n)) * rng.uniform(0.5, 2.0, (100, m, n))).astype(np.float32)
    u, s, v, info = svd(cuda, a)
    us, ss, vs, infos = svd(cuda, np.ldexp(a, k).astype(np.float32))
    assert np.array_equal(u, us) and np.array_equal(v, vs) and np.array_equal(info, infos)
    assert np.array_equal(np.ldexp(s, k).astype(np.float32), ss)


@pytest.mark.parametrize("magnitude", [1e-38, 1e38])
@pytest.mark.parametrize("m,n", [(20, 3), (3, 3), (5, 7), (32, 32)])
def test_extreme_magnitudes(cuda, m, n, magnitude):
    a64 = np.random.default_rng(9).standard_normal((50, m, n))
    a64 /= np.abs(a64).max(axis=(1, 2), keepdims=True)
    if magnitude > 1:   # keep sigma_max below the fp32 maximum
        a64 /= np.linalg.norm(a64, axis=(1, 2), keepdims=True)
    a = (a64 * magnitude).astype(np.float32)
    u, s, v, info = svd(cuda, a)
    assert np.isfinite(u).all() and np.isfinite(v).all()
    check_contract(a, u, s, v, True, scale=1.0 / magnitude)


# ------------------------------------------------------------------------------------------------------- non-finite
@pytest.mark.parametrize("full", [True, False], ids=["full", "thin"])
@pytest.mark.parametrize("m,n", [(20, 3), (3, 20), (7, 5), (32, 32), (1, 1)])
def test_non_finite_matrix_is_nan_and_others_are_untouched(cuda, m, n, full):
    a = gaussian(np.random.default_rng(4), 100, m, n)
    clean = svd(cuda, a, full)
    bad = a.copy()
    bad[17, m - 1, n - 1] = np.nan
    bad[50, 0, 0] = np.inf
    bad[51, m // 2, n // 2] = -np.inf
    got = svd(cuda, bad, full)
    hit = np.zeros(100, bool)
    hit[[17, 50, 51]] = True
    for x, y in zip(got[:3], clean[:3]):
        assert np.isnan(x[hit]).all()
        assert np.array_equal(x[~hit], y[~hit])
    assert (got[3][hit] == -2).all() and np.array_equal(got[3][~hit], clean[3][~hit])


# ---------------------------------------------------------------------------------------------------------- autograd
@pytest.mark.parametrize("m,n", [(20, 3), (7, 5), (5, 7), (16, 16)])
def test_batch_svd_gradient_equals_torch_fp64(cuda, m, n):
    from pytorch_points_amd.network.operations import batch_svd
    rng = np.random.default_rng(m * 10 + n)
    k = min(m, n)
    spec = np.linspace(2.0, 1.0, k)
    a = ((orthogonal(rng, 8, m)[:, :, :k] * spec) @ np.swapaxes(orthogonal(rng, 8, n)[:, :, :k], 1, 2)).astype(np.float32)
    ws, wu, wv = (torch.from_numpy(rng.standard_normal(sh)) for sh in ((8, k), (8, m, k), (8, n, k)))

    def loss(u, s, v):
        return (ws * s).sum() + (wu * u * u).sum() + (wv * v * v).sum()

    x = torch.from_numpy(a).to(cuda).requires_grad_(True)
    u, s, v = batch_svd(x)
    assert u.shape == (8, m, k) and s.shape == (8, k) and v.shape == (8, n, k)
    loss(u.double().cpu(), s.double().cpu(), v.double().cpu()).backward()
    x64 = torch.from_numpy(a).double().requires_grad_(True)
    u64, s64, vh64 = torch.linalg.svd(x64, full_matrices=False)
    loss(u64, s64, vh64.transpose(-2, -1)).backward()
    assert x.grad.device == x.device
    err = (x.grad.double().cpu() - x64.grad).abs().max().item()
    assert err <= 1e-3 * x64.grad.abs().max().item()


def test_cpu_input_gives_cpu_outputs_and_gradient(cuda):
    from pytorch_points_amd.network.operations import batch_svd
    x = torch.from_numpy(gaussian(np.random.default_rng(6), 4, 20, 3)).requires_grad_(True)
    u, s, v = batch_svd(x)
    assert u.device.type == s.device.type == v.device.type == "cpu"
    (s.sum() + (u * u).sum()).backward()
    assert x.grad is not None and x.grad.device.type == "cpu" and torch.isfinite(x.grad).all()
    expected = torch.linalg.svd(x.detach().double(), full_matrices=False)
    assert torch.allclose(s.double(), expected[1], rtol=1e-5, atol=1e-5)


# ------------------------------------------------------------------------------------------------------ batch_normals
def test_normals_of_planes_are_the_plane_normals(cuda):
    from pytorch_points_amd.network.geo_operations import batch_normals
    rng = np.random.default_rng(21)
    b, npts = 3, 2048
    normal = rng.standard_normal((b, 3))
    normal /= np.linalg.norm(normal, axis=1, keepdims=True)
    e1 = np.cross(normal, rng.standard_normal((b, 3)))
    e1 /= np.linalg.norm(e1, axis=1, keepdims=True)
    e2 = np.cross(normal, e1)
    c = rng.uniform(-1, 1, (b, npts, 2))
    pts = (c[..., :1] * e1[:, None] + c[..., 1:] * e2[:, None] + 0.3 * normal[:, None]).astype(np.float32)
    x = torch.from_numpy(pts).to(cuda).transpose(1, 2)                     # (B, 3, N)
    normals, idx = batch_normals(x, nn_size=20)
    assert normals.shape == (b, 3, npts) and idx.shape == (b, npts, 20)
    dots = np.abs(np.einsum("bcn,bc->bn", normals.cpu().numpy().astype(np.float64), normal))
    assert (dots >= 1 - 1e-5).all(), dots.min()


def sphere(rng, b, npts):
    p = rng.standard_normal((b, npts, 3))
    return (p / np.linalg.norm(p, axis=2, keepdims=True)).astype(np.float32)


def test_normals_on_a_sphere_equal_fp64_pca(cuda):
    from pytorch_points_amd.network.geo_operations import batch_normals
    pts = sphere(np.random.default_rng(22), 2, 4096)
    normals, idx = batch_normals(torch.from_numpy(pts).to(cuda), nn_size=16, NCHW=False)
    idx = idx.cpu().numpy()
    nb = np.take_along_axis(pts.astype(np.float64)[:, None], idx[..., None], axis=2)      # (B, N, K, 3)
    nb = nb - nb.mean(axis=2, keepdims=True)
    expected = np.linalg.svd(nb)[2][..., -1, :]
    dots = np.abs(np.einsum("bnc,bnc->bn", normals.cpu().numpy().astype(np.float64), expected))
    assert (dots >= 1 - 1e-5).all(), dots.min()
    # and on a unit sphere the PCA normal is the radial direction, to the curvature of a small cap
    assert (np.abs(np.einsum("bnc,bnc->bn", normals.cpu().numpy(), pts)) >= 0.95).all()


def test_normals_idx_path_and_layouts_agree(cuda):
    from pytorch_points_amd.network.geo_operations import batch_normals
    pts = torch.from_numpy(sphere(np.random.default_rng(23), 2, 3000)).to(cuda)
    base = torch.from_numpy(sphere(np.random.default_rng(24), 2, 5000)).to(cuda)
    n_last, idx = batch_normals(pts, base, nn_size=20, NCHW=False)
    n_first, idx2 = batch_normals(pts.transpose(1, 2), base.transpose(1, 2), nn_size=20, NCHW=True)
    n_idx, idx3 = batch_normals(pts, base, nn_size=20, NCHW=False, idx=idx)
    assert torch.equal(idx, idx2) and idx3 is idx
    assert torch.equal(n_first.transpose(1, 2), n_last)
    assert torch.equal(n_idx, n_last)


def test_normals_gradient_reaches_points(cuda):
    from pytorch_points_amd.network.geo_operations import batch_normals
    pts = torch.from_numpy(sphere(np.random.default_rng(25), 2, 1024)).to(cuda).transpose(1, 2).contiguous()
    pts.requires_grad_(True)
    normals, _ = batch_normals(pts, nn_size=12)
    (normals[:, 0] ** 2).sum().backward()
    assert pts.grad is not None and pts.grad.shape == pts.shape
    assert torch.isfinite(pts.grad).all() and pts.grad.abs().max() > 0


def test_normals_keep_the_reference_size_checks(cuda):
    from pytorch_points_amd.network.geo_operations import batch_normals
    pts = torch.from_numpy(sphere(np.random.default_rng(26), 1, 64)).to(cuda)
    with pytest.raises(AssertionError):
        batch_normals(pts, nn_size=64, NCHW=False)
    with pytest.raises(RuntimeError):
        batch_normals(pts, nn_size=33, NCHW=False)


# ------------------------------------------------------------------------------------------------------------ errors
def test_raw_call_preconditions(cuda):
    linalg = _linalg()
    for shape in [(2, 33, 3), (2, 3, 33)]:
        with pytest.raises(RuntimeError):
            linalg.batch_svd_forward(torch.zeros(shape, device=cuda), True)
    with pytest.raises(RuntimeError):
        linalg.batch_svd_forward(torch.zeros(2, 3, 3, dtype=torch.float64, device=cuda), True)
    with pytest.raises(RuntimeError):
        linalg.batch_svd_forward(torch.zeros(2, 3, 3), True)
    with pytest.raises(RuntimeError):
        linalg.batch_svd_forward(torch.zeros(3, 3, device=cuda), True)
    u, s, v = linalg.batch_svd_forward(torch.zeros(0, 4, 2, device=cuda), True)
    assert u.shape == (0, 4, 4) and s.shape == (0, 2) and v.shape == (0, 2, 2)
