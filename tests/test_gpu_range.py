"""Every operator, on every path the knobs of include/pp_hip_debug.h select, against the CPU oracle at the extremes of
the fp32 range (finite inputs at any magnitude are in the contract): FPS temps saturated at 1e10,
squared distances that overflow to inf (and box extents hi - lo that do), squared distances that underflow to
subnormals or 0 (distinct points tie at 0: the lowest index wins), subnormal coordinates -- the magnitudes where the
grid searches' and the bucketed FPS's fp32 distance bounds change meaning, and where an instruction that flushes
denormals would change bits.  The families are those of tests/golden/gen_range.py, in a lattice-exact and a jittered
variant; batch element 1 is always a clean unit cloud.  Bitwise where the oracle is bitwise (NaN and inf compared as
values); the scatter-adds within a scale-aware bound against float64.  Also FPS with NaN / inf points, and the
default paths against the reference's own kernel bodies (tests/golden/ref_xcheck_range.npz)."""
import contextlib
import ctypes
import glob
import importlib.util
import os

import numpy as np
import pytest
import torch

import oracle

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("gen_range", os.path.join(GOLD, "gen_range.py"))
R = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(R)

CASES = [(f, v) for f in R.FAMILIES for v in R.VARIANTS]
IDS = ["%s-%s" % c for c in CASES]
EPS32 = 2.0 ** -24
TINY = 2.0 ** -149


@contextlib.contextmanager
def knobs(**kw):
    """set pp_debug_set_<name>(value) for every keyword; every one back to 0 afterwards"""
    from pytorch_points_amd import _lib
    fns = {}
    for k in kw:
        f = getattr(_lib.lib(), "pp_debug_set_" + k)
        f.argtypes = [ctypes.c_int]
        f.restype = None
        fns[k] = f
    try:
        for k, v in kw.items():
            fns[k](v)
        yield
    finally:
        for f in fns.values():
            f(0)


def _t(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _eq(got, exp):
    """bitwise equality of values, NaN equal to NaN"""
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    exp = np.asarray(exp)
    if got.shape != exp.shape or (got.dtype != exp.dtype and not (got.dtype.kind == exp.dtype.kind == "i")):
        return False
    if got.dtype.kind == "f":
        both_nan = np.isnan(got) & np.isnan(exp)
        return bool(((got == exp) | both_nan).all())
    return bool((got.astype(np.int64) == exp.astype(np.int64)).all())


def _first(got, exp):
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else got
    bad = np.argwhere(~((got == exp) | (np.isnan(got.astype(np.float64)) & np.isnan(np.asarray(exp, np.float64)))))
    return "%d differ, first at %s: %r against %r" % (len(bad), tuple(bad[0]), got[tuple(bad[0])], exp[tuple(bad[0])]) if len(bad) else "signs of zero differ"


def _bounded(got, exact, absterms, nterms, k=4, what=""):
    """|got - exact| <= k eps32 (n + 2) sum|terms| + k 2^-149 (n + 2): a sum of n fp32-rounded terms in any order"""
    got = got.detach().cpu().numpy().astype(np.float64) if isinstance(got, torch.Tensor) else got
    fin = np.isfinite(exact) & np.isfinite(absterms)   # (a term that overflowed: the result is not finite either)
    assert not np.isfinite(got[~fin]).any(), "%s: finite where a term overflowed" % what
    got, exact, absterms, nterms = got[fin], exact[fin], absterms[fin], np.broadcast_to(nterms, fin.shape)[fin]
    tol = k * (nterms + 2) * (EPS32 * absterms + TINY)
    err = np.abs(got - exact)
    assert np.isfinite(got).all() and (err <= tol).all(), "%s: %d beyond the bound, worst %.3g (bound %.3g)" % (
        what, int((err > tol).sum()), float(err.max()), float(tol.ravel()[np.argmax(err - tol)]))


def _pair(fam, var, n, seed):
    return R.pair(fam, var, n, seed)


# ------------------------------------------------------------------------------------------------ Chamfer fp32
CHAMFER_PATHS = [{}, {"nmdistance_search": 1}, {"nmdistance_search": 2},
                 {"nmdistance_search": 2, "nmdistance_routing": 1}, {"nmdistance_search": 2, "nmdistance_routing": 2},
                 {"nmdistance_search": 2, "nmdistance_build": 1}, {"nmdistance_search": 2, "nmdistance_tile": -1}] + \
                [{"nmdistance_search": 1, "nmdistance_variant": v} for v in (1, 1002, 1416)]


def _nnd(cuda, x1, x2):
    from pytorch_points_amd.network.model_loss import nndistance
    out = nndistance(_t(x1, cuda), _t(x2, cuda))
    torch.cuda.synchronize()
    return out[0], out[2], out[1], out[3]   # dist1, idx1, dist2, idx2: the oracle's order


@pytest.mark.parametrize("n,m", [(700, 900), (9000, 8192)])
@pytest.mark.parametrize("fam,var", CASES, ids=IDS)
def test_chamfer_forward_every_path(cuda, fam, var, n, m):
    x1, x2 = _pair(fam, var, n, 11), _pair(fam, var, m, 12)
    exp = oracle.chamfer_forward(x1, x2)
    for path in CHAMFER_PATHS:
        with knobs(**path):
            got = _nnd(cuda, x1, x2)
        for g, e, name in zip(got, exp, ("dist1", "idx1", "dist2", "idx2")):
            assert _eq(g, e), "%s %s %s: %s" % (fam, path, name, _first(g, e))


def _graddist(fam, b, n, seed):
    g = np.abs(np.random.default_rng(seed).normal(size=(b, n))).astype(np.float32) + np.float32(0.25)
    if fam in ("inf_spread", "inf_outliers", "huge_box"):   # no partial sum may overflow (then the order would matter)
        g *= np.float32(2.0 ** -40)
    return g


def _exact_backward(x1, x2, g1, g2, i1, i2):
    """float64 sums of the fp32-rounded terms 2 g (a - b) the kernels add, their sums of |terms| and term counts"""
    b, n, c = x1.shape
    m = x2.shape[1]
    ex = [np.zeros((b, n, c)), np.zeros((b, m, c))]
    ab = [np.zeros((b, n, c)), np.zeros((b, m, c))]
    cnt = [np.zeros((b, n, 1)), np.zeros((b, m, 1))]
    for s, (xa, xb, ga, ia) in enumerate(((x1, x2, g1, i1), (x2, x1, g2, i2))):
        for k in range(b):
            with np.errstate(over="ignore", invalid="ignore"):
                v = ((ga[k] * np.float32(2))[:, None] * (xa[k] - xb[k][ia[k]])).astype(np.float32).astype(np.float64)
            ex[s][k] += v
            ab[s][k] += np.abs(v)
            cnt[s][k] += 1
            np.subtract.at(ex[1 - s][k], ia[k], v)
            np.add.at(ab[1 - s][k], ia[k], np.abs(v))
            np.add.at(cnt[1 - s][k], ia[k], 1)
    return ex, ab, cnt


@pytest.mark.parametrize("fam,var", CASES, ids=IDS)
def test_chamfer_backward(cuda, fam, var):
    from pytorch_points_amd.network.model_loss import nndistance
    n, m = 3000, 2500
    x1, x2 = _pair(fam, var, n, 13), _pair(fam, var, m, 14)
    g1, g2 = _graddist(fam, 2, n, 15), _graddist(fam, 2, m, 16)
    d1, i1, d2, i2 = oracle.chamfer_forward(x1, x2)
    ex, ab, cnt = _exact_backward(x1, x2, g1, g2, i1, i2)
    o1, o2 = oracle.chamfer_backward(x1, x2, g1, g2, i1, i2)

    def run():
        t1 = _t(x1, cuda).requires_grad_(True)
        t2 = _t(x2, cuda).requires_grad_(True)
        a, b_, _, _ = nndistance(t1, t2)
        torch.autograd.backward([a, b_], [_t(g1, cuda), _t(g2, cuda)])
        torch.cuda.synchronize()
        return t1.grad, t2.grad

    before = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)
    try:
        r1, r2 = run()
    finally:
        torch.use_deterministic_algorithms(before)
    assert _eq(r1, o1) and _eq(r2, o2), "%s: the ordered backward differs from the oracle: %s" % (fam, _first(r1, o1))
    for v in (0, 1, 2):
        with knobs(nmdistance_backward_variant=v):
            r1, r2 = run()
        _bounded(r1, ex[0], ab[0], cnt[0], what="%s gradxyz1 variant %d" % (fam, v))
        _bounded(r2, ex[1], ab[1], cnt[1], what="%s gradxyz2 variant %d" % (fam, v))


# half: overflow from coordinates of about 200, underflow of differences below about 2e-4; double: overflow at about
# 1e154, underflow below about 1e-162
_F16 = {"h_over": 2.0 ** 5, "h_sub": 2.0 ** -10, "h_zero": 2.0 ** -14}
_F64 = {"d_over": 2.0 ** 510, "d_sub": 2.0 ** -535, "d_zero": 2.0 ** -545}


def _nnd_raw(cuda, x1, x2):
    """the _ext entry point, which serves half and double clouds: -> dist1, idx1, dist2, idx2"""
    from pytorch_points_amd._ext import losses
    t1, t2 = _t(x1, cuda), _t(x2, cuda)
    b, n, _ = x1.shape
    m = x2.shape[1]
    d1 = torch.empty(b, n, dtype=t1.dtype, device=cuda)
    d2 = torch.empty(b, m, dtype=t1.dtype, device=cuda)
    i1 = torch.empty(b, n, dtype=torch.int32, device=cuda)
    i2 = torch.empty(b, m, dtype=torch.int32, device=cuda)
    assert losses.nmdistance_forward(t1, t2, d1, d2, i1, i2) == 1
    torch.cuda.synchronize()
    return d1, i1, d2, i2


def _scaled(scale, var, b, n, seed, dtype):
    rng = np.random.default_rng([seed, int(np.log2(scale)) + 2000])
    x = rng.integers(-8, 9, (b, n, 3)).astype(np.float64)
    if var == "jitter":
        x = x + rng.normal(size=(b, n, 3)) * 0.25
    x = (x * scale).astype(dtype)
    x[1] = rng.normal(size=(n, 3)).astype(dtype)
    assert np.isfinite(x).all()
    return x


@pytest.mark.parametrize("var", R.VARIANTS)
@pytest.mark.parametrize("scale", sorted(_F16), ids=str)
def test_chamfer_forward_half(cuda, scale, var):
    x1 = _scaled(_F16[scale], var, 2, 600, 1, np.float16)
    x2 = _scaled(_F16[scale], var, 2, 700, 2, np.float16)
    exp = oracle.chamfer_forward_f16(x1, x2)
    got = _nnd_raw(cuda, x1, x2)
    for g, e, name in zip(got, exp, ("dist1", "idx1", "dist2", "idx2")):
        assert _eq(g, e), "%s %s: %s" % (scale, name, _first(g, e))


@pytest.mark.parametrize("var", R.VARIANTS)
@pytest.mark.parametrize("scale", sorted(_F64), ids=str)
def test_chamfer_forward_double(cuda, scale, var):
    x1 = _scaled(_F64[scale], var, 2, 1500, 3, np.float64)
    x2 = _scaled(_F64[scale], var, 2, 1300, 4, np.float64)
    exp = oracle.chamfer_forward_f64(x1, x2)
    got = _nnd_raw(cuda, x1, x2)
    for g, e, name in zip(got, exp, ("dist1", "idx1", "dist2", "idx2")):
        assert _eq(g, e), "%s %s: %s" % (scale, name, _first(g, e))


@pytest.mark.parametrize("fam,var", [c for c in CASES if c[0] == "saturated" or c[0] in R.UNDERFLOW],
                         ids=["%s-%s" % c for c in CASES if c[0] == "saturated" or c[0] in R.UNDERFLOW])
@pytest.mark.parametrize("n,m", [(700, 900), (5000, 4500)])
def test_labeled_chamfer(cuda, fam, var, n, m):
    from pytorch_points_amd.network.model_loss import labeled_nndistance
    x1, x2 = _pair(fam, var, n, 17), _pair(fam, var, m, 18)
    l1 = np.stack([R.labels(n, 0)] * 2).astype(np.float32)
    l2 = np.stack([R.labels(m, 0)] * 2).astype(np.float32)
    exp = oracle.labeled_chamfer_forward(x1, x2, l1, l2)
    assert (exp[0] < 1e10).all() and (exp[2] < 1e10).all()
    for v in (0, 1):
        with knobs(labeled_variant=v):
            d1, d2, i1, i2 = labeled_nndistance(_t(x1, cuda), _t(x2, cuda), _t(l1, cuda), _t(l2, cuda))
            torch.cuda.synchronize()
        for g, e, name in zip((d1, i1, d2, i2), exp, ("dist1", "idx1", "dist2", "idx2")):
            assert _eq(g, e), "%s variant %d %s: %s" % (fam, v, name, _first(g, e))


# ------------------------------------------------------------------------------------------- knn, three_nn, ball
@pytest.mark.parametrize("fam,var", CASES, ids=IDS)
def test_knn(cuda, fam, var):
    from pytorch_points_amd.ops import knn_points
    q, r = _pair(fam, var, 1500, 19), _pair(fam, var, 6000, 20)
    for K in (1, 8, 17):
        e_d, e_i = oracle.knn(q, r, K)
        for mode in (0, 1):
            with knobs(knn_search=mode):
                d, i = knn_points(_t(q, cuda), _t(r, cuda), K=K)[:2]
                torch.cuda.synchronize()
            assert _eq(i, e_i) and _eq(d, e_d), "%s K=%d search %d: %s" % (fam, K, mode, _first(i, e_i))


def _three_nn(cuda, u, k):
    from pytorch_points_amd._ext import sampling
    b, n, _ = u.shape
    d2 = torch.empty(b, n, 3, device=cuda)
    idx = torch.empty(b, n, 3, dtype=torch.int32, device=cuda)
    sampling.three_nn_wrapper(b, n, k.shape[1], _t(u, cuda), _t(k, cuda), d2, idx)
    torch.cuda.synchronize()
    return d2, idx


@pytest.mark.parametrize("fam,var", CASES, ids=IDS)
def test_three_nn(cuda, fam, var):
    u, k = _pair(fam, var, 1200, 21), _pair(fam, var, 8192, 22)
    e_d, e_i = oracle.three_nn(u, k)
    for mode in (0, 1):
        with knobs(three_nn_search=mode):
            d, i = _three_nn(cuda, u, k)
        assert _eq(i, e_i) and _eq(d, e_d), "%s search %d: %s" % (fam, mode, _first(i, e_i))


@pytest.mark.parametrize("m", [2, 40, 5000])
@pytest.mark.parametrize("finite", [1, 2])
def test_three_nn_fewer_than_three_finite_knowns(cuda, finite, m):
    """the empty slots are (inf, 0): the reference's double 1e40 initial bests, cast to float"""
    u, k = R.three_nn_sparse(900, max(m, finite), finite, 23)
    e_d, e_i = oracle.three_nn(u, k)
    assert np.isinf(e_d[..., finite:]).all()
    for mode in (0, 1):
        with knobs(three_nn_search=mode):
            d, i = _three_nn(cuda, u, k)
        assert _eq(i, e_i) and _eq(d, e_d), "finite=%d m=%d search %d: %s" % (finite, m, mode, _first(d, e_d))


BALL_PATHS = [{"ball_query_search": s, "ball_query_lpc": l} for s, l in ((2, 1), (2, 2), (2, 4), (2, 8), (1, 0))] + \
             [{"ball_query_search": 1, "ball_query_variant": 1}]


@pytest.mark.parametrize("fam,var", CASES, ids=IDS)
def test_ball_query(cuda, fam, var):
    from pytorch_points_amd._ext import sampling
    ctr, x = _pair(fam, var, 600, 24), _pair(fam, var, 8192, 25)
    ctr[0, ::5] = x[0, :120]   # duplicates of reference points: inside unless r * r is 0
    for r in R.radii(fam):
        for ns in (16, 40):
            exp = oracle.ball_query(ctr, x, float(r), ns)
            for path in BALL_PATHS:
                with knobs(**path):
                    got = sampling.ball_query(_t(ctr, cuda), _t(x, cuda), float(r), ns)
                    torch.cuda.synchronize()
                assert _eq(got, exp), "%s r=%g ns=%d %s: %s" % (fam, r, ns, path, _first(got, exp))


# --------------------------------------------------------------------- gathers and interpolation, extreme values
def _values(kind, shape, seed):
    rng = np.random.default_rng([seed, len(kind)])
    v = rng.normal(size=shape)
    if kind == "subnormal":
        v = np.round(v * 2 ** 12) * 2.0 ** -149
    elif kind == "huge":
        v = v * 2.0 ** 100
    return v.astype(np.float32)


@pytest.mark.parametrize("kind", ["subnormal", "huge"])
def test_group_and_gather_extreme_values(cuda, kind):
    from pytorch_points_amd._ext import sampling
    b, c, n, npoint, ns = 2, 5, 3000, 400, 24
    feats = _values(kind, (b, c, n), 1)
    x = R.pair("tiny_21", "lattice", n, 26)
    idx = oracle.ball_query(x[:, :npoint], x, 2.0 ** -69, ns)
    exp = oracle.group_points(feats, idx)
    for v in (0, 1, 2, 4, 8, 604):
        with knobs(group_points_variant=v):
            got = sampling.group_points(_t(feats, cuda), _t(idx, cuda))
            torch.cuda.synchronize()
        assert _eq(got, exp), "%s group_points variant %d: %s" % (kind, v, _first(got, exp))
    go = _values(kind, (b, c, npoint, ns), 2)
    ex = np.zeros((b, c, n))
    ab = np.zeros((b, c, n))
    cnt = np.zeros((b, 1, n))
    for k in range(b):
        for j in range(c):
            np.add.at(ex[k, j], idx[k].ravel(), go[k, j].ravel().astype(np.float64))
            np.add.at(ab[k, j], idx[k].ravel(), np.abs(go[k, j].ravel().astype(np.float64)))
        np.add.at(cnt[k, 0], idx[k].ravel(), 1)
    for v in (0, 1, 2):
        with knobs(group_points_grad_variant=v):
            got = sampling.group_points_grad(_t(go, cuda), _t(idx, cuda), n)
            torch.cuda.synchronize()
        _bounded(got, ex, ab, cnt, what="%s group_points_grad variant %d" % (kind, v))
    gi = np.ascontiguousarray(idx[:, :, 0])
    e_g = oracle.gather_forward(feats, gi)
    gg = _values(kind, (b, c, npoint), 3)
    ex = np.zeros((b, c, n))
    ab = np.zeros((b, c, n))
    cnt = np.zeros((b, 1, n))
    for k in range(b):
        for j in range(c):
            np.add.at(ex[k, j], gi[k], gg[k, j].astype(np.float64))
            np.add.at(ab[k, j], gi[k], np.abs(gg[k, j].astype(np.float64)))
        np.add.at(cnt[k, 0], gi[k], 1)
    for v in (0, 1):
        with knobs(gather_variant=v):
            out = torch.empty(b, c, npoint, device=cuda)
            sampling.gather_forward(b, c, n, npoint, _t(feats, cuda), _t(gi, cuda), out)
            torch.cuda.synchronize()
        assert _eq(out, e_g), "%s gather variant %d: %s" % (kind, v, _first(out, e_g))
    for mode in (0, 1):
        with knobs(scatter_mode=mode):
            gp = torch.zeros(b, c, n, device=cuda)
            sampling.gather_backward(b, c, n, npoint, _t(gg, cuda), _t(gi, cuda), gp)
            torch.cuda.synchronize()
        _bounded(gp, ex, ab, cnt, what="%s gather_backward scatter mode %d" % (kind, mode))


@pytest.mark.parametrize("wkind", ["subnormal", "huge"])
@pytest.mark.parametrize("fkind", ["subnormal", "huge"])
def test_three_interpolate_extreme_values(cuda, fkind, wkind):
    from pytorch_points_amd._ext import sampling
    b, c, m, n = 2, 6, 2000, 5000
    u, k = R.pair("tiny_21", "jitter", n, 27), R.pair("tiny_21", "jitter", m, 28)
    _, idx = oracle.three_nn(u, k)
    pts = _values(fkind, (b, c, m), 4)
    w = _values(wkind, (b, n, 3), 5)
    if fkind == "huge" and wkind == "huge":
        w *= np.float32(2.0 ** -80)   # products near 2^120: no overflow in the sums
    elif wkind == "huge":
        w *= np.float32(2.0 ** -60)
    exp = oracle.three_interpolate(pts, idx, w)
    for v in (0, 1, 2):
        with knobs(three_interpolate_variant=v):
            out = torch.empty(b, c, n, device=cuda)
            sampling.three_interpolate_wrapper(b, c, m, n, _t(pts, cuda), _t(idx, cuda), _t(w, cuda), out)
            torch.cuda.synchronize()
        assert _eq(out, exp), "%s/%s three_interpolate variant %d: %s" % (fkind, wkind, v, _first(out, exp))
    go = _values(fkind, (b, c, n), 6)
    ex = np.zeros((b, c, m))
    ab = np.zeros((b, c, m))
    cnt = np.zeros((b, 1, m))
    for kk in range(b):
        terms = (go[kk][:, :, None] * w[kk][None]).astype(np.float32).astype(np.float64)   # (c, n, 3) fp32 products
        for j in range(c):
            np.add.at(ex[kk, j], idx[kk].ravel(), terms[j].ravel())
            np.add.at(ab[kk, j], idx[kk].ravel(), np.abs(terms[j].ravel()))
        np.add.at(cnt[kk, 0], idx[kk].ravel(), 1)
    for v in (0, 1, 2, 3):
        with knobs(three_interpolate_grad_variant=v):
            gp = torch.zeros(b, c, m, device=cuda)
            sampling.three_interpolate_grad_wrapper(b, c, n, m, _t(go, cuda), _t(idx, cuda), _t(w, cuda), gp)
            torch.cuda.synchronize()
        _bounded(gp, ex, ab, cnt, what="%s/%s three_interpolate_grad variant %d" % (fkind, wkind, v))


# --------------------------------------------------------------------------------------------------------- FPS
FPS_PATHS = [(0, 0, 0), (1, 0, 0), (2, 0, 0), (3, 1, 0), (3, 1, 1), (3, 2, 0), (3, 2, 1)]   # (form, chain, sort)


def _fps_all_paths(cuda, x, m, what):
    from pytorch_points_amd._ext import sampling
    b, n, _ = x.shape
    e_idx, e_temp = oracle.furthest_sampling(x, m, 0)
    xt = _t(x, cuda)
    for form, chain, sort in FPS_PATHS:
        with knobs(fps_v1=form, fps_bucket_chain=chain, fps_bucket_sort=sort):
            idx = torch.empty(b, m, dtype=torch.int32, device=cuda)
            temp = torch.full((b, n), 1e10, dtype=torch.float32, device=cuda)
            sampling.furthest_sampling(m, 0, xt, temp, idx)
            torch.cuda.synchronize()
        assert sampling.furthest_sampling_status(cuda) == 0
        path = (form, chain, sort)
        assert _eq(idx, e_idx), "%s %s idx: %s" % (what, path, _first(idx, e_idx))
        assert _eq(temp, e_temp), "%s %s temp: %s" % (what, path, _first(temp, e_temp))
    return e_idx, e_temp


@pytest.mark.parametrize("n", [4096, 40000])
@pytest.mark.parametrize("fam,var", CASES, ids=IDS)
def test_fps(cuda, fam, var, n):
    x = _pair(fam, var, n, 29)
    _, e_temp = _fps_all_paths(cuda, x, 300, fam)
    if fam == "saturated":   # the picks after the first 64 clusters' worth: temps far below, the first ones at 1e10
        assert (oracle.furthest_sampling(x, 8, 0)[1][0] == np.float32(1e10)).any()


_NONFINITE = {"nan": [(1000, 1, np.nan)], "inf": [(1000, 0, np.inf)], "neg_inf": [(1000, 2, -np.inf)],
              "several": [(5, 0, np.nan), (800, 2, np.inf), (1000, 1, -np.inf), (2000, 0, np.nan), (3000, 1, -np.inf)]}


@pytest.mark.parametrize("n", [4096, 40000])
@pytest.mark.parametrize("case", sorted(_NONFINITE))
@pytest.mark.parametrize("fam", ["saturated", "tiny_21"])
def test_fps_nonfinite(cuda, fam, case, n):
    """a point with a NaN or inf coordinate keeps its temp (its distance to itself is NaN): once it wins it is every
    later pick, in the reference and on every path"""
    x = _pair(fam, "jitter", n, 30)
    for k, c, v in _NONFINITE[case]:
        x[0, k, c] = v
    e_idx, _ = _fps_all_paths(cuda, x, 300, "%s %s" % (fam, case))
    assert (e_idx[0, -5:] == e_idx[0, -1]).all()


# ----------------------------------------------------------------- the reference's kernel bodies, default paths
REF = np.load(os.path.join(GOLD, "ref_xcheck_range.npz"))


def _against_ref(key, got, lattice, dist=False):
    got = got.detach().cpu().numpy()
    a, b = REF["nocontract/" + key], REF["fma/" + key]
    if dist:
        u = np.abs(got.view(np.int32).astype(np.int64) - a.view(np.int32).astype(np.int64))
        ok = (u <= 2) | (got == a) | (np.isnan(got) & np.isnan(a))
        assert ok.all(), "%s: %d distances beyond 2 ulp of the reference" % (key, int((~ok).sum()))
    else:
        bad = (got != a) & ((got != b) if not lattice else True)
        assert not bad.any(), "%s: %d indices differ from the reference" % (key, int(bad.sum()))


@pytest.mark.parametrize("path", sorted(glob.glob(os.path.join(GOLD, "range_*.npz"))), ids=os.path.basename)
def test_default_paths_equal_reference_bodies(cuda, path):
    from pytorch_points_amd._ext import sampling
    name = os.path.basename(path)[:-4]
    g = dict(np.load(path))
    if name == "range_special":
        for f in (1, 2):
            d, i = _three_nn(cuda, g["tn_unknown%d" % f], g["tn_known%d" % f])
            _against_ref("%s/tn%d/idx" % (name, f), i, True)
            _against_ref("%s/tn%d/dist2" % (name, f), d, True, dist=True)
        keys = [(name + "/fps", g["fps_xyz"])]
        lattice = True
    else:
        lattice = name.endswith("_lattice")
        x1, x2 = g["xyz1"], g["xyz2"]
        d1, i1, d2, i2 = _nnd(cuda, x1, x2)
        _against_ref(name + "/chamfer/idx1", i1, lattice)
        _against_ref(name + "/chamfer/idx2", i2, lattice)
        if lattice:
            _against_ref(name + "/chamfer/dist1", d1, lattice, dist=True)
            _against_ref(name + "/chamfer/dist2", d2, lattice, dist=True)
        for j, r in enumerate(g["radii"]):
            got = sampling.ball_query(_t(g["new_xyz"], cuda), _t(x2, cuda), float(r), int(g["nsample"]))
            _against_ref("%s/ball_r%d" % (name, j), got, lattice)
        d, i = _three_nn(cuda, g["new_xyz"], x2)
        _against_ref(name + "/three_nn/idx", i, lattice)
        keys = [(name + "/fps", g["fps_xyz"])]
    for key, x in keys:
        b, n, _ = x.shape
        m = int(g["fps_npoint"])
        idx = torch.empty(b, m, dtype=torch.int32, device=cuda)
        temp = torch.full((b, n), 1e10, dtype=torch.float32, device=cuda)
        sampling.furthest_sampling(m, 0, _t(x, cuda), temp, idx)
        torch.cuda.synchronize()
        _against_ref(key + "/idx", idx, lattice)
        if lattice:
            _against_ref(key + "/temp", temp, lattice, dist=True)
