"""float16 / bfloat16 FEATURE tensors through gather_points, grouping_operation / QueryAndGroup and three_interpolate
(DESIGN.md §4 "16-bit features").

The contract under test: copies move the 2-byte words unchanged; three_interpolate is the fp32 chain on the widened
values rounded once, i.e. bit-identical to R_T(fp32 operator(W(x))); the backwards sum wide, round once and WRITE
their output, so that they equal R_T(fp32 backward(W(g))) bit for bit wherever the fp32 backward is reproducible and
to one unit of T otherwise (positive terms, at most 256 per destination: the fp32 order error is <= 256 * 2^-24, far
below half a unit of either type).  Shapes are the smallest that reach each kernel form: odd extents (2-byte aligned
rows), P % 8 == 0 with odd rows, aligned rows, the LDS threshold B * P = 256 * 2048 with every LDS form forced by its
knob, a ragged last chunk."""
import contextlib
import ctypes

import pytest
import torch

from pytorch_points_amd import _lib
from pytorch_points_amd._ext import sampling
from pytorch_points_amd.network import operations as ops
from pytorch_points_amd.network import pointnet2_utils as pn2

pytestmark = pytest.mark.gpu

TYPES = [torch.float16, torch.bfloat16]
TYPE_IDS = ["f16", "bf16"]


def set_knob(name, value):
    fn = getattr(_lib.lib(), "pp_debug_set_" + name)
    fn.argtypes = [ctypes.c_int]
    fn.restype = None
    fn(value)


@contextlib.contextmanager
def knob(name, value):
    set_knob(name, value)
    try:
        yield
    finally:
        set_knob(name, 0)


# the scatter-add backwards' operators and forms (include/pp_hip_debug.h: pp_debug_scatter_plan)
GATHER, GROUP, INTERP = 0, 1, 2
NONE, ATOMICS, COLUMN, SORTED, ORDERED = 0, 1, 2, 3, 4


def assert_plan(dtype, op, b, c, sources, destinations, form):
    """the knobs as they stand select `form` for the shim's call on `dtype` tensors (with the workspace it passes)"""
    per_source = 3 if op == INTERP else 1
    ws = int(_lib.lib().pp_scatter_workspace_bytes(b, per_source * sources, destinations, per_source, int(op == INTERP)))
    fn = _lib.lib().pp_debug_scatter_plan
    fn.argtypes = [ctypes.c_int] * 6 + [ctypes.c_longlong, ctypes.c_int, ctypes.c_size_t]
    fn.restype = ctypes.c_int
    elem = 4 if dtype is torch.float32 else 2
    assert fn(op, elem, int(elem == 2 or op == GROUP), 0, b, c, sources, destinations, ws) == form


@contextlib.contextmanager
def deterministic():
    before = torch.are_deterministic_algorithms_enabled()
    warn = torch.is_deterministic_algorithms_warn_only_enabled()
    torch.use_deterministic_algorithms(True)
    try:
        yield
    finally:
        torch.use_deterministic_algorithms(before, warn_only=warn)


def gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def bits(x):
    return x.contiguous().view(torch.int16)


def random_words(shape, dtype, g, dev):
    """every 2-byte pattern is possible: NaN payloads, both zeros, subnormals, infinities"""
    return torch.randint(-32768, 32768, shape, generator=g, dtype=torch.int16).to(dev).view(dtype)


def ref_group_bits(points, idx):
    b, c, _ = points.shape
    flat = idx.reshape(b, 1, -1).expand(b, c, -1).long()
    return torch.gather(bits(points), 2, flat).view(b, c, *idx.shape[1:])


def units_apart(a, b):
    """largest distance in units of the last place between two tensors of non-negative T values"""
    ia, ib = bits(a).int(), bits(b).int()
    assert (ia >= 0).all() and (ib >= 0).all()
    return int((ia - ib).abs().max())


def ball_style_idx(b, npoint, nsample, n, g):
    """rows like ball_query's: a run of hits, then the first index repeated to the row's end"""
    idx = torch.randint(0, n, (b, npoint, nsample), generator=g, dtype=torch.int32)
    hits = torch.randint(1, nsample + 1, (b, npoint, 1), generator=g)
    pad = torch.arange(nsample).view(1, 1, -1) >= hits
    return torch.where(pad, idx[:, :, :1].expand_as(idx), idx)


def positive(shape, dtype, g, dev):
    return (torch.rand(shape, generator=g) + 0.5).to(dev).to(dtype)


def interp_inputs(b, n, m, g, dev):
    unknown = torch.rand(b, n, 3, generator=g).to(dev)
    known = torch.rand(b, m, 3, generator=g).to(dev)
    dist, idx = pn2.three_nn(unknown, known)
    recip = 1.0 / (dist + 1e-8)
    return idx, (recip / recip.sum(2, keepdim=True)).contiguous()


# ---------------------------------------------------------------------------------------------- 1. bit-exact copies
GROUP_SHAPES = [(2, 3, 7, 3, 5), (2, 5, 1023, 16, 8), (2, 4, 1024, 32, 16), (8, 4, 4096, 1024, 64),
                (8, 4, 4096, 1023, 64)]


@pytest.mark.parametrize("dtype", TYPES, ids=TYPE_IDS)
@pytest.mark.parametrize("shape", GROUP_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_group_points_moves_bits(cuda, dtype, shape):
    b, c, n, npoint, nsample = shape
    g = gen(sum(shape))
    points = random_words((b, c, n), dtype, g, cuda)
    idx = torch.randint(0, n, (b, npoint, nsample), generator=g, dtype=torch.int32).to(cuda)
    ref = ref_group_bits(points, idx)
    # 0: what the shape selects; 1: global gathers; 2: the register-staged LDS form; 604 / 608 / 616: the LDS-DMA form
    # with 8192 / 16384 / 32768 positions per chunk (the ragged shape: the register-staged form, its last chunk partial)
    variants = (0, 1, 2, 604, 608, 616) if n == 4096 else (0, 1)
    for v in variants:
        with knob("group_points_variant", v):
            out = sampling.group_points(points, idx)
        assert out.dtype == dtype and out.shape == (b, c, npoint, nsample)
        assert torch.equal(bits(out), ref), v
    out = ops.grouping_operation(points, idx)
    assert out.dtype == dtype and torch.equal(bits(out), ref)


@pytest.mark.parametrize("dtype", TYPES, ids=TYPE_IDS)
def test_group_points_every_bit_pattern(cuda, dtype):
    words = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16)
    g = gen(5)
    points = words[torch.randperm(65536, generator=g)].view(1, 4, 16384).to(cuda).view(dtype)
    idx = torch.randperm(16384, generator=g).to(torch.int32).view(1, 256, 64).to(cuda)
    out = sampling.group_points(points, idx)
    assert torch.equal(bits(out), ref_group_bits(points, idx))
    assert torch.equal(bits(out).flatten().sort()[0].cpu(), words)          # every pattern came through once


@pytest.mark.parametrize("dtype", TYPES, ids=TYPE_IDS)
@pytest.mark.parametrize("shape,variant", [((2, 3, 7, 5), 0), ((2, 4, 1024, 256), 0), ((4, 8, 2048, 512), 2),
                                           ((4, 8, 2047, 511), 2)], ids=["odd", "aligned", "lds", "lds_odd"])
def test_gather_points_moves_bits(cuda, dtype, shape, variant):
    b, c, n, m = shape
    g = gen(sum(shape))
    points = random_words((b, c, n), dtype, g, cuda)
    idx = torch.randint(0, n, (b, m), generator=g, dtype=torch.int32).to(cuda)
    ref = torch.gather(bits(points), 2, idx.view(b, 1, m).expand(b, c, m).long())
    with knob("gather_variant", variant):          # 2: the LDS form although the shape is small
        out = ops.gather_points(points, idx)
    assert out.dtype == dtype and torch.equal(bits(out), ref)
    with knob("gather_variant", 1):
        assert torch.equal(bits(ops.gather_points(points, idx)), ref)


# ------------------------------------------------------------------------------------------------ 2. strided slice
@pytest.mark.parametrize("dtype", TYPES, ids=TYPE_IDS)
def test_group_points_into_odd_slice_leaves_the_rest_untouched(cuda, dtype):
    b, c, n, npoint, nsample, ctot, off = 2, 3, 7, 3, 5, 5, 1      # P = 15: the slice starts at byte 30 of the tensor
    g = gen(2)
    points = random_words((b, c, n), dtype, g, cuda)
    idx = torch.randint(0, n, (b, npoint, nsample), generator=g, dtype=torch.int32).to(cuda)
    sentinel = 0x5A3C
    out = torch.full((b, ctot, npoint, nsample), sentinel, dtype=torch.int16, device=cuda).view(dtype)
    sampling.group_points_into(points, idx, out, off)
    got = bits(out)
    assert torch.equal(got[:, off:off + c], ref_group_bits(points, idx))
    assert (got[:, :off] == sentinel).all() and (got[:, off + c:] == sentinel).all()


# ------------------------------------------------------------------------------------------ 3. interpolation forward
def interp_reference(features, idx, weight):
    b, c, m = features.shape
    wide = torch.empty(b, c, idx.shape[1], dtype=torch.float32, device=features.device)
    sampling.three_interpolate_wrapper(b, c, m, idx.shape[1], features.float(), idx, weight, wide)
    return wide


def same_bits_or_both_nan(a, b):
    nan = torch.isnan(a)
    return torch.equal(nan, torch.isnan(b)) and torch.equal(bits(a)[~nan], bits(b)[~nan])


@pytest.mark.parametrize("dtype", TYPES, ids=TYPE_IDS)
@pytest.mark.parametrize("shape,variant", [((2, 3, 5, 7), 0), ((2, 8, 512, 2048), 0), ((8, 4, 4096, 16384), 3),
                                           ((2, 5, 509, 2047), 3)], ids=["odd", "global", "lds", "lds_odd"])
def test_three_interpolate_is_the_rounded_fp32_result(cuda, dtype, shape, variant):
    b, c, m, n = shape
    g = gen(sum(shape))
    idx, weight = interp_inputs(b, n, m, g, cuda)
    features = torch.randn(b, c, m, generator=g).to(cuda).to(dtype)
    ref = interp_reference(features, idx, weight).to(dtype)
    with knob("three_interpolate_variant", variant):     # 3: the LDS-staged form although the grid is small
        out = pn2.three_interpolate(features, idx, weight)
    assert out.dtype == dtype and same_bits_or_both_nan(out, ref)
    with knob("three_interpolate_variant", 1):
        assert same_bits_or_both_nan(pn2.three_interpolate(features, idx, weight), ref)


def test_three_interpolate_half_overflows_to_infinity(cuda):
    b, c, m, n = 2, 4, 64, 256
    g = gen(9)
    idx, weight = interp_inputs(b, n, m, g, cuda)
    weight = (weight * 1.5).contiguous()                  # weights summing to 1.5: the fp32 result passes 65520
    sign = torch.where(torch.rand(b, c, m, generator=g) < 0.5, -1.0, 1.0)
    features = (sign * (65504.0 - 32.0 * torch.randint(0, 64, (b, c, m), generator=g))).to(cuda).to(torch.float16)
    features[0, 0, :4] = torch.tensor([float("nan"), float("inf"), float("-inf"), 0.0], device=cuda)
    ref = interp_reference(features, idx, weight).to(torch.float16)
    for v in (0, 3):
        with knob("three_interpolate_variant", v):
            out = pn2.three_interpolate(features, idx, weight)
        assert same_bits_or_both_nan(out, ref)
        assert (out == float("inf")).any() and (out == float("-inf")).any()


# ----------------------------------------------------------------------------------------------------- 4, 5. backwards
def group_grad_case(shape, dtype, dev):
    b, c, n, npoint, nsample = shape
    g = gen(sum(shape))
    idx = ball_style_idx(b, npoint, nsample, n, g)
    assert int(torch.stack([torch.bincount(r.flatten().long(), minlength=n) for r in idx]).max()) <= 256
    return positive((b, c, npoint, nsample), dtype, g, dev), idx.to(dev)


def raw_group_grad(grad_out, idx, n, ordered=0, prefill=float("nan")):
    """the 16-bit entry point itself, on an output pre-filled with NaN -> (code, grad_points)"""
    b, c, npoint, nsample = grad_out.shape
    out = torch.full((b, c, n), prefill, dtype=grad_out.dtype, device=grad_out.device)
    ws, nbytes = sampling._scatter_ws(grad_out.device, b, npoint * nsample, n, 1, 0)
    fn = sampling._entry16("pp_group_points_grad_out_ws", grad_out.dtype)
    with _lib.on_device(grad_out.device) as stream:
        code = fn(_lib.ptr(grad_out), _lib.ptr(idx), _lib.ptr(out), b, c, n, npoint, nsample, c * npoint * nsample,
                  _lib.ptr(ws) if ws is not None else None, nbytes, ordered, stream)
    return code, out


def check_written(out, dst, n):
    """no NaN of the pre-fill survives; destinations without a source are +0"""
    assert not torch.isnan(out).any()
    for bi in range(out.shape[0]):
        empty = torch.bincount(dst[bi].flatten().long(), minlength=n) == 0
        assert (bits(out)[bi][:, empty] == 0).all()


GROUP_GRAD_SHAPES = [(2, 4, 1000, 64, 64), (2, 4, 1000, 241, 17), (2, 3, 7, 3, 5)]
# the automatic forms (16-bit, fp32 reference): the column from 4096 positions; the last shape has 15, where 16-bit sorts
# and fp32 -- too small to sort -- takes its atomics
GROUP_GRAD_FORMS = {GROUP_GRAD_SHAPES[0]: (COLUMN, COLUMN), GROUP_GRAD_SHAPES[1]: (COLUMN, COLUMN),
                    GROUP_GRAD_SHAPES[2]: (SORTED, ATOMICS)}


@pytest.mark.parametrize("dtype", TYPES, ids=TYPE_IDS)
@pytest.mark.parametrize("shape", GROUP_GRAD_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_group_points_grad(cuda, dtype, shape):
    n = shape[2]
    plan = (GROUP, shape[0], shape[1], shape[3] * shape[4], n)
    assert_plan(dtype, *plan, GROUP_GRAD_FORMS[shape][0])
    assert_plan(torch.float32, *plan, GROUP_GRAD_FORMS[shape][1])
    grad_out, idx = group_grad_case(shape, dtype, cuda)
    ref = sampling.group_points_grad(grad_out.float(), idx, n).to(dtype)
    code, out = raw_group_grad(grad_out, idx, n)
    assert code == 0
    check_written(out, idx, n)
    assert units_apart(out, ref) <= 1
    assert units_apart(sampling.group_points_grad(grad_out, idx, n), ref) <= 1
    with knob("group_points_grad_variant", 2):            # the double column, for the fp32 reference as well
        assert_plan(dtype, *plan, COLUMN)
        assert_plan(torch.float32, *plan, COLUMN)
        ref2 = sampling.group_points_grad(grad_out.float(), idx, n).to(dtype)
        code, out2 = raw_group_grad(grad_out, idx, n)
    assert code == 0
    check_written(out2, idx, n)
    assert torch.equal(bits(out2), bits(ref2))
    with deterministic():
        ref3 = sampling.group_points_grad(grad_out.float(), idx, n).to(dtype)
        first = sampling.group_points_grad(grad_out, idx, n)
        code, second = raw_group_grad(grad_out, idx, n, ordered=1)
    assert code == 0
    check_written(second, idx, n)
    assert first.dtype == dtype and torch.equal(bits(first), bits(ref3)) and torch.equal(bits(first), bits(second))


@pytest.mark.parametrize("dtype", TYPES, ids=TYPE_IDS)
def test_group_points_grad_through_autograd(cuda, dtype):
    grad_out, idx = group_grad_case((2, 4, 1000, 64, 64), dtype, cuda)
    features = torch.zeros(2, 4, 1000, dtype=dtype, device=cuda, requires_grad=True)
    ops.grouping_operation(features, idx).backward(grad_out)
    ref = sampling.group_points_grad(grad_out.float(), idx, 1000).to(dtype)
    assert features.grad.dtype == dtype and units_apart(features.grad, ref) <= 1


@pytest.mark.parametrize("dtype", TYPES, ids=TYPE_IDS)
def test_gather_backward(cuda, dtype):
    b, c, n, m = 2, 3, 100, 300
    g = gen(17)
    idx = torch.randint(0, n - 5, (b, m), generator=g, dtype=torch.int32).to(cuda)      # the last five stay empty
    grad_out = positive((b, c, m), dtype, g, cuda)

    def fp32():
        wide = torch.zeros(b, c, n, device=cuda)
        sampling.gather_backward(b, c, n, m, grad_out.float(), idx, wide)
        return wide.to(dtype)

    def run():
        out = torch.full((b, c, n), float("nan"), dtype=dtype, device=cuda)
        sampling.gather_backward(b, c, n, m, grad_out, idx, out)
        check_written(out, idx, n)
        return out

    assert units_apart(run(), fp32()) <= 1
    with deterministic():
        ref, first, second = fp32(), run(), run()
    assert torch.equal(bits(first), bits(ref)) and torch.equal(bits(first), bits(second))
    features = torch.zeros(b, c, n, dtype=dtype, device=cuda, requires_grad=True)
    ops.gather_points(features, idx).backward(grad_out)
    assert features.grad.dtype == dtype and units_apart(features.grad, fp32()) <= 1


@pytest.mark.parametrize("dtype", TYPES, ids=TYPE_IDS)
@pytest.mark.parametrize("shape,variant", [((2, 4, 2048, 512), 0), ((2, 3, 100, 30), 0), ((2, 3, 100, 30), 2)],
                         ids=["columns", "sorted", "columns_forced"])
def test_three_interpolate_grad(cuda, dtype, shape, variant):
    b, c, n, m = shape                                    # n interpolated points, m known points
    g = gen(sum(shape) + variant)
    idx, weight = interp_inputs(b, n, m, g, cuda)
    assert int(torch.stack([torch.bincount(r.flatten().long(), minlength=m) for r in idx.cpu()]).max()) <= 256
    grad_out = positive((b, c, n), dtype, g, cuda)

    def fp32():
        wide = torch.zeros(b, c, m, device=cuda)
        sampling.three_interpolate_grad_wrapper(b, c, n, m, grad_out.float(), idx, weight, wide)
        return wide.to(dtype)

    def run():
        out = torch.full((b, c, m), float("nan"), dtype=dtype, device=cuda)
        sampling.three_interpolate_grad_wrapper(b, c, n, m, grad_out, idx, weight, out)
        check_written(out, idx, m)
        return out

    # the form each id names, and the fp32 reference's: 100 points are too few for fp32 to sort -- its atomics
    form16, form32 = {((2, 4, 2048, 512), 0): (COLUMN, COLUMN), ((2, 3, 100, 30), 0): (SORTED, ATOMICS),
                      ((2, 3, 100, 30), 2): (COLUMN, COLUMN)}[(shape, variant)]
    with knob("three_interpolate_grad_variant", variant):
        assert_plan(dtype, INTERP, b, c, n, m, form16)
        assert_plan(torch.float32, INTERP, b, c, n, m, form32)
        out, ref = run(), fp32()
    if variant == 2 or shape[2] >= 2048:                  # the double columns: the fp32 operator's own bits
        assert torch.equal(bits(out), bits(ref))
    assert units_apart(out, ref) <= 1
    with deterministic():
        ref, first, second = fp32(), run(), run()
    assert torch.equal(bits(first), bits(ref)) and torch.equal(bits(first), bits(second))
    features = torch.zeros(b, c, m, dtype=dtype, device=cuda, requires_grad=True)
    pn2.three_interpolate(features, idx, weight).backward(grad_out)
    assert features.grad.dtype == dtype and units_apart(features.grad, fp32()) <= 1


# ------------------------------------------------------------------------------------------------------- 6. fallback
@pytest.mark.parametrize("dtype", TYPES, ids=TYPE_IDS)
def test_backward_without_an_atomic_free_form_falls_back_to_fp32(cuda, dtype):
    b, c, n, npoint, nsample = 2, 3, 20481, 8, 8          # no sorted-scatter workspace (> 20480), P < 4096: no column
    g = gen(6)
    idx = torch.randint(0, n, (b, npoint, nsample), generator=g, dtype=torch.int32).to(cuda)
    grad_out = positive((b, c, npoint, nsample), dtype, g, cuda)
    assert _lib.lib().pp_scatter_workspace_bytes(b, npoint * nsample, n, 1, 0) == 0
    code, _ = raw_group_grad(grad_out, idx, n)
    assert code == _lib.PP_ENOTSUP
    out = sampling.group_points_grad(grad_out, idx, n)
    ref = sampling.group_points_grad(grad_out.float(), idx, n).to(dtype)
    assert out.dtype == dtype and units_apart(out, ref) <= 1
    check_written(out, idx, n)
    wide = torch.zeros(b, c, n, device=cuda)
    m = npoint * nsample
    sampling.gather_backward(b, c, n, m, grad_out.view(b, c, m).float(), idx.view(b, m), wide)
    got = torch.full((b, c, n), float("nan"), dtype=dtype, device=cuda)
    sampling.gather_backward(b, c, n, m, grad_out.view(b, c, m), idx.view(b, m), got)
    assert units_apart(got, wide.to(dtype)) <= 1


# ------------------------------------------------------------------------------------------------- 7. QueryAndGroup
@pytest.mark.parametrize("dtype", TYPES, ids=TYPE_IDS)
def test_query_and_group(cuda, dtype):
    b, n, npoint, c, nsample = 2, 256, 32, 5, 8
    g = gen(7)
    xyz = torch.rand(b, n, 3, generator=g).to(cuda)
    new_xyz = xyz[:, :npoint].contiguous()
    features = torch.randn(b, c, n, generator=g).to(cuda).to(dtype)
    idx = ops.ball_query(0.3, nsample, xyz, new_xyz)
    alone = ops.QueryAndGroup(0.3, nsample, use_xyz=False)
    f = features.clone().requires_grad_(True)
    out = alone(xyz, new_xyz, f)
    assert out.dtype == dtype and torch.equal(bits(out), ref_group_bits(features, idx))
    assert torch.equal(bits(alone.forward_unfused(xyz, new_xyz, features)), bits(out))
    out.backward(torch.ones_like(out))
    assert f.grad.dtype == dtype and f.grad.shape == features.shape
    counts = torch.stack([torch.bincount(r.flatten().long(), minlength=n) for r in idx]).float()
    assert torch.equal(f.grad.float(), counts[:, None].expand(b, c, n).to(dtype).float())      # small integers: exact
    both = ops.QueryAndGroup(0.3, nsample, use_xyz=True)
    f2 = features.clone().requires_grad_(True)
    out2 = both(xyz, new_xyz, f2)
    ref2 = both.forward_unfused(xyz, new_xyz, features)
    assert out2.dtype == torch.float32 and ref2.dtype == torch.float32 and torch.equal(out2, ref2)
    out2.backward(torch.ones_like(out2))
    assert f2.grad.dtype == dtype and torch.equal(f2.grad, f.grad)


# -------------------------------------------------------------------------------------------------- 8. dtype errors
def test_dtype_errors(cuda):
    g = gen(8)
    half = torch.randn(2, 3, 16, generator=g).to(cuda).half()
    idx2 = torch.zeros(2, 4, dtype=torch.int32, device=cuda)
    with pytest.raises(RuntimeError, match="out is torch.bfloat16"):
        sampling.gather_forward(2, 3, 16, 4, half, idx2, torch.empty(2, 3, 4, dtype=torch.bfloat16, device=cuda))
    with pytest.raises(RuntimeError, match="grad_points is torch.float16"):
        sampling.gather_backward(2, 3, 16, 4, half[:, :, :4].contiguous().bfloat16(), idx2, torch.empty_like(half))
    idx3 = torch.zeros(2, 8, 3, dtype=torch.int32, device=cuda)
    weight = torch.full((2, 8, 3), 1 / 3, device=cuda)
    with pytest.raises(RuntimeError, match="weight must be a float tensor"):
        pn2.three_interpolate(half, idx3, weight.half())
    with pytest.raises(RuntimeError, match="weight must be a float tensor"):
        sampling.three_interpolate_grad_wrapper(2, 3, 8, 16, half[:, :, :8].contiguous(), idx3, weight.bfloat16(),
                                                torch.empty_like(half))
    with pytest.raises(RuntimeError, match="out is torch.float32"):
        sampling.three_interpolate_wrapper(2, 3, 16, 8, half, idx3, weight, torch.empty(2, 3, 8, device=cuda))
    with pytest.raises(RuntimeError, match="out is torch.float16"):
        sampling.group_points_into(half.bfloat16(), idx3, torch.empty(2, 3, 8, 3, dtype=torch.float16, device=cuda), 0)
    for call in (lambda: ops.gather_points(half.double(), idx2), lambda: ops.grouping_operation(half.double(), idx3),
                 lambda: pn2.three_interpolate(half.double(), idx3, weight)):
        with pytest.raises(RuntimeError, match="must be a float tensor"):
            call()


# ----------------------------------------------------------------------------------------- 9. autocast, end to end
class _RoundBoth(torch.autograd.Function):
    """bf16 rounding of the value on the way forward and of the gradient on the way back: what a bf16 tensor between
    two operators does to both"""

    @staticmethod
    def forward(ctx, x):
        return x.bfloat16().to(x.dtype)

    @staticmethod
    def backward(ctx, g):
        return g.bfloat16().to(g.dtype)


def _composed_pipeline(w, x, idx1, idx2, idx3, weight, rnd):
    """the pipeline of the test from torch's own operators, on any device and dtype; rnd() stands where the autocast
    run holds a bf16 tensor: the matmul's operands and result, and the three operators' results"""
    b, c = x.shape[0], w.shape[0]
    feats = rnd(torch.matmul(rnd(w), rnd(x)))
    picked = rnd(torch.gather(feats, 2, idx1.long().view(b, 1, -1).expand(b, c, -1)))
    grouped = rnd(torch.gather(picked, 2, idx2.long().view(b, 1, -1).expand(b, c, -1)).view(b, c, *idx2.shape[1:]))
    pooled = grouped.max(-1)[0]
    three = torch.gather(pooled, 2, idx3.long().view(b, 1, -1).expand(b, c, -1)).view(b, c, -1, 3)
    return rnd((three * weight.to(x.dtype)[:, None]).sum(-1))


def test_autocast_end_to_end(cuda, capsys):
    """Outputs: the fp32 operators on the widened bf16 features, rounded where the autocast run holds bf16, must agree
    to one unit of bf16 (the copies and the maximum are exact, the interpolation is rounded once from the same fp32
    value).  Parameter gradient: figure = max |g - g64| / max |g64| against the unrounded fp64 composition g64; the
    bound is 4 x the same figure of the fp32 composition with the bf16 roundings put in, run on the CPU -- what bf16
    alone does to this gradient (the rule of DESIGN.md "k-NN edge operators"); both figures are printed."""
    b, cin, c, n, m1, npoint, nsample, nq = 2, 6, 8, 256, 64, 32, 8, 100
    g = gen(99)
    w = torch.randn(c, cin, generator=g)
    x = torch.randn(b, cin, n, generator=g)
    idx1 = torch.randint(0, n, (b, m1), generator=g, dtype=torch.int32)
    idx2 = torch.randint(0, m1, (b, npoint, nsample), generator=g, dtype=torch.int32)
    idx3, weight = interp_inputs(b, nq, npoint, g, cuda)
    param = w.to(cuda).requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        feats = torch.matmul(param, x.to(cuda))
        picked = ops.gather_points(feats, idx1.to(cuda))
        grouped = ops.grouping_operation(picked, idx2.to(cuda))
        pooled = grouped.max(-1)[0]
        out = pn2.three_interpolate(pooled, idx3, weight)
        loss = out.sum()
    loss.backward()
    assert all(t.dtype == torch.bfloat16 for t in (feats, picked, grouped, pooled, out))
    assert param.grad.dtype == torch.float32 and torch.isfinite(param.grad).all()
    # the fp32 operators on the widened features, rounded at the same three places
    f32 = feats.detach().float()
    p32 = ops.gather_points(f32, idx1.to(cuda)).bfloat16()
    g32 = ops.grouping_operation(p32.float(), idx2.to(cuda)).bfloat16()
    o32 = pn2.three_interpolate(g32.float().max(-1)[0], idx3, weight).bfloat16()
    for got, ref in ((picked, p32), (grouped, g32), (out, o32)):
        d = (bits(got.detach()).int() - bits(ref).int()).abs().max()
        assert int(d) <= 1 and torch.equal(got.detach() < 0, ref < 0)
    # the parameter gradient
    def grad_of(dtype, rnd):
        wp = w.to(dtype).requires_grad_(True)
        _composed_pipeline(wp, x.to(dtype), idx1, idx2, idx3.cpu(), weight.cpu(), rnd).sum().backward()
        return wp.grad.double()
    g64 = grad_of(torch.float64, lambda t: t)
    scale = g64.abs().max()
    cpu_figure = float((grad_of(torch.float32, _RoundBoth.apply) - g64).abs().max() / scale)
    gpu_figure = float((param.grad.double().cpu() - g64).abs().max() / scale)
    with capsys.disabled():
        print("\nautocast parameter gradient: GPU figure %.3e, rounded fp32 composition on the CPU %.3e, bound %.3e"
              % (gpu_figure, cpu_figure, 4 * cpu_figure))
    assert gpu_figure <= 4 * cpu_figure


# ------------------------------------------------------------------------------------------- 10. graphs and streams
def _graph_cases(dtype, dev):
    g = gen(10)
    b, c, n, npoint, nsample = 8, 4, 4096, 1024, 64
    gidx = ball_style_idx(b, npoint, nsample, n, g).to(dev)
    gb, gc, gn, gm = 4, 8, 2048, 512
    aidx = torch.randint(0, gn, (gb, gm), generator=g, dtype=torch.int32).to(dev)
    ib, ic, im, inn = 8, 4, 4096, 16384
    iidx, iw = interp_inputs(ib, inn, im, g, dev)

    def group(feat, grad):
        return sampling.group_points(feat, gidx), sampling.group_points_grad(grad, gidx, n)

    def gather(feat, grad):
        out = torch.empty(gb, gc, gm, dtype=dtype, device=dev)
        back = torch.empty(gb, gc, gn, dtype=dtype, device=dev)
        sampling.gather_forward(gb, gc, gn, gm, feat, aidx, out)
        sampling.gather_backward(gb, gc, gn, gm, grad, aidx, back)
        return out, back

    def interp(feat, grad):
        out = torch.empty(ib, ic, inn, dtype=dtype, device=dev)
        back = torch.empty(ib, ic, im, dtype=dtype, device=dev)
        sampling.three_interpolate_wrapper(ib, ic, im, inn, feat, iidx, iw, out)
        sampling.three_interpolate_grad_wrapper(ib, ic, inn, im, grad, iidx, iw, back)
        return out, back

    return {"group": (group, (b, c, n), (b, c, npoint, nsample), {}),
            "gather": (gather, (gb, gc, gn), (gb, gc, gm), {"gather_variant": 2}),
            "interp": (interp, (ib, ic, im), (ib, ic, inn), {"three_interpolate_variant": 3})}


@pytest.mark.parametrize("dtype", TYPES, ids=TYPE_IDS)
@pytest.mark.parametrize("name", ["group", "gather", "interp"])
def test_graph_replay_and_side_stream_match_eager(cuda, dtype, name):
    """Forwards in their LDS forms; the backwards of group_points and three_interpolate in their default form, the
    double columns (a sum of doubles rounded to fp32, then to T: the same bytes whatever the order); gather's only
    form is the sorted scatter, whose fp32 order is fixed in deterministic mode alone, so it runs in that mode."""
    step, fshape, gshape, knobs = _graph_cases(dtype, cuda)[name]
    g = gen(11)
    sets = [(positive(fshape, dtype, g, cuda), positive(gshape, dtype, g, cuda)) for _ in range(2)]
    feat, grad = sets[0][0].clone(), sets[0][1].clone()
    with contextlib.ExitStack() as stack:
        for k, v in knobs.items():
            stack.enter_context(knob(k, v))
        if name == "gather":
            stack.enter_context(deterministic())
        eager = [step(f, gr) for f, gr in sets]
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            on_side = step(*sets[1])
            step(feat, grad)                               # warm-up of the capture's inputs, off the default stream
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            captured = step(feat, grad)
        feat.copy_(sets[1][0])
        grad.copy_(sets[1][1])
        graph.replay()
        torch.cuda.synchronize()
    for got in (on_side, captured):
        for a, ref in zip(got, eager[1]):
            assert torch.equal(bits(a), bits(ref))
    assert not torch.equal(bits(eager[0][0]), bits(eager[1][0]))
