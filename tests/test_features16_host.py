"""CPU tests (no GPU) of the 16-bit feature path of gather_points, group_points and three_interpolate (DESIGN.md §4
"16-bit features"): the C ABI declares, binds and exports the new entry points, they check their sizes before any
pointer or device, and the fp32 -> bf16 / fp16 narrowing functions of csrc/pp_b16.h -- compiled for the host in a
stand-alone program -- equal torch's CPU conversion."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from pytorch_points_amd import _build, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COPIES = ["pp_gather_forward_b16", "pp_group_points_strided_b16"]
INTERP = ["pp_three_interpolate_f16", "pp_three_interpolate_bf16"]
GATHER_BWD = ["pp_gather_backward_out_ws_f16", "pp_gather_backward_out_ws_bf16"]
GROUP_BWD = ["pp_group_points_grad_out_ws_f16", "pp_group_points_grad_out_ws_bf16"]
INTERP_BWD = ["pp_three_interpolate_grad_out_ws_f16", "pp_three_interpolate_grad_out_ws_bf16"]
SYMBOLS = COPIES + INTERP + GATHER_BWD + GROUP_BWD + INTERP_BWD


def test_header_declares_and_library_exports_the_16_bit_entry_points():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pp_hip.h")).read(), flags=re.S)
    _build.build()
    handle = ctypes.CDLL(_build.LIB)
    for s in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, text), s
        assert s in _lib.SIGNATURES, s
        assert hasattr(handle, s), s


def test_argument_checks_are_host_only():
    """B == 0 (and every other empty problem) is served and a negative size is PP_EINVAL before a pointer or the
    device is looked at: all pointers are NULL here and there is no GPU."""
    L = _lib.lib()
    n3, n4 = [None] * 3, [None] * 4
    for ordered in (0, 1):
        for f in GATHER_BWD:
            fn = getattr(L, f)
            assert fn(*n3, 0, 4, 8, 8, None, 0, ordered, None) == 0
            assert fn(*n3, 2, 0, 8, 8, None, 0, ordered, None) == 0
            for bad in ((-1, 4, 8, 8), (1, -4, 8, 8), (1, 4, -8, 8), (1, 4, 8, -8)):
                assert fn(*n3, *bad, None, 0, ordered, None) == 1
            assert fn(*n3, 1, 4, 8, 8, None, 0, ordered, None) == 1            # null pointers with work to do
        for f in GROUP_BWD:
            fn = getattr(L, f)
            assert fn(*n3, 0, 4, 8, 2, 2, 16, None, 0, ordered, None) == 0
            assert fn(*n3, 2, 4, 0, 2, 2, 16, None, 0, ordered, None) == 0
            for bad in ((-1, 4, 8, 2, 2), (1, -4, 8, 2, 2), (1, 4, -8, 2, 2), (1, 4, 8, -2, 2), (1, 4, 8, 2, -2)):
                assert fn(*n3, *bad, 16, None, 0, ordered, None) == 1
            assert fn(*n3, 1, 4, 8, 2, 2, 16, None, 0, ordered, None) == 1
        for f in INTERP_BWD:
            fn = getattr(L, f)
            assert fn(*n4, 0, 4, 8, 8, None, 0, ordered, None) == 0
            assert fn(*n4, 2, 4, 8, 0, None, 0, ordered, None) == 0
            for bad in ((-1, 4, 8, 8), (1, -4, 8, 8), (1, 4, -8, 8), (1, 4, 8, -8)):
                assert fn(*n4, *bad, None, 0, ordered, None) == 1
            assert fn(*n4, 1, 4, 8, 8, None, 0, ordered, None) == 1
    fn = L.pp_gather_forward_b16
    assert fn(*n3, 0, 4, 8, 8, None) == 0 and fn(*n3, 2, 4, 8, 0, None) == 0
    for bad in ((-1, 4, 8, 8), (1, -4, 8, 8), (1, 4, -8, 8), (1, 4, 8, -8)):
        assert fn(*n3, *bad, None) == 1
    assert fn(*n3, 1, 4, 8, 8, None) == 1
    fn = L.pp_group_points_strided_b16
    assert fn(*n3, 0, 4, 8, 2, 2, 16, None) == 0 and fn(*n3, 2, 4, 8, 0, 2, 0, None) == 0
    for bad in ((-1, 4, 8, 2, 2), (1, -4, 8, 2, 2), (1, 4, -8, 2, 2), (1, 4, 8, -2, 2), (1, 4, 8, 2, -2)):
        assert fn(*n3, *bad, 16, None) == 1
    assert fn(*n3, 1, 4, 8, 2, 2, 15, None) == 1                               # a batch stride below C * P
    assert fn(*n3, 1, 4, 8, 2, 2, 16, None) == 1
    for f in INTERP:
        fn = getattr(L, f)
        assert fn(*n4, 0, 4, 8, 8, None) == 0 and fn(*n4, 2, 4, 8, 0, None) == 0
        for bad in ((-1, 4, 8, 8), (1, -4, 8, 8), (1, 4, -8, 8), (1, 4, 8, -8)):
            assert fn(*n4, *bad, None) == 1
        assert fn(*n4, 1, 4, 8, 8, None) == 1


def test_feature_dtype_rule():
    f32, f16, b16 = (torch.zeros(2, dtype=d) for d in (torch.float32, torch.float16, torch.bfloat16))
    assert _lib.require_feature_dtype(("points", f32), ("out", f32)) is torch.float32
    assert _lib.require_feature_dtype(("points", f16), ("out", f16)) is torch.float16
    assert _lib.require_feature_dtype(("points", b16)) is torch.bfloat16
    with pytest.raises(RuntimeError, match="out is torch.bfloat16"):
        _lib.require_feature_dtype(("points", f16), ("out", b16))
    with pytest.raises(RuntimeError, match="grad_points is torch.float32"):
        _lib.require_feature_dtype(("grad_out", b16), ("grad_points", f32))
    with pytest.raises(RuntimeError, match="points must be a float tensor"):
        _lib.require_feature_dtype(("points", f32.double()))
    with pytest.raises(RuntimeError, match="weight must be a float tensor"):
        _lib.require_float(("weight", b16))


PROGRAM = r"""
#include <stdio.h>
#include <stdlib.h>
#include "pp_b16.h"
int main(int argc, char** argv) {
  if (argc != 4) return 2;
  FILE* in = fopen(argv[1], "rb");
  FILE* ob = fopen(argv[2], "wb");
  FILE* oh = fopen(argv[3], "wb");
  if (!in || !ob || !oh) return 3;
  float f;
  while (fread(&f, 4, 1, in) == 1) {
    const uint16_t b = pp::narrow_bf16_bits(f), h = pp::narrow_f16_bits(f);
    if (pp::narrow<pp::bf16>(f).bits != b) return 4;
    fwrite(&b, 2, 1, ob);
    fwrite(&h, 2, 1, oh);
  }
  // widening is exact and narrowing it again is the identity on every non-NaN pattern
  for (unsigned u = 0; u < 65536; ++u) {
    pp::bf16 v;
    v.bits = (uint16_t)u;
    const bool nan = (u & 0x7fffu) > 0x7f80u;
    if (!nan && pp::narrow_bf16_bits(pp::widen(v)) != u) return 5;
    if (pp::f32_bits(pp::widen(v)) != (u << 16)) return 6;
  }
  fclose(ob);
  fclose(oh);
  return 0;
}
"""


def patterns():
    """fp32 bit patterns: every bf16 tie (low half 0x8000) with its two neighbours, every fp16 tie -- normal range
    (low 13 bits 0x1000) and the subnormal range ((k + 1/2) 2^-24) -- with neighbours, the overflow threshold of half,
    +-inf, NaNs of both signs and several payloads, both zeros, and 2048 random mantissas for each of the 512
    (sign, exponent) classes."""
    rng = np.random.RandomState(16)
    hi = np.arange(65536, dtype=np.uint32) << 16
    parts = [hi | 0x8000, hi | 0x7fff, hi | 0x8001, hi]
    exps = (np.arange(127 - 14, 127 + 16, dtype=np.uint32) << 23)[:, None]
    man = (np.arange(1024, dtype=np.uint32) << 13)[None, :]
    for low in (0x1000, 0x0fff, 0x1001):
        t = (exps | man | low).ravel()
        parts += [t, t | 0x80000000]
    sub = ((np.arange(1025, dtype=np.float64) + 0.5) * 2.0 ** -24).astype(np.float32)
    assert (sub.astype(np.float64) == (np.arange(1025) + 0.5) * 2.0 ** -24).all()
    subb = sub.view(np.uint32)
    parts += [subb, subb + 1, subb - 1, subb | 0x80000000]
    edge = np.array([65504.0, 65519.996, 65520.0, 65520.004, 65536.0, 1e38, 3.4028235e38, 2.0 ** -25, 2.0 ** -26,
                     np.inf, 0.0], dtype=np.float32).view(np.uint32)
    parts += [edge, edge | 0x80000000]
    parts.append(np.array([0x7fc00000, 0xffc00000, 0x7f800001, 0xff800001, 0x7fffffff, 0x7f80ffff, 0x7fa00000,
                           0x7f808000], dtype=np.uint32))
    cls = (np.arange(512, dtype=np.uint32) << 23)[:, None]
    parts.append((cls | rng.randint(0, 1 << 23, size=(512, 2048)).astype(np.uint32)).ravel())
    return np.concatenate([p.astype(np.uint32) for p in parts])


def test_narrowing_equals_torch_on_the_cpu(tmp_path):
    """NaN inputs are compared by class: torch itself does not fix the payload (its scalar bf16 conversion gives
    0x7fc0, its vectorised one 0xffff; F16C keeps the payload's top bits, the portable half conversion gives 0x7e00)."""
    src = tmp_path / "narrow.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "narrow"
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, "-x", "c++", "-std=c++17", "-O1", "-I" + _build.CSRC, str(src), "-o", str(exe)], check=True)
    bits = patterns()
    (tmp_path / "in.bin").write_bytes(bits.tobytes())
    subprocess.run([str(exe), str(tmp_path / "in.bin"), str(tmp_path / "bf16.bin"), str(tmp_path / "f16.bin")],
                   check=True)
    x = torch.from_numpy(bits.view(np.float32).copy())
    nan = torch.isnan(x).numpy()
    assert nan.sum() >= 8
    for name, dt, nan_test in (("bf16", torch.bfloat16, lambda b: (b & 0x7fff) > 0x7f80),
                               ("f16", torch.float16, lambda b: (b & 0x7fff) > 0x7c00)):
        got = np.fromfile(str(tmp_path / (name + ".bin")), dtype=np.uint16)
        ref = x.to(dt).view(torch.int16).numpy().view(np.uint16)
        assert got.shape == ref.shape
        assert nan_test(got[nan]).all() and nan_test(ref[nan]).all()
        bad = np.flatnonzero((got != ref) & ~nan)
        assert bad.size == 0, (name, [hex(int(bits[i])) for i in bad[:8]])
    # what the issue names: overflow of half gives +-inf, the bf16 rounding can carry into inf, infinities stay
    h = torch.tensor([65520.0, -65520.0, 65519.996]).to(torch.float16)
    assert h[0] == float("inf") and h[1] == float("-inf") and h[2] == 65504.0
