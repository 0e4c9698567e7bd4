"""Times the 16-bit feature path (DESIGN.md §4 "16-bit features") of group_points, gather_points and
three_interpolate, forward and backward, in fp32, bf16 and fp16:

    python tools/features16_time.py [--reps 20] [--commit <id>] [--out profiles/r14/features16_time.txt]

  group_points       at config 4: B=32, C=128, N=16384, npoint=4096, nsample=64 (ball-query-style rows: a third pads)
  gather_points      at B=32, C=128, N=16384, M=4096
  three_interpolate  at B=32, C=128, M=4096 known, N=16384 interpolated

Beside each 16-bit operator runs what a user had to write without it -- x.float() -> the fp32 operator -> .to(T) --
and the fp32 operator alone on the widened tensor; the three alternate in one loop, device events after warm-up,
medians of --reps runs.  Every call allocates its output, in all three columns.  The traffic floor of a line is its
bytes at 8 TB/s: the feature streams (half the fp32 bytes in 16-bit) plus the index and weight bytes, which do not
change.  Two conditions are reported: (a) every 16-bit operator below the widening composition, (b) group_points in
bf16, forward and backward, below the fp32 operator.
"""
import argparse
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pytorch_points_amd._ext import sampling  # noqa: E402

HBM = 8e12


def timed(fns, reps, warmup=2):
    """medians (ms) of the functions, run alternately"""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(reps):
        for fn, out in zip(fns, times):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            out.append(a.elapsed_time(b))
    return [float(np.median(t)) for t in times]


def commit_id():
    try:
        return subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True,
                              check=True).stdout.strip()
    except Exception:
        return "unknown"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    out, verdict = [], {"a": True, "b": True}

    def line(text):
        print(text, flush=True)
        out.append(text)

    line("# tools/features16_time.py --reps %d, one MI355X" % args.reps)
    line("commit: %s" % (args.commit or commit_id()))
    line("device: %s | torch %s" % (torch.cuda.get_device_name(dev), torch.__version__))
    line("medians of %d runs (ms), the three columns alternating; floor = bytes at 8 TB/s" % args.reps)

    def report(what, name, t16, tcomp, t32, bytes32_feat, bytes_other, gated_b):
        floor32 = (bytes32_feat + bytes_other) / HBM * 1e3
        floor16 = (bytes32_feat / 2 + bytes_other) / HBM * 1e3
        a_ok = t16 < tcomp
        verdict["a"] &= a_ok
        text = ("%-26s %-4s 16-bit %.3f | widen+fp32+round %.3f (a: %s) | fp32 %.3f | 16-bit/fp32 %.2f | floor fp32 %.3f, "
                "16-bit %.3f (at %.2f of it)" % (what, name, t16, tcomp, "ok" if a_ok else "FAIL", t32, t16 / t32, floor32,
                                                 floor16, floor16 / t16))
        if gated_b:
            b_ok = t16 < t32
            verdict["b"] &= b_ok
            text += " (b: %s)" % ("ok" if b_ok else "FAIL")
        line(text)

    g = torch.Generator(device=dev).manual_seed(0)
    B, C, N = 32, 128, 16384
    types = ((torch.bfloat16, "bf16"), (torch.float16, "fp16"))

    # ---- group_points at config 4
    npoint, nsample = 4096, 64
    P = npoint * nsample
    idx = torch.randint(0, N, (B, npoint, nsample), generator=g, device=dev, dtype=torch.int32)
    hits = torch.randint(nsample // 3, nsample + 1, (B, npoint, 1), generator=g, device=dev)
    idx = torch.where(torch.arange(nsample, device=dev).view(1, 1, -1) >= hits, idx[:, :, :1].expand_as(idx), idx)
    idx = idx.contiguous()
    feat32 = torch.randn(B, C, N, generator=g, device=dev)
    line("group_points: B=%d C=%d N=%d npoint=%d nsample=%d" % (B, C, N, npoint, nsample))
    for dt, name in types:
        feat = feat32.to(dt)
        wide = feat.float()
        t16, tc, t32 = timed([lambda: sampling.group_points(feat, idx),
                              lambda: sampling.group_points(feat.float(), idx).to(dt),
                              lambda: sampling.group_points(wide, idx)], args.reps)
        report("group_points forward", name, t16, tc, t32, 4.0 * B * C * (P + N), 4.0 * B * P, dt is torch.bfloat16)
    del feat, wide
    grad32 = torch.rand(B, C, npoint, nsample, generator=g, device=dev)
    for dt, name in types:
        grad = grad32.to(dt)
        t16, tc, t32 = timed([lambda: sampling.group_points_grad(grad, idx, N),
                              lambda: sampling.group_points_grad(grad.float(), idx, N).to(dt),
                              lambda: sampling.group_points_grad(grad32, idx, N)], args.reps)
        report("group_points backward", name, t16, tc, t32, 4.0 * B * C * (P + N), 4.0 * B * P, dt is torch.bfloat16)
        del grad
    del grad32, idx
    torch.cuda.empty_cache()

    # ---- gather_points
    M = 4096
    gidx = torch.randint(0, N, (B, M), generator=g, device=dev, dtype=torch.int32)
    line("gather_points: B=%d C=%d N=%d M=%d" % (B, C, N, M))

    def gather_fwd(x):
        o = torch.empty(B, C, M, dtype=x.dtype, device=dev)
        sampling.gather_forward(B, C, N, M, x, gidx, o)
        return o

    def gather_bwd(x):
        o = (torch.zeros if x.dtype is torch.float32 else torch.empty)(B, C, N, dtype=x.dtype, device=dev)
        sampling.gather_backward(B, C, N, M, x, gidx, o)
        return o

    ggrad32 = torch.rand(B, C, M, generator=g, device=dev)
    for dt, name in types:
        feat = feat32.to(dt)
        wide = feat.float()
        t16, tc, t32 = timed([lambda: gather_fwd(feat), lambda: gather_fwd(feat.float()).to(dt),
                              lambda: gather_fwd(wide)], args.reps)
        report("gather_points forward", name, t16, tc, t32, 4.0 * B * C * (N + M), 4.0 * B * M, False)
        grad = ggrad32.to(dt)
        t16, tc, t32 = timed([lambda: gather_bwd(grad), lambda: gather_bwd(grad.float()).to(dt),
                              lambda: gather_bwd(ggrad32)], args.reps)
        report("gather_points backward", name, t16, tc, t32, 4.0 * B * C * (N + M), 4.0 * B * M, False)
    del feat32, feat, wide

    # ---- three_interpolate: M known points, N interpolated
    Mk, Nq = 4096, 16384
    known = torch.rand(B, Mk, 3, generator=g, device=dev)
    unknown = torch.rand(B, Nq, 3, generator=g, device=dev)
    dist2 = torch.empty(B, Nq, 3, device=dev)
    iidx = torch.empty(B, Nq, 3, dtype=torch.int32, device=dev)
    sampling.three_nn_wrapper(B, Nq, Mk, unknown, known, dist2, iidx)
    recip = 1.0 / (dist2.sqrt() + 1e-8)
    weight = (recip / recip.sum(2, keepdim=True)).contiguous()
    line("three_interpolate: B=%d C=%d M=%d N=%d" % (B, C, Mk, Nq))

    def interp_fwd(x):
        o = torch.empty(B, C, Nq, dtype=x.dtype, device=dev)
        sampling.three_interpolate_wrapper(B, C, Mk, Nq, x, iidx, weight, o)
        return o

    def interp_bwd(x):
        o = (torch.zeros if x.dtype is torch.float32 else torch.empty)(B, C, Mk, dtype=x.dtype, device=dev)
        sampling.three_interpolate_grad_wrapper(B, C, Nq, Mk, x, iidx, weight, o)
        return o

    kfeat32 = torch.randn(B, C, Mk, generator=g, device=dev)
    igrad32 = torch.rand(B, C, Nq, generator=g, device=dev)
    for dt, name in types:
        feat = kfeat32.to(dt)
        t16, tc, t32 = timed([lambda: interp_fwd(feat), lambda: interp_fwd(feat.float()).to(dt),
                              lambda: interp_fwd(kfeat32)], args.reps)
        report("three_interpolate forward", name, t16, tc, t32, 4.0 * B * C * (Mk + Nq), 24.0 * B * Nq, False)
        grad = igrad32.to(dt)
        t16, tc, t32 = timed([lambda: interp_bwd(grad), lambda: interp_bwd(grad.float()).to(dt),
                              lambda: interp_bwd(igrad32)], args.reps)
        report("three_interpolate backward", name, t16, tc, t32, 4.0 * B * C * (Mk + Nq), 24.0 * B * Nq, False)

    line("condition (a), every 16-bit operator below the widening composition: %s" % ("met" if verdict["a"] else "NOT MET"))
    line("condition (b), group_points bf16 forward and backward below the fp32 operator: %s"
         % ("met" if verdict["b"] else "NOT MET"))
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
