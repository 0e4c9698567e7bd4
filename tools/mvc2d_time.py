"""Times the 2-D mean_value_coordinates at B=8, N=16384, M=64 (a 64-gon cage, queries in and around it): the HIP
forward and forward plus backward in fp32 and fp64, and the in-tree torch composition on the same device and data,
the two alternating in one run; and the floors.

    python tools/mvc2d_time.py [--reps 20] [--out profiles/r13/mvc2d_time.txt]

Device events after warm-up, seeded data, the median of --reps runs.  Write floor: the B*M*N*4 bytes of phi at
8 TB/s.  Compute floor: the vector instructions of the forward kernel's second walk (counted in the gfx950 assembly
of csrc/mvc2d.hip, built here with --save-temps; sqrt and the divisions are inlined there) per (vertex, query) pair,
both walks counted as two of them, times B*M*N pairs, at the fp64 vector issue rate of 256 CUs x 4 SIMDs x 16 lanes
x 2.4 GHz / 2 = 19.7e12 lane instructions/s (an fp64 instruction issues at half the fp32 rate; the loop is almost
all fp64).  A straight-line count of the loop body: an estimate, not a bound.
"""
import argparse
import glob
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pytorch_points_amd import _build, mvc2d  # noqa: E402

ISSUE_F64 = 256 * 4 * 16 * 2.4e9 / 2
HBM = 8e12


def timed_pair(fa, fb, reps, warmup=2):
    """medians (ms) of fa and fb, run alternately"""
    for _ in range(warmup):
        fa()
        fb()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(reps):
        for fn, out in ((fa, ta), (fb, tb)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            out.append(a.elapsed_time(b))
    return float(np.median(ta)), float(np.median(tb))


def loop_valu_count():
    """vector instructions of the longest loop (backward branch span) in mvc2d_forward_kernel<float>"""
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), *[f for f in _build.HIPCC_FLAGS if f != "-shared"],
               "-I" + _build.INCLUDE, "-I" + _build.CSRC, "--save-temps", "-c",
               os.path.join(_build.CSRC, "mvc2d.hip"), "-o", os.path.join(tmp, "mvc2d.o")]
        subprocess.run(cmd, cwd=tmp, check=True, capture_output=True)
        asm = open(glob.glob(os.path.join(tmp, "*gfx950*.s"))[0]).read()
    name = re.search(r"^(_ZN\S*mvc2d_forward_kernelIfE\S*):", asm, re.M).group(1)
    body = asm[asm.index(name + ":"):]
    lines = body[:body.index("s_endpgm")].splitlines()
    labels = {m.group(1): i for i, m in enumerate(re.match(r"^(\.LBB\w+):", ln) for ln in lines) if m}
    best = None
    for i, ln in enumerate(lines):
        m = re.match(r"\s+s_cbranch_\w+\s+(\.LBB\w+)|\s+s_branch\s+(\.LBB\w+)", ln)
        if m:
            tgt = m.group(1) or m.group(2)
            if tgt in labels and labels[tgt] < i and (best is None or i - labels[tgt] > best[1] - best[0]):
                best = (labels[tgt], i)
    seg = lines[best[0]:best[1] + 1]
    return sum(1 for ln in seg if re.match(r"\s+v_", ln)), sum(1 for ln in seg if re.match(r"\s+(v_|s_|global_)", ln))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    B, N, M = 8, 16384, 64
    rng = np.random.default_rng(0)
    ang = 2 * np.pi * np.arange(M) / M
    poly = np.stack([np.stack([np.cos(ang), np.sin(ang)]) * rng.uniform(0.9, 1.1, (2, 1)) for _ in range(B)])
    qa, qr = rng.uniform(0, 2 * np.pi, (B, N)), rng.uniform(0.05, 1.5, (B, N))
    pts = np.stack([qr * np.cos(qa), qr * np.sin(qa)], 1)
    out = []

    def line(text):
        print(text)
        out.append(text)

    line("# tools/mvc2d_time.py --reps %d, one MI355X" % args.reps)
    line("device: %s | torch %s" % (torch.cuda.get_device_name(dev), torch.__version__))
    line("B=%d N=%d M=%d (%d pairs); medians of %d runs, kernel and composition alternating" % (B, N, M, B * N * M,
                                                                                                args.reps))
    fwd32 = None
    for dt, name in ((torch.float32, "fp32"), (torch.float64, "fp64")):
        q = torch.from_numpy(pts).to(dev, dt).requires_grad_(True)
        p = torch.from_numpy(poly).to(dev, dt).requires_grad_(True)
        G = torch.randn(B, M, N, device=dev, dtype=dt)

        def forward(fn):
            with torch.no_grad():
                fn(q, p)

        def both(fn):
            torch.autograd.grad(fn(q, p), (q, p), G)

        kf, cf = timed_pair(lambda: forward(mvc2d.mean_value_coordinates), lambda: forward(mvc2d.composition), args.reps)
        kb, cb = timed_pair(lambda: both(mvc2d.mean_value_coordinates), lambda: both(mvc2d.composition), args.reps)
        line("%s forward: HIP %.3f ms | composition %.3f ms -> %.1fx" % (name, kf, cf, cf / kf))
        line("%s forward + backward: HIP %.3f ms | composition %.3f ms -> %.1fx" % (name, kb, cb, cb / kb))
        if dt == torch.float32:
            fwd32 = kf
    line("write floor (fp32 phi, %.1f MB at 8 TB/s): %.4f ms" % (B * M * N * 4 / 1e6, B * M * N * 4 / HBM * 1e3))
    try:
        valu, allins = loop_valu_count()
        floor = 2 * valu * B * N * M / ISSUE_F64 * 1e3
        line("second walk of the forward: %d vector instructions (%d in all) per pair; two walks -> compute floor %.3f ms "
             "at the fp64 issue rate; the fp32 forward runs at %.0f%% of it" % (valu, allins, floor, 100 * floor / fwd32))
    except Exception as exc:  # the assembly count needs hipcc; the timings stand without it
        line("compute floor not computed: %s" % exc)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
