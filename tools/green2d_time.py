"""Times green_coordinates_2D at B=8, P=16384, N=F=64 (a 64-gon cage, queries in and around it): the HIP forward and
forward plus backward in fp32 and fp64, and the in-tree torch composition on the same device and data, the two
alternating in one run; and the write floor.

    python tools/green2d_time.py [--reps 20] [--out profiles/green2d/time.txt]

Device events after warm-up, seeded data, the median of --reps runs.  Write floor: the (N+F)*B*P*4 bytes of phi and
psi at 8 TB/s.  The composition evaluates every pair in fp64 for either data type, as the kernels do.
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pytorch_points_amd import green2d  # noqa: E402

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    B, P, N = 8, 16384, 64
    F = N
    rng = np.random.default_rng(0)
    ang = 2 * np.pi * np.arange(N) / N
    cage = np.stack([np.stack([np.cos(ang), np.sin(ang)], 1) * rng.uniform(0.9, 1.1, (1, 2)) for _ in range(B)])
    qa, qr = rng.uniform(0, 2 * np.pi, (B, P)), rng.uniform(0.05, 1.5, (B, P))
    pts = np.stack([qr * np.cos(qa), qr * np.sin(qa)], 2)
    faces = torch.from_numpy(np.stack([np.arange(N), (np.arange(N) + 1) % N], 1)).to(dev).expand(B, -1, -1).contiguous()
    out = []

    def line(text):
        print(text)
        out.append(text)

    line("# tools/green2d_time.py --reps %d, one MI355X" % args.reps)
    line("device: %s | torch %s" % (torch.cuda.get_device_name(dev), torch.__version__))
    line("B=%d P=%d N=F=%d (%d pairs); medians of %d runs, kernel and composition alternating" % (
        B, P, N, B * P * F, args.reps))
    for dt, name in ((torch.float32, "fp32"), (torch.float64, "fp64")):
        q = torch.from_numpy(pts).to(dev, dt).requires_grad_(True)
        v = torch.from_numpy(cage).to(dev, dt).requires_grad_(True)
        g_phi = torch.randn(B, P, N, device=dev, dtype=dt)
        g_psi = torch.randn(B, P, F, device=dev, dtype=dt)

        def forward(fn):
            with torch.no_grad():
                fn(q, v, faces)

        def both(fn):
            phi, psi, _ = fn(q, v, faces)
            torch.autograd.grad((phi, psi), (q, v), (g_phi, g_psi))

        kf, cf = timed_pair(lambda: forward(green2d.green_coordinates_2D), lambda: forward(green2d.composition),
                            args.reps)
        kb, cb = timed_pair(lambda: both(green2d.green_coordinates_2D), lambda: both(green2d.composition), args.reps)
        line("%s forward: HIP %.3f ms | composition %.3f ms -> %.1fx" % (name, kf, cf, cf / kf))
        line("%s forward + backward: HIP %.3f ms | composition %.3f ms -> %.1fx" % (name, kb, cb, cb / kb))
    nbytes = (N + F) * B * P * 4
    line("write floor (fp32 phi and psi, %.1f MB at 8 TB/s): %.4f ms" % (nbytes / 1e6, nbytes / HBM * 1e3))
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
