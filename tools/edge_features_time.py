"""Times knn_edge_features and DenseEdgeConv at the layer's shape, B=32, C=64, N=4096, k=16, in fp32 and bf16: the
operator's forward, and forward plus backward in the default and the ordered mode, each beside the in-tree torch
composition on the same device and data in the same run; and DenseEdgeConv(64, 32, 3, 16) from the search to the
gradients, ``forward`` beside ``forward_unfused``.

    python tools/edge_features_time.py [--reps 20] [--out profiles/r15/edge_features_time.txt]

Device events after warm-up, seeded data, the two forms alternating.  The forward is also given as a fraction of its
write floor: the output written once, idx and x read once (a channel's row of x, 16 KB, stays in cache for the
gathers), over the 8 TB/s peak of MI355X_MICROARCH's table.  In the ordered mode torch fills every torch.empty with NaN
(torch.utils.deterministic.fill_uninitialized_memory); that is switched off here for both forms, so that the row
compares the two backwards and not a 1 GB fill.
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pytorch_points_amd import edge_features, ops, synthetic  # noqa: E402
from pytorch_points_amd.network import layers  # noqa: E402

HBM = 8.0e12


def timed_pair(fa, fb, reps, warmup=3):
    """median and best ms of fa and of fb, one call of each in turn"""
    for _ in range(warmup):
        fa()
        fb()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(reps):
        for fn, times in ((fa, ta), (fb, tb)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            times.append(a.elapsed_time(b))
    return (float(np.median(ta)), float(np.min(ta))), (float(np.median(tb)), float(np.min(tb)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    B, C, N, K = 32, 64, 4096, 16
    out = []

    def line(text):
        print(text, flush=True)
        out.append(text)

    line("# tools/edge_features_time.py --reps %d, one MI355X" % args.reps)
    line("device: %s | torch %s" % (torch.cuda.get_device_name(dev), torch.__version__))
    line("B=%d C=%d N=%d k=%d (%d edges, output %d elements); ms as median (best); HIP | torch composition"
         % (B, C, N, K, B * N * K, B * 2 * C * N * K))

    def report(label, hip, comp, floor_bytes=None):
        (hm, hb), (cm, cb) = timed_pair(hip, comp, args.reps)
        text = "%-44s %8.3f (%7.3f) | %8.3f (%7.3f)  -> %5.2fx" % (label, hm, hb, cm, cb, cm / hm)
        if floor_bytes is not None:
            floor = floor_bytes / HBM * 1e3
            text += "; write floor %.3f ms (%.0f MB): the forward runs at %.0f%% of it" % (
                floor, floor_bytes / 1e6, 100 * floor / hm)
        line(text)

    x32 = torch.from_numpy(synthetic.normal(1, (B, C, N))).to(dev)
    idx = ops.knn_points(x32.transpose(1, 2).contiguous(), x32.transpose(1, 2).contiguous(), K=K + 1).idx[:, :, 1:]
    for dtype in (torch.float32, torch.bfloat16):
        size = torch.empty(0, dtype=dtype).element_size()
        x = x32.to(dtype).requires_grad_(True)
        w = (torch.rand(B, 2 * C, N, K, device=dev) * 2 - 1).to(dtype)
        floor = B * 2 * C * N * K * size + B * N * K * 8 + B * C * N * size

        def fb(fn):
            return lambda: torch.autograd.grad(fn(x, idx), x, w)

        line("-- %s" % dtype)
        with torch.no_grad():
            report("knn_edge_features forward", lambda: edge_features.knn_edge_features(x, idx),
                   lambda: edge_features.composition(x, idx), floor)
        report("knn_edge_features forward + backward", fb(edge_features.knn_edge_features), fb(edge_features.composition))
        torch.use_deterministic_algorithms(True)
        fill = torch.utils.deterministic.fill_uninitialized_memory
        torch.utils.deterministic.fill_uninitialized_memory = False
        try:
            report("  ... with the ordered backward", fb(edge_features.knn_edge_features), fb(edge_features.composition))
        finally:
            torch.utils.deterministic.fill_uninitialized_memory = fill
            torch.use_deterministic_algorithms(False)

        torch.manual_seed(0)
        module = layers.DenseEdgeConv(C, 32, 3, K).to(device=dev, dtype=dtype)
        params = list(module.parameters())
        wy = (torch.rand(B, module.out_channels, N, device=dev) * 2 - 1).to(dtype)

        def end_to_end(forward):
            return lambda: torch.autograd.grad(forward(x)[0], [x] + params, wy)

        report("DenseEdgeConv(64,32,3,16), search to grads", end_to_end(module.forward), end_to_end(module.forward_unfused))
        del module, params, wy, w, x
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
