"""Times the k-NN edge operators at B=32, N=16384, D=3, K=20 (fp32): forward and forward plus backward of
knn_edge_lengths and knn_laplacian, and PointEdgeLengthLoss end to end, each beside the in-tree torch composition on the
same device and data in the same run.

    python tools/knn_edges_time.py [--reps 20] [--out profiles/r10/knn_edges_time.txt]

Device events after warm-up, seeded data, the two forms alternating.  The forwards are also given as a fraction of
their HBM floor: idx read once (8 B per edge), the output written once, the cloud read once (a batch element's cloud,
196 KB, stays in L2 for the gathers), over the 8 TB/s peak of MI355X_MICROARCH's table.
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pytorch_points_amd import knn_edges, ops, synthetic  # noqa: E402
from pytorch_points_amd.network import model_loss  # noqa: E402

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
    B, N, D, K = 32, 16384, 3, 20
    x = torch.from_numpy(synthetic.unit_sphere(1, B, N, D)).to(dev).requires_grad_(True)
    y = (x.detach() + 0.01 * torch.from_numpy(synthetic.unit_sphere(2, B, N, D)).to(dev)).requires_grad_(True)
    idx = ops.knn_points(x.detach(), x.detach(), K=K + 1).idx[:, :, 1:].contiguous()
    wk = torch.rand(B, N, K, device=dev) * 2 - 1
    wd = torch.rand(B, N, D, device=dev) * 2 - 1
    out = []

    def line(text):
        print(text, flush=True)
        out.append(text)

    line("# tools/knn_edges_time.py --reps %d, one MI355X" % args.reps)
    line("device: %s | torch %s" % (torch.cuda.get_device_name(dev), torch.__version__))
    line("B=%d N=%d D=%d K=%d fp32 (%d edges); ms as median (best); HIP | torch composition" % (B, N, D, K, B * N * K))
    edges, cloud = B * N * K, B * N * D * 4
    floors = {"knn_edge_lengths": edges * 8 + edges * 4 + cloud, "knn_laplacian": edges * 8 + 2 * cloud}

    def report(label, hip, comp, floor_bytes=None):
        (hm, hb), (cm, cb) = timed_pair(hip, comp, args.reps)
        text = "%-38s %8.3f (%7.3f) | %8.3f (%7.3f)  -> %5.1fx" % (label, hm, hb, cm, cb, cm / hm)
        if floor_bytes is not None:
            floor = floor_bytes / HBM * 1e3
            text += "; HBM floor %.3f ms (%.0f MB): the forward runs at %.0f%% of it" % (
                floor, floor_bytes / 1e6, 100 * floor / hm)
        line(text)

    def fb(fn, w):
        return lambda: torch.autograd.grad(fn(x, idx), x, w)

    with torch.no_grad():
        report("knn_edge_lengths forward", lambda: knn_edges.knn_edge_lengths(x, idx),
               lambda: knn_edges.edge_lengths_composition(x, idx), floors["knn_edge_lengths"])
        report("knn_laplacian forward", lambda: knn_edges.knn_laplacian(x, idx),
               lambda: knn_edges.laplacian_composition(x, idx), floors["knn_laplacian"])
    report("knn_edge_lengths forward + backward", fb(knn_edges.knn_edge_lengths, wk),
           fb(knn_edges.edge_lengths_composition, wk))
    report("knn_laplacian forward + backward", fb(knn_edges.knn_laplacian, wd), fb(knn_edges.laplacian_composition, wd))
    torch.use_deterministic_algorithms(True)
    report("  ... with the ordered backward", fb(knn_edges.knn_edge_lengths, wk),
           fb(knn_edges.edge_lengths_composition, wk))
    torch.use_deterministic_algorithms(False)

    loss = model_loss.PointEdgeLengthLoss(K, torch.nn.L1Loss())

    def end_to_end(composed):
        hip = knn_edges.knn_edge_lengths

        def run():
            knn_edges.knn_edge_lengths = knn_edges.edge_lengths_composition if composed else hip
            try:
                torch.autograd.grad(loss(x, y), (x, y))
            finally:
                knn_edges.knn_edge_lengths = hip
        return run

    report("PointEdgeLengthLoss, search to grads", end_to_end(False), end_to_end(True))
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
