"""Times the mesh Laplacians at B=32 on a triangulated 128x128 vertex grid with one shared topology (N=16384, F=32258,
fp32): the corner build, cotangent, both applies forward and forward plus backward, and the two Laplacian losses to
gradients, each beside the index_add_ composition (mesh_laplacian.*_composition) on the same device and data in the
same run; the cotangent apply also beside the reference's way, a scipy CSR matrix applied on the host with the copies
there and back, where scipy can be imported.

    timeout -k 10 600 python tools/mesh_laplacian_time.py [--reps 20] [--out profiles/r12/mesh_laplacian_time.txt]

One process, one GPU step: run it under a time limit of its own, as above, and chain it to other steps with &&.
Device events after warm-up, the two forms alternating.  The apply's traffic floor stands beside the forward: the slot
tables read once (start, nbr; codes and weights too for the cotangent form), x read once, out written once, over the
8 TB/s peak of MI355X.
"""
import argparse
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pytorch_points_amd import mesh_laplacian as ml  # noqa: E402
from pytorch_points_amd.network import model_loss  # noqa: E402
from tools.mesh_edges_time import HBM, grid, timed_pair  # noqa: E402


def scipy_operator(faces, cot, n):
    """the reference's computeLaplacian (geo_operations.py:227-253) for the whole batch: a (B*n, B*n) CSR matrix"""
    from scipy import sparse
    b = cot.shape[0]
    stacked = (faces[None] + (np.arange(b) * n)[:, None, None]).reshape(-1, 3)
    size = b * n
    half = sparse.coo_matrix((cot.reshape(-1), (np.roll(stacked, -1, 1).reshape(-1), np.roll(stacked, -2, 1).reshape(-1))),
                             shape=(size, size)).tocsr()
    sym = half + half.T
    return (sym - sparse.diags(np.asarray(sym.sum(axis=1)).ravel())).tocsr()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    B, R = 32, 128
    v, f = grid(R, R)
    N, F = v.shape[0], f.shape[0]
    rng = np.random.default_rng(1)
    jitter = lambda: (v[None] + 0.2 / (R - 1) * rng.uniform(-1, 1, size=(B, N, 3))).astype(np.float32)   # noqa: E731
    x1 = torch.from_numpy(jitter()).to(dev).requires_grad_(True)
    x2 = torch.from_numpy(jitter()).to(dev).requires_grad_(True)
    faces = torch.from_numpy(f).to(dev)[None].expand(B, -1, -1)      # one topology, shared by the batch
    corners = ml.MeshCorners.from_faces(faces, N)
    assert corners.batch == 1
    weights = ml.cotangent(x1.detach(), faces)
    g = torch.rand(B, N, 3, device=dev) * 2 - 1
    out = []

    def line(text):
        print(text, flush=True)
        out.append(text)

    try:
        commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True,
                                text=True).stdout.strip() or "unknown"
    except OSError:
        commit = "unknown"
    line("# tools/mesh_laplacian_time.py --reps %d, one MI355X; commit %s" % (args.reps, os.environ.get("PP_COMMIT", commit)))
    line("device: %s | torch %s" % (torch.cuda.get_device_name(dev), torch.__version__))
    line("B=%d, %dx%d vertex grid, one shared topology: N=%d F=%d fp32; ms as median (best); HIP | index_add_ composition"
         % (B, R, R, N, F))
    tables = 4 * (N + 1) + 8 * 3 * F
    floor_uniform = tables + 2 * B * N * 12
    floor_cot = floor_uniform + 4 * 3 * F + B * F * 12

    def report(label, hip, comp, floor=None):
        (hm, hb), (cm, cb) = timed_pair(hip, comp, args.reps)
        text = "%-46s %8.3f (%7.3f) | %8.3f (%7.3f)  -> %5.1fx" % (label, hm, hb, cm, cb, cm / hm)
        if floor is not None:
            ms = floor / HBM * 1e3
            text += "; traffic floor %.4f ms (%.1f MB): %.0f%% of it" % (ms, floor / 1e6, 100 * ms / hm)
        line(text)

    def host_build():   # the composition needs no lists: its build is the index arithmetic of one apply
        return ml._corner_rows(x1, corners)

    with torch.no_grad():
        report("corner build (1 host read | index arithmetic)", lambda: ml.MeshCorners.from_faces(faces, N), host_build)
        report("cotangent", lambda: ml.cotangent(x1, faces), lambda: ml.cotangent_composition(x1, faces))
        report("uniform apply forward", lambda: ml.mesh_uniform_laplacian(x1, corners),
               lambda: ml.uniform_laplacian_composition(x1, corners), floor_uniform)
        report("cotangent apply forward", lambda: ml.mesh_cot_laplacian(x1, corners, weights),
               lambda: ml.cot_laplacian_composition(x1, corners, weights), floor_cot)
    report("uniform apply forward + backward", lambda: torch.autograd.grad(ml.mesh_uniform_laplacian(x1, corners), x1, g),
           lambda: torch.autograd.grad(ml.uniform_laplacian_composition(x1, corners), x1, g))
    report("cotangent apply forward + backward",
           lambda: torch.autograd.grad(ml.mesh_cot_laplacian(x1, corners, weights), x1, g),
           lambda: torch.autograd.grad(ml.cot_laplacian_composition(x1, corners, weights), x1, g))
    try:
        lap = scipy_operator(f, weights.cpu().numpy().astype(np.float32), N)
    except ImportError:
        line("cotangent apply, the reference's way (scipy CSR on the host): skipped, scipy cannot be imported here")
    else:
        def scipy_step():   # forward and backward of reference :276-302: two round trips
            y = torch.from_numpy(lap.dot(x1.detach().reshape(-1, 3).cpu().numpy())).to(dev)
            return y, torch.from_numpy(lap.dot(g.reshape(-1, 3).cpu().numpy())).to(dev)
        report("cotangent apply fwd + bwd | scipy CSR on the host",
               lambda: torch.autograd.grad(ml.mesh_cot_laplacian(x1, corners, weights), x1, g), scipy_step)

    class CompositionLaplacian(torch.nn.Module):
        """geo_operations' modules over the compositions, for the losses' baseline"""

        def __init__(self, use_cot):
            super().__init__()
            self.use_cot, self.L = use_cot, None

        def forward(self, verts, face=None):
            if self.L is None:
                self.L = ml.cotangent_composition(verts.detach(), face).detach() if self.use_cot else True
            if self.use_cot:
                return ml.cot_laplacian_composition(verts, corners, self.L)
            return ml.uniform_laplacian_composition(verts, corners)

    l1 = torch.nn.L1Loss()
    for use_cot in (False, True):
        for keep in (True, False):
            mod = model_loss.MeshLaplacianLoss(l1, use_cot=use_cot, consistent_topology=keep)
            base = model_loss.MeshLaplacianLoss(l1, use_cot=use_cot, consistent_topology=keep)
            base.laplacian = CompositionLaplacian(use_cot)
            mod(x1, x2, faces)
            base(x1, x2, faces)
            report("MeshLaplacianLoss(L1%s), %s, to grads" % (", cot" if use_cot else "", "kept Laplacian" if keep else
                                                              "rebuilt every call"),
                   lambda m=mod: torch.autograd.grad(m(x1, x2, faces), (x1, x2)),
                   lambda m=base: torch.autograd.grad(m(x1, x2, faces), (x1, x2)))
    smooth = model_loss.UniformLaplacianSmoothnessLoss(N, faces, None)
    report("UniformLaplacianSmoothnessLoss, to grads", lambda: torch.autograd.grad(smooth(x1).mean(), x1),
           lambda: torch.autograd.grad(torch.norm(ml.uniform_laplacian_composition(x1, corners), p=2, dim=-1).mean(), x1))
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
