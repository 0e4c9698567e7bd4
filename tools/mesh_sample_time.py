"""Times the mesh surface sampling at B=32 on a triangulated 128x128 vertex grid (N=16384, F=32258 per element, fp32)
with S=16384 samples per element, with B separate topologies and with one shared one: the CDF build, the sample forward
and forward plus backward, mesh_interpolate forward and forward plus backward, and SampledMeshChamferLoss to the
gradient, each beside the torch composition of the same contract (mesh_sample.sample_composition: cumsum, searchsorted,
gathers, autograd's index_add_ backward) on the same device and data in the same run.

    python tools/mesh_sample_time.py [--reps 20] [--out profiles/mesh_sample/time.txt]

Device events after warm-up, the two forms alternating.  The traffic floor stands beside the forwards: per sample u
(12 B), points (12 B), face (8 B) and bary (12 B), and the faces, the vertices and the CDF read once, over the 8 TB/s
peak of MI355X.
"""
import argparse
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from mesh_edges_time import grid, timed_pair  # noqa: E402
from pytorch_points_amd import mesh_normals, mesh_sample  # noqa: E402
from pytorch_points_amd.mesh_laplacian import MeshCorners  # noqa: E402
from pytorch_points_amd.network import model_loss  # noqa: E402

HBM = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    B, R, S = 32, 128, 16384
    v, f = grid(R, R)
    N, F = v.shape[0], f.shape[0]
    rng = np.random.default_rng(1)
    jitter = (v[None] + 0.2 / (R - 1) * rng.uniform(-1, 1, size=(B, N, 3))).astype(np.float32)
    x = torch.from_numpy(jitter).to(dev).requires_grad_(True)
    faces = torch.from_numpy(f).to(dev)[None].repeat(B, 1, 1)       # B topologies, as a loader would hand them over
    topologies = {"": MeshCorners.from_faces(faces, N), ", shared topology": MeshCorners.from_faces(faces[0], N)}
    u = torch.rand(B, S, 3, device=dev)
    g_p = torch.rand(B, S, 3, device=dev) * 2 - 1
    target = torch.rand(B, S, 3, device=dev) * torch.tensor([1.0, 1.0, 0.01], device=dev)
    out = []

    def line(text):
        print(text, flush=True)
        out.append(text)

    try:
        commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True,
                                text=True).stdout.strip() or "unknown"
    except OSError:
        commit = "unknown"
    line("# tools/mesh_sample_time.py --reps %d, one MI355X; commit %s" % (args.reps, os.environ.get("PP_COMMIT", commit)))
    line("device: %s | torch %s" % (torch.cuda.get_device_name(dev), torch.__version__))
    line("B=%d, %dx%d vertex grid: N=%d F=%d, S=%d samples, fp32; ms as median (best); HIP | the torch composition"
         % (B, R, R, N, F, S))

    def report(label, hip, other, floor=None):
        (hm, hb), (cm, cb) = timed_pair(hip, other, args.reps)
        text = "%-58s %8.3f (%7.3f) | %9.3f (%8.3f)  -> %6.1fx" % (label, hm, hb, cm, cb, cm / hm)
        if floor is not None:
            ms = floor / HBM * 1e3
            text += "; traffic floor %.4f ms (%.1f MB): %.0f%% of it" % (ms, floor / 1e6, 100 * ms / hm)
        line(text)

    for tag, topo in topologies.items():
        bt = topo.batch
        tables = bt * F * 24 + 12 * B * N                              # faces and vertices in
        sample_floor = B * S * (12 + 12 + 8 + 12) + tables + 8 * B * F
        interpolate_floor = B * S * (8 + 12 + 12) + tables
        with torch.no_grad():
            areas = mesh_normals.mesh_face_normals(x, topo)[1]
            if not tag:
                report("CDF build", lambda: mesh_sample._cdf(areas), lambda: torch.cumsum(areas.double(), dim=1))
            kept = mesh_sample.sample_points_from_meshes(x, topo, u=u)
            report("sample_points_from_meshes forward" + tag, lambda: mesh_sample.sample_points_from_meshes(x, topo, u=u),
                   lambda: mesh_sample.sample_composition(x, topo, u=u), sample_floor)
            report("mesh_interpolate forward" + tag, lambda: mesh_sample.mesh_interpolate(x, topo, kept.face, kept.bary),
                   lambda: mesh_sample.sample_composition(x, topo, face=kept.face, bary=kept.bary), interpolate_floor)
        report("sample_points_from_meshes forward + backward" + tag,
               lambda: torch.autograd.grad(mesh_sample.sample_points_from_meshes(x, topo, u=u).points, x, g_p),
               lambda: torch.autograd.grad(mesh_sample.sample_composition(x, topo, u=u)[0], x, g_p))
        report("mesh_interpolate forward + backward" + tag,
               lambda: torch.autograd.grad(mesh_sample.mesh_interpolate(x, topo, kept.face, kept.bary), x, g_p),
               lambda: torch.autograd.grad(mesh_sample.sample_composition(x, topo, face=kept.face, bary=kept.bary)[0],
                                           x, g_p))
        loss = model_loss.SampledMeshChamferLoss(S, consistent_topology=True)
        loss.E = topo

        def composed():
            d1, d2, _, _ = model_loss.nndistance(mesh_sample.sample_composition(x, topo, u=u)[0], target)
            return d1.mean() + d2.mean()

        report("SampledMeshChamferLoss, to the gradient" + tag,
               lambda: torch.autograd.grad(loss(x, None, target, u=u), x), lambda: torch.autograd.grad(composed(), x))
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
