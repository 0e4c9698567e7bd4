"""Times the mesh dihedral angles at B=32 on a triangulated 128x128 vertex grid (N=16384, F=32258, E=48641 per element,
fp32): the topology build, mesh_dihedral_angle forward and forward plus backward, and MeshDihedralAngleLoss to the
gradients with a kept and with a rebuilt topology, each beside the torch composition of the same contract
(mesh_dihedral.dihedral_composition: gathers, cross, normalize, acos, autograd's scatter backward) on the same device
and data in the same run.  The composition's table comes from edge_points_composition, a CPU build, and is uploaded.

    python tools/mesh_dihedral_time.py [--reps 20] [--out profiles/r16/mesh_dihedral_time.txt]

Device events after warm-up, the two forms alternating.  The step's traffic floor stands beside the forward: the table
read once (32 B per edge), the output written once, the vertices read once, over the 8 TB/s peak of MI355X.
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
from pytorch_points_amd import mesh_dihedral  # noqa: E402
from pytorch_points_amd.network import model_loss  # noqa: E402

HBM = 8.0e12


def composition_topology(faces, n):
    """the table built on the CPU, element by element, and uploaded"""
    host = faces.cpu()
    tables = [mesh_dihedral.edge_points_composition(host[b]) for b in range(host.shape[0])]
    return mesh_dihedral.MeshEdgePoints._unchecked(torch.stack(tables).to(faces.device), n)


def composition_loss(x1, x2, topo):
    diff = mesh_dihedral.dihedral_composition(x1, topo) - mesh_dihedral.dihedral_composition(x2, topo)
    return model_loss._reduce_edges(diff * diff, topo, "mean")


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
    faces = torch.from_numpy(f).to(dev)[None].repeat(B, 1, 1)       # B topologies, as a loader would hand them over
    topo = mesh_dihedral.MeshEdgePoints.from_faces(faces, N)
    E = topo.counts_host[0]
    shared = mesh_dihedral.MeshEdgePoints.from_faces(faces[:1].expand(B, -1, -1), N)
    comp = composition_topology(faces, N)                            # (B,E,4): no padding rows to compute
    w = torch.rand(B, topo.capacity, device=dev) * 2 - 1
    out = []

    def line(text):
        print(text, flush=True)
        out.append(text)

    try:
        commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True,
                                text=True).stdout.strip() or "unknown"
    except OSError:
        commit = "unknown"
    line("# tools/mesh_dihedral_time.py --reps %d, one MI355X; commit %s" % (args.reps, os.environ.get("PP_COMMIT", commit)))
    line("device: %s | torch %s" % (torch.cuda.get_device_name(dev), torch.__version__))
    line("B=%d, %dx%d vertex grid: N=%d F=%d E=%d fp32; ms as median (best); HIP | the torch composition"
         % (B, R, R, N, F, E))
    floor_bytes = B * E * 32 + B * E * 4 + B * N * 12

    def report(label, hip, other, floor=None):
        (hm, hb), (cm, cb) = timed_pair(hip, other, args.reps)
        text = "%-50s %8.3f (%7.3f) | %9.3f (%8.3f)  -> %6.1fx" % (label, hm, hb, cm, cb, cm / hm)
        if floor is not None:
            ms = floor / HBM * 1e3
            text += "; traffic floor %.4f ms (%.1f MB): %.0f%% of it" % (ms, floor / 1e6, 100 * ms / hm)
        line(text)

    with torch.no_grad():
        report("topology build, B topologies (1 host read | CPU)", lambda: mesh_dihedral.MeshEdgePoints.from_faces(faces, N),
               lambda: composition_topology(faces, N))
        report("topology build, one shared topology",
               lambda: mesh_dihedral.MeshEdgePoints.from_faces(faces[:1].expand(B, -1, -1), N),
               lambda: composition_topology(faces[:1], N))
        report("mesh_dihedral_angle forward", lambda: mesh_dihedral.mesh_dihedral_angle(x1, topo),
               lambda: mesh_dihedral.dihedral_composition(x1, comp), floor_bytes)
        report("mesh_dihedral_angle forward, shared topology", lambda: mesh_dihedral.mesh_dihedral_angle(x1, shared),
               lambda: mesh_dihedral.dihedral_composition(x1, comp), floor_bytes - (B - 1) * E * 32)
    report("mesh_dihedral_angle forward + backward",
           lambda: torch.autograd.grad(mesh_dihedral.mesh_dihedral_angle(x1, topo), x1, w),
           lambda: torch.autograd.grad(mesh_dihedral.dihedral_composition(x1, comp), x1, w[:, :E]))
    kept = model_loss.MeshDihedralAngleLoss(consistent_topology=True)
    kept(x1, x2, faces)
    report("MeshDihedralAngleLoss, kept topology, to grads", lambda: torch.autograd.grad(kept(x1, x2), (x1, x2)),
           lambda: torch.autograd.grad(composition_loss(x1, x2, comp), (x1, x2)))
    fresh = model_loss.MeshDihedralAngleLoss()
    report("MeshDihedralAngleLoss, topology every call", lambda: torch.autograd.grad(fresh(x1, x2, faces), (x1, x2)),
           lambda: torch.autograd.grad(composition_loss(x1, x2, composition_topology(faces, N)), (x1, x2)))
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
