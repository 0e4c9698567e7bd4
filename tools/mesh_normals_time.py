"""Times the mesh normals at B=32 on a triangulated 128x128 vertex grid (N=16384, F=32258 per element, fp32), with B
separate topologies and with one shared one: mesh_face_normals forward and forward plus backward, mesh_vertex_normals
forward and forward plus backward for both weightings, and MeshNormalLoss to the gradients of both meshes, each beside
the torch composition of the same contract (mesh_normals.face_normals_composition / vertex_normals_composition: gathers,
a cross product, index_add_, autograd's scatter backward) on the same device and data in the same run.

    python tools/mesh_normals_time.py [--reps 20] [--out profiles/mesh_normals/time.txt]

Device events after warm-up, the two forms alternating.  The traffic floor stands beside the forwards: every table and
the vertices read once, the output written once, over the 8 TB/s peak of MI355X.
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
from pytorch_points_amd import mesh_normals  # noqa: E402
from pytorch_points_amd.mesh_laplacian import MeshCorners  # noqa: E402
from pytorch_points_amd.network import model_loss  # noqa: E402

HBM = 8.0e12


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
    topologies = {"": MeshCorners.from_faces(faces, N), ", shared topology": MeshCorners.from_faces(faces[0], N)}
    g_n = torch.rand(B, F, 3, device=dev) * 2 - 1
    g_a = torch.rand(B, F, device=dev) * 2 - 1
    g_v = torch.rand(B, N, 3, device=dev) * 2 - 1
    out = []

    def line(text):
        print(text, flush=True)
        out.append(text)

    try:
        commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True,
                                text=True).stdout.strip() or "unknown"
    except OSError:
        commit = "unknown"
    line("# tools/mesh_normals_time.py --reps %d, one MI355X; commit %s" % (args.reps, os.environ.get("PP_COMMIT", commit)))
    line("device: %s | torch %s" % (torch.cuda.get_device_name(dev), torch.__version__))
    line("B=%d, %dx%d vertex grid: N=%d F=%d fp32; ms as median (best); HIP | the torch composition" % (B, R, R, N, F))

    def report(label, hip, other, floor=None):
        (hm, hb), (cm, cb) = timed_pair(hip, other, args.reps)
        text = "%-58s %8.3f (%7.3f) | %9.3f (%8.3f)  -> %6.1fx" % (label, hm, hb, cm, cb, cm / hm)
        if floor is not None:
            ms = floor / HBM * 1e3
            text += "; traffic floor %.4f ms (%.1f MB): %.0f%% of it" % (ms, floor / 1e6, 100 * ms / hm)
        line(text)

    for tag, topo in topologies.items():
        bt = topo.batch
        face_floor = B * F * 16 + bt * F * 24 + 12 * B * N             # normals and areas out, faces and vertices in
        vertex_floor = B * N * 24 + bt * N * 4 + bt * F * 24           # vertices in and out, start and nbr in
        with torch.no_grad():
            report("mesh_face_normals forward" + tag, lambda: mesh_normals.mesh_face_normals(x1, topo),
                   lambda: mesh_normals.face_normals_composition(x1, topo), face_floor)
        report("mesh_face_normals forward + backward" + tag,
               lambda: torch.autograd.grad(mesh_normals.mesh_face_normals(x1, topo), x1, (g_n, g_a)),
               lambda: torch.autograd.grad(mesh_normals.face_normals_composition(x1, topo), x1, (g_n, g_a)))
        for w in ("area", "uniform"):
            with torch.no_grad():
                report("mesh_vertex_normals %s forward%s" % (w, tag),
                       lambda: mesh_normals.mesh_vertex_normals(x1, topo, w),
                       lambda: mesh_normals.vertex_normals_composition(x1, topo, w), vertex_floor)
            report("mesh_vertex_normals %s forward + backward%s" % (w, tag),
                   lambda: torch.autograd.grad(mesh_normals.mesh_vertex_normals(x1, topo, w), x1, g_v),
                   lambda: torch.autograd.grad(mesh_normals.vertex_normals_composition(x1, topo, w), x1, g_v))
        kept = model_loss.MeshNormalLoss(torch.nn.MSELoss(), consistent_topology=True)
        kept.E = topo
        metric = torch.nn.MSELoss()
        report("MeshNormalLoss (vertex, area), to grads" + tag, lambda: torch.autograd.grad(kept(x1, x2), (x1, x2)),
               lambda: torch.autograd.grad(metric(mesh_normals.vertex_normals_composition(x1, topo),
                                                  mesh_normals.vertex_normals_composition(x2, topo)), (x1, x2)))
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
