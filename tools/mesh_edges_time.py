"""Times the mesh edge operators at B=32 on a triangulated 128x128 vertex grid (N=16384, F=32258, E=48641 per element,
fp32): the topology build, mesh_edge_sqrlen forward and forward plus backward, and the three mesh losses end to end,
each beside the composition written the reference's way (a Python loop over the batch, torch.unique per element, an
index gather, autograd's index_put backward) on the same device and data in the same run.

    python tools/mesh_edges_time.py [--reps 20] [--out profiles/r11/mesh_edges_time.txt]

Device events after warm-up, the two forms alternating.  The step's traffic floor stands beside the forward: the edge
list read once (16 B per edge), the output written once, the vertices read once, over the 8 TB/s peak of MI355X.
"""
import argparse
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pytorch_points_amd import mesh_edges  # noqa: E402
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


def grid(rows, cols):
    r, c = np.meshgrid(np.arange(rows - 1), np.arange(cols - 1), indexing="ij")
    v00 = (r * cols + c).reshape(-1)
    faces = np.concatenate([np.stack([v00, v00 + 1, v00 + cols], -1), np.stack([v00 + 1, v00 + cols + 1, v00 + cols], -1)])
    y, x = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    verts = np.stack([x / (cols - 1), y / (rows - 1), np.zeros_like(x, float)], -1).reshape(-1, 3)
    return verts.astype(np.float32), faces.astype(np.int64)


# ---- the reference's way, as torch operations on the same device (model_loss.py:166-308, geo_operations.py:562-600)
def ref_edges(faces):
    pairs = torch.stack([faces, faces[:, [1, 2, 0]]], dim=-1)
    return torch.unique(torch.sort(pairs, dim=-1)[0].reshape(-1, 2), dim=0)


def ref_sqrlen(vertices, edges):
    ends = vertices[edges[:, :2]]
    t = ends[:, 0, :] - ends[:, 1, :]
    return torch.sum(t * t, dim=-1)


def ref_edge_length(metric, v1, v2, faces):
    ev = [ref_edges(faces[b]) for b in range(v1.shape[0])]
    return torch.stack([metric(ref_sqrlen(v1[b], ev[b]), ref_sqrlen(v2[b], ev[b])) for b in range(v1.shape[0])]).mean()


def ref_stretch(v1, v2, faces):
    loss = []
    for b in range(v1.shape[0]):
        ev = ref_edges(faces[b])
        sq1, sq2 = ref_sqrlen(v1[b], ev), ref_sqrlen(v2[b], ev)
        loss.append(torch.max(sq2 / sq1 - 1, torch.zeros_like(sq1)).mean())
    return torch.stack(loss).mean()


def ref_repulsion(threshold2, v, edges):
    loss = []
    for b in range(v.shape[0]):
        sq = ref_sqrlen(v[b], edges)
        tmp = 1 / (sq + 1e-6)
        loss.append(torch.where(sq < threshold2, tmp, torch.zeros_like(tmp)).mean())
    return torch.stack(loss).mean()


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
    topo = mesh_edges.MeshEdges.from_faces(faces, N)
    E = topo.counts_host[0]
    shared = mesh_edges.MeshEdges.from_faces(faces[:1].expand(B, -1, -1), N)
    edges = topo.edge_list(0).contiguous()
    ev = [topo.edge_list(b) for b in range(B)]
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
    line("# tools/mesh_edges_time.py --reps %d, one MI355X; commit %s" % (args.reps, os.environ.get("PP_COMMIT", commit)))
    line("device: %s | torch %s" % (torch.cuda.get_device_name(dev), torch.__version__))
    line("B=%d, %dx%d vertex grid: N=%d F=%d E=%d fp32; ms as median (best); HIP | the reference's composition"
         % (B, R, R, N, F, E))
    floor_bytes = B * E * 16 + B * E * 4 + B * N * 12

    def report(label, hip, comp, floor=None):
        (hm, hb), (cm, cb) = timed_pair(hip, comp, args.reps)
        text = "%-46s %8.3f (%7.3f) | %8.3f (%7.3f)  -> %5.1fx" % (label, hm, hb, cm, cb, cm / hm)
        if floor is not None:
            ms = floor / HBM * 1e3
            text += "; traffic floor %.4f ms (%.1f MB): %.0f%% of it" % (ms, floor / 1e6, 100 * ms / hm)
        line(text)

    def ref_all_sqrlen(x):
        return [ref_sqrlen(x[b], ev[b]) for b in range(B)]

    with torch.no_grad():
        report("topology build, B topologies (1 host read | B)", lambda: mesh_edges.MeshEdges.from_faces(faces, N),
               lambda: [ref_edges(faces[b]) for b in range(B)])
        report("topology build, one shared topology", lambda: mesh_edges.MeshEdges.from_faces(faces[:1].expand(B, -1, -1), N),
               lambda: ref_edges(faces[0]))
        report("mesh_edge_sqrlen forward", lambda: mesh_edges.mesh_edge_sqrlen(x1, topo), lambda: ref_all_sqrlen(x1),
               floor_bytes)
        report("mesh_edge_sqrlen forward, shared topology", lambda: mesh_edges.mesh_edge_sqrlen(x1, shared),
               lambda: ref_all_sqrlen(x1), floor_bytes - (B - 1) * E * 16)
    report("mesh_edge_sqrlen forward + backward",
           lambda: torch.autograd.grad(mesh_edges.mesh_edge_sqrlen(x1, topo), x1, w),
           lambda: torch.autograd.grad(ref_all_sqrlen(x1), x1, [w[b, :E] for b in range(B)]))
    l1 = torch.nn.L1Loss()
    kept = model_loss.MeshEdgeLengthLoss(l1, consistent_topology=True)
    kept(x1, x2, faces)
    report("MeshEdgeLengthLoss(L1), kept topology, to grads", lambda: torch.autograd.grad(kept(x1, x2, faces), (x1, x2)),
           lambda: torch.autograd.grad(torch.stack([l1(ref_sqrlen(x1[b], ev[b]), ref_sqrlen(x2[b], ev[b]))
                                                    for b in range(B)]).mean(), (x1, x2)))
    fresh = model_loss.MeshEdgeLengthLoss(l1)
    report("MeshEdgeLengthLoss(L1), topology every call", lambda: torch.autograd.grad(fresh(x1, x2, faces), (x1, x2)),
           lambda: torch.autograd.grad(ref_edge_length(l1, x1, x2, faces), (x1, x2)))
    stretch_kept = model_loss.MeshStretchLoss("mean", consistent_topology=True)
    stretch_kept(x1, x2, faces)
    report("MeshStretchLoss, kept topology, to grads", lambda: torch.autograd.grad(stretch_kept(x1, x2, faces), (x1, x2)),
           lambda: torch.autograd.grad(torch.stack([torch.max(ref_sqrlen(x2[b], ev[b]) / ref_sqrlen(x1[b], ev[b]) - 1,
                                                              torch.zeros_like(w[b, :E])).mean()
                                                    for b in range(B)]).mean(), (x1, x2)))
    stretch = model_loss.MeshStretchLoss("mean")
    report("MeshStretchLoss, topology every call", lambda: torch.autograd.grad(stretch(x1, x2, faces), (x1, x2)),
           lambda: torch.autograd.grad(ref_stretch(x1, x2, faces), (x1, x2)))
    threshold = 1.0 / (R - 1)
    repulsion = model_loss.SimpleMeshRepulsionLoss(threshold, edges)
    report("SimpleMeshRepulsionLoss, to grads", lambda: torch.autograd.grad(repulsion(x1), x1),
           lambda: torch.autograd.grad(ref_repulsion(threshold * threshold, x1, edges), x1))
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
