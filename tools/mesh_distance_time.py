"""Times the point-to-mesh distances (fp32) on three tables:

    grid          B=8, P=16384 points against a triangulated 128x128 vertex grid (N=16384, F=32258), B topologies
    grid-shared   the same with one shared topology
    cage          B=32, P=16384 points against a 162-vertex / 320-face cage, the shape the cage operators are timed at

each forward, each forward plus backward and PointMeshDistanceLoss to both gradients, each beside the torch
composition of the same contract (mesh_distance.distance_composition) on the same device and data in the same run,
and SampledMeshChamferLoss at S=16384 on the same mesh and cloud for scale.

    python tools/mesh_distance_time.py [--reps 20] [--table grid] [--out profiles/mesh_distance/time.txt]

Device events after warm-up, the two forms alternating, median of --reps.  Every line is appended to --out as soon as
it is measured, so a run that is cut short leaves what it had; a table is one process (run the tool once per table).
The floor beside the forwards is the pair function's operation count taken from csrc/mesh_distance.hip (pd_pair and the
choice: 129 separately rounded fp32 operations, compares and selects per pair, the division counted as one) times the
pairs, at the fp32 non-packed issue rate of MI355X: its 157.3 TFLOPS peak counts packed fused multiply-adds, four
flops per lane and cycle, so plain operations issue at a quarter of it, 39.3e12 per second.  The composition evaluates
its pair matrix in blocks of 2^26 pairs here (mesh_distance.CHUNK_PAIRS), which the device's memory allows and which
favours it.
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
from pytorch_points_amd import mesh_distance, mesh_sample, synthetic  # noqa: E402
from pytorch_points_amd.mesh_laplacian import MeshCorners  # noqa: E402
from pytorch_points_amd.network import model_loss  # noqa: E402

OPS_PER_PAIR = 129
ISSUE_RATE = 157.3e12 / 4
TABLES = ("grid", "grid-shared", "cage")


def icosphere(level):
    """(vertices (N,3), faces (F,3)) of an icosahedron subdivided ``level`` times: 162 / 320 at level 2"""
    t = (1 + 5 ** 0.5) / 2
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t),
         (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6),
         (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7),
         (9, 8, 1)]
    v = [np.array(p, float) / np.linalg.norm(p) for p in v]
    for _ in range(level):
        mid, out = {}, []

        def middle(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                m = v[a] + v[b]
                v.append(m / np.linalg.norm(m))
                mid[key] = len(v) - 1
            return mid[key]

        for a, b, c in f:
            ab, bc, ca = middle(a, b), middle(b, c), middle(c, a)
            out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = out
    return np.array(v, np.float32), np.array(f, np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--table", choices=TABLES, default="grid")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    mesh_distance.CHUNK_PAIRS = 1 << 26
    rng = np.random.default_rng(1)
    P = S = 16384
    if args.table == "cage":
        B = 32
        v, f = icosphere(2)
        what = "a %d-vertex / %d-face cage" % (v.shape[0], f.shape[0])
        cloud = 1.1 * synthetic.unit_sphere(3, B, P)
    else:
        B = 8
        v, f = grid(128, 128)
        what = "a 128x128 vertex grid: N=%d F=%d" % (v.shape[0], f.shape[0])
        cloud = rng.uniform(0, 1, size=(B, P, 3)) * np.array([1.0, 1.0, 0.02]) - np.array([0.0, 0.0, 0.01])
    N, F = v.shape[0], f.shape[0]
    jitter = (v[None] + 0.2 / 127 * rng.uniform(-1, 1, size=(B, N, 3))).astype(np.float32)
    x = torch.from_numpy(jitter).to(dev).requires_grad_(True)
    pts = torch.from_numpy(np.ascontiguousarray(cloud, dtype=np.float32)).to(dev).requires_grad_(True)
    faces = torch.from_numpy(f).to(dev)
    shared = args.table != "grid"
    topo = MeshCorners.from_faces(faces if shared else faces[None].repeat(B, 1, 1), N)
    g1 = torch.rand(B, P, device=dev) * 2 - 1
    g2 = torch.rand(B, F, device=dev) * 2 - 1
    u = torch.rand(B, S, 3, device=dev)

    def line(text):
        print(text, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(args.out), exist_ok=True)
            with open(args.out, "a") as fh:
                fh.write(text + "\n")

    try:
        commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True,
                                text=True).stdout.strip() or "unknown"
    except OSError:
        commit = "unknown"
    line("# tools/mesh_distance_time.py --table %s --reps %d, one MI355X; commit %s"
         % (args.table, args.reps, os.environ.get("PP_COMMIT", commit)))
    line("device: %s | torch %s" % (torch.cuda.get_device_name(dev), torch.__version__))
    line("B=%d, P=%d points against %s, %s, fp32; ms as median (best); HIP | the torch composition"
         % (B, P, what, "one shared topology" if shared else "B topologies"))
    pairs = B * P * F
    floor = pairs * OPS_PER_PAIR / ISSUE_RATE * 1e3
    line("%.3g pairs of %d operations at %.3g operations/s: issue floor %.3f ms" % (pairs, OPS_PER_PAIR, ISSUE_RATE, floor))

    def report(label, hip, other, with_floor=False):
        (hm, hb), (cm, cb) = timed_pair(hip, other, args.reps, warmup=2)
        text = "%-48s %9.3f (%8.3f) | %10.3f (%9.3f)  -> %7.1fx" % (label, hm, hb, cm, cb, cm / hm)
        if with_floor:
            text += "; issue floor %.3f ms: %.0f%% of it" % (floor, 100 * floor / hm)
        line(text)

    compose = mesh_distance.distance_composition
    with torch.no_grad():
        hip, ref = mesh_distance.point_face_distance(pts, x, topo), compose(pts, x, topo, face_point=False)[0]
        line("point -> face: HIP and the composition on this device agree on %d of %d faces and to %.3g in dist"
             % (int((hip.face == ref.face).sum()), B * P, float((hip.dist - ref.dist).abs().max())))
        report("point_face_distance forward", lambda: mesh_distance.point_face_distance(pts, x, topo),
               lambda: compose(pts, x, topo, face_point=False), True)
        report("face_point_distance forward", lambda: mesh_distance.face_point_distance(pts, x, topo),
               lambda: compose(pts, x, topo, point_face=False), True)
    report("point_face_distance forward + backward",
           lambda: torch.autograd.grad(mesh_distance.point_face_distance(pts, x, topo).dist, (pts, x), g1),
           lambda: torch.autograd.grad(compose(pts, x, topo, face_point=False)[0].dist, (pts, x), g1))
    report("face_point_distance forward + backward",
           lambda: torch.autograd.grad(mesh_distance.face_point_distance(pts, x, topo).dist, (pts, x), g2),
           lambda: torch.autograd.grad(compose(pts, x, topo, point_face=False)[1].dist, (pts, x), g2))
    loss = model_loss.PointMeshDistanceLoss(consistent_topology=True)
    loss.E = topo

    def composed_loss():
        pf, fp = compose(pts, x, topo)
        return pf.dist.mean() + fp.dist.mean()

    report("PointMeshDistanceLoss, to both gradients", lambda: torch.autograd.grad(loss(pts, x), (pts, x)),
           lambda: torch.autograd.grad(composed_loss(), (pts, x)))
    sampled = model_loss.SampledMeshChamferLoss(S, consistent_topology=True)
    sampled.E = topo

    def sampled_composed():
        d1, d2, _, _ = model_loss.nndistance(mesh_sample.sample_composition(x, topo, u=u)[0], pts.detach())
        return d1.mean() + d2.mean()

    report("SampledMeshChamferLoss S=%d, to the vertices" % S,
           lambda: torch.autograd.grad(sampled(x, None, pts.detach(), u=u), x),
           lambda: torch.autograd.grad(sampled_composed(), x))


if __name__ == "__main__":
    main()
