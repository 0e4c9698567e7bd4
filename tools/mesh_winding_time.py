"""Times the mesh winding number and the signed point-to-mesh distance (fp32) on two tables:

    grid    B=8, P=16384 points against a triangulated 128x128 vertex grid (N=16384, F=32258), B topologies
    cage    B=32, P=16384 points against a 162-vertex / 320-face cage, the shape the cage operators are timed at

the winding number alone, the fused signed distance forward and forward plus backward, and MeshEnclosureLoss to both
gradients, each beside the torch composition of the same contract (mesh_winding.winding_composition and
signed_distance_composition) on the same device and data in the same run; and the fused signed distance beside the
unfused way, point_face_distance followed by the winding-alone walk, HIP on both sides.

    python tools/mesh_winding_time.py [--reps 20] [--table grid] [--out profiles/mesh_winding/time.txt]

Device events after warm-up, the two forms alternating, median of --reps.  Every line is appended to --out as soon as
it is measured, so a run that is cut short leaves what it had; a table is one process (run the tool once per table).
The floor beside the forwards is the pair's operation count taken from csrc/mesh_winding.hip times the pairs, at the
fp32 non-packed issue rate of MI355X (39.3e12 per second: tools/mesh_distance_time.py says why).  mw_half_angle is 67
separately rounded operations: 9 subtractions, three lengths of 5 + 1, the cross product's 9, the determinant's 5, the
denominator's three dot products and 8 more, atan2f, the conversion to fp64 and the fp64 addition; atan2f and each of
the three square roots are counted as ONE operation, as the division of pd_pair is, although the device's atan2f alone
is some forty instructions, so the floor of the winding number is a loose one.  The fused walk adds pd_pair's 129.  The
compositions evaluate their pair matrices in blocks of 2^26 pairs here (CHUNK_PAIRS), which the device's memory allows
and which favours them.
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
from mesh_distance_time import icosphere  # noqa: E402
from mesh_edges_time import grid, timed_pair  # noqa: E402
from pytorch_points_amd import mesh_distance, mesh_winding, synthetic  # noqa: E402
from pytorch_points_amd.mesh_laplacian import MeshCorners  # noqa: E402
from pytorch_points_amd.network import model_loss  # noqa: E402

OPS_WINDING = 67
OPS_DISTANCE = 129
ISSUE_RATE = 157.3e12 / 4
TABLES = ("grid", "cage")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--table", choices=TABLES, default="grid")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    mesh_distance.CHUNK_PAIRS = mesh_winding.CHUNK_PAIRS = 1 << 26
    rng = np.random.default_rng(1)
    P = 16384
    if args.table == "cage":
        B = 32
        v, f = icosphere(2)
        what = "a %d-vertex / %d-face cage" % (v.shape[0], f.shape[0])
        cloud = 1.1 * synthetic.unit_sphere(3, B, P) * rng.uniform(0.2, 1.0, size=(B, P, 1))   # inside and outside
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
    g = torch.rand(B, P, device=dev) * 2 - 1

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
    line("# tools/mesh_winding_time.py --table %s --reps %d, one MI355X; commit %s"
         % (args.table, args.reps, os.environ.get("PP_COMMIT", commit)))
    line("device: %s | torch %s" % (torch.cuda.get_device_name(dev), torch.__version__))
    line("B=%d, P=%d points against %s, %s, fp32; ms as median (best); HIP | the torch composition"
         % (B, P, what, "one shared topology" if shared else "B topologies"))
    pairs = B * P * F
    floors = {ops: pairs * ops / ISSUE_RATE * 1e3 for ops in (OPS_WINDING, OPS_WINDING + OPS_DISTANCE)}
    line("%.3g pairs at %.3g operations/s: issue floor %.3f ms for the winding number's %d operations, %.3f ms for the "
         "fused walk's %d" % (pairs, ISSUE_RATE, floors[OPS_WINDING], OPS_WINDING,
                              floors[OPS_WINDING + OPS_DISTANCE], OPS_WINDING + OPS_DISTANCE))

    def report(label, hip, other, ops=None, versus="x"):
        (hm, hb), (cm, cb) = timed_pair(hip, other, args.reps, warmup=2)
        text = "%-48s %9.3f (%8.3f) | %10.3f (%9.3f)  -> %7.2f%s" % (label, hm, hb, cm, cb, cm / hm, versus)
        if ops:
            text += "; issue floor %.3f ms: %.0f%% of it" % (floors[ops], 100 * floors[ops] / hm)
        line(text)

    signed, compose = mesh_winding.point_mesh_signed_distance, mesh_winding.signed_distance_composition
    with torch.no_grad():
        hip, ref = signed(pts, x, topo), compose(pts, x, topo)
        line("HIP and the composition on this device agree on %d of %d faces and %d of %d sides, to %.3g in winding"
             % (int((hip.face == ref.face).sum()), B * P, int(((hip.winding > 0.5) == (ref.winding > 0.5)).sum()), B * P,
                float((hip.winding - ref.winding).abs().max())))
        report("mesh_winding_number", lambda: mesh_winding.mesh_winding_number(pts, x, topo),
               lambda: mesh_winding.winding_composition(pts, x, topo), OPS_WINDING)
        report("point_mesh_signed_distance forward (fused)", lambda: signed(pts, x, topo),
               lambda: compose(pts, x, topo), OPS_WINDING + OPS_DISTANCE)

        def unfused():
            return mesh_distance.point_face_distance(pts, x, topo), mesh_winding.mesh_winding_number(pts, x, topo)

        line("the fused walk | point_face_distance, then the winding-alone walk (both HIP, two launches | four)")
        report("fused | unfused, forward", lambda: signed(pts, x, topo), unfused, versus="x the fused time")
    report("point_mesh_signed_distance forward + backward",
           lambda: torch.autograd.grad(signed(pts, x, topo).signed, (pts, x), g),
           lambda: torch.autograd.grad(compose(pts, x, topo).signed, (pts, x), g))
    for side in ("inside", "outside"):
        loss = model_loss.MeshEnclosureLoss(side, consistent_topology=True)
        loss.E = topo

        def composed_loss():
            s = compose(pts, x, topo).signed
            return (torch.relu(s if side == "inside" else -s) ** 2).mean()

        report("MeshEnclosureLoss(%s), to both gradients" % side, lambda: torch.autograd.grad(loss(pts, x), (pts, x)),
               lambda: torch.autograd.grad(composed_loss(), (pts, x)))


if __name__ == "__main__":
    main()
