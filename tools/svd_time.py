"""Times the batched SVD (pp_batch_svd_f32) at the shapes that matter, next to torch.linalg.svd on the same device and
data and the HBM / VALU floors, and batch_normals end to end split into its phases.

    python tools/svd_time.py [--reps 20] [--out FILE]

Device events after warm-up, seeded data.  Floors: HBM = bytes the call must move (input read, outputs written) at
6.29 TB/s (the measured float4-copy rate, MI355X_MICROARCH); VALU = the lane operations of the sweeps the kernel
reported (mean info) at the fp32 vector peak, 157.3e12 FLOP/s = 78.6e12 lane operations/s counting an FMA as one.
"""
import argparse
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from pytorch_points_amd import ops  # noqa: E402
from pytorch_points_amd._ext import linalg  # noqa: E402
from pytorch_points_amd.network.operations import batch_svd  # noqa: E402

HBM = 6.29e12
VALU_OPS = 157.3e12 / 2


def timed(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times)), float(np.min(times))


def svd_ops(m, n, sweeps):
    """lane operations of `sweeps` sweeps: per pair 3 dot products of R (FMA), 2R rotated W entries and 2K rotated Z
    entries at 3 operations each (two multiplies, one add), the rotation's ~12; plus the scan, norms and outputs"""
    r, k = max(m, n), min(m, n)
    pairs = k * (k - 1) / 2
    return sweeps * pairs * (3 * r + 6 * r + 6 * k + 12) + 4 * r * k


def line(out, text):
    print(text)
    out.append(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    out = []
    line(out, "device: %s | torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    gen = torch.Generator(device=dev).manual_seed(0)
    for b, m, n, full in [(524288, 20, 3, False), (65536, 32, 32, True), (1048576, 3, 3, False)]:
        a = torch.randn(b, m, n, generator=gen, device=dev)
        k = min(m, n)
        ucols, vcols = (m, n) if full else (k, k)
        nbytes = 4 * b * (m * n + m * ucols + k + n * vcols)
        _, _, _, info = linalg.batch_svd_forward(a, True, 1e-7, 100, return_info=True, full=full)
        infos = info.cpu().numpy()
        sweeps = float(infos[infos > 0].mean())
        med, best = timed(lambda: linalg.batch_svd_forward(a, True, 1e-7, 100, full=full), args.reps)
        hbm_ms = nbytes / HBM * 1e3
        valu_ms = b * svd_ops(m, n, sweeps) / VALU_OPS * 1e3
        line(out, "(%d, %d, %d) %s: %.3f ms median, %.3f best | sweeps mean %.2f max %d, not converged %d | "
             "HBM floor %.3f ms (%.1f MB), VALU floor %.3f ms -> %s-bound floor; %.1f%% of it"
             % (b, m, n, "full" if full else "thin", med, best, sweeps, infos.max(), int((infos == -1).sum()),
                hbm_ms, nbytes / 1e6, valu_ms, "HBM" if hbm_ms >= valu_ms else "VALU",
                100 * max(hbm_ms, valu_ms) / med))
        try:   # (torch's batched SVD is timed on a slice first: where the whole batch would take over 10 s, only the
            #        slice is timed and the whole is projected from it, and the line says so)
            sub = a[:8192]
            t0 = time.time()
            torch.linalg.svd(sub, full_matrices=full)
            torch.cuda.synchronize()
            projected = (time.time() - t0) * b / sub.shape[0]
            if projected <= 10:
                tmed, tbest = timed(lambda: torch.linalg.svd(a, full_matrices=full), 3, warmup=1)
                line(out, "    torch.linalg.svd same device and data: %.3f ms median, %.3f best (3 reps) -> %.1fx the kernel"
                     % (tmed, tbest, tmed / med))
            else:
                smed, _ = timed(lambda: torch.linalg.svd(sub, full_matrices=full), 3, warmup=1)
                line(out, "    torch.linalg.svd same device and data: first %d matrices %.3f ms median (3 reps); whole batch "
                     "not run, projected %.0f ms -> ~%.0fx the kernel" % (sub.shape[0], smed, smed * b / sub.shape[0],
                                                                       smed * b / sub.shape[0] / med))
        except Exception as exc:   # record, do not hide: the comparison is part of the record
            line(out, "    torch.linalg.svd failed: %s: %s" % (type(exc).__name__, str(exc).splitlines()[0][:200]))
        del a
        torch.cuda.empty_cache()

    # batch_normals, B=32, N=16384, nn=20, end to end and by phase (the phases as batch_normals runs them)
    B, N, K = 32, 16384, 20
    p = torch.randn(B, N, 3, generator=gen, device=dev)
    p = p / p.norm(dim=2, keepdim=True)

    def phase_knn():
        return ops.knn_points(p, p, K=K, return_nn=True)

    knn = phase_knn()

    def phase_centre():
        g = knn.knn
        return (g - g.mean(dim=2, keepdim=True)).reshape(-1, K, 3)

    centred = phase_centre()

    def phase_svd():
        return batch_svd(centred)

    def end_to_end():
        from pytorch_points_amd.network.geo_operations import batch_normals
        return batch_normals(p, nn_size=K, NCHW=False)

    t_knn = timed(phase_knn, args.reps)[0]
    t_cen = timed(phase_centre, args.reps)[0]
    t_svd = timed(phase_svd, args.reps)[0]
    t_all = timed(end_to_end, args.reps)[0]
    line(out, "batch_normals B=%d N=%d nn=%d (unit sphere): %.3f ms end to end | knn_points with return_nn (search + "
         "gather) %.3f ms, centring %.3f ms, batch_svd (thin, autograd node) %.3f ms" % (B, N, K, t_all, t_knn, t_cen, t_svd))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
