"""Times the earth mover's distance (fp32) at two shapes:

    2048   B=32, N=M=2048
    4096   B=8,  N=M=4096

approx_match, match_cost forward, forward + backward, EarthMoverLoss to both gradients and EmdMatch.dense(), each
beside the torch composition of the same contract (emd.emd_composition's parts) on the same device and data in the same
run.

    python tools/emd_time.py [--reps 20] [--table 2048] [--out profiles/emd/time.txt] [--exp-probe tools/exp_rate_probe]

Device events after warm-up, the two forms alternating, median of --reps.  Every line is appended to --out as soon as
it is measured; a table is one process.  The composition evaluates its pair matrix in blocks of 2^26 pairs here
(emd.CHUNK_PAIRS), which the device's memory allows and which favours it.

The issue floor beside a row counts, from csrc/emd.hip, the separately rounded fp32 operations and the exps of a pair:

    a sweep with one sum     8 (d) + 3 (scale, weight, add)        = 11 operations and 1 exp
    the fused row sweep      8 + 2 * 3                              = 14 operations and 2 exps
    a match                  1 + 10 single sweeps and 9 fused ones  = 247 operations and 29 exps
    the cost                 8 + 10 * 4 (match) + sqrt, mul, add    = 51 operations and 10 exps
    a gradient               8 + 40 + sqrt, max, div, 3 mul, 3 add  = 57 operations and 10 exps
    dense                    8 + 40                                 = 48 operations and 10 exps

times the pairs, at the fp32 non-packed issue rate of MI355X (its 157.3 TFLOPS peak counts packed fused multiply-adds,
four flops per lane and cycle, so plain operations issue at 39.3e12 per second), an exp counted as the number of
plain operations whose issue time it takes.  That number is measured here: --exp-probe is tools/exp_rate_probe.hip
built with hipcc, run once before the table, and the ratio at 4 waves per SIMD is taken.  The sqrt and the division
are counted as one operation each although they expand to several, so the floors of the cost and the gradients are
low.
"""
import argparse
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from mesh_edges_time import timed_pair  # noqa: E402
from pytorch_points_amd import emd  # noqa: E402
from pytorch_points_amd.network import model_loss  # noqa: E402

ISSUE_RATE = 157.3e12 / 4
COUNTS = {"match": (247, 29), "cost": (51, 10), "grad": (57, 10), "dense": (48, 10)}   # (operations, exps) per pair
TABLES = {"2048": (32, 2048), "4096": (8, 4096)}


def exp_slots(probe):
    """plain-operation issue slots of one v_exp_f32, from the probe's last line (the ratio at 4 waves per SIMD)"""
    if not os.path.exists(probe):
        raise SystemExit("%s is not built: hipcc --offload-arch=gfx950 -O3 tools/exp_rate_probe.hip -o %s" % (probe, probe))
    out = subprocess.run([probe], capture_output=True, text=True, check=True, timeout=120).stdout
    last = out.strip().splitlines()[-1]
    return float(last.split(":")[1].split()[2]), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--table", choices=sorted(TABLES), default="2048")
    ap.add_argument("--out", default=None)
    ap.add_argument("--exp-probe", default=os.path.join(ROOT, "tools", "exp_rate_probe"))
    args = ap.parse_args()
    slots, probe_text = exp_slots(args.exp_probe)   # (a child process of its own, before this one opens the GPU)
    dev = torch.device("cuda:0")
    emd.CHUNK_PAIRS = 1 << 26
    B, N = TABLES[args.table]
    M = N
    gen = torch.Generator(device="cpu").manual_seed(1)
    x1 = torch.rand(B, N, 3, generator=gen).to(dev).requires_grad_(True)
    x2 = torch.rand(B, M, 3, generator=gen).to(dev).requires_grad_(True)

    def line(text):
        print(text, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(args.out), exist_ok=True)
            with open(args.out, "a") as fh:
                fh.write(text + "\n")

    line("# tools/emd_time.py --table %s --reps %d, one MI355X" % (args.table, args.reps))
    line("device: %s | torch %s" % (torch.cuda.get_device_name(dev), torch.__version__))
    for text in probe_text.strip().splitlines():
        line("exp probe: " + text)
    pairs = B * N * M
    line("B=%d, N=M=%d uniform in the unit cube, fp32: %.3g pairs; ms as median (best); HIP | the torch composition, "
         "same B" % (B, N, pairs))
    line("the dense match would take %.1f MB, the factors take %.2f MB"
         % (4.0 * B * N * M / 2 ** 20, 40.0 * B * (N + M) / 2 ** 20))

    def floor(*kinds):
        return sum(pairs * (COUNTS[k][0] + slots * COUNTS[k][1]) for k in kinds) / ISSUE_RATE * 1e3

    def report(label, hip, other, fl):
        (hm, hb), (cm, cb) = timed_pair(hip, other, args.reps, warmup=2)
        line("%-40s %9.3f (%8.3f) | %10.3f (%9.3f)  -> %7.1fx; issue floor %.3f ms: %.0f%% of it"
             % (label, hm, hb, cm, cb, cm / hm, fl, 100 * fl / hm))

    def composed_match():
        with torch.no_grad():
            return emd.EmdMatch(x1.detach(), x2.detach(), *emd.factors_composition(x1.detach(), x2.detach()), hip=False)

    with torch.no_grad():
        hip, ref = emd.approx_match(x1, x2), composed_match()
        line("HIP and the composition on this device: cost differs by %.3g of %.3g at most"
             % (float((emd.match_cost(x1, x2, hip) - emd.match_cost(x1, x2, ref)).abs().max()),
                float(emd.match_cost(x1, x2, ref).abs().max())))
        report("approx_match", lambda: emd.approx_match(x1, x2), composed_match, floor("match"))
        report("match_cost forward", lambda: emd.match_cost(x1, x2, hip), lambda: emd.match_cost(x1, x2, ref),
               floor("cost"))
    report("match_cost forward + backward",
           lambda: torch.autograd.grad(emd.match_cost(x1, x2, hip).sum(), (x1, x2)),
           lambda: torch.autograd.grad(emd.match_cost(x1, x2, ref).sum(), (x1, x2)), floor("cost", "grad", "grad"))
    loss = model_loss.EarthMoverLoss()
    report("EarthMoverLoss, to both gradients", lambda: torch.autograd.grad(loss(x1, x2), (x1, x2)),
           lambda: torch.autograd.grad((emd.emd_composition(x1, x2)[1] / N).mean(), (x1, x2)),
           floor("match", "cost", "grad", "grad"))
    with torch.no_grad():
        report("EmdMatch.dense()", hip.dense, ref.dense, floor("dense"))


if __name__ == "__main__":
    main()
