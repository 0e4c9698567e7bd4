"""Times mean_value_coordinates_3D at the Neural-Cages size (B=8, P=16384, icosphere cage 162 V / 320 F, fp32): the
HIP forward, forward plus backward, and the in-tree torch composition on the same device and data; and a VALU floor.

    python tools/mvc_time.py [--reps 10] [--out profiles/r8/mvc_time.txt]

Device events after warm-up, seeded data.  VALU floor: the vector instructions of the forward kernel's face loop
(counted in the gfx950 assembly of csrc/mvc.hip, built here with --save-temps; libm calls are inlined there) per
(query, face) pair, times B*P*F pairs, at the vector issue rate of 256 CUs x 4 SIMDs x 16 lanes x 2.4 GHz = 39.3e12
lane instructions/s.  Straight-line count of the loop body, both branch sides included, at the fp32 rate (the pair is
evaluated in fp64, whose instructions issue more slowly): an estimate, not a bound.
"""
import argparse
import glob
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pytorch_points_amd import _build, mvc  # noqa: E402

ISSUE = 256 * 4 * 16 * 2.4e9


def timed(fn, reps, warmup=2):
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


def loop_valu_count():
    """vector instructions between the face loop's head label and its back edge in mvc_forward_kernel<float, true>"""
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), *[f for f in _build.HIPCC_FLAGS if f != "-shared"],
               "-I" + _build.INCLUDE, "-I" + _build.CSRC, "--save-temps", "-c",
               os.path.join(_build.CSRC, "mvc.hip"), "-o", os.path.join(tmp, "mvc.o")]
        subprocess.run(cmd, cwd=tmp, check=True, capture_output=True)
        asm = open(glob.glob(os.path.join(tmp, "*gfx950*.s"))[0]).read()
    name = re.search(r"^(_ZN\S*mvc_forward_kernelIfLb1E\S*):", asm, re.M).group(1)
    body = asm[asm.index(name + ":"):]
    body = body[:body.index("s_endpgm")]
    lines = body.splitlines()
    labels = {m.group(1): i for i, m in enumerate(re.match(r"^(\.LBB\w+):", ln) for ln in lines) if m}
    best = None
    for i, ln in enumerate(lines):                  # the longest backward branch is the face loop
        m = re.match(r"\s+s_cbranch_\w+\s+(\.LBB\w+)|\s+s_branch\s+(\.LBB\w+)", ln)
        if m:
            tgt = m.group(1) or m.group(2)
            if tgt in labels and labels[tgt] < i and (best is None or i - labels[tgt] > best[1] - best[0]):
                best = (labels[tgt], i)
    seg = lines[best[0]:best[1] + 1]
    return sum(1 for ln in seg if re.match(r"\s+v_", ln)), sum(1 for ln in seg if re.match(r"\s+(v_|s_|ds_|global_)", ln))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import importlib.util
    spec = importlib.util.spec_from_file_location("gen", os.path.join(ROOT, "tools", "gen_mvc_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    dev = torch.device("cuda:0")
    B, P = 8, 16384
    v0, f0 = gen.icosphere(2)
    N, F = len(v0), len(f0)
    rng = np.random.default_rng(0)
    dirs = rng.normal(size=(B, P, 3))
    dirs /= np.linalg.norm(dirs, axis=-1, keepdims=True)
    q = torch.from_numpy((dirs * rng.uniform(0.05, 0.9, (B, P, 1))).astype(np.float32)).to(dev).requires_grad_(True)
    v = torch.from_numpy(np.stack([v0 * rng.uniform(0.9, 1.1, 3) for _ in range(B)]).astype(np.float32)).to(dev)
    v.requires_grad_(True)
    f = torch.from_numpy(f0).to(dev)[None].expand(B, -1, -1)
    G = torch.randn(B, P, N, device=dev)
    out = []

    def line(text):
        print(text)
        out.append(text)

    line("# tools/mvc_time.py --reps %d, one MI355X" % args.reps)
    line("device: %s | torch %s" % (torch.cuda.get_device_name(dev), torch.__version__))
    with torch.no_grad():
        fwd = timed(lambda: mvc.mean_value_coordinates_3D(q, v, f), args.reps)

    def both(fn):
        wj = fn(q, v, f)
        torch.autograd.grad(wj, (q, v), G)

    fb = timed(lambda: both(mvc.mean_value_coordinates_3D), args.reps)
    line("B=%d P=%d N=%d F=%d fp32 (%d pairs)" % (B, P, N, F, B * P * F))
    line("HIP forward: %.3f ms median, %.3f best" % fwd)
    line("HIP forward + backward: %.3f ms median, %.3f best" % fb)
    with torch.no_grad():
        cf = timed(lambda: mvc.composition(q, v, f), 3, warmup=1)
    cfb = timed(lambda: both(mvc.composition), 3, warmup=1)
    line("torch composition forward: %.3f ms median | forward + backward: %.3f ms median -> %.1fx / %.1fx the kernels"
         % (cf[0], cfb[0], cf[0] / fwd[0], cfb[0] / fb[0]))
    try:
        valu, allins = loop_valu_count()
        floor = valu * B * P * F / ISSUE * 1e3
        line("face loop of the forward: %d vector instructions (%d in all) per pair -> VALU floor %.3f ms; the forward "
             "runs at %.0f%% of it" % (valu, allins, floor, 100 * floor / fwd[0]))
    except Exception as exc:  # the assembly count needs hipcc; the timings stand without it
        line("VALU floor not computed: %s" % exc)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
