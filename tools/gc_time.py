"""Times green_coordinates_3D at the Neural-Cages size (B=8, P=16384, icosphere cage 162 V / 320 F, fp32): the HIP
forward, forward plus backward, and the in-tree torch composition on the same device and data (or the point where it
runs out of memory); and a per-pair instruction estimate.

    python tools/gc_time.py [--reps 5] [--out profiles/r9/gc_time.txt]

Device events after warm-up, seeded data.  Instruction estimate: the vector instructions of the forward kernel's
per-pair code (counted in the gfx950 assembly of csrc/green.hip, built here with --save-temps; libm calls are inlined
there): the body of the rolled loop over the six _gcTriInt evaluations, times six, plus the rest of the face loop,
straight-line, both branch sides included.  Times B*P*F pairs at the vector issue rate of 256 CUs x 4 SIMDs x 16 lanes
x 2.4 GHz = 39.3e12 lane instructions/s gives a floor at the fp32 rate; the pair is evaluated in fp64, whose
instructions issue more slowly, so this is an estimate, not a bound.
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
from pytorch_points_amd import _build, green  # noqa: E402

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
    """vector instructions (and all instructions) of one pair in gc_forward_kernel<float, true>: the face loop's body,
    which holds the loop over the six _gcTriInt evaluations once, plus five more of that loop's bodies"""
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), *[f for f in _build.HIPCC_FLAGS if f != "-shared"],
               "-I" + _build.INCLUDE, "-I" + _build.CSRC, "--save-temps", "-c",
               os.path.join(_build.CSRC, "green.hip"), "-o", os.path.join(tmp, "green.o")]
        subprocess.run(cmd, cwd=tmp, check=True, capture_output=True)
        asm = open(glob.glob(os.path.join(tmp, "*gfx950*.s"))[0]).read()
    name = re.search(r"^(_ZN\S*gc_forward_kernelIfLb1E\S*):", asm, re.M).group(1)
    body = asm[asm.index(name + ":"):]
    body = body[:body.index("s_endpgm")]
    lines = body.splitlines()
    labels = {m.group(1): i for i, m in enumerate(re.match(r"^(\.LBB\w+):", ln) for ln in lines) if m}
    loops = []
    for i, ln in enumerate(lines):
        m = re.match(r"\s+s_cbranch_\w+\s+(\.LBB\w+)|\s+s_branch\s+(\.LBB\w+)", ln)
        if m:
            tgt = m.group(1) or m.group(2)
            if tgt in labels and labels[tgt] < i:
                loops.append((i - labels[tgt], labels[tgt], i))
    loops.sort(reverse=True)

    def count(a, b):
        seg = lines[a:b + 1]
        return (sum(1 for ln in seg if re.match(r"\s+v_", ln)),
                sum(1 for ln in seg if re.match(r"\s+(v_|s_|ds_|global_)", ln)))

    # the chunk loop over 64 faces holds the face loop, which holds the rolled loop over the six evaluations
    chain = [loops[0]]
    for _ in range(2):
        chain.append(max(lp for lp in loops if lp[1] > chain[-1][1] and lp[2] <= chain[-1][2]))
    fv, fa = count(chain[1][1], chain[1][2])
    ev, ea = count(chain[2][1], chain[2][2])
    return fv + 5 * ev, fa + 5 * ea


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
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
    Gv, Gf = torch.randn(B, P, N, device=dev), torch.randn(B, P, F, device=dev)
    out = []

    def line(text):
        print(text)
        out.append(text)

    line("# tools/gc_time.py --reps %d, one MI355X" % args.reps)
    line("device: %s | torch %s" % (torch.cuda.get_device_name(dev), torch.__version__))
    with torch.no_grad():
        fwd = timed(lambda: green.green_coordinates_3D(q, v, f), args.reps)

    def both(fn):
        gcv, gcf, _ = fn(q, v, f)
        torch.autograd.grad((gcv, gcf), (q, v), (Gv, Gf))

    fb = timed(lambda: both(green.green_coordinates_3D), args.reps)
    line("B=%d P=%d N=%d F=%d fp32 (%d pairs)" % (B, P, N, F, B * P * F))
    line("HIP forward: %.3f ms median, %.3f best" % fwd)
    line("HIP forward + backward: %.3f ms median, %.3f best" % fb)
    for label, fn, ref in (("forward", lambda: green.composition(q.detach(), v.detach(), f), fwd),
                           ("forward + backward", lambda: both(green.composition), fb)):
        torch.cuda.empty_cache()
        try:
            t = timed(fn, 2, warmup=1)
            line("torch composition %s: %.3f ms median -> %.1fx the kernels" % (label, t[0], t[0] / ref[0]))
        except torch.cuda.OutOfMemoryError:
            line("torch composition %s: out of device memory (%.1f GB in use at the failure)" % (
                label, torch.cuda.max_memory_allocated() / 1e9))
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
    try:
        valu, allins = loop_valu_count()
        floor = valu * B * P * F / ISSUE * 1e3
        line("one pair of the forward: %d vector instructions (%d in all), straight-line -> VALU estimate %.3f ms; "
             "the forward runs at %.0f%% of it" % (valu, allins, floor, 100 * floor / fwd[0]))
    except Exception as exc:  # the assembly count needs hipcc; the timings stand without it
        line("instruction estimate not computed: %s" % exc)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
