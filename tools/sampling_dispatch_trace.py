#!/usr/bin/env python3
"""Which kernels do the entry points of csrc/sampling.hip launch?  Two sets of calls, a store_ceiling_kernel launch in
front of and behind each, one line per call with its return code:

  scatter  every C-ABI entry point of gather_backward, group_points_grad and three_interpolate_grad (fp32 plain / _ws /
           _out_ws / _ordered, f16 and bf16 with and without the ordered flag) over the shapes of
           tests/test_scatter_plan_host.py's table with every knob at 0
  forward  pp_gather_forward_f32 / _b16, pp_group_points_strided_f32 / _b16 and pp_three_interpolate_f32 / _f16 / _bf16
           over FORWARD below: every threshold of the three forward dispatches from both sides, every alignment test
           both ways, and the knob values the tests use

  rocprofv3 --kernel-trace --output-format csv -d OUT -- python tools/sampling_dispatch_trace.py run [--tree DIR] [SET]
  python tools/sampling_dispatch_trace.py compare OUT_A OUT_B [OLD_KERNEL=NEW_KERNEL ...]

`run --tree DIR` loads the package of another checkout (the parent's) with this script and these tables; SET is
scatter, forward or (default) both.  `compare` cuts the two traces at the separators and compares the kernel-name
sequence of every call (template arguments kept, parameter lists dropped); where both OUT directories hold the run's
output as calls.log, the CALL lines (the return codes) are compared too."""
import csv
import ctypes
import glob
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEPARATOR = "store_ceiling_kernel"

# (operator, knob, shape, misaligned, dtypes).  Shapes: gather (B, C, N, M); group (B, C, N, npoint, nsample);
# interp (B, C, M, N).  misaligned: the tensors that start one element into a larger one -- p points, i idx, w weight,
# o out -- and for group "s": a batch stride of the output one element longer than C * P.  dtypes: "" all, "4" fp32
# only, "2" 16-bit only (where the other element size would only repeat a large global-gather call).
# L = 16 / element size = 4 (fp32) or 8 (16-bit) elements per 16 bytes.
FORWARD = [
    # ---- gather: the LDS form needs N * size <= 152 KiB, N <= 16 M, B C >= 512, M >= 1024
    ("gather", 0, (8, 64, 4096, 1024), "", ""),        # all hold; fp32 KR 1 (N / 4 <= 1024)
    ("gather", 0, (8, 64, 4100, 1024), "", ""),        # fp32 KR 2, 16-bit scalar (N % 8)
    ("gather", 0, (8, 64, 4104, 1024), "", ""),        # 16-bit vector again
    ("gather", 0, (8, 64, 8192, 1024), "", ""),        # fp32 KR 2 (N / 4 <= 2048)
    ("gather", 0, (8, 64, 8196, 1024), "", ""),        # fp32 KR 4
    ("gather", 0, (8, 64, 16384, 1024), "", ""),       # N = 16 M, and fp32's N <= 16384 inside vec
    ("gather", 0, (8, 64, 16392, 1024), "", ""),       # N > 16 M: global
    ("gather", 0, (8, 64, 16392, 1032), "", ""),       # N <= 16 M again; fp32 N > 16384: the scalar LDS kernel
    ("gather", 0, (7, 73, 4096, 1024), "", ""),        # B C = 511
    ("gather", 0, (8, 64, 4096, 1016), "", ""),        # M < 1024
    ("gather", 0, (8, 64, 38912, 2432), "", "4"),      # fp32 row = 152 KiB
    ("gather", 0, (8, 64, 38916, 2440), "", "4"),      # fp32 row too long
    ("gather", 0, (8, 64, 77824, 4864), "", "2"),      # 16-bit row = 152 KiB
    ("gather", 0, (8, 64, 77832, 4872), "", "2"),      # 16-bit row too long
    ("gather", 2, (1, 2, 77824, 64), "", ""),          # knob 2 (16-bit: wherever the row fits; fp32: as 0)
    ("gather", 2, (1, 2, 77832, 64), "", ""),
    ("gather", 0, (8, 64, 4097, 1024), "", ""),        # N % L
    ("gather", 0, (8, 64, 4096, 1027), "", ""),        # M % L
    ("gather", 0, (8, 64, 4096, 1024), "p", ""),
    ("gather", 0, (8, 64, 4096, 1024), "i", ""),
    ("gather", 0, (8, 64, 4096, 1024), "o", ""),
    ("gather", 1, (8, 64, 4096, 1024), "", ""),
    ("gather", 2, (8, 64, 4096, 1024), "", ""),
    ("gather", 0, (4, 8, 2048, 512), "", ""),          # the small shape of the 16-bit test, knobs 0 / 1 / 2
    ("gather", 1, (4, 8, 2048, 512), "", ""),
    ("gather", 2, (4, 8, 2048, 512), "", ""),
    ("gather", 2, (2, 3, 7, 5), "", ""),
    # ---- group: the LDS forms need vec, N % L, aligned points, N * size <= 64 KiB, C >= 4, B P >= 256 * 2048 (16-bit:
    # or a knob value other than 0 and 1); LDS-DMA on whole chunks of 32768 / 16384 / 8192 positions
    ("group", 0, (16, 4, 4096, 512, 64), "", ""),      # P = 32768: LDS-DMA, the largest chunk
    ("group", 0, (16, 4, 4096, 768, 64), "", ""),      # P = 3 * 16384: the middle chunk
    ("group", 0, (16, 4, 4096, 640, 64), "", ""),      # P = 5 * 8192: the smallest chunk
    ("group", 0, (16, 4, 4096, 576, 64), "", ""),      # P = 9 * 4096: ragged, VGPR-staged (fp32: 2 quads)
    ("group", 0, (8, 4, 4096, 1024, 64), "", ""),      # B P = 256 * 2048 exactly
    ("group", 0, (8, 4, 4096, 1023, 64), "", ""),      # B P below the floor
    ("group", 0, (16, 3, 4096, 512, 64), "", ""),      # C < 4
    ("group", 0, (16, 4, 16384, 512, 64), "", "4"),    # fp32 row = 64 KiB
    ("group", 0, (16, 4, 16388, 512, 64), "", "4"),    # fp32 row too long for the 16-byte forms
    ("group", 0, (16, 4, 32768, 512, 64), "", "2"),    # 16-bit row = 64 KiB
    ("group", 0, (16, 4, 32776, 512, 64), "", "2"),    # 16-bit row too long
    ("group", 0, (16, 4, 64, 131073, 4), "", ""),      # ragged, B P / 512 >= 512 * 4 * 8: fp32 8 quads
    ("group", 0, (16, 4, 64, 131071, 4), "", ""),      # just below: fp32 4 quads
    ("group", 0, (16, 4, 64, 65537, 4), "", ""),       # B P / 512 >= 512 * 4 * 4: fp32 4 quads
    ("group", 0, (16, 4, 64, 65535, 4), "", ""),       # just below: fp32 2 quads
    ("group", 0, (16, 4, 2048, 576, 64), "", "4"),     # the VGPR-staged kernel's KR: N / 4 <= 512
    ("group", 0, (16, 4, 2052, 576, 64), "", "4"),     # <= 1024
    ("group", 0, (16, 4, 4100, 576, 64), "", "4"),     # <= 2048
    ("group", 0, (16, 4, 8196, 576, 64), "", "4"),     # beyond
    ("group", 0, (16, 4, 4096, 262144, 16), "i", "4"), # fp32 scalar LDS form: unaligned and B P C = 2^28
    ("group", 0, (16, 4, 4096, 262143, 16), "i", "4"), # below 2^28: global
    ("group", 2, (16, 4, 38912, 512, 65), "", ""),     # the same form by the knob, row = 152 KiB (fp32); 16-bit: global
    ("group", 2, (16, 4, 38913, 512, 65), "", ""),     # row too long
    ("group", 2, (8, 4, 4096, 1023, 64), "", ""),      # B P below the floor: the knob waives it for 16-bit only
    ("group", 0, (16, 4, 4096, 512, 65), "", ""),      # P % L
    ("group", 0, (16, 4, 4097, 512, 64), "", ""),      # N % L
    ("group", 0, (16, 4, 4096, 512, 64), "s", ""),     # batch stride % L
    ("group", 0, (16, 4, 4096, 512, 64), "p", ""),
    ("group", 0, (16, 4, 4096, 512, 64), "i", ""),
    ("group", 0, (16, 4, 4096, 512, 64), "o", ""),
] + [("group", v, shape, "", "") for v in (0, 1, 2, 4, 8, 604, 608, 616, 300)
     for shape in ((8, 4, 4096, 1024, 64),             # the 16-bit test's shape: whole chunks, B P at the floor
                   (16, 4, 4096, 576, 64),             # ragged chunks
                   (2, 4, 4096, 128, 64),              # below the floor (16-bit: waived by the knob), one 8192 chunk
                   (2, 5, 509, 37, 3))                 # nothing aligned
     ] + [
    # ---- interp: the channel-group form needs M * size <= 152 KiB, N >= 2048, 8 ceil(B / 8) ceil(C / 4) >= 256 (16-bit:
    # or knob 3); fp32 else the row-at-a-time form: vec, M <= 16384, C >= 4, B N >= 64 * 2048
    ("interp", 0, (1, 125, 4096, 2048), "", ""),       # four rows in 64 KiB (fp32 at its limit)
    ("interp", 0, (1, 125, 4100, 2048), "", "4"),      # fp32: two rows
    ("interp", 0, (1, 125, 19456, 2048), "", "4"),     # fp32: two rows = 152 KiB
    ("interp", 0, (1, 125, 19460, 2048), "", "4"),     # fp32: one row
    ("interp", 0, (1, 125, 38912, 2048), "", "4"),     # fp32 row = 152 KiB
    ("interp", 0, (1, 125, 38916, 2048), "", "4"),     # fp32 row too long
    ("interp", 0, (1, 125, 8192, 2048), "", "2"),      # 16-bit: four rows = 64 KiB
    ("interp", 0, (1, 125, 8200, 2048), "", "2"),      # 16-bit: one row
    ("interp", 0, (1, 125, 77824, 2048), "", "2"),     # 16-bit row = 152 KiB
    ("interp", 0, (1, 125, 77832, 2048), "", "2"),     # 16-bit row too long
    ("interp", 0, (1, 3, 4096, 2048), "", ""),         # C < 4 (and the grid floor)
    ("interp", 3, (1, 3, 4096, 2048), "", ""),         # ... 16-bit with knob 3: one row
    ("interp", 0, (1, 125, 4096, 2044), "", ""),       # N < 2048
    ("interp", 0, (1, 124, 4096, 2048), "", ""),       # grid floor: 248 workgroups
    ("interp", 0, (64, 4, 4096, 2048), "", ""),        # below the floor, fp32 row-at-a-time: B N = 64 * 2048, C = 4
    ("interp", 0, (64, 3, 4096, 2048), "", ""),        # C < 4: global
    ("interp", 0, (63, 4, 4096, 2048), "", ""),        # B N below
    ("interp", 2, (64, 4, 16384, 2048), "", "4"),      # fp32 row-at-a-time: M = 16384
    ("interp", 2, (64, 4, 16388, 2048), "", "4"),      # M beyond
    ("interp", 2, (64, 4, 2048, 2048), "", "4"),       # its KR: M / 4 <= 512
    ("interp", 2, (64, 4, 2052, 2048), "", "4"),       # <= 1024
    ("interp", 2, (64, 4, 4100, 2048), "", "4"),       # <= 2048
    ("interp", 2, (64, 4, 8196, 2048), "", "4"),       # beyond
    ("interp", 0, (1, 125, 4097, 2048), "", ""),       # M % L
    ("interp", 0, (1, 125, 4100, 2048), "", "2"),      # M % 8 only
    ("interp", 0, (1, 125, 4096, 2049), "", ""),       # N % 4
    ("interp", 0, (1, 125, 4101, 2049), "", "4"),      # fp32: two rows, unaligned
    ("interp", 0, (1, 125, 19461, 2049), "", "4"),     # fp32: one row, unaligned
    ("interp", 0, (1, 125, 4096, 2048), "p", ""),
    ("interp", 0, (1, 125, 4096, 2048), "i", ""),
    ("interp", 0, (1, 125, 4096, 2048), "w", ""),
    ("interp", 0, (1, 125, 4096, 2048), "o", ""),
] + [("interp", v, shape, "", "") for v in (0, 1, 2, 3)
     for shape in ((1, 125, 4096, 2048), (8, 4, 4096, 16384), (2, 5, 509, 2047), (2, 3, 5, 7))]


def scatter_cases():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_scatter_plan_host as t
    seen = []
    for op, shape, ws, knobs, _ in t.TABLE:
        if knobs == t.K0 and (op, shape, ws) not in seen:
            seen.append((op, shape, ws))
    return seen


def run_scatter(torch, _lib, L, dev, stream, mark):
    g = torch.Generator(device="cpu").manual_seed(5)
    for op, (b, c, sources, dests), ws_kind in scatter_cases():
        per = 3 if op == 2 else 1
        need = int(L.pp_scatter_workspace_bytes(b, per * sources, dests, per, int(op == 2)))
        nbytes = {"full": need, "short": max(need - 1, 0), "none": 0}[ws_kind]
        ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
        wsp = _lib.ptr(ws) if nbytes else None
        idx = torch.randint(0, dests, (b, sources, per), generator=g, dtype=torch.int32).to(dev)
        weight = torch.rand((b, sources, 3), generator=g).to(dev)
        for dt, suffix in ((torch.float32, "f32"), (torch.float16, "f16"), (torch.bfloat16, "bf16")):
            src = torch.rand((b, c, sources), generator=g).to(dev).to(dt)
            out = torch.zeros((b, c, dests), dtype=dt, device=dev)
            lead = (_lib.ptr(src), _lib.ptr(idx)) + ((_lib.ptr(weight),) if op == 2 else ()) + (_lib.ptr(out),)
            if op == 0:
                stem, sizes, strided = "pp_gather_backward", (b, c, dests, sources), ()
            elif op == 1:
                stem, sizes, strided = "pp_group_points_grad", (b, c, dests, sources, 1), (c * sources,)
            else:
                stem, sizes, strided = "pp_three_interpolate_grad", (b, c, sources, dests), ()
            tail = (wsp, nbytes)
            if suffix == "f32":
                calls = [("_f32", lead + sizes), ("_ws_f32", lead + sizes + strided + tail),
                         ("_ordered_f32", lead + sizes + strided + tail)]
                if op == 1:
                    calls += [("_strided_f32", lead + sizes + strided), ("_out_ws_f32", lead + sizes + strided + tail)]
            else:
                calls = [("_out_ws_%s" % suffix, lead + sizes + strided + tail + (0,)),
                         ("_out_ws_%s" % suffix, lead + sizes + strided + tail + (1,))]
            for name, args in calls:
                torch.cuda.synchronize()
                mark()
                code = getattr(L, stem + name)(*args, stream)
                mark()
                torch.cuda.synchronize()
                flag = " ordered=%d" % args[-1] if suffix != "f32" else ""
                print("CALL %s%s%s %s ws=%s -> %d" % (stem, name, flag, "x".join(map(str, (b, c, sources, dests))),
                                                    ws_kind, code), flush=True)


def run_forward(torch, _lib, L, dev, stream, mark):
    def tensor(count, dtype, off):
        """`count` elements, 16-byte aligned or (off) one element past that"""
        return torch.empty(count + 1, dtype=dtype, device=dev)[1:] if off else torch.empty(count, dtype=dtype, device=dev)

    def indices(count, high, off):
        t = tensor(count, torch.int32, off)
        t.copy_(torch.randint(0, high, (count,), dtype=torch.int32, device=dev))
        return t

    setters = {"gather": L.pp_debug_set_gather_variant, "group": L.pp_debug_set_group_points_variant,
               "interp": L.pp_debug_set_three_interpolate_variant}
    dtypes = ((torch.float32, "f32", "4"), (torch.float16, "f16", "2"), (torch.bfloat16, "bf16", "2"))
    for op, knob, shape, mis, only in FORWARD:
        for dt, suffix, size in dtypes:
            if (only and only != size) or (op != "interp" and suffix == "bf16"):  # the copies have one 16-bit entry
                continue
            if op == "gather":
                b, c, n, m = shape
                idx = indices(b * m, n, "i" in mis)
                points, out = tensor(b * c * n, dt, "p" in mis), tensor(b * c * m, dt, "o" in mis)
                entry = "pp_gather_forward_" + ("f32" if size == "4" else "b16")
                args = (_lib.ptr(points), _lib.ptr(idx), _lib.ptr(out), b, c, n, m)
            elif op == "group":
                b, c, n, npoint, nsample = shape
                obs = c * npoint * nsample + ("s" in mis)
                idx = indices(b * npoint * nsample, n, "i" in mis)
                points, out = tensor(b * c * n, dt, "p" in mis), tensor(b * obs, dt, "o" in mis)
                entry = "pp_group_points_strided_" + ("f32" if size == "4" else "b16")
                args = (_lib.ptr(points), _lib.ptr(idx), _lib.ptr(out), b, c, n, npoint, nsample, obs)
            else:
                b, c, m, n = shape
                idx = indices(b * n * 3, m, "i" in mis)
                weight = tensor(b * n * 3, torch.float32, "w" in mis)
                points, out = tensor(b * c * m, dt, "p" in mis), tensor(b * c * n, dt, "o" in mis)
                entry = "pp_three_interpolate_" + suffix
                args = (_lib.ptr(points), _lib.ptr(idx), _lib.ptr(weight), _lib.ptr(out), b, c, m, n)
            torch.cuda.synchronize()
            setters[op](knob)
            mark()
            code = getattr(L, entry)(*args, stream)
            mark()
            setters[op](0)
            torch.cuda.synchronize()
            print("CALL %s %s knob=%d misaligned=%s -> %d" % (entry, "x".join(map(str, shape)), knob, mis or "-", code),
                  flush=True)
            del idx, points, out


def run(tree, which):
    sys.path.insert(0, tree)
    import torch
    from pytorch_points_amd import _lib
    L = _lib.lib()
    dev = torch.device("cuda")
    sep = torch.empty(4096, device=dev)
    L.pp_debug_store_ceiling.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    with _lib.on_device(dev) as stream:
        def mark():
            assert L.pp_debug_store_ceiling(_lib.ptr(sep), 4096, 0, 1, stream) == 0

        if which in ("scatter", "both"):
            run_scatter(torch, _lib, L, dev, stream, mark)
        if which in ("forward", "both"):
            run_forward(torch, _lib, L, dev, stream, mark)


def kernel_sequences(out_dir, renames):
    files = glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"), recursive=True)
    assert len(files) == 1, files
    rows = sorted(csv.DictReader(open(files[0])), key=lambda r: int(r["Start_Timestamp"]))
    names = [re.sub(r"\(.*$", "", re.sub(r"\(anonymous namespace\)::|^void ", "", r["Kernel_Name"])) for r in rows]
    names = [renames.get(n, n) for n in names]
    cuts = [i for i, n in enumerate(names) if n.endswith(SEPARATOR)]
    assert len(cuts) % 2 == 0
    return [names[a + 1:b] for a, b in zip(cuts[0::2], cuts[1::2])]


def call_lines(out_dir):
    path = os.path.join(out_dir, "calls.log")
    return [ln.strip() for ln in open(path) if ln.startswith("CALL ")] if os.path.exists(path) else None


def compare(dir_a, dir_b, pairs):
    renames = dict(p.split("=", 1) for p in pairs)
    a, b = kernel_sequences(dir_a, renames), kernel_sequences(dir_b, {})
    print("calls: %d and %d; kernel launches inside them: %d and %d" % (len(a), len(b), sum(map(len, a)), sum(map(len, b))))
    differ = [i for i, (x, y) in enumerate(zip(a, b)) if x != y]
    for i in differ[:20]:
        print("call %d: %s | %s" % (i, a[i], b[i]))
    kinds = sorted({n for s in b for n in s})
    print("kernels seen: " + ", ".join(kinds))
    print("calls whose kernel sequences differ: %d" % (len(differ) + abs(len(a) - len(b))))
    la, lb = call_lines(dir_a), call_lines(dir_b)
    codes = 0
    if la is not None and lb is not None:
        codes = sum(x != y for x, y in zip(la, lb)) + abs(len(la) - len(lb))
        tally = {}
        for ln in lb:
            tally[ln.rsplit(" ", 1)[1]] = tally.get(ln.rsplit(" ", 1)[1], 0) + 1
        print("CALL lines: %d and %d, return codes %s; lines that differ: %d" % (len(la), len(lb), tally, codes))
        if len(lb) != len(b):
            print("CALL lines and traced calls disagree: %d against %d" % (len(lb), len(b)))
            codes += 1
    return 1 if differ or len(a) != len(b) or codes else 0


if __name__ == "__main__":
    if len(sys.argv) >= 2 and sys.argv[1] == "run":
        rest = sys.argv[2:]
        tree = ROOT
        if rest[:1] == ["--tree"]:
            tree, rest = os.path.abspath(rest[1]), rest[2:]
        run(tree, rest[0] if rest else "both")
    elif len(sys.argv) >= 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3], sys.argv[4:]))
    else:
        sys.exit(__doc__)
