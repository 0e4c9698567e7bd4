#!/usr/bin/env python3
"""Which kernels do the scatter-add backwards launch?  Calls every C-ABI entry point of gather_backward,
group_points_grad and three_interpolate_grad (fp32 plain / _ws / _out_ws / _ordered, f16 and bf16 with and without the
ordered flag) over the shapes of tests/test_scatter_plan_host.py's table with every knob at 0, a store_ceiling_kernel
launch in front of and behind each call, and prints one line per call with its return code.

  rocprofv3 --kernel-trace --output-format csv -d OUT -- python tools/scatter_dispatch_trace.py run [--tree DIR]
  python tools/scatter_dispatch_trace.py compare OUT_A OUT_B [OLD_KERNEL=NEW_KERNEL ...]

`run --tree DIR` loads the package of another checkout (the parent's) with this script and this table.  `compare`
cuts the two traces at the separators and compares the kernel-name sequence of every call (template arguments kept,
parameter lists dropped)."""
import csv
import ctypes
import glob
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEPARATOR = "store_ceiling_kernel"


def cases():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_scatter_plan_host as t
    seen = []
    for op, shape, ws, knobs, _ in t.TABLE:
        if knobs == t.K0 and (op, shape, ws) not in seen:
            seen.append((op, shape, ws))
    return seen


def run(tree):
    sys.path.insert(0, tree)
    import torch
    from pytorch_points_amd import _lib
    L = _lib.lib()
    dev = torch.device("cuda")
    g = torch.Generator(device="cpu").manual_seed(5)
    sep = torch.empty(4096, device=dev)
    L.pp_debug_store_ceiling.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    with _lib.on_device(dev) as stream:
        def mark():
            assert L.pp_debug_store_ceiling(_lib.ptr(sep), 4096, 0, 1, stream) == 0

        for op, (b, c, sources, dests), ws_kind in cases():
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


def kernel_sequences(out_dir, renames):
    files = glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"), recursive=True)
    assert len(files) == 1, files
    rows = sorted(csv.DictReader(open(files[0])), key=lambda r: int(r["Start_Timestamp"]))
    names = [re.sub(r"\(.*$", "", re.sub(r"\(anonymous namespace\)::|^void ", "", r["Kernel_Name"])) for r in rows]
    names = [renames.get(n, n) for n in names]
    cuts = [i for i, n in enumerate(names) if n.endswith(SEPARATOR)]
    assert len(cuts) % 2 == 0
    return [names[a + 1:b] for a, b in zip(cuts[0::2], cuts[1::2])]


def compare(dir_a, dir_b, pairs):
    renames = dict(p.split("=", 1) for p in pairs)
    a, b = kernel_sequences(dir_a, renames), kernel_sequences(dir_b, {})
    print("calls: %d and %d; kernel launches inside them: %d and %d" % (len(a), len(b), sum(map(len, a)), sum(map(len, b))))
    differ = [i for i, (x, y) in enumerate(zip(a, b)) if x != y]
    for i in differ[:20]:
        print("call %d: %s | %s" % (i, a[i], b[i]))
    kinds = sorted({n for s in a for n in s})
    print("kernels seen: " + ", ".join(kinds))
    print("calls whose kernel sequences differ: %d" % (len(differ) + abs(len(a) - len(b))))
    return 1 if differ or len(a) != len(b) else 0


if __name__ == "__main__":
    if len(sys.argv) >= 2 and sys.argv[1] == "run":
        run(os.path.abspath(sys.argv[3]) if len(sys.argv) > 3 and sys.argv[2] == "--tree" else ROOT)
    elif len(sys.argv) >= 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3], sys.argv[4:]))
    else:
        sys.exit(__doc__)
