"""Which device functions differ between two gfx950 assembly files (hipcc --save-temps: *-hip-amdgcn-*.s)?

  python tools/isa_diff.py OLD.s NEW.s [OLD_SYMBOL=NEW_SYMBOL ...]

A function is the text between its `.type NAME,@function` line and its `.Lfunc_end` label, comments dropped and
local labels (.LBBn_m, .Lfunc_*, .Ltmp*) renumbered in order of appearance, so that code which only moved inside
the file compares equal.  Functions are paired by mangled name; a pair whose name changed (a template parameter that
became a constant) is given as OLD=NEW.  Prints one line per function: same / DIFFERS / only in one file, and for
the pairs that differ a unified diff.  Exit status 1 when a paired function differs.
"""
import difflib
import re
import sys


def functions(path):
    out, name, body = {}, None, []
    for line in open(path):
        m = re.match(r"\s*\.type\s+([\w.$]+),@function", line)
        if m:
            name, body = m.group(1), []
            continue
        if name is None:
            continue
        if re.match(r"\.Lfunc_end\d+:", line):
            out[name] = normalise(body, name)
            name = None
            continue
        line = re.sub(r"\s*;.*", "", line).rstrip()
        if line:
            body.append(line)
    return out


def normalise(body, name):
    seen = {}

    def label(m):
        return seen.setdefault(m.group(0), ".L%d" % len(seen))

    text = [re.sub(r"\.L(BB\d+_\d+|func_\w+|tmp\d+)", label, ln) for ln in body]
    return [ln.replace(name, "<self>") for ln in text]


def main():
    old, new = functions(sys.argv[1]), functions(sys.argv[2])
    renamed = dict(a.split("=") for a in sys.argv[3:])
    differs = 0
    for o in sorted(old):
        n = renamed.get(o, o)
        if n not in new:
            print("only in old   ", o)
        elif old[o] == new[n]:
            print("same          ", n)
        else:
            differs += 1
            print("DIFFERS       ", n)
            sys.stdout.write("\n".join(difflib.unified_diff(old[o], new[n], o, n, n=2, lineterm="")) + "\n")
    for n in sorted(set(new) - {renamed.get(o, o) for o in old}):
        print("only in new   ", n)
    return 1 if differs else 0


if __name__ == "__main__":
    sys.exit(main())
