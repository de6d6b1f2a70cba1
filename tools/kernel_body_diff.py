"""Instruction diff of one kernel family between two builds of a translation unit.

    hipcc ... --save-temps -c csrc/device/UNIT.hip      (once per commit; keeps UNIT-hip-amdgcn-amd-amdhsa-gfx950.s)
    python tools/kernel_body_diff.py PARENT.s NEW.s k_range

A kernel body is what stands between a kernel's label and its .Lfunc_end; comments, directives and blank lines are dropped, and the
kernel's own (mangled) name is replaced by its demangled template arguments cut to the parent's count, so a template parameter
appended with a default does not show.  Kernels are paired by that key.  Prints one line per kernel and the first differing lines;
exit status 1 when any body differs or a kernel of the parent is missing."""
import re
import subprocess
import sys


def bodies(path, family):
    out, name, cur = {}, None, []
    for line in open(path):
        s = line.split(";")[0].rstrip()
        m = re.match(r"^(_Z\w+):", s)
        if m and family in m.group(1):
            name, cur = m.group(1), []
            continue
        if name is None:
            continue
        if s.startswith(".Lfunc_end"):
            out[name] = cur
            name = None
            continue
        t = s.strip()
        if not t or t.startswith("."):
            if not re.match(r"^\.LBB\d+_\d+:", t):
                continue
        cur.append(t.replace(name, "<kernel>"))
    return out


def key(mangled, nargs=None):
    d = subprocess.run(["c++filt", mangled], capture_output=True, text=True).stdout.strip()
    m = re.search(r"<(.*?)>\(", d)
    args = [a.strip() for a in m.group(1).split(",")] if m else []
    return tuple(re.sub(r"^\(\w+\)", "", a) for a in (args[:nargs] if nargs else args))


def main():
    parent, new, family = sys.argv[1:4]
    pb, nb = bodies(parent, family), bodies(new, family)
    pk = {key(n): n for n in pb}
    nargs = max(len(k) for k in pk)
    nk = {}
    for n in nb:
        full = key(n)
        nk.setdefault(full[:nargs], []).append((full, n))
    bad = 0
    for k, pn in sorted(pk.items()):
        # the new build's kernel with the same leading arguments and the fewest extra ones set (the defaults)
        cands = sorted(nk.get(k, []), key=lambda c: c[0])
        if not cands:
            print("%s<%s>: missing in the new build" % (family, ", ".join(k)))
            bad += 1
            continue
        a, b = pb[pn], nb[cands[0][1]]
        if a == b:
            print("%s<%s>: %d instructions and labels, identical" % (family, ", ".join(k), len(a)))
        else:
            bad += 1
            print("%s<%s>: DIFFERS (%d against %d lines)" % (family, ", ".join(k), len(a), len(b)))
            for i, (x, y) in enumerate(zip(a, b)):
                if x != y:
                    print("  line %d: %s  |  %s" % (i, x, y))
                    break
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
