#!/usr/bin/env python3
"""Per-kernel comparison of two sets of gfx950 assembly listings (what `hipcc -save-temps=obj` leaves as
*-hip-amdgcn-amd-amdhsa-gfx950.s): for a change that only moves kernels between translation units.

    python tools/isa_diff.py BEFORE AFTER        (each a .s file or a directory of them)

A kernel's text runs from `<symbol>:` to its `.Lfunc_end` -- the .amdhsa_kernel descriptor block included -- with the
`;` comments stripped and the function-local labels renumbered (.LBB<n>_, .Ltmp<n>: they encode only the function's
position in its unit).  Prints the counts and every symbol that is missing on one side or differs; exit status 1 then."""
import difflib
import glob
import os
import re
import sys


def kernels(path):
    files = sorted(glob.glob(os.path.join(path, "*gfx950.s"))) if os.path.isdir(path) else [path]
    out = {}
    for f in files:
        with open(f) as h:
            text = h.read()
        names = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M))
        for m in re.finditer(r"^(\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", text, re.M | re.S):
            if m.group(1) not in names:
                continue
            body = re.sub(r"\.LBB\d+_", ".LBB_", m.group(2))
            body = re.sub(r"\.Ltmp\d+", ".Ltmp", body)
            body = re.sub(r"[ \t]*;.*$", "", body, flags=re.M)
            assert m.group(1) not in out, "kernel %s defined twice" % m.group(1)
            out[m.group(1)] = (os.path.basename(f), body)
        assert names <= set(out), "no text found for %s" % sorted(names - set(out))[:3]
    return out


def main(before, after):
    a, b = kernels(before), kernels(after)
    differ = sorted(k for k in set(a) & set(b) if a[k][1] != b[k][1])
    print("kernels: %d before, %d after, %d in both, %d equal" % (len(a), len(b), len(set(a) & set(b)),
                                                                   len(set(a) & set(b)) - len(differ)))
    for side, only in (("before", set(a) - set(b)), ("after", set(b) - set(a))):
        for k in sorted(only):
            print("only %s: %s" % (side, k))
    for k in differ:
        print("DIFFERS %s (%s / %s)" % (k, a[k][0], b[k][0]))
        d = difflib.unified_diff(a[k][1].split("\n"), b[k][1].split("\n"), lineterm="", n=0)
        print("\n".join(list(d)[:40]))
    per_unit = {}
    for unit, _ in b.values():
        per_unit[unit] = per_unit.get(unit, 0) + 1
    print("after, per unit: " + ", ".join("%s %d" % (u.split("-hip-")[0], n) for u, n in sorted(per_unit.items())))
    same = not differ and set(a) == set(b)
    print("verdict: %s" % ("EQUAL" if same else "NOT EQUAL"))
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
