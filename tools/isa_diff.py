#!/usr/bin/env python3
"""Per-kernel comparison of two sets of gfx950 assembly listings (what `hipcc -save-temps=obj` leaves as
*-hip-amdgcn-amd-amdhsa-gfx950.s): for a change that only moves kernels between translation units.

    python tools/isa_diff.py BEFORE AFTER        (each a .s file or a directory of them)

A kernel's text runs from `<symbol>:` to its `.Lfunc_end` -- the .amdhsa_kernel descriptor block included -- with the
`;` comments stripped and the function-local labels renumbered (.LBB<n>_, .Ltmp<n>: they encode only the function's
position in its unit).  Prints the counts and every symbol that is missing on one side or differs; exit status 1 then.

    python tools/isa_diff.py --counts BEFORE AFTER

for a change that renames kernels and lets the compiler reorder them: kernels are paired by lsm_key (the fused log-softmax
families under their old per-map, per-clamp names and as one template each) and compared by instruction counts per class,
LDS and scratch bytes and the waves per SIMD their registers allow -- one line per kernel (counts_main)."""
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


_ARG = re.compile(r"f|DF16b|DF16_|Li(\d+)E|Lb([01])E|NS_8DenseMapE|NS_10CompactMapILb[01]EEE")
_TYPES = {"f": "float", "DF16b": "bf16", "DF16_": "f16"}
_OWN_ARGS = {"small": 4, "large": 4, "generic": 2, "rows": 3}


def lsm_key(symbol):
    """One name for a fused log-softmax kernel in either spelling -- k_lsm_small_compact_clamped<E, L, MODE, WP> and
    k_lsm_small<E, L, MODE, WP, true, CompactMap<false>> -- read off the mangled symbol; other kernels keep theirs."""
    m = re.match(r"_ZN4rnnt\d+k_lsm_(small|large|generic|rows)(_compact)?(_clamped)?I", symbol)
    if not m:
        return symbol
    args, pos = [], m.end()
    while True:
        a = _ARG.match(symbol, pos)
        if not a:
            break
        args.append(_TYPES.get(a.group(0), a.group(1) or a.group(2) or a.group(0)))
        pos = a.end()
    own = _OWN_ARGS[m.group(1)]
    extra = args[own:]                                 # one template per family: [CLAMP,] Map
    compact = bool(m.group(2)) or any("CompactMap" in e for e in extra)
    clamped = bool(m.group(3)) or (len(extra) == 2 and extra[0] == "1")
    return "k_lsm_%s<%s> %s%s" % (m.group(1), ",".join(args[:own]), "compact" if compact else "dense",
                                   " clamped" if clamped else "")


_CLASSES = (("vmem", r"(global|buffer|flat|scratch)_"), ("lds", r"ds_"),
            ("trans", r"v_(exp|log|rcp|rsq|sqrt|sin|cos)_"), ("valu", r"v_"))


def profile(body):
    """Instruction counts by class and the descriptor's resources of one kernel's text."""
    p = dict.fromkeys([c for c, _ in _CLASSES], 0)
    for line in body.split("\n"):
        op = line.strip().split(" ")[0]
        for c, pat in _CLASSES:
            if re.match(pat, op):
                p[c] += 1
                break
    d = dict(re.findall(r"\.amdhsa_(next_free_vgpr|next_free_sgpr|group_segment_fixed_size|private_segment_fixed_size)\s+(\d+)",
                        body))
    p["lds_bytes"], p["scratch"] = int(d["group_segment_fixed_size"]), int(d["private_segment_fixed_size"])
    p["vgpr"], p["sgpr"] = int(d["next_free_vgpr"]), int(d["next_free_sgpr"])
    p["waves"] = min(8, 512 // (-(-p["vgpr"] // 8) * 8))      # gfx950: 512 unified VGPRs per lane, granule 8 (SGPRs do not bound it)
    return p


def counts_main(before, after):
    """--counts: for a change that renames kernels and may reorder their code.  Pairs the kernels by lsm_key and compares the
    instruction counts per class, LDS and scratch bytes and the waves per SIMD the registers allow; one line per kernel."""
    a = {}
    for k, (unit, body) in kernels(before).items():
        assert (unit, lsm_key(k)) not in a, k
        a[(unit, lsm_key(k))] = profile(body)
    b = {}
    for k, (unit, body) in kernels(after).items():
        assert (unit, lsm_key(k)) not in b, k
        b[(unit, lsm_key(k))] = profile(body)
    must = ("vmem", "lds", "trans", "valu", "lds_bytes", "scratch", "waves")
    cols = must + ("vgpr", "sgpr")
    bad = 0
    print("%-14s %-46s %s  verdict" % ("unit", "kernel", " ".join("%9s" % c for c in cols)))
    for key in sorted(set(a) | set(b)):
        unit, name = key[0].split("-hip-")[0], key[1] if len(key[1]) <= 46 else key[1][:43] + "..."
        if key not in a or key not in b:
            print("%-14s %-46s only %s" % (unit, name, "before" if key in a else "after"))
            bad += 1
            continue
        pa, pb = a[key], b[key]
        ok = all(pa[c] == pb[c] for c in must) and pb["scratch"] == 0
        bad += not ok
        cell = lambda c: "%9s" % (pa[c] if pa[c] == pb[c] else "%d>%d" % (pa[c], pb[c]))
        print("%-14s %-46s %s  %s" % (unit, name, " ".join(cell(c) for c in cols), "same" if ok else "DIFFERS"))
    print("kernels: %d before, %d after, %d paired; %d not the same" % (len(a), len(b), len(set(a) & set(b)), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    if sys.argv[1] == "--counts":
        sys.exit(counts_main(sys.argv[2], sys.argv[3]))
    sys.exit(main(sys.argv[1], sys.argv[2]))
