#!/usr/bin/env python
"""The error grid behind the bars of tests/test_gpu_pruned_hidden.py.

    python tools/pruned_hidden_values.py [--out profiles/pruned_hidden_values.txt]

Per dtype, case and activation of that test: max |x - ref| / max |ref| of h, df and dg against its fp64 reference, for the
torch chain (prune_joint_inputs, add, activation, autograd in the dtype: the yardstick) and for pruned_joint_hidden; then,
per dtype, the largest of each over the grid -- the chain's are the test's YARDSTICK."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pruned_hidden_values.txt"))
    a = ap.parse_args()
    import test_gpu_pruned_hidden as t
    from warp_rnnt_amd import _build
    _build.ensure_built()
    lines = ["# dtype case activation | chain (yardstick): h df dg | pruned_joint_hidden: h df dg"]
    fmt = lambda e: " ".join(f"{x:.3e}" for x in e)  # noqa: E731
    for name in t.DTYPES:
        worst = {"chain": (0.0,) * 3, "hip": (0.0,) * 3}
        for case in t.CASES:
            for act in ("tanh", "relu"):
                ref = t.reference(case, name, act)
                e = {"chain": t.errors(t.chain(case, name, act), ref), "hip": t.errors(t.kernel(case, name, act), ref)}
                worst = {k: tuple(map(max, worst[k], e[k])) for k in e}
                lines.append(f"{name} {case.replace(' ', '_')} {act} | {fmt(e['chain'])} | {fmt(e['hip'])}")
        lines.append(f"{name} LARGEST | {fmt(worst['chain'])} | {fmt(worst['hip'])}")
    print("\n".join(lines), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
