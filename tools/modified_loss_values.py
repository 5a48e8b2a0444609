#!/usr/bin/env python
"""The errors of the modified topology and the delay penalty against fp64 beside those of the regular entries without a
penalty, over the cases of tests/test_gpu_modified.py.

    python tools/modified_loss_values.py [--out profiles/modified_loss_values.txt]

Per case: the errors of pruned_rnnt_loss_from_logits / simple_rnnt_loss with rnnt_type and delay_penalty against
tests/modified_reference.py, then the yardstick's -- the same entry called without the keywords, on the same generator,
shapes and lengths, against tests/pruned_reference.py / tests/simple_reference.py.  The last lines are the yardstick's
maxima per group: the YARDSTICK table of the test, whose bars are four times them."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch  # noqa: E402

import test_gpu_modified as tg  # noqa: E402


def main(out):
    lines = ["# pruned: N T U S V blank lambda dp topology | cost rel, d/d logits abs | yardstick (regular, no penalty) "
             "cost rel, d/d logits abs | sweep kernel"]
    worst = {}

    def note(group, mine, yard):
        m, y = worst.get(group, ((0.0,) * len(mine), (0.0,) * len(yard)))
        worst[group] = (tuple(map(max, m, mine)), tuple(map(max, y, yard)))

    for group, cases, dps in (("pruned values", tg.PRUNED_VALUE_CASES, tg.VALUE_DPS),
                              ("pruned sweeps", tg.PRUNED_SWEEP_CASES, tg.SWEEP_DPS)):
        for shape, blank in cases:
            for lam in tg.LAMS:
                yard = tg.pruned_yardstick_errors(shape, blank, lam)
                for dp in dps:
                    for rnnt_type in tg.topologies_of(shape, dp):
                        cost, grad, kernel = tg.pruned_errors(shape, blank, lam, dp, rnnt_type)
                        note(group, (cost, grad), yard)
                        lines.append("%d %d %d %d %d blank %4d lambda %.2f dp %.2f %-8s | %.3e %.3e | %.3e %.3e | %s" %
                                     (*shape, blank, lam, dp, rnnt_type, cost, grad, *yard, kernel))
                        print(lines[-1], flush=True)
    lines.append("# simple: N T U V lambda dp topology | cost rel, pair_grads abs, d am abs, d lm abs | yardstick (regular, no "
                 "penalty) the same four")
    for group, cases, dps in (("simple values", tg.SIMPLE_VALUE_CASES, tg.VALUE_DPS),
                              ("simple sweeps", tg.SIMPLE_SWEEP_CASES, tg.SWEEP_DPS)):
        for shape, V in cases:
            for lam in tg.LAMS:
                yard = tg.simple_errors(shape, V, lam, 0.0, None)
                for dp in dps:
                    for rnnt_type in tg.topologies_of(shape, dp):
                        mine = tg.simple_errors(shape, V, lam, dp, rnnt_type)
                        note(group, mine, yard)
                        lines.append("%d %d %d %d lambda %.2f dp %.2f %-8s | %s | %s" %
                                     (*shape[:3], V, lam, dp, rnnt_type, " ".join("%.3e" % v for v in mine),
                                      " ".join("%.3e" % v for v in yard)))
                        print(lines[-1], flush=True)
    lines.append("# largest per group: the entries with a topology | the yardstick")
    for group, (m, y) in worst.items():
        lines.append("# %s: %s | %s" % (group, " ".join("%.3e" % v for v in m), " ".join("%.3e" % v for v in y)))
    lines.append("YARDSTICK = {")
    for group, (_, y) in worst.items():
        lines.append('    "%s": (%s),' % (group, ", ".join("%.3e" % v for v in y)))
    lines.append("}")
    print("\n".join(lines[-(2 * len(worst) + 3):]), flush=True)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "modified_loss_values.txt"))
    a = p.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    main(a.out)
