#!/usr/bin/env python
"""The errors of the factorised-blank (HAT) loss on the pruned band against fp64 beside those of the softmax pruned loss, over
the cases of tests/test_gpu_pruned_hat.py.

    python tools/pruned_hat_values.py [--out profiles/pruned_hat_loss_values.txt]

Per case: pruned_rnnt_loss_from_logits(..., use_hat_loss=True) against tests/pruned_hat_reference.py, then the yardstick --
the same call without the keyword against tests/modified_reference.py.  The last lines are the maxima with the case they
occurred at: the named constants of the test, whose bars are four times the yardstick's."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch  # noqa: E402

import test_gpu_pruned_hat as tg  # noqa: E402


def main(out):
    lines = ["# N T U S V blank lambda dp topology | HAT cost rel, d/d logits abs | yardstick (softmax) cost rel, d/d logits abs"]
    worst = {}
    for shape, blank in tg.CASES:
        for lam, dp, rnnt_type in tg.AXES:
            where = "(%d, %d, %d, %d, %d), blank %d, lambda %.2f, dp %.1f, %s" % (*shape, blank, lam, dp, rnnt_type)
            hat, yard = tg.errors(shape, blank, lam, dp, rnnt_type, True), tg.errors(shape, blank, lam, dp, rnnt_type, False)
            for name, value in zip(("HAT_COST_REL", "HAT_GRAD_ABS", "YARDSTICK_COST_REL", "YARDSTICK_GRAD_ABS"), hat + yard):
                if value >= worst.get(name, (0.0, ""))[0]:
                    worst[name] = (value, where)
            lines.append("%d %d %d %d %d blank %4d lambda %.2f dp %.1f %-8s | %.3e %.3e | %.3e %.3e" %
                         (*shape, blank, lam, dp, rnnt_type, *hat, *yard))
            print(lines[-1], flush=True)
    lines.append("# largest, and where")
    for name in sorted(worst, reverse=True):
        lines.append("%s = %.3e   # at %s" % (name, *worst[name]))
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "pruned_hat_loss_values.txt"))
    a = p.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    main(a.out)
