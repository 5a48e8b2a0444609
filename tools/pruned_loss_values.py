#!/usr/bin/env python
"""The errors of the pruned transducer loss against fp64 beside those of the standard fused loss, over the grid of
tests/test_gpu_pruned.py.

    python tools/pruned_loss_values.py [--out profiles/pruned_loss_values.txt]

Per case (shape (N,T,U,S,V), blank, fastemit_lambda): the pruned loss's largest cost error relative to the fp64 cost and
largest absolute d/d logits error (tests/pruned_reference.py: the band recursion with true -inf outside the band), then the
yardstick's -- rnnt_loss_from_logits on dense (N,T,U,V) logits of the same generator, shapes and lengths against the fp64
standard loss -- and the sweep kernel the pruned call ran.  The last lines are the yardstick's maxima: the two constants of
the test, whose bars are four times them."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch  # noqa: E402

import test_gpu_pruned as tg  # noqa: E402


if __name__ == "__main__":
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "pruned_loss_values.txt"))
    a = p.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    lines = ["# N T U S V blank lambda | pruned cost rel, grad abs | standard (yardstick) cost rel, grad abs | sweep kernel"]
    worst = [0.0, 0.0, 0.0, 0.0]
    for shape, blank in tg.GRID_CASES:
        for lam in tg.LAMS:
            cost, grad, ycost, ygrad, kernel = tg.errors(shape, blank, lam)
            worst = [max(w, v) for w, v in zip(worst, (cost, grad, ycost, ygrad))]
            lines.append("%d %d %d %d %d blank %4d lambda %.2f | %.3e %.3e | %.3e %.3e | %s" %
                         (*shape, blank, lam, cost, grad, ycost, ygrad, kernel))
            print(lines[-1], flush=True)
    lines.append("# largest: pruned cost rel %.3e grad abs %.3e; yardstick cost rel %.3e grad abs %.3e" % tuple(worst))
    lines.append("YARDSTICK_COST_REL = %.3e" % worst[2])
    lines.append("YARDSTICK_GRAD_ABS = %.3e" % worst[3])
    print("\n".join(lines[-3:]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
