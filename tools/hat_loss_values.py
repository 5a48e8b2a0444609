#!/usr/bin/env python
"""The errors of the HAT loss against fp64 beside those of the standard fused loss, over the grid of tests/test_gpu_hat.py.

    python tools/hat_loss_values.py [--out profiles/hat_loss_values.txt]

Per case (shape, blank, fastemit_lambda): HAT's largest cost error relative to the fp64 cost and largest absolute d/d logits
error (tests/hat_reference.py), then the yardstick's -- rnnt_loss_from_logits: its costs on the identity's shifted logits z'
rounded to fp32 against the same fp64 costs, its d/d logits on z against the fp64 standard gradient -- and the distance
between HAT's costs and the standard loss's on z'.  The last lines are the yardstick's maxima: the two constants of the
test, whose bars are four times them."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch  # noqa: E402

import test_gpu_hat as tg  # noqa: E402


if __name__ == "__main__":
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "hat_loss_values.txt"))
    a = p.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    lines = ["# N T U V blank lambda | HAT cost rel, grad abs | standard (yardstick) cost rel, grad abs | HAT vs standard on z'"]
    worst = [0.0, 0.0, 0.0, 0.0]
    for shape, blank in tg.GRID_CASES:
        for lam in tg.LAMS:
            cost, grad, ycost, ygrad, cross = tg.errors(shape, blank, lam)
            worst = [max(w, v) for w, v in zip(worst, (cost, grad, ycost, ygrad))]
            lines.append("%d %d %d %d blank %4d lambda %.2f | %.3e %.3e | %.3e %.3e | %.3e" %
                         (*shape, blank, lam, cost, grad, ycost, ygrad, cross))
            print(lines[-1], flush=True)
    lines.append("# largest: HAT cost rel %.3e grad abs %.3e; yardstick cost rel %.3e grad abs %.3e" % tuple(worst))
    lines.append("YARDSTICK_COST_REL = %.3e" % worst[2])
    lines.append("YARDSTICK_GRAD_ABS = %.3e" % worst[3])
    print("\n".join(lines[-3:]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
