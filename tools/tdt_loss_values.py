#!/usr/bin/env python
"""The errors of the TDT loss against fp64 beside those of the standard fused loss, over the grid of tests/test_gpu_tdt.py.

    python tools/tdt_loss_values.py [--out profiles/tdt_loss_values.txt]

Per case (shape, durations, blank, fastemit_lambda): the yardstick's largest cost error relative to its fp64 cost and
largest absolute d/d logits error -- rnnt_loss_from_logits on the token slice z[..., :V] against the fp64 standard loss
(oracle/transduce_np.py) -- then TDT's own two figures against tests/tdt_reference.py at sigma = 0 and 0.05.  The last
lines are the yardstick's maxima: the two constants of the test, whose bars are four times them."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch  # noqa: E402

import test_gpu_tdt as tg  # noqa: E402


if __name__ == "__main__":
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "tdt_loss_values.txt"))
    a = p.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    lines = ["# N T U V durations blank lambda | standard on z[..., :V] (yardstick) cost rel, grad abs | "
             "TDT sigma 0 cost rel, grad abs | TDT sigma 0.05 cost rel, grad abs"]
    worst = [0.0, 0.0, 0.0, 0.0]
    for shape, blank in tg.GRID_CASES:
        for lam in tg.LAMS:
            ycost, ygrad = tg.yardstick_errors(shape, blank, lam)
            own = [tg.errors(shape, blank, sigma, lam) for sigma in tg.SIGMAS]
            worst = [max(w, v) for w, v in zip(worst, (ycost, ygrad, max(o[0] for o in own), max(o[1] for o in own)))]
            lines.append("%d %d %d %d d%s blank %4d lambda %.2f | %.3e %.3e | %.3e %.3e | %.3e %.3e" %
                         (*shape[:4], "".join(map(str, shape[4])), blank, lam, ycost, ygrad, *own[0], *own[1]))
            print(lines[-1], flush=True)
    lines.append("# largest: yardstick cost rel %.3e grad abs %.3e; TDT cost rel %.3e grad abs %.3e" % tuple(worst))
    lines.append("YARDSTICK_COST_REL = %.3e" % worst[0])
    lines.append("YARDSTICK_GRAD_ABS = %.3e" % worst[1])
    print("\n".join(lines[-3:]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
