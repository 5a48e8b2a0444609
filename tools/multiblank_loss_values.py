#!/usr/bin/env python
"""The errors of the multi-blank loss against fp64 beside those of the standard fused loss, over the grid of
tests/test_gpu_multiblank.py.

    python tools/multiblank_loss_values.py [--out profiles/multiblank_loss_values.txt]

Per case (shape, big-blank durations, id layout, fastemit_lambda): the yardstick's largest cost error relative to its fp64
cost and largest absolute d/d logits error -- rnnt_loss_from_logits on the same logits, the standard blank as its blank,
against the fp64 standard loss (oracle/transduce_np.py) -- then the multi-blank loss's own two figures against
tests/multiblank_reference.py at sigma = 0 and 0.05.  The last lines are the maxima with the case at which each occurs; the
yardstick's two are the constants of the test, whose bars are four times them."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch  # noqa: E402

import test_gpu_multiblank as tg  # noqa: E402


if __name__ == "__main__":
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "multiblank_loss_values.txt"))
    a = p.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    lines = ["# N T U V big-blank durations layout lambda | standard on the same logits (yardstick) cost rel, grad abs | "
             "multi-blank sigma 0 cost rel, grad abs | multi-blank sigma 0.05 cost rel, grad abs"]
    names = ("yardstick cost rel", "yardstick grad abs", "multi-blank cost rel", "multi-blank grad abs")
    worst = [(0.0, "")] * 4
    for shape, layout in tg.GRID_CASES:
        for lam in tg.LAMS:
            ycost, ygrad = tg.yardstick_errors(shape, layout, lam)
            own = [tg.errors(shape, layout, sigma, lam) for sigma in tg.SIGMAS]
            tag = "%d %d %d %d d%s %-6s lambda %.2f" % (*shape[:4], "".join(map(str, shape[4])) or "none", layout, lam)
            figures = (ycost, ygrad, max(o[0] for o in own), max(o[1] for o in own))
            worst = [max(w, (v, tag)) for w, v in zip(worst, figures)]
            lines.append("%s | %.3e %.3e | %.3e %.3e | %.3e %.3e" % (tag, ycost, ygrad, *own[0], *own[1]))
            print(lines[-1], flush=True)
    for name, (v, tag) in zip(names, worst):
        lines.append("# largest %s: %.3e at %s" % (name, v, tag))
    lines.append("YARDSTICK_COST_REL = %.3e" % worst[0][0])
    lines.append("YARDSTICK_GRAD_ABS = %.3e" % worst[1][0])
    print("\n".join(lines[-6:]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
