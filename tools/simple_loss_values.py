#!/usr/bin/env python
"""The errors of the fused simple transducer loss against fp64 beside those of the unfused chain, over the grid of
tests/test_gpu_simple.py.

    python tools/simple_loss_values.py [--out profiles/simple_loss_values.txt]

Per case (shape (N,T,U,V), blank, (lm_only_scale, am_only_scale), fastemit_lambda): the fused entry's largest cost error
relative to the fp64 cost and largest absolute errors of the gradient pairs, d am, d lm with q held fixed and d lm through
the batch unigram (tests/simple_reference.py: simple_loss64), then the same five figures of the yardstick -- chain32, the
same definition in plain fp32 torch with warp_rnnt.rnnt_loss(blank=-1) and autograd behind it, on the same inputs -- and
the sweep kernel the fused call ran.  The last lines are the yardstick's maxima per shape: the constants of the test, whose
bars are four times them."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch  # noqa: E402

import test_gpu_simple as tg  # noqa: E402


if __name__ == "__main__":
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "simple_loss_values.txt"))
    a = p.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    lines = ["# N T U V blank scales lambda | fused: " + ", ".join(tg.FIGURES) + " | chain32 (yardstick): the same five | "
             "sweep kernel"]
    worst_f, worst_y = {}, {}          # per shape: the five maxima
    for shape, blank in tg.GRID_CASES:
        for k, scales in enumerate(tg.SCALES):
            lam = tg.lam_of(k, tg.blanks_of(shape[3]).index(blank))
            got, yard, kernel = tg.errors(shape, blank, scales, lam)
            worst_f[shape] = [max(w, v) for w, v in zip(worst_f.get(shape, [0.0] * 5), got)]
            worst_y[shape] = [max(w, v) for w, v in zip(worst_y.get(shape, [0.0] * 5), yard)]
            lines.append("%d %d %d %d blank %4d scales (%.2f, %.2f) lambda %.2f | %s | %s | %s" %
                         (*shape, blank, *scales, lam, " ".join("%.3e" % v for v in got),
                          " ".join("%.3e" % v for v in yard), kernel))
            print(lines[-1], flush=True)
    tail = len(lines)
    lines.append("# per shape, the largest of each figure over blanks, scales and lambdas: fused | yardstick | the largest "
                 "fused / (4 x yardstick) of the five")
    for shape in tg.GRID:
        f, y = worst_f[shape], worst_y[shape]
        lines.append("# %s | %s | %s | %.2f" % (shape, " ".join("%.3e" % v for v in f), " ".join("%.3e" % v for v in y),
                                               max(a / (4 * b) for a, b in zip(f, y))))
    lines.append("YARDSTICK = {")
    for shape in tg.GRID:
        lines.append("    %s: (%s)," % (shape, ", ".join("%.3e" % v for v in worst_y[shape])))
    lines.append("}")
    print("\n".join(lines[tail:]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
