#!/usr/bin/env python
"""The fp32 errors of tdt_loss_from_joint against fp64 beside those of the unfused chain, over the grid of
tests/test_gpu_tdt_joint.py.

    python tools/tdt_joint_values.py [--out profiles/tdt_joint_values.txt]

Per case, sigma and fastemit_lambda: the cost error relative to the fp64 cost and the normwise errors of df, dg, dW and
db -- the chain's (a torch fp32 joint, then tdt_loss_from_logits: the yardstick) and the fused entry's, both against
tests/tdt_joint_reference.py with the upstream gradients 0.5 + 0.25 n.  The last lines are the chain's maxima per quantity
with the case each was reached at: the constants of the test, whose bars are four times them."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch  # noqa: E402

import test_gpu_tdt_joint as tj  # noqa: E402


if __name__ == "__main__":
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "tdt_joint_values.txt"))
    a = p.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    Q = tj.QUANTITIES
    lines = ["# case sigma lambda | chain (yardstick): " + " ".join(Q) + " | fused: " + " ".join(Q)]
    worst = {k: {q: (0.0, "") for q in Q} for k in ("chain", "fused")}
    for case in tj.CASES:
        inputs = tj.make(case)
        for sigma in tj.SIGMAS:
            for lam in tj.LAMS:
                ref = tj.reference(case, sigma, lam)
                e = {"chain": tj.errors(tj.chain(case, inputs, sigma, lam), ref),
                     "fused": tj.errors(tj.fused(case, inputs, sigma, lam), ref)}
                where = "%s sigma %.2f lambda %.2f" % (tj.case_id(case), sigma, lam)
                for k in e:
                    for q in Q:
                        if e[k][q] > worst[k][q][0]:
                            worst[k][q] = (e[k][q], where)
                lines.append(where + " | " + " ".join("%.3e" % e["chain"][q] for q in Q) + " | " +
                             " ".join("%.3e" % e["fused"][q] for q in Q))
                print(lines[-1], flush=True)
    for k in ("chain", "fused"):
        for q in Q:
            lines.append("# largest %s %s: %.3e at %s" % (k, q, *worst[k][q]))
    for q in Q:
        lines.append('YARDSTICK["%s"] = %.3e   # %s; fused: %.3e' % (q, *worst["chain"][q], worst["fused"][q][0]))
    print("\n".join(lines[-3 * len(Q):]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
