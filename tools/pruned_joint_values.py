#!/usr/bin/env python
"""The errors of pruned_rnnt_loss_from_joint against fp64 beside those of the unfused chain, over the grid of
tests/test_gpu_pruned_joint.py.

    python tools/pruned_joint_values.py [--out profiles/pruned_joint_values.txt]

Per dtype, case and fastemit_lambda: the cost error relative to the fp64 cost and the normwise errors of df, dg, dW and db --
the chain's (prune_joint_inputs, a torch joint, under autocast for half inputs, then pruned_rnnt_loss_from_logits: the
yardstick) and the fused entry's, both against tests/pruned_joint_reference.py with the upstream gradients 0.5 + 0.25 n.
The last lines are the chain's maxima per dtype and quantity with the case each was reached at: the constants of the test,
whose bars are four times them."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch  # noqa: E402

import test_gpu_pruned_joint as pj  # noqa: E402


if __name__ == "__main__":
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "pruned_joint_values.txt"))
    a = p.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    Q = pj.QUANTITIES
    lines = ["# dtype case lambda | chain (yardstick): " + " ".join(Q) + " | fused: " + " ".join(Q)]
    tail = []
    for name, dtype in pj.DTYPES.items():
        worst = {k: {q: (0.0, "") for q in Q} for k in ("chain", "fused")}
        for case in (pj.CASES if name == "fp32" else pj.HALF_CASES):
            inputs = pj.make(case, dtype)
            for lam in pj.LAMS:
                ref = pj.reference(case, lam, dtype)
                e = {"chain": pj.errors(pj.chain(case, inputs, lam, None if name == "fp32" else dtype), ref),
                     "fused": pj.errors(pj.fused(case, inputs, lam), ref)}
                where = "%s lambda %.2f" % (pj.case_id(case), lam)
                for k in e:
                    for q in Q:
                        if e[k][q] > worst[k][q][0]:
                            worst[k][q] = (e[k][q], where)
                lines.append(name + " " + where + " | " + " ".join("%.3e" % e["chain"][q] for q in Q) + " | " +
                             " ".join("%.3e" % e["fused"][q] for q in Q))
                print(lines[-1], flush=True)
        for q in Q:
            tail.append('YARDSTICK["%s"]["%s"] = %.3e   # at %s; the fused entry\'s largest: %.3e at %s' %
                        (name, q, *worst["chain"][q], *worst["fused"][q]))
    print("\n".join(tail), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines + tail) + "\n")
