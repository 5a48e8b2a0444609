#!/usr/bin/env python
"""The errors of ctc_loss_from_logits against float64 beside those of the float32 reference, over the grid of
tests/test_gpu_ctc.py.

    python tools/ctc_loss_values.py [--out profiles/ctc_loss_values.txt]

Per case (L, V, blank, dtype): the kernels' cost and d/d logits errors against torch's ctc_loss in float64 on the CPU
(tests/ctc_reference.py; max |x - ref| / max |ref| over the finite entries, the half types against the reference rounded
to the dtype), then the yardstick's -- the same reference evaluated in float32.  The test's bars are four times the
yardstick's figures of the very case; the last line is the largest ratio of a kernel error to its yardstick."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch  # noqa: E402

import test_gpu_ctc as tg  # noqa: E402


if __name__ == "__main__":
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "ctc_loss_values.txt"))
    a = p.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    lines = ["# L V blank dtype | kernels: cost, grad | fp32 reference (yardstick): cost, grad"]
    worst = 0.0
    for L, V in tg.SHAPES:
        for last_blank in (False, True):
            for name in tg.DTYPES:
                (ref_costs, ref_grad), yard = tg.reference(L, V, last_blank, name)
                e = tg.errors(tg.kernel(L, V, last_blank, name), (ref_costs, ref_grad.to(tg.DTYPES[name])))
                if name == "fp32":
                    worst = max(worst, *(x / max(y, tg.EPS["fp32"]) for x, y in zip(e, yard)))
                lines.append("%3d %4d blank %4d %s | %.3e %.3e | %.3e %.3e" %
                             (L, V, V - 1 if last_blank else 0, name, *e, *yard))
                print(lines[-1], flush=True)
    lines.append("# fp32: the largest kernel error over its yardstick (floored at one fp32 ulp): %.2f" % worst)
    print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
