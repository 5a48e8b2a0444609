#!/usr/bin/env python
"""Worst error / bound of the log-softmax kernels over the logit value range, on the device: per planned family, profile
and dtype, (a) ops.log_softmax against fp64 under the log-prob bound and (b) ops.logits_backward with synthetic gradient
pairs on every row under the gradient bound (tests/lsm_values.py has profiles, reference and bounds; the cases are those
of tests/test_gpu_lsm_routes.py).  A figure above 1 is outside the bound.
Then, per case and profile, the worst d/d logits error against fp64 autograd (over the three dtypes) of logits -> loss ->
d/d logits two ways: torch.log_softmax in fp32 followed by this library's loss on log-probs, and the fused
rnnt_loss_from_logits -- the first is what sets the tolerance of a profile on which the fp32 LATTICE, not the log-softmax,
loses the digits (tests/test_gpu_lsm_values.py).

    python tools/lsm_value_range.py [> profiles/lsm_value_range.txt]

Another build of the library: WARP_RNNT_AMD_LIB=<path>."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np
import torch

import lsm_values as lv
from helpers import make_case
from test_gpu_lsm_routes import CASES, DEV, DTYPES, LAM, N, ROWS, TM, UM, _fused, _place, _reference
from warp_rnnt_amd import _lib, debug, ops


def main():
    print(f"# {os.path.relpath(_lib.lib_path(), ROOT)}: worst error / bound, {ROWS} rows (N={N}, T={TM}, U={UM})")
    print(f"# {'case':<15}{'families norm/bwd':<20}{'profile':<13}" + "".join(f"{'lsm ' + d:>10}" for d in DTYPES) +
          "".join(f"{'bwd ' + d:>10}" for d in DTYPES))
    for V, aligned, *_ in CASES:
        facts = dict(dtype="f32", rows=ROWS, V=V, aligned=aligned)
        norm = debug.lsm_plan("norm", **facts)
        fam = norm["family"] + ("+" + norm["tail"] if norm["tail"] else "") + "/" + \
            debug.lsm_plan("bwd", T=TM, U=UM, **facts)["family"]
        _, labels, _, _ = make_case(900 + V, N, TM, UM, V, ragged=True)
        z = lv.base(ROWS, V, 900 + V)
        gB, gL, go = lv.pair_gradients(ROWS, V)
        lab = lv.cell_labels(labels[0], TM, UM)
        pairs = np.stack([gB, gL], -1).reshape(N, TM, UM, 2)
        diag = torch.tensor(lv.to_diagonal(pairs), device=DEV)
        tgo, tl = torch.tensor([go], device=DEV), torch.tensor(labels, device=DEV)
        for name in lv.PROFILES:
            fwd, bwd = [], []
            for dtype in DTYPES.values():
                xa = lv.profile(name, z, dtype, keep=np.unique(labels), single=True)
                x64, lp64 = lv.reference(xa)
                lp = ops.log_softmax(_place(xa.float().view(N, TM, UM, V), aligned))
                fwd.append(_figure(lv.log_prob_ratio, lp, x64, lp64))
                xh = lv.profile(name, z, dtype, keep=np.unique(labels))
                x64, lp64 = lv.reference(xh)
                ref, bound = lv.gradient_reference(x64, lp64, gB, gL, go, lab)
                dz = ops.logits_backward(_place(xh.float().view(N, TM, UM, V), aligned), tl, diag, tgo)
                bwd.append(_figure(lv.gradient_ratio, dz, ref, bound, lp64))
            case = f"V={V}" + ("" if aligned else " unaligned")
            print(f"  {case:<15}{fam:<20}{name:<13}" + "".join(f"{v:>10}" for v in fwd + bwd))


def torch_chain(x32, labels, xn, yn, up):
    """costs, d/d logits of torch's fp32 log_softmax followed by the library's loss on log-probs."""
    import warp_rnnt
    z = x32.detach().clone().requires_grad_(True)
    costs = warp_rnnt.rnnt_loss(torch.log_softmax(z, -1), labels, xn, yn, gather=True, fastemit_lambda=LAM)
    costs.backward(up)
    return costs.detach(), z.grad


def chain_table():
    print("# d/d logits of logits -> loss: worst |error| against fp64 autograd over fp32 / bf16 / fp16 values")
    print(f"# {'case':<15}{'profile':<13}{'torch fp32 chain':>18}{'fused':>12}")
    worst = {}
    for V, aligned, *_ in CASES:
        _, labels, xn, yn = make_case(900 + V, N, TM, UM, V, ragged=True)
        z = lv.base(ROWS, V, 900 + V)
        up = np.random.RandomState(V).rand(N).astype(np.float32) + 0.5
        tl, txn, tyn, tup = (torch.tensor(a, device=DEV) for a in (labels, xn, yn, up))
        for name in lv.PROFILES:
            chain = fused = 0.0
            for dtype in DTYPES.values():
                xh = lv.profile(name, z, dtype, keep=np.unique(labels)).view(N, TM, UM, V)
                x32 = _place(xh.float(), aligned)
                _, _, dz64 = _reference(x32, labels, xn, yn, up)
                chain = max(chain, (torch_chain(x32, tl, txn, tyn, tup)[1].double().cpu() - dz64).abs().max().item())
                fused = max(fused, (_fused(x32, tl, txn, tyn, tup)[1].double().cpu() - dz64).abs().max().item())
            case = f"V={V}" + ("" if aligned else " unaligned")
            print(f"  {case:<15}{name:<13}{chain:>18.2e}{fused:>12.2e}")
            w = worst.setdefault(name, [0.0, 0.0])
            w[0], w[1] = max(w[0], chain), max(w[1], fused)
    for name, (chain, fused) in worst.items():
        print(f"  {'worst':<15}{name:<13}{chain:>18.2e}{fused:>12.2e}")


def _figure(fn, *args):
    try:
        return f"{fn(*args):.3f}"
    except AssertionError as e:       # -inf out of place, or something not finite
        return "FAIL:" + str(e).split()[0]


if __name__ == "__main__":
    main()
    chain_table()
