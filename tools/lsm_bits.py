#!/usr/bin/env python
"""One SHA-256 per case of what the log-softmax kernel family (csrc/lsm.h) writes, for whichever library the process loaded
(WARP_RNNT_AMD_LIB, WARP_RNNT_AMD_NO_NATIVE_BINDING=1): run it once per build, each in a process of its own, and compare the
two outputs line for line -- for a change that must not move a bit.

    python tools/lsm_bits.py > bits.txt

A case is (operation, route case, dtype, input profile).  Route cases: the V / alignment pairs of
tests/test_gpu_lsm_routes.py at its 85 rows (N=1, T=17, U=5; the compact map sees the same rows as two utterances of 9 and 8
frames).  Profiles: `plain` and `masked` of tests/lsm_values.py, seeded.  Operations:

    norm, norm+plane              ops.log_softmax without / with the blank plane (the plane: fp32 only); result [+ plane]
    gather dense / compact        the fused logits -> loss call: costs and gradient pairs, which are functions of every pair
                                  the gather kernel stored (no entry hands the gathered pairs out on their own)
    bwd dense / compact, clamp=0 / clamp=0.25
                                  the fused d/d logits from synthetic gradient pairs (lsm_values.pair_gradients)"""
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import lsm_values as lv                                      # noqa: E402
from test_gpu_lsm_routes import CASES, N, TM, UM, ROWS, _place   # noqa: E402

CLAMP = 0.25
COMPACT_XN, COMPACT_YN = (9, 8), (UM - 1, UM - 1)            # 9 * 5 + 8 * 5 = 85 rows


def sha(*tensors):
    h = hashlib.sha256()
    torch.cuda.synchronize()
    for t in tensors:
        h.update(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def main():
    from warp_rnnt_amd import ops
    dev = torch.device("cuda:0")
    assert sum(t * (u + 1) for t, u in zip(COMPACT_XN, COMPACT_YN)) == ROWS
    for V, aligned, *_ in CASES:
        case = "V%d%s" % (V, "" if aligned else "-unaligned")
        rng = np.random.RandomState(V)
        labels = rng.randint(1, V, (N, UM - 1)).astype(np.int32)
        gB, gL, go = lv.pair_gradients(ROWS, V)
        pairs = np.stack([gB, gL], -1).reshape(N, TM, UM, 2)
        tl = torch.tensor(labels, device=dev)
        xn, yn = (torch.tensor([v], dtype=torch.int32, device=dev) for v in (TM, UM - 1))
        up = torch.full((N,), float(go), device=dev)
        g_diag = torch.tensor(lv.to_diagonal(pairs), device=dev)
        # compact: the same rows as two utterances that share the label row
        cys = torch.tensor(np.concatenate([labels[0], labels[0]]), device=dev)
        cxn, cyn = (torch.tensor(v, dtype=torch.int32, device=dev) for v in (COMPACT_XN, COMPACT_YN))
        cup = torch.full((2,), float(go), device=dev)
        g_rows = torch.tensor(pairs.reshape(ROWS, 2), device=dev)
        z = lv.base(ROWS, V, 7000 + V)
        for prof in ("plain", "masked"):
            for name, dtype in lv.DTYPES.items():
                x = _place(lv.profile(prof, z, dtype, keep=labels[0]).view(N, TM, UM, V), aligned)
                x2 = x.view(ROWS, V)

                def line(op, *tensors):
                    print("%-24s %-16s %-4s %-6s %s" % (op, case, name, prof, sha(*tensors)), flush=True)

                if dtype is torch.float32:
                    line("norm", ops.log_softmax(x, blank_plane=False))
                    lp = ops.log_softmax(x, blank_plane=True)
                    line("norm+plane", lp, ops.blank_plane_of(lp, 0))
                else:
                    line("norm", ops.log_softmax(x))
                line("gather dense", *ops.loss(x, tl, xn, yn, ops.IN_LOGITS_DENSE, ops.GRADS_GATHERED_DIAGONAL))
                costs, grads, offs, loffs = ops.loss_compact_logits(x2, cys, cxn, cyn)
                line("gather compact", costs, grads)
                for clamp in (0.0, CLAMP):
                    line("bwd dense clamp=%g" % clamp, ops.logits_backward(x, tl, g_diag, up, 0, clamp=clamp))
                    line("bwd compact clamp=%g" % clamp,
                         ops.compact_logits_backward(x2, cys, cxn, cyn, offs, loffs, g_rows, cup, clamp=clamp))


if __name__ == "__main__":
    main()
