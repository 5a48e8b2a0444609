#!/usr/bin/env python
"""Worst error / bound of rnnt_loss_from_joint over the logit value range, on the device (tests/joint_values.py has the
profiles and bounds; the cases are those of tests/test_gpu_joint_values.py): per profile and dtype, worst over the three
(V, H) shapes, for the fused path and for the unfused chain (torch's joint in fp32, then rnnt_loss_from_logits) on the same
values, both against tests/joint_reference.py in fp64:

  costs               |error| / (1e-5 |ref| + 1e-6)
  df dg dW db         the larger of normwise error / 1e-4 and elementwise error / 1e-3, beyond the output dtype's rounding
  cell, cell-db       (fused only) single-cell utterances: the cost, -lp[blank] of one log-softmax row, and db = p - e_blank
                      against the log-softmax bounds of tests/lsm_values.py

A figure above 1 is outside the bound; nan / inf is a result that is not finite.  On the peaked profiles (spread, natural-*)
the fp32 lattice itself loses digits: there the test holds the fused path to 4x the chain's error plus the tolerance, and
the table shows both.

    python tools/joint_value_range.py [> profiles/joint_value_range.txt]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np
import torch

import joint_values as jv
from test_gpu_joint_edges import ATOL_REL, NORM_TOL, errors
from test_gpu_joint_values import N_DB_CELLS, chain_errors, chain_with_upstream, run_fused, run_reference
from warp_rnnt_amd import _lib

OUTPUTS = ("costs", "df", "dg", "dW", "db")


def ratios(outs, refs, err):
    out = [jv.cost_ratio(outs[0].double().cpu().numpy(), refs[0].numpy())]
    for got, ref in zip(outs[1:], refs[1:]):
        if float(ref.abs().max()) == 0.0:
            out.append(0.0 if torch.count_nonzero(got) == 0 else float("inf"))
            continue
        n, e = err(got, ref)
        out.append(max(n / NORM_TOL, e / ATOL_REL))
    return out


def cell_ratios(name, V, H, dtype):
    blank = jv.BLANK[V]
    c = jv.cells(name, V, H, dtype)
    _, lp64, tol = jv.row_bounds(jv.logits64(c).reshape(-1, V))
    costs = run_fused(c, need="b")[0].double().cpu().numpy()
    with np.errstate(invalid="ignore"):
        rc = float(np.nan_to_num(np.abs(costs + lp64[:, blank]) / tol[:, blank], nan=np.inf).max())
    rd = 0.0
    for i in range(N_DB_CELLS):
        p = run_fused(jv.one_cell(c, i), need="b")[4].double().cpu().numpy().copy()
        p[blank] += 1.0
        try:
            rd = max(rd, jv.probability_ratio(p, lp64[i], tol[i]))
        except AssertionError:
            rd = float("inf")
    return rc, rd


def fmt(v):
    return f"{v:>9.3g}" if np.isfinite(v) else f"{'nan':>9}"


def main():
    print(f"# {os.path.relpath(_lib.lib_path(), ROOT)} (C ABI {_lib.load().rnnt_amd_version()}): worst error / bound over "
          f"(V, H) = {jv.SHAPES}, N={jv.N}, T={jv.T}, U={jv.U}")
    print(f"# {'profile':<14}{'dtype':<6}{'path':<7}" + "".join(f"{o:>9}" for o in OUTPUTS + ("cell", "cell-db")))
    for name in jv.EXACT + jv.RELATIVE:
        for dname, dtype in jv.DTYPES.items():
            ours, theirs, cell = np.zeros(5), np.zeros(5), np.zeros(2)
            for V, H in jv.SHAPES:
                c = jv.case(name, V, H, dtype)
                refs = run_reference(c)
                with np.errstate(invalid="ignore"):
                    ours = np.fmax(ours, np.nan_to_num(ratios(run_fused(c), refs, errors), nan=np.inf))
                    theirs = np.fmax(theirs, np.nan_to_num(ratios(chain_with_upstream(c), refs, chain_errors), nan=np.inf))
                if name in jv.EXACT:
                    cell = np.fmax(cell, cell_ratios(name, V, H, dtype))
            tail = "".join(fmt(v) for v in cell) if name in jv.EXACT else ""
            print(f"  {name:<14}{dname:<6}{'fused':<7}" + "".join(fmt(v) for v in ours) + tail)
            print(f"  {name:<14}{dname:<6}{'chain':<7}" + "".join(fmt(v) for v in theirs), flush=True)


if __name__ == "__main__":
    main()
