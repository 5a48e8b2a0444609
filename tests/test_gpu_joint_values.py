"""rnnt_loss_from_joint across the logit VALUE range (joint_values.py: profiles with exact logits, bounds), at
(V, H) = (17, 32), (33, 64), (50, 128), fp32 / bf16 / fp16, N = 3, T = 9, U = 6 with ragged lengths, fastemit 0.01 and
upstream weights -- against joint_reference in fp64, compared as test_gpu_joint_edges.py compares.

(a) plain, bias shifted by +100 / -1000 / +60000, tied rows at 60000 and a masked vocabulary (bias = -inf): the project's
    tolerances, unchanged and not growing with |bias| -- costs 1e-5 |ref| + 1e-6, gradients 1e-4 normwise and 1e-3
    elementwise beyond the output dtype's rounding; masked: everything finite, db and the dW rows exactly 0 at masked entries.
(b) single-cell utterances (T = 1, no labels), where ONE log-softmax row shows through the public API: the cost is
    -lp[blank], and with N = 1 and upstream 1, db = p - e_blank in fp32.  Held to the log-softmax bounds of lsm_values.py:
    tol_j = 4 eps (|z_j - mx| + |lp_j|) + 2e-6 max(1, ln V) on the cost, p_j tol_j + 4 eps on db.
(c) spread (W * 8: peaked rows) and natural (tanh / relu, random data, |z| of a few hundred): the fp32 LATTICE loses digits
    on peaked rows, so the yardstick is the unfused path on the same values -- torch's joint in
    fp32, then rnnt_loss_from_logits (test_gpu_joint.chain) -- against the same fp64 reference: the fused error may be at
    most 4x the chain's plus the tolerance of (a), per tensor over the batch.  For bf16 / fp16 the chain runs in fp32 on the
    upcast values with W rounded as the kernels stage it; the reference models the kernels' rounding of h and dz, which the chain does not do,
    so its yardstick is wider there than at fp32.

Every (profile, dtype, shape) is asserted; every figure is printed before it is asserted (pytest -s).

Measured on the MI355X (tools/joint_value_range.py, profiles/joint_value_range.txt), worst over shapes and dtypes.  The
library before C ABI 110 (the log-normaliser as one float, max + log(sum)) failed 23 of the 45 cases: (a) costs 17x the
tolerance on shift+60000 and 55x on ties, gradients up to 8.5x, shift-1000 outside in fp16 at two shapes, every output NaN on
masked; (b) cost / db 239x / 227x the bound on shift+60000, 213x / 114x on ties, 3.6x / 4.8x on shift-1000, NaN on masked;
(c) passed.  Now: (a) at most 0.025 (costs), 0.05 (gradients) of the tolerances, (b) 0.04 / 0.12 of the bounds, the same
figures at every shift; (c) in fp32 the fused path is at or below the chain's own error."""
import numpy as np
import pytest
import torch

import joint_values as jv
from test_gpu_joint_edges import ATOL_REL, COST_ATOL, COST_RTOL, NORM_TOL, check_all, compare, errors, fused, reference

pytestmark = pytest.mark.gpu
IDS = [f"V{V}_H{H}" for V, H in jv.SHAPES]
N_DB_CELLS = 4          # N = 1 calls per (profile, dtype, shape) for db


def run_fused(c, need="fgwb"):
    return fused(*jv.args(c), c["act"], c["blank"], c["lam"], c["up"], need)


def run_reference(c):
    return reference(*jv.args(c), c["act"], c["blank"], c["lam"], c["up"])


def worst_ratios(outs, refs):
    """error / tolerance of (a), worst over the utterances and tensors: (costs, normwise, elementwise); inf for NaN."""
    cost = jv.cost_ratio(outs[0].double().cpu().numpy(), refs[0].numpy())
    nrm = el = 0.0
    for got, ref in zip(outs[1:], refs[1:]):
        a, b = errors(got, ref)
        nrm, el = max(nrm, np.nan_to_num(a, nan=np.inf) / NORM_TOL), max(el, np.nan_to_num(b, nan=np.inf) / ATOL_REL)
    return cost, nrm, el


@pytest.mark.parametrize("name", jv.EXACT)
@pytest.mark.parametrize("V,H", jv.SHAPES, ids=IDS)
def test_exact_logit_profiles_hold_the_project_tolerances(V, H, name):
    for dname, dtype in jv.DTYPES.items():
        c = jv.case(name, V, H, dtype)
        outs, refs = run_fused(c), run_reference(c)
        tag = f"{name} V{V} H{H} {dname}"
        r = worst_ratios(outs, refs)
        print(f"{tag}: error / tolerance costs {r[0]:.3f}, normwise {r[1]:.3f}, elementwise {r[2]:.3f}")
        if name == "masked":
            m = list(jv.MASKED[V])
            for x in outs:
                assert torch.isfinite(x).all(), tag
            assert torch.count_nonzero(outs[4][m]) == 0 and torch.count_nonzero(outs[3][m]) == 0, tag
        check_all(outs, refs, c["xn"], c["yn"], tag)


@pytest.mark.parametrize("name", jv.EXACT)
@pytest.mark.parametrize("V,H", jv.SHAPES, ids=IDS)
def test_single_cells_hold_the_log_softmax_bounds(V, H, name):
    blank = jv.BLANK[V]
    for dname, dtype in jv.DTYPES.items():
        c = jv.cells(name, V, H, dtype)
        tag = f"{name} V{V} H{H} {dname}"
        z = jv.logits64(c).reshape(-1, V)
        _, lp64, tol = jv.row_bounds(z)
        # sixteen cells in one call: cost = -lp[blank]
        costs = run_fused(c, need="b")[0].double().cpu().numpy()
        r = float(np.nan_to_num(np.abs(costs + lp64[:, blank]) / tol[:, blank], nan=np.inf).max())
        print(f"{tag}: single-cell cost error / bound {r:.3f}")
        assert r <= 1.0, (tag, r)
        # one cell per call, upstream 1: db = p - e_blank
        worst = 0.0
        for i in range(N_DB_CELLS):
            db = run_fused(jv.one_cell(c, i), need="b")[4]
            assert db.dtype == torch.float32
            p = db.double().cpu().numpy().copy()
            p[blank] += 1.0
            worst = max(worst, jv.probability_ratio(p, lp64[i], tol[i]))
        print(f"{tag}: single-cell db error / bound {worst:.3f}")
        assert worst <= 1.0, (tag, worst)


def chain_with_upstream(c):
    """test_gpu_joint.chain -- torch's joint in fp32, then rnnt_loss_from_logits -- on the values of the case (upcast; W
    rounded as the kernels stage it), one utterance per call so that the upstream weights can be applied (chain() takes
    none): costs, df, dg, dW, db in fp64 on the CPU."""
    from test_gpu_joint import chain
    E = c["f"].dtype
    w = c["w"].to(E).float()
    outs = [torch.zeros(jv.N, dtype=torch.float64), torch.zeros(c["f"].shape, dtype=torch.float64),
            torch.zeros(c["g"].shape, dtype=torch.float64), torch.zeros(w.shape, dtype=torch.float64),
            torch.zeros(w.shape[0], dtype=torch.float64)]
    for n in range(jv.N):
        s = slice(n, n + 1)
        r = chain(c["f"][s].float(), c["g"][s].float(), w, c["b"], c["labels"][s], c["xn"][s], c["yn"][s], c["act"],
                  c["blank"], c["lam"])
        r = [x.double().cpu() for x in r]
        up = float(c["up"][n])
        outs[0][n] = r[0][0]
        outs[1][n], outs[2][n] = up * r[1][0], up * r[2][0]
        outs[3] += up * r[3]
        outs[4] += up * r[4]
    return outs


def chain_errors(x, ref):
    """(normwise, elementwise) error of the chain's fp64-accumulated result, as test_gpu_joint_edges.errors takes them
    (fp32 results: no output rounding to set aside)."""
    d = (x - ref).abs()
    return float(d.norm() / ref.norm()), float(d.max() / ref.abs().max())


@pytest.mark.parametrize("name", jv.RELATIVE)
@pytest.mark.parametrize("V,H", jv.SHAPES, ids=IDS)
def test_peaked_rows_against_the_unfused_chain(V, H, name):
    for dname, dtype in jv.DTYPES.items():
        c = jv.case(name, V, H, dtype)
        tag = f"{name} V{V} H{H} {dname}"
        outs, refs, theirs = run_fused(c), run_reference(c), chain_with_upstream(c)
        ours_c = np.abs(outs[0].double().cpu().numpy() - refs[0].numpy())
        chain_c = np.abs(theirs[0].numpy() - refs[0].numpy())
        print(f"{tag}: costs {refs[0].numpy().round(1)}, |error| fused {ours_c.max():.2e}, chain {chain_c.max():.2e}")
        assert (ours_c <= 4 * chain_c + COST_RTOL * np.abs(refs[0].numpy()) + COST_ATOL).all(), (tag, ours_c, chain_c)
        for got, their, ref, what in zip(outs[1:], theirs[1:], refs[1:], ("df", "dg", "dW", "db")):
            assert got.dtype == (dtype if what in ("df", "dg") else torch.float32)
            (on, oe), (cn, ce) = errors(got, ref), chain_errors(their, ref)
            print(f"{tag}: {what} normwise / elementwise fused {on:.2e} / {oe:.2e}, chain {cn:.2e} / {ce:.2e}")
            compare(got, ref, what, tag, norm_tol=4 * cn + NORM_TOL, atol_rel=4 * ce + ATOL_REL)
        for n in range(jv.N):
            assert torch.count_nonzero(outs[1][n, int(c["xn"][n]):]) == 0
            assert torch.count_nonzero(outs[2][n, int(c["yn"][n]) + 1:]) == 0
