"""The value-range profiles and bounds of joint_values.py, checked where no GPU is needed -- in both directions.

The inputs are what they claim: every dyadic profile has logits that are exact in fp32 in any summation order, at every
shape and dtype test_gpu_joint_values.py uses; the fp64 reference does not move under a shift of the bias (costs and every
gradient to 7.3e-12 relative, one fp64 ulp of 60000; measured 1.7e-12); a masked vocabulary leaves it finite with
exactly zero db[v] and dW[v, :] at masked v.

The bounds are honest: torch's own fp32 chain (relu, linear, log_softmax and their autograd in fp32 around the fp64 lattice)
is inside every one of them.  And they can see the defect: the numpy model of the kernels' arithmetic as it was --
lse = max + log(sum) in one fp32 -- is outside them where the row maximum is large, the corrected one inside everywhere.

Measured, worst over the three shapes (error / bound: cost and p on the project's tolerances, 1e-5 |ref| + 1e-6 and 1e-4
normwise over the live cells; lp and p-row on the per-row bounds of lsm_values.py):

    profile       torch fp32 chain            model, lse in one float         model, corrected
                  cost   grads  lp     p-row  cost   p      lp     p-row      cost   p      lp     p-row
    plain         0.003  0.002  0.067  0.032  0.002  0.003  0.098  0.089      0.002  0.001  0.065  0.041
    shift+100     0.003  0.002  0.067  0.032  0.029  0.024  0.65   0.60       0.002  0.001  0.065  0.041
    shift-1000    0.003  0.002  0.067  0.032  0.21   0.19   5.3    5.0        0.002  0.001  0.065  0.041
    shift+60000   0.003  0.002  0.067  0.032  17.1   12.1   341    325        0.002  0.001  0.065  0.041
    ties          0.003  0.001  0.011  0.006  55.2   18.7   213    114        0.003  0.001  0.011  0.006
    masked        0.003  0.001  0.063  0.028  NaN    NaN    NaN    NaN        0.003  0.001  0.072  0.033

The LEAST the old arithmetic is outside, over the shapes, where the test asserts that it is: shift+60000 cost 5.4x, p 11x,
lp 248x, p-row 241x; ties 13.9x, 4.1x, 53x, 26x; shift-1000 lp 3.9x, p-row 3.7x; masked: NaN costs at every shape.
(Every figure is printed by the tests, pytest -s.)"""
import numpy as np
import pytest
import torch

import joint_values as jv
from test_gpu_joint_edges import check_all, errors

SHAPES = jv.SHAPES
IDS = [f"V{V}_H{H}" for V, H in SHAPES]
# The fp64 reference forms lse = max + log(sum) too, in fp64: at max = 60000 that rounds at ulp(60000) = 2^-37 = 7.3e-12, an
# absolute error of every log-prob of the cell and so a relative one of every probability -- and nothing else moves.
SHIFT_TOL = 2.0 ** -37
# where the arithmetic with lse in one float must be OUTSIDE a bound: (profile, figure)
SEES_THE_DEFECT = {"shift+60000": ("cost", "p", "lp", "p-row"), "ties": ("cost", "p", "lp", "p-row"),
                   "shift-1000": ("lp", "p-row"), "masked": ("cost", "p", "lp", "p-row")}


@pytest.mark.parametrize("dname", list(jv.DTYPES))
@pytest.mark.parametrize("name", jv.CLAIMS_EXACT)
@pytest.mark.parametrize("V,H", SHAPES, ids=IDS)
def test_logits_are_exact_in_fp32(V, H, name, dname):
    jv.assert_exact(jv.case(name, V, H, jv.DTYPES[dname]))
    jv.assert_exact(jv.cells(name, V, H, jv.DTYPES[dname]))


def test_exactness_check_sees_an_inexact_case():
    with pytest.raises(AssertionError):
        c = jv.case("plain", 17, 32)
        c["w"] = c["w"] / 3
        jv.assert_exact(c)
    with pytest.raises(AssertionError):
        c = jv.case("shift+60000", 50, 128)
        c["b"] = c["b"] + 10000.0                      # sum |terms| + |bias| reaches 2^16
        jv.assert_exact(c)
    with pytest.raises(AssertionError):
        jv.assert_exact(dict(jv.case("natural-relu", 17, 32), name="plain"))


def test_masked_sets_and_blanks_are_what_the_docstring_says():
    for V, _ in SHAPES:
        m, blank = set(jv.MASKED[V]), jv.BLANK[V]
        assert {0, 4, 8, 12, 6, V - 1} <= m and blank not in m and (V - 1) % 16 != 15
        assert V < 33 or 21 in m
        assert V < 33 or any(all(v in m for v in range(b, b + 16)) for b in range(0, V - 15, 16))
        for name in ("masked", "plain"):
            for c in (jv.case(name, V, 32), jv.cells(name, V, 32)):
                assert not set(c["labels"].reshape(-1).tolist()) & (m | {blank})
    assert [jv.BLANK[V] < 16 for V, _ in SHAPES] == [True, False, False]


@pytest.mark.parametrize("V,H", SHAPES, ids=IDS)
def test_reference_is_shift_invariant(V, H):
    base = jv.reference(jv.case("plain", V, H))
    for name in ("shift+100", "shift-1000", "shift+60000"):
        for got, ref, what in zip(jv.reference(jv.case(name, V, H)), base, ("costs", "df", "dg", "dW", "db")):
            err = float((got - ref).abs().max() / ref.abs().max())
            print(f"V={V} H={H} {name} {what}: relative to the unshifted reference {err:.1e}")
            assert err <= SHIFT_TOL, (name, what, err)


@pytest.mark.parametrize("V,H", SHAPES, ids=IDS)
def test_masked_reference_is_finite_with_exact_zeros(V, H):
    c = jv.case("masked", V, H)
    costs, df, dg, dw, db = jv.reference(c)
    m = list(jv.MASKED[V])
    for x in (costs, df, dg, dw, db):
        assert torch.isfinite(x).all()
    assert torch.count_nonzero(db[m]) == 0 and torch.count_nonzero(dw[m]) == 0
    keep = [v for v in range(V) if v not in m]
    assert torch.count_nonzero(db[keep]) == len(keep) and (dw[keep].abs().sum(1) > 0).all()


def _row_figures(c, lp, p):
    """error / bound of log-probs and probabilities (n,t,u+1,V) of a case on the per-row bounds; inf when -inf is out of
    place or something is not finite."""
    z = jv.logits64(c)
    x64, lp64, tol = jv.row_bounds(z.reshape(-1, z.shape[-1]))
    try:
        return lv_ratio(lp, x64, lp64), jv.probability_ratio(p, lp64, tol)
    except AssertionError:
        return float("inf"), float("inf")


def lv_ratio(lp, x64, lp64):
    return jv.lv.log_prob_ratio(np.asarray(lp, np.float64), x64, lp64)


@pytest.mark.parametrize("name", jv.EXACT)
@pytest.mark.parametrize("V,H", SHAPES, ids=IDS)
def test_torch_fp32_chain_is_inside_every_bound(V, H, name):
    """The reference arithmetic alone passes: the comparison of test_gpu_joint_values.py (a), unchanged, and the per-row
    bounds of (b) under half of their value."""
    c = jv.case(name, V, H)
    outs, refs = jv.torch_chain32(c), jv.reference(c)
    check_all(list(outs), list(refs), c["xn"], c["yn"], f"torch fp32 {name} V{V}")
    worst = max(max(errors(g, r)[0] / jv.NORM_TOL, errors(g, r)[1] / jv.ATOL_REL) for g, r in zip(outs[1:], refs[1:])
                if float(r.abs().max()) > 0)                  # (ties: W = 0, so df = dg = 0, which check_all asserts)
    lp = torch.log_softmax(jv.logits64(c).float(), -1)
    r_lp, r_p = _row_figures(c, lp.numpy(), lp.exp().numpy())
    print(f"V={V} H={H} {name}: torch fp32 chain error / bound: cost {jv.cost_ratio(outs[0], refs[0]):.3f}, "
          f"gradients {worst:.3f}, lp {r_lp:.3f}, p-row {r_p:.3f}")
    assert r_lp < 0.5 and r_p < 0.5, (r_lp, r_p)
    if name == "masked":
        m = list(jv.MASKED[V])
        assert torch.count_nonzero(outs[4][m]) == 0 and torch.count_nonzero(outs[3][m]) == 0


@pytest.mark.parametrize("name", jv.EXACT)
@pytest.mark.parametrize("V,H", SHAPES, ids=IDS)
def test_model_of_the_kernels_both_directions(V, H, name):
    c = jv.case(name, V, H)
    ref_costs = jv.reference(c)[0].numpy()
    p64 = np.exp(jv.lv.reference(jv.logits64(c))[1])
    fig = {}
    for corrected in (False, True):
        costs, lp, p = jv.model_costs(c, corrected)
        live = np.zeros(p64.shape[:3], bool)
        for n in range(p64.shape[0]):
            live[n, :int(c["xn"][n]), :int(c["yn"][n]) + 1] = True
        with np.errstate(invalid="ignore"):
            pn = np.linalg.norm((p.astype(np.float64) - p64)[live]) / np.linalg.norm(p64[live]) / jv.NORM_TOL
        r_lp, r_p = _row_figures(c, lp, p)
        fig[corrected] = dict(zip(("cost", "p", "lp", "p-row"),
                                  (jv.cost_ratio(costs, ref_costs), float(np.nan_to_num(pn, nan=np.inf)), r_lp, r_p)))
        print(f"V={V} H={H} {name}: model {'corrected' if corrected else 'lse in one float'} error / bound: " +
              ", ".join(f"{k} {v:.3g}" for k, v in fig[corrected].items()))
    assert all(v < 0.5 for v in fig[True].values()), fig[True]
    for k in SEES_THE_DEFECT.get(name, ()):
        assert fig[False][k] > 1.0, (k, fig[False])
