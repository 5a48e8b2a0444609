"""The value-range bound of lattice_values.py, checked where no GPU is needed -- in both directions.

The bound is honest: the C oracle, the reference's fp32 arithmetic with libm's expf / log1pf, stays inside it on every profile,
shape and ragged setting of test_gpu_lattice_values.py -- alphas, betas, cost, alpha-side log-likelihood and gradients -- and so
does the numpy model of the kernels' step, at the oracle's distance from fp64.  The bound can see a wrong step: three wrong
variants of the log-sum-exp each leave it on a NAMED profile.  (Loosened by hand, once, to LSE_CONSTANT = 1e4: variant (a)
then passes everywhere -- the constant is what catches it.)  And the fp64 reference itself is held to the closed form of the
ties profile."""
import numpy as np
import pytest

import lattice_values as lv

CASES = [(name, shape, ragged) for name in lv.PROFILES for shape in lv.SHAPES for ragged in (False, True)]
IDS = [f"{name}-{'x'.join(map(str, shape))}-{'ragged' if ragged else 'full'}" for name, shape, ragged in CASES]
RMS_FACTOR, RMS_SLACK = 2.0, 0.01      # two fp32 implementations of one operation order (test_gpu_lattice_values.py)


def _emulate(c, lse):
    """Padded (N, T, U) alphas / betas of the numpy model on the batch of case ``c``."""
    N, T, U, _ = c["pairs"].shape
    al = np.zeros((N, T, U), np.float32)
    be = np.zeros((N, T, U), np.float32)
    for n in range(N):
        Tn, Un = int(c["xn"][n]), int(c["yn"][n]) + 1
        al[n, :Tn, :Un], be[n, :Tn, :Un] = lv.emulate_sweeps(c["pairs"][n], Tn, Un, lse)
    return al, be


@pytest.mark.parametrize("name,shape,ragged", CASES, ids=IDS)
def test_the_oracle_and_the_model_of_the_step_stay_inside_the_bound(name, shape, ragged):
    c = lv.case(name, shape, ragged)
    r = c["oracle_ratios"]
    print(f"{name} {shape} ragged={ragged}: oracle worst/rms " + ", ".join(
        f"{k} {w:.3f}" + ("" if rms is None else f"/{rms:.4f}") for k, (w, rms) in r.items()))
    assert not c["oracle"]["mismatch"].any()
    for k, (worst, _) in r.items():
        assert worst <= 1.0, (k, worst)
    e = lv.batch_ratios(c["refs"], c["xn"], c["yn"], *_emulate(c, lv.lse_kernel), what="model")
    print("    model  worst/rms " + ", ".join(f"{k} {w:.3f}/{rms:.4f}" for k, (w, rms) in e.items()))
    for k, (worst, rms) in e.items():
        assert worst <= 1.0, (k, worst)
        assert rms <= RMS_FACTOR * r[k][1] + RMS_SLACK and r[k][1] <= RMS_FACTOR * rms + RMS_SLACK, (k, rms, r[k][1])


# (variant, the profile that must see it, shape): seeds and shapes are the GPU test's own
TEETH = [(lv.lse_log1p_2m12, "plain", (2, 40, 33)),
         (lv.lse_log1p_2m12, "ties", (2, 40, 33)),
         (lv.lse_cut10, "shift+3", (2, 40, 130)),
         (lv.lse_max, "ties", (2, 40, 33))]


@pytest.mark.parametrize("lse,name,shape", TEETH, ids=[f"{f.__name__}-{n}" for f, n, _ in TEETH])
def test_a_wrong_step_leaves_the_bound_on_its_named_profile(lse, name, shape):
    c = lv.case(name, shape, False)
    good = lv.batch_ratios(c["refs"], c["xn"], c["yn"], *_emulate(c, lv.lse_kernel))
    wrong = lv.batch_ratios(c["refs"], c["xn"], c["yn"], *_emulate(c, lse))
    print(f"{lse.__name__} on {name} {shape}: worst alphas {wrong['alphas'][0]:.3f}, betas {wrong['betas'][0]:.3f} "
          f"(the kernels' step: {good['alphas'][0]:.3f}, {good['betas'][0]:.3f})")
    assert max(good["alphas"][0], good["betas"][0]) <= 1.0
    assert max(wrong["alphas"][0], wrong["betas"][0]) > 1.0


@pytest.mark.parametrize("T,U", [(40, 33), (130, 400), (1100, 70)])
def test_the_reference_gives_the_closed_form_on_ties(T, U):
    r = lv.reference(lv.profile("ties", lv.SEED, T, U), T, U)
    want = lv.ties_alpha(T, U)
    # lgamma to a few ulp of values up to 6e3, and T + U log-sum-exps in fp64
    np.testing.assert_allclose(r["alphas"], want, rtol=0, atol=1e-9)
    # beta[t, u] = alpha[T-1-t, U-1-u] + the final blank, by the symmetry of the profile
    np.testing.assert_allclose(r["betas"], want[::-1, ::-1] + float(lv.NEG_LN2), rtol=0, atol=1e-9)
    assert abs(r["cost"] + want[-1, -1] + float(lv.NEG_LN2)) <= 1e-9


def test_profiles_are_what_the_docstring_says():
    T, U = 40, 33
    p = lv.profile("plain", 3, T, U)
    assert p.dtype == np.float32 and p.shape == (T, U, 2) and (p < 0).all() and p.min() > -12
    np.testing.assert_array_equal(p[:, U - 1, 1], p[:, U - 1, 0])            # the last column's label slot: the blank
    np.testing.assert_array_equal(lv.profile("shift-100", 3, T, U), p - np.float32(100))
    assert (lv.profile("shift+3", 3, T, U) > 0).any()
    assert lv.profile("spread30", 3, T, U).min() < -150
    f = lv.profile("floor-1e4", 3, T, U)
    assert (f[..., 0] == p[..., 0]).all() and 0.2 < (f[..., 1] == -1e4).mean() < 0.4
    q = lv.profile("path", 3, T, U)
    on = q > -1
    assert on.sum() == T + U - 1 and (q[~on] <= -60).all() and on[T - 1, U - 1, 0]
    r = lv.reference(q, T, U)
    assert 0 < r["cost"] < 1
    # ragged batches: utterance 1 is short in both directions, a batch of three carries one utterance without labels
    _, xn, yn = lv.batch("plain", 3, 1030, 129, True)
    assert xn.tolist() == [1030, 343, 1023] and yn.tolist() == [128, 84, 0]
