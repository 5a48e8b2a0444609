"""The factorised-blank (HAT) loss without a GPU: the two C entries of include/warp_rnnt_amd_hat.h (the argument
lists of the standard logits entries, refusing bad arguments before any HIP call), hat_log_probs in fp64 on the CPU
against the NumPy reference, the reference's own gradient against central differences, and the public function's
signature and argument errors."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import hat_reference as hr
from helpers import make_case

ENTRIES = {"rnnt_amd_hat_loss_logits", "rnnt_amd_hat_logits_backward"}
INVALID, SUCCESS = 5, 0


def _lib():
    import warp_rnnt_amd
    from warp_rnnt_amd import _build
    _build.build()          # hipcc cross-compiles for gfx950 without a GPU; no-op when up to date
    return warp_rnnt_amd.load()


def test_hat_entries_take_the_arguments_of_the_standard_logits_entries_and_their_unit_holds_no_assembly():
    """(What every additive header owes -- declared, bound, exported, a stale library refused: test_host_additive_abi.py.)"""
    from warp_rnnt_amd import _build, _lib as lib
    assert set(lib.HAT_SYMBOLS) == ENTRIES
    # the forward: rnnt_amd_loss_logits without its grads_kind; the backward: the typed dense backward
    full = lib.SYMBOLS["rnnt_amd_loss_logits"][1]
    assert lib.HAT_SYMBOLS["rnnt_amd_hat_loss_logits"][1] == full[:9] + full[10:]
    assert lib.HAT_SYMBOLS["rnnt_amd_hat_logits_backward"][1] == lib.SYMBOLS["rnnt_amd_logits_backward_typed"][1]
    assert "hat.hip" in _build.SOURCES and "hat.hip" not in _build.HAZARD_CHECKED


def test_hat_entries_refuse_before_any_hip_call():
    """Dummy device pointers that are never dereferenced: each call is refused by the host-side check it names."""
    if torch.cuda.is_available():
        pytest.skip("host-only table: replayed where no GPU is visible (its pointers are made up)")
    L = _lib()
    p = ctypes.c_void_p(256)                 # aligned, non-null, never dereferenced

    def fwd(ws=p, dtype=0, logits=p, labels=p, xn=p, yn=p, costs=p, grads=p, N=2, T=3, U=2, V=5, blank=0):
        return L.rnnt_amd_hat_loss_logits(None, ws, dtype, logits, labels, xn, yn, costs, grads, N, T, U, V, blank, 0.0)

    def bwd(dtype=0, logits=p, labels=p, grads=p, go=p, out=p, N=2, T=3, U=2, V=5, blank=0):
        return L.rnnt_amd_hat_logits_backward(None, dtype, logits, labels, grads, go, out, N, T, U, V, blank)

    shared = [dict(dtype=-1), dict(dtype=3), dict(V=1), dict(V=0), dict(blank=5), dict(blank=-1), dict(logits=None),
              dict(labels=None), dict(N=-1), dict(N=70000), dict(T=0), dict(U=0), dict(T=1 << 15, U=1 << 14),
              dict(N=65535, T=1 << 10, U=1 << 7)]
    for kw in shared:
        assert fwd(**kw) == INVALID, kw
        assert bwd(**kw) == INVALID, kw
        # ... whatever else is asked: a refused argument is not answered as an empty batch
        if "N" not in kw:
            assert fwd(N=0, **kw) == INVALID and bwd(N=0, **kw) == INVALID, kw
    for kw in (dict(ws=None), dict(ws=ctypes.c_void_p(264)), dict(costs=None), dict(xn=None), dict(yn=None)):
        assert fwd(**kw) == INVALID, kw
    for kw in (dict(grads=None), dict(out=None), dict(grads=ctypes.c_void_p(260))):
        assert bwd(**kw) == INVALID, kw
    for dtype in (0, 1, 2):
        # no utterances: success without a launch; a column of blanks needs no labels
        assert fwd(dtype=dtype, N=0) == SUCCESS and bwd(dtype=dtype, N=0) == SUCCESS
        assert fwd(dtype=dtype, N=0, grads=None) == SUCCESS
        assert fwd(dtype=dtype, N=0, U=1, labels=None) == SUCCESS and bwd(dtype=dtype, N=0, U=1, labels=None) == SUCCESS
        assert bwd(dtype=dtype, N=0, go=None) == SUCCESS


# ---- hat_log_probs (plain torch) against the NumPy reference, fp64 on the CPU ----

def _z(seed=5, shape=(2, 4, 3, 7)):
    return np.random.RandomState(seed).randn(*shape) * 3.0


@pytest.mark.parametrize("blank", [0, 3, 6])
def test_hat_log_probs_is_the_reference_and_the_shifted_softmax(blank):
    from warp_rnnt_amd.hat import hat_log_probs
    z = _z()
    got = hat_log_probs(torch.tensor(z), blank).numpy()
    assert got.dtype == np.float64
    np.testing.assert_allclose(got, hr.hat_log_probs64(z, blank), rtol=0, atol=1e-12)
    zs = torch.tensor(hr.shifted_logits64(z, blank))
    np.testing.assert_allclose(got, torch.log_softmax(zs, -1).numpy(), rtol=0, atol=1e-12)
    np.testing.assert_allclose(np.exp(got).sum(-1), 1.0, rtol=0, atol=1e-12)


def test_hat_log_probs_over_the_value_range():
    from warp_rnnt_amd.hat import hat_log_probs
    z = _z()
    blank = 2
    keep = np.arange(z.shape[-1]) != blank
    for zb in (80.0, -80.0):
        x = z.copy()
        x[..., blank] = zb
        got = hat_log_probs(torch.tensor(x), blank).numpy()
        assert np.isfinite(got).all()
        np.testing.assert_allclose(got, hr.hat_log_probs64(x, blank), rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(np.exp(got).sum(-1), 1.0, rtol=0, atol=1e-12)
    base = hat_log_probs(torch.tensor(z), blank).numpy()
    for shift in (60000.0, -60000.0):
        x = z.copy()
        x[..., keep] += shift
        got = hat_log_probs(torch.tensor(x), blank).numpy()
        assert np.isfinite(got).all()
        np.testing.assert_allclose(got, base, rtol=0, atol=1e-10)        # (z + 60000 is rounded at 7e-12 in fp64)
    # a masked (-inf) non-blank entry: -inf there, the others as if the column were not there
    x = z.copy()
    x[..., 4] = -np.inf
    got = hat_log_probs(torch.tensor(x), blank).numpy()
    assert np.isneginf(got[..., 4]).all()
    cols = [v for v in range(z.shape[-1]) if v != 4]
    smaller = hat_log_probs(torch.tensor(z[..., cols]), blank).numpy()        # (blank = 2 < 4 keeps its index)
    np.testing.assert_allclose(got[..., cols], smaller, rtol=0, atol=1e-12)
    for bad in (-1, 7):
        with pytest.raises(ValueError, match="blank"):
            hat_log_probs(torch.tensor(z), bad)
    with pytest.raises(ValueError, match="V >= 2"):
        hat_log_probs(torch.zeros(3, 1), 0)


@pytest.mark.parametrize("blank,lam", [(0, 0.0), (2, 0.01), (4, 0.0)])
def test_reference_gradient_against_central_differences(blank, lam):
    """hat_loss64 is what judges the kernels: its d/d z against central differences of its own costs, fp64."""
    N, T, U, V = 2, 4, 3, 5
    logits, labels, xn, yn = make_case(11, N, T, U, V, ragged=True, blank=blank)
    z = logits.astype(np.float64)
    costs, dz = hr.hat_loss64(z, labels, xn, yn, blank, lam)
    assert np.isfinite(costs).all()
    h = 1e-5
    num = np.zeros_like(z)
    for idx in np.ndindex(*z.shape):
        zp, zm = z.copy(), z.copy()
        zp[idx] += h
        zm[idx] -= h
        cp, _ = hr.hat_loss64(zp, labels, xn, yn, blank, lam)
        cm, _ = hr.hat_loss64(zm, labels, xn, yn, blank, lam)
        num[idx] = (cp[idx[0]] - cm[idx[0]]) / (2 * h)
    if lam == 0.0:
        np.testing.assert_allclose(dz, num, rtol=0, atol=1e-6)
    else:
        # FastEmit scales the label gradient and leaves the cost alone: (1 + lam) on the label path, by its definition --
        # checked as the lam = 0 gradient with gL scaled, which central differences of the cost confirm at lam = 0
        _, dz0 = hr.hat_loss64(z, labels, xn, yn, blank, 0.0)
        np.testing.assert_allclose(dz0, num, rtol=0, atol=1e-6)
        assert not np.allclose(dz, dz0)
    for n in range(N):       # zero outside the window
        assert (dz[n, xn[n]:] == 0).all() and (dz[n, :, yn[n] + 1:] == 0).all()


def test_identity_holds_for_the_reference_costs():
    """HAT on z = the standard loss on z' (fp64): the cross-check the GPU tests run against rnnt_loss_from_logits."""
    from oracle import transduce_np
    logits, labels, xn, yn = make_case(3, 2, 6, 4, 9, ragged=True, blank=4)
    costs, _ = hr.hat_loss64(logits, labels, xn, yn, 4)
    lp = transduce_np.log_softmax(hr.shifted_logits64(logits, 4))
    std, _ = transduce_np.transduce_batch(lp, labels, xn, yn, blank=4, fast=True)
    np.testing.assert_allclose(costs, std, rtol=1e-13)


def test_public_signature_and_argument_errors_on_cpu_tensors():
    from warp_rnnt_amd import hat, ops
    params = inspect.signature(hat.hat_loss_from_logits).parameters
    assert list(params) == ["logits", "labels", "frames_lengths", "labels_lengths", "average_frames", "reduction", "blank",
                            "fastemit_lambda"]
    assert [params[k].default for k in list(params)[4:]] == [False, "none", 0, 0.0]
    assert list(inspect.signature(ops.hat_loss).parameters) == ["logits", "labels", "xn", "yn", "blank",
                                                                 "fastemit_lambda", "with_grads"]
    assert list(inspect.signature(ops.hat_logits_backward).parameters) == ["logits", "labels", "grads", "grad_costs", "blank"]
    batch = (torch.zeros((2, 3, 2, 7)), torch.ones((2, 1), dtype=torch.int32), torch.tensor([3, 2], dtype=torch.int32),
             torch.tensor([1, 1], dtype=torch.int32))
    with pytest.raises(AssertionError):
        hat.hat_loss_from_logits(*batch, reduction="avg")
    with pytest.raises(AssertionError):
        hat.hat_loss_from_logits(*batch, blank=1.0)
    # the checks of check_logits_inputs, with their texts: these tensors are not on the GPU
    with pytest.raises(RuntimeError, match="must be located in the CUDA"):
        hat.hat_loss_from_logits(*batch)
    with pytest.raises(RuntimeError, match="ys must be a Int tensor"):
        hat.hat_loss_from_logits(batch[0], batch[1].long(), batch[2], batch[3])
    module = hat.HATLoss(blank=3, fastemit_lambda=0.01, reduction="sum")
    assert isinstance(module, torch.nn.Module)
    assert (module.blank, module.fastemit_lambda, module.reduction) == (3, 0.01, "sum")
    import warp_rnnt_amd
    assert "hat.py" in warp_rnnt_amd.__doc__ and not hasattr(warp_rnnt_amd, "hat_loss_from_logits")
