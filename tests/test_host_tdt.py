"""The token-and-duration (TDT) loss without a GPU: the fp64 reference (tests/tdt_reference.py) against exhaustive path
enumeration and its gradient against central differences, tdt_log_probs against the reference's two softmaxes, the
three C entries of include/warp_rnnt_amd_tdt.h -- every refusal with pointers that are never dereferenced, the workspace
size -- and the public signature."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import tdt_reference as tr

ENTRIES = {"rnnt_amd_tdt_workspace_size", "rnnt_amd_tdt_loss_logits", "rnnt_amd_tdt_logits_backward"}
INVALID, SUCCESS = 5, 0

# (durations, T, U, V): lattices of at most 7 x 4 cells; (0, 1, 8) with T_n < 8: its longest jump never fits
LATTICES = [((0, 1), 6, 4, 3), ((0, 1, 2, 3, 4), 5, 3, 3), ((1, 2), 7, 4, 2), ((2, 0, 1), 6, 3, 4), ((0, 1, 8), 7, 3, 3)]
IDS = ["d" + "".join(map(str, d)) for d, *_ in LATTICES]


def _lib():
    import warp_rnnt_amd
    from warp_rnnt_amd import _build
    _build.build()          # hipcc cross-compiles for gfx950 without a GPU; no-op when up to date
    return warp_rnnt_amd.load()


def small_case(seed, T, U, V, D, blank, lengths):
    """fp64 logits (N,T,U,V+D) with labels that avoid the blank; lengths: the (T_n, U_n) of the batch."""
    rng = np.random.RandomState(seed)
    N = len(lengths)
    z = rng.randn(N, T, U, V + D) * 1.5
    choices = np.array([v for v in range(V) if v != blank], np.int32)
    labels = choices[rng.randint(0, len(choices), size=(N, U - 1))].astype(np.int32)
    xn = np.array([l[0] for l in lengths], np.int32)
    yn = np.array([l[1] for l in lengths], np.int32)
    return z, labels, xn, yn


def _lengths(T, U):
    """A full utterance, a ragged one, one of a single frame, one without labels."""
    return [(T, U - 1), (T - 1, max(U - 2, 0)), (1, 0), (T, 0), (2, 1)]


# ---- the reference ----

@pytest.mark.parametrize("sigma", [0.0, 0.05])
@pytest.mark.parametrize("durations,T,U,V", LATTICES, ids=IDS)
def test_reference_costs_are_the_sum_over_every_path(durations, T, U, V, sigma):
    D = len(durations)
    for blank in range(V):
        z, labels, xn, yn = small_case(10 * V + blank, T, U, V, D, blank, _lengths(T, U))
        costs, _, _ = tr.tdt_loss64(z, labels, xn, yn, durations, blank, sigma)
        tok, dur = tr.tdt_log_probs64(z, D)
        for n in range(len(xn)):
            want = -tr.enumerate_paths(tok[n] - sigma, dur[n], labels[n], int(xn[n]), int(yn[n]), durations, blank)
            assert np.isfinite(want)            # duration 1 is there: every lattice has a path
            assert abs(costs[n] - want) <= 1e-12 * max(1.0, abs(want)), (blank, n, costs[n], want)


@pytest.mark.parametrize("durations,T,U,V", LATTICES, ids=IDS)
def test_reference_gradient_against_central_differences(durations, T, U, V):
    """tdt_loss64 is what judges the kernels: its d/d z against central differences of its own costs, fp64; beta(0,0) is
    the log-likelihood; FastEmit leaves the costs alone and scales the label edges."""
    D = len(durations)
    blank = V // 2
    sigma = 0.05
    z, labels, xn, yn = small_case(3 + V, T, U, V, D, blank, _lengths(T, U)[:3])
    costs, dz, G = tr.tdt_loss64(z, labels, xn, yn, durations, blank, sigma)
    h = 1e-5
    num = np.zeros_like(z)
    for idx in np.ndindex(*z.shape):
        zp, zm = z.copy(), z.copy()
        zp[idx] += h
        zm[idx] -= h
        cp = tr.tdt_loss64(zp, labels, xn, yn, durations, blank, sigma)[0]
        cm = tr.tdt_loss64(zm, labels, xn, yn, durations, blank, sigma)[0]
        num[idx] = (cp[idx[0]] - cm[idx[0]]) / (2 * h)
    np.testing.assert_allclose(dz, num, rtol=0, atol=2e-8)
    tok, dur = tr.tdt_log_probs64(z, D)
    for n in range(len(xn)):
        ll, _, beta, _ = tr.utterance(tok[n] - sigma, dur[n], labels[n], int(xn[n]), int(yn[n]), durations, blank)
        assert abs(beta[0, 0] - ll) <= 1e-12 * max(1.0, abs(ll))
        assert (dz[n, xn[n]:] == 0).all() and (dz[n, :, yn[n] + 1:] == 0).all()
    costs_l, dz_l, G_l = tr.tdt_loss64(z, labels, xn, yn, durations, blank, sigma, lam=0.25)
    assert np.array_equal(costs_l, costs)
    np.testing.assert_allclose(G_l[..., 1], 1.25 * G[..., 1], rtol=1e-14)
    assert np.array_equal(G_l[..., 0], G[..., 0]) and not np.allclose(dz_l, dz)


def test_reference_refuses_lengths_out_of_range_and_takes_masked_logits():
    durations, blank = (0, 1, 2), 1
    z, labels, xn, yn = small_case(1, 5, 3, 4, 3, blank, [(5, 2), (6, 1), (3, 3), (0, 0)])
    costs, dz, G = tr.tdt_loss64(z, labels, xn, yn, durations, blank)
    assert np.isfinite(costs[0]) and np.isnan(costs[1:]).all()
    assert (dz[1:] == 0).all() and (G[1:] == 0).all()
    # a masked token that is no label, and a masked duration other than 1
    unused = [v for v in range(4) if v != blank and v not in set(labels[0].tolist())]
    z[0, ..., unused[0]] = -np.inf
    z[0, ..., 4 + 2] = -np.inf
    costs, dz, _ = tr.tdt_loss64(z, labels, xn, yn, durations, blank)
    assert np.isfinite(costs[0]) and np.isfinite(dz).all()
    assert (dz[0, ..., unused[0]] == 0).all() and (dz[0, ..., 4 + 2] == 0).all()


# ---- tdt_log_probs (plain torch) ----

@pytest.mark.parametrize("D", [1, 2, 5])
def test_tdt_log_probs_are_the_reference_softmaxes(D):
    from warp_rnnt_amd.tdt import tdt_log_probs
    z = np.random.RandomState(D).randn(2, 4, 3, 7 + D) * 3.0
    z[0, 0, 0, 2] = -np.inf
    tok, dur = tdt_log_probs(torch.tensor(z), D, blank=6)
    want_tok, want_dur = tr.tdt_log_probs64(z, D)
    assert tok.dtype == torch.float64 and tok.shape[-1] == 7 and dur.shape[-1] == D
    np.testing.assert_allclose(tok.numpy(), want_tok, rtol=0, atol=1e-12)
    np.testing.assert_allclose(dur.numpy(), want_dur, rtol=0, atol=1e-12)
    np.testing.assert_allclose(np.exp(tok.numpy()).sum(-1), 1.0, rtol=0, atol=1e-12)
    np.testing.assert_allclose(np.exp(dur.numpy()).sum(-1), 1.0, rtol=0, atol=1e-12)
    assert np.isneginf(tok.numpy()[0, 0, 0, 2])
    for kw in (dict(num_durations=0), dict(num_durations=D, blank=7), dict(num_durations=D, blank=-1),
               dict(num_durations=6 + D)):
        with pytest.raises(ValueError, match="tdt_log_probs needs"):
            tdt_log_probs(torch.tensor(z), **kw)


# ---- the C entries ----

def test_tdt_entries_are_the_three_of_the_header_and_their_unit_holds_no_assembly():
    """What is TDT's own; the contract of an additive header holds this family through test_host_additive_abi.py."""
    from warp_rnnt_amd import _build, _lib as lib
    assert set(lib.TDT_SYMBOLS) == ENTRIES
    assert "tdt.hip" in _build.SOURCES and "tdt.hip" not in _build.HAZARD_CHECKED and "tdt.hip" not in _build.RELOAD_CHECKED
    assert "asm" not in re.sub(r"//.*", "", open(os.path.join(_build.CSRC, "tdt.hip")).read())


def _entries():
    L = _lib()
    p = ctypes.c_void_p(256)                 # aligned, non-null, never dereferenced
    good = (ctypes.c_int * 5)(0, 1, 2, 3, 4)

    def fwd(ws=p, dtype=0, logits=p, labels=p, xn=p, yn=p, durations=good, D=5, costs=p, grads=p, N=2, T=3, U=2, V=5,
            blank=0, sigma=0.0):
        if isinstance(durations, (tuple, list)):
            durations = (ctypes.c_int * max(len(durations), 1))(*durations)
        return L.rnnt_amd_tdt_loss_logits(None, ws, dtype, logits, labels, xn, yn, durations, D, costs, grads, N, T, U, V,
                                          blank, sigma, 0.0)

    def bwd(dtype=0, logits=p, labels=p, grads=p, go=p, out=p, N=2, T=3, U=2, V=5, D=5, blank=0):
        return L.rnnt_amd_tdt_logits_backward(None, dtype, logits, labels, grads, go, out, N, T, U, V, D, blank)

    return L, fwd, bwd


def test_tdt_entries_refuse_before_any_hip_call():
    """Dummy device pointers that are never dereferenced: each call is refused by the host-side check it names; what is
    not refused is an empty batch, which succeeds without a launch."""
    if torch.cuda.is_available():
        pytest.skip("host-only table: replayed where no GPU is visible (its pointers are made up)")
    L, fwd, bwd = _entries()
    odd = ctypes.c_void_p(258)
    shared = [dict(dtype=-1), dict(dtype=3), dict(V=1), dict(V=0), dict(blank=5), dict(blank=-1), dict(logits=None),
              dict(labels=None), dict(N=-1), dict(N=70000), dict(T=0), dict(U=0), dict(U=1025), dict(U=1025, T=1),
              dict(T=1 << 20, U=1 << 10), dict(D=0), dict(D=10), dict(logits=ctypes.c_void_p(257)),
              dict(labels=odd)]
    for kw in shared:
        assert fwd(**kw) == INVALID, kw
        assert bwd(**kw) == INVALID, kw
        if "N" not in kw:       # a refused argument is not answered as an empty batch
            assert fwd(N=0, **kw) == INVALID and bwd(N=0, **kw) == INVALID, kw
    # bad durations: no 1, a repeat, out of [0, 8], a null pointer, D that does not fit
    for durations in ((0, 2, 3), (0, 1, 1), (0, 1, 9), (-1, 0, 1), (1, 1)):
        assert fwd(durations=durations, D=len(durations)) == INVALID, durations
    assert fwd(durations=None) == INVALID
    for sigma in (-0.01, float("inf"), float("nan")):
        assert fwd(sigma=sigma) == INVALID, sigma
    for kw in (dict(ws=None), dict(ws=ctypes.c_void_p(264)), dict(costs=None), dict(xn=None), dict(yn=None),
               dict(costs=odd), dict(grads=odd), dict(xn=odd), dict(yn=odd)):
        assert fwd(**kw) == INVALID, kw
    for kw in (dict(grads=None), dict(out=None), dict(grads=odd), dict(go=odd), dict(out=ctypes.c_void_p(257))):
        assert bwd(**kw) == INVALID, kw
    assert fwd(dtype=1, logits=odd, N=0) == SUCCESS and fwd(dtype=0, logits=odd) == INVALID      # two-byte elements
    for dtype in (0, 1, 2):
        assert fwd(dtype=dtype, N=0) == SUCCESS and bwd(dtype=dtype, N=0) == SUCCESS
        assert fwd(dtype=dtype, N=0, grads=None) == SUCCESS
        assert fwd(dtype=dtype, N=0, U=1, labels=None) == SUCCESS and bwd(dtype=dtype, N=0, U=1, labels=None) == SUCCESS
        assert bwd(dtype=dtype, N=0, go=None) == SUCCESS
        assert fwd(dtype=dtype, N=0, U=1024, sigma=0.05) == SUCCESS
    for durations in ((1,), (0, 1), (2, 0, 1), (1, 2), (0, 1, 8), tuple(range(9))):
        assert fwd(durations=durations, D=len(durations), N=0) == SUCCESS, durations


def test_a_lattice_of_1025_columns_is_refused():
    L, fwd, bwd = _entries()
    assert L.rnnt_amd_tdt_workspace_size(1, 4, 1025, 5) == 0 and L.rnnt_amd_tdt_workspace_size(1, 4, 1024, 5) > 0
    if not torch.cuda.is_available():       # (made-up pointers: only where nothing can be launched)
        assert fwd(N=1, T=4, U=1025) == INVALID and bwd(N=1, T=4, U=1025) == INVALID
        assert fwd(N=0, T=4, U=1024) == SUCCESS
    from warp_rnnt_amd import ops
    with pytest.raises(RuntimeError, match="status 5.*unsupported sizes.*U=1025"):
        ops._workspace("cpu", L.rnnt_amd_tdt_workspace_size, "N T U D", 1, 4, 1025, 5)


def test_workspace_size_is_a_function_of_the_shape_and_monotone():
    L = _lib()
    size = L.rnnt_amd_tdt_workspace_size
    assert len(size.argtypes) == 4          # (N, T, U, D) and nothing else
    base = (3, 20, 7, 4)
    assert size(*base) == size(*base) > 0
    # at least the planes the header names: 2 + D channels, alpha, beta
    assert size(*base) >= 4 * 3 * 20 * 7 * (2 + 4 + 2)
    for k, hi in enumerate((40, 200, 1024, 9)):
        sizes = [size(*(base[:k] + (v,) + base[k + 1:])) for v in range(1, hi + 1)]
        assert all(s > 0 for s in sizes), k
        assert all(a <= b for a, b in zip(sizes, sizes[1:])), k
    for bad in ((-1, 20, 7, 4), (3, 0, 7, 4), (3, 20, 0, 4), (3, 20, 7, 0), (3, 20, 7, 10), (3, 20, 1025, 4), (70000, 20, 7, 4)):
        assert size(*bad) == 0, bad


# ---- Python ----

def test_public_signature_and_argument_errors_on_cpu_tensors():
    from warp_rnnt_amd import ops, tdt
    params = inspect.signature(tdt.tdt_loss_from_logits).parameters
    assert list(params) == ["logits", "labels", "frames_lengths", "labels_lengths", "durations", "sigma", "blank",
                            "fastemit_lambda", "average_frames", "reduction"]
    assert [params[k].default for k in list(params)[4:]] == [(0, 1, 2, 3, 4), 0.0, 0, 0.0, False, "none"]
    assert list(inspect.signature(ops.tdt_loss).parameters) == ["logits", "labels", "xn", "yn", "durations", "blank",
                                                                 "sigma", "fastemit_lambda", "with_grads"]
    assert list(inspect.signature(ops.tdt_logits_backward).parameters) == ["logits", "labels", "grads", "grad_costs",
                                                                            "num_durations", "blank"]
    assert list(inspect.signature(tdt.tdt_log_probs).parameters) == ["logits", "num_durations", "blank"]
    batch = (torch.zeros((2, 3, 2, 7 + 5)), torch.ones((2, 1), dtype=torch.int32), torch.tensor([3, 2], dtype=torch.int32),
             torch.tensor([1, 1], dtype=torch.int32))
    with pytest.raises(AssertionError):
        tdt.tdt_loss_from_logits(*batch, reduction="avg")
    with pytest.raises(AssertionError):
        tdt.tdt_loss_from_logits(*batch, blank=1.0)
    with pytest.raises(RuntimeError, match="must be located in the CUDA"):
        tdt.tdt_loss_from_logits(*batch)
    with pytest.raises(RuntimeError, match="ys must be a Int tensor"):
        tdt.tdt_loss_from_logits(batch[0], batch[1].long(), batch[2], batch[3])
    # what depends on values is refused with its reason before anything touches the device
    for durations in ((0, 2), (0, 1, 1), (1, 9), ()):
        with pytest.raises(RuntimeError, match="status 5.*durations"):
            ops._tdt_check(7, len(durations), 0, durations, 0.0)
    for V, blank in ((1, 0), (7, 7), (7, -1)):
        with pytest.raises(RuntimeError, match="status 5.*blank"):
            ops._tdt_check(V, 2, blank, (0, 1), 0.0)
    for sigma in (-1.0, float("nan"), float("inf")):
        with pytest.raises(RuntimeError, match="status 5.*sigma"):
            ops._tdt_check(7, 2, 0, (0, 1), sigma)
    assert ops._tdt_check(7, 3, 6, (2, 0, 1), 0.05) == [2, 0, 1]
    module = tdt.TDTLoss(durations=[0, 1, 2], sigma=0.05, blank=6, fastemit_lambda=0.01, reduction="sum")
    assert isinstance(module, torch.nn.Module)
    assert (module.durations, module.sigma, module.blank, module.fastemit_lambda, module.reduction) == \
        ((0, 1, 2), 0.05, 6, 0.01, "sum")
    for word in ("omega", "clamp", "mismatch guard", "compact layout", "joint entry", "U > 1024"):
        assert word in tdt.tdt_loss_from_logits.__doc__ or word in tdt.__doc__, word
    import warp_rnnt_amd
    assert "tdt.py" in warp_rnnt_amd.__doc__ and not hasattr(warp_rnnt_amd, "tdt_loss_from_logits")
