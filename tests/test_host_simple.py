"""The smoothed simple transducer loss without a GPU: the fp64 reference (tests/simple_reference.py) against enumeration of
all paths and central differences (d q and nonzero scales included); scales (0,0) reproduce pruned.simple_pairs; the batch
unigram against a loop; the plain-torch yardstick's pairs against the fp64 ones; the C entries' refusals with pointers that
are never dereferenced; the additive contract of include/warp_rnnt_amd_simple.h and its table; the front end's signature
and argument errors."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import simple_reference as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "warp_rnnt_amd_simple.h"
ENTRIES = {"rnnt_amd_simple_workspace_size", "rnnt_amd_simple_loss", "rnnt_amd_simple_backward"}
INVALID, SUCCESS = 5, 0
SCALES = [(0.0, 0.0), (0.25, 0.0), (0.25, 0.1), (0.6, 0.4), (0.0, 0.3)]


def _lib():
    import warp_rnnt_amd
    from warp_rnnt_amd import _build
    _build.build()          # hipcc cross-compiles for gfx950 without a GPU; no-op when up to date
    return warp_rnnt_amd.load()


# ---- the reference ----

@pytest.mark.parametrize("T,U", [(4, 4), (4, 3), (3, 4), (2, 3), (1, 1), (4, 1), (1, 4)])
def test_reference_against_enumeration_of_all_paths(T, U):
    N, V, blank = 3, 4, 1
    am, lm, labels, xn, yn = sr.make_case(10 * T + U, N, T, U, V, blank=blank)
    for c1, c2 in SCALES:
        ref = sr.simple_loss64(am, lm, labels, xn, yn, blank, c1, c2)
        for n in range(N):
            want = sr.brute_force_cost(ref["pairs"][n], int(xn[n]), int(yn[n]) + 1)
            print(f"T{T} U{U} scales {(c1, c2)} utterance {n}: {ref['costs'][n]:.12f} enumeration {want:.12f}")
            assert np.isfinite(want)
            np.testing.assert_allclose(ref["costs"][n], want, rtol=1e-13)


def test_reference_pairs_are_the_dense_definition():
    """pairs64 against the (N,T,U,V) tensors it avoids: log_softmax(am + lm), log_softmax(lm), log_softmax(am + q)."""
    N, T, U, V, blank = 2, 5, 4, 6, 2
    am, lm, labels, xn, yn = sr.make_case(3, N, T, U, V, blank=blank)
    labels[0, 1] = -7                                                     # outside [0,V): the blank
    q = sr.log_unigram64(lm)
    np.testing.assert_allclose(np.exp(q).sum(), 1.0, rtol=1e-12)
    c0, c1, c2 = sr.scales(0.25, 0.1)
    got = sr.pairs64(am, lm, labels, blank, 0.25, 0.1, q)
    a, l = am.astype(np.float64), lm.astype(np.float64)
    joint = torch.log_softmax(torch.tensor(a[:, :, None, :] + l[:, None, :, :]), -1).numpy()
    lmo = torch.log_softmax(torch.tensor(l), -1).numpy()
    amo = torch.log_softmax(torch.tensor(a + q), -1).numpy()
    for n in range(N):
        for t in range(T):
            for u in range(U):
                y = labels[n, u] if u < U - 1 and 0 <= labels[n, u] < V else blank
                for ch, s in ((0, blank), (1, y)):
                    want = c0 * joint[n, t, u, s] + c1 * lmo[n, u, s] + c2 * amo[n, t, s]
                    assert abs(got[n, t, u, ch] - want) < 1e-12, (n, t, u, ch)


@pytest.mark.parametrize("blank,lam,c1,c2", [(0, 0.0, 0.0, 0.0), (2, 0.01, 0.25, 0.0), (4, 0.0, 0.25, 0.1), (1, 0.0, 0.6, 0.4),
                                             (3, 0.0, 0.0, 0.3)])
def test_reference_gradients_against_central_differences(blank, lam, c1, c2):
    """simple_loss64 is what judges the kernels: its d am, d lm (q held fixed), d q and d lm through q against central
    differences of its own costs."""
    N, T, U, V = 2, 4, 4, 5
    am, lm, labels, xn, yn = sr.make_case(21 + blank, N, T, U, V, blank=blank, scale=1.0)
    a, l = am.astype(np.float64), lm.astype(np.float64)
    go = sr.upstream(N)
    q = sr.log_unigram64(l) + 0.1 * np.arange(V) if c2 else None      # (any q: the d q formula does not need a distribution)
    ref = sr.simple_loss64(a, l, labels, xn, yn, blank, c1, c2, lam, q=q)
    ref0 = sr.simple_loss64(a, l, labels, xn, yn, blank, c1, c2, 0.0, q=q)
    h = 1e-5

    def cost(aa, ll, qq):
        return float((go * sr.simple_loss64(aa, ll, labels, xn, yn, blank, c1, c2, 0.0, q=qq)["costs"]).sum())

    def numeric(x, f):
        out = np.zeros_like(x)
        for idx in np.ndindex(*x.shape):
            xp, xm = x.copy(), x.copy()
            xp[idx] += h
            xm[idx] -= h
            out[idx] = (f(xp) - f(xm)) / (2 * h)
        return out

    # FastEmit scales the label gradient and leaves the cost alone: the lam = 0 gradient is the cost's derivative
    np.testing.assert_allclose(ref0["dam"], numeric(a, lambda x: cost(x, l, q)), rtol=0, atol=1e-6)
    np.testing.assert_allclose(ref0["dlm"], numeric(l, lambda x: cost(a, x, q)), rtol=0, atol=1e-6)
    if c2:
        np.testing.assert_allclose(ref0["dq"], numeric(q, lambda x: cost(a, l, x)), rtol=0, atol=1e-6)
        # ... and with q the batch unigram of lm, the total derivative
        tot = sr.simple_loss64(a, l, labels, xn, yn, blank, c1, c2, 0.0)
        num = numeric(l, lambda x: cost(a, x, sr.log_unigram64(x)))
        np.testing.assert_allclose(tot["dlm_total"], num, rtol=0, atol=1e-6)
        assert not np.allclose(tot["dlm_total"], tot["dlm"], atol=1e-6)
    else:
        assert (ref0["dq"] == 0).all() and np.array_equal(ref0["dlm_total"], ref0["dlm"])
    if lam:
        np.testing.assert_allclose(ref["pair_grads"][..., 1], (1.0 + lam) * ref0["pair_grads"][..., 1], rtol=1e-14)
        np.testing.assert_array_equal(ref["pair_grads"][..., 0], ref0["pair_grads"][..., 0])
    # zero outside the windows, not inside
    for n in range(N):
        assert (ref["dam"][n, xn[n]:] == 0).all() and (ref["dlm"][n, yn[n] + 1:] == 0).all()
        assert (ref["dam"][n, :xn[n]] != 0).any() and (ref["dlm"][n, :yn[n] + 1] != 0).any()


@pytest.mark.parametrize("blank", [0, 3])
def test_scales_zero_reproduce_simple_pairs(blank):
    from warp_rnnt_amd.pruned import simple_pairs
    N, T, U, V = 2, 6, 4, 7
    am, lm, labels, xn, yn = sr.make_case(5, N, T, U, V, blank=blank)
    labels[0, 1] = -7
    a, l = torch.tensor(am, dtype=torch.float64), torch.tensor(lm, dtype=torch.float64)
    want = simple_pairs(a, l, torch.tensor(labels), blank).numpy()
    np.testing.assert_allclose(sr.pairs64(am, lm, labels, blank), want, rtol=0, atol=1e-12)
    # the yardstick's torch form: the very same tensor at scales (0,0), and the fp64 definition at the others
    got = sr.pairs32(a, l, torch.tensor(labels), blank)
    np.testing.assert_allclose(got.numpy(), want, rtol=0, atol=1e-12)
    for c1, c2 in SCALES[1:]:
        q = sr.log_unigram32(l).double()
        got = sr.pairs32(a, l, torch.tensor(labels), blank, c1, c2, q if c2 else None)
        np.testing.assert_allclose(got.numpy(), sr.pairs64(am, lm, labels, blank, c1, c2, q.numpy() if c2 else None),
                                   rtol=0, atol=1e-11)


def test_batch_log_unigram_against_a_loop():
    from warp_rnnt_amd.simple import batch_log_unigram
    gen = torch.Generator().manual_seed(7)
    N, U, V = 3, 5, 6
    lm = torch.randn(N, U, V, generator=gen) * 2
    want = np.zeros(V)
    for n in range(N):
        for u in range(U):
            row = lm[n, u].double().numpy()
            want += np.exp(row - row.max()) / np.exp(row - row.max()).sum()
    want = np.log(want / (N * U) + sr.TINY)
    got = batch_log_unigram(lm)
    assert got.dtype == torch.float32 and tuple(got.shape) == (V,)
    np.testing.assert_allclose(got.numpy(), want, rtol=0, atol=1e-6)
    np.testing.assert_allclose(sr.log_unigram64(lm.numpy()), want, rtol=0, atol=1e-13)
    assert torch.equal(batch_log_unigram(lm.bfloat16()), batch_log_unigram(lm.bfloat16().float()))     # fp32 arithmetic
    x = lm.clone().requires_grad_(True)
    batch_log_unigram(x)[2].backward()                                                                 # differentiable
    assert torch.isfinite(x.grad).all() and (x.grad != 0).any()


# ---- the C entries ----

def test_entries_refuse_before_any_hip_call():
    """Dummy device pointers that are never dereferenced: each call is refused by the host-side check it names."""
    if torch.cuda.is_available():
        pytest.skip("host-only table: replayed where no GPU is visible (its pointers are made up)")
    L = _lib()
    p = ctypes.c_void_p(256)                 # aligned, non-null, never dereferenced
    odd2, odd4 = ctypes.c_void_p(258), ctypes.c_void_p(260)

    def fwd(ws=p, dtype=0, am=p, lm=p, q=p, labels=p, xn=p, yn=p, costs=p, grads=p, znorm=p, N=2, T=3, U=4, V=5, blank=0,
            c1=0.25, c2=0.0):
        return L.rnnt_amd_simple_loss(None, ws, dtype, am, lm, q, labels, xn, yn, costs, grads, znorm, N, T, U, V, blank,
                                      c1, c2, 0.0)

    def bwd(ws=p, dtype=0, am=p, lm=p, q=p, labels=p, xn=p, yn=p, grads=p, znorm=p, go=p, dam=p, dlm=p, dq=p, N=2, T=3,
            U=4, V=5, blank=0, c1=0.25, c2=0.0):
        return L.rnnt_amd_simple_backward(None, ws, dtype, am, lm, q, labels, xn, yn, grads, znorm, go, dam, dlm, dq, N, T,
                                          U, V, blank, c1, c2)

    inf, nan = float("inf"), float("nan")
    shared = [dict(dtype=-1), dict(dtype=3),                                   # an unknown dtype
              dict(V=1), dict(V=0), dict(V=(1 << 24) + 1),                     # V < 2 (and beyond the bound)
              dict(blank=5), dict(blank=-1),                                   # a blank outside [0,V)
              # sizes rnnt_amd_workspace_size refuses
              dict(N=-1), dict(N=70000), dict(T=0), dict(U=0), dict(T=1 << 15, U=1 << 14), dict(N=65535, T=1 << 10, U=1 << 7),
              dict(T=65535 * 64 + 1, U=1, labels=None),                        # more tiles than a grid dimension numbers
              # scales that are negative, not finite or sum above 1
              dict(c1=-0.1), dict(c2=-0.1), dict(c1=inf), dict(c2=inf), dict(c1=nan), dict(c2=nan), dict(c1=0.7, c2=0.4),
              dict(c1=1.5), dict(c2=1.5),
              dict(c2=0.1, q=None),                                            # am_only_scale != 0 without q
              # null or misaligned pointers
              dict(ws=None), dict(ws=ctypes.c_void_p(264)), dict(am=None), dict(lm=None), dict(labels=None), dict(xn=None),
              dict(yn=None), dict(am=odd2), dict(lm=odd2), dict(q=odd2), dict(labels=odd2), dict(xn=odd2), dict(yn=odd2),
              dict(grads=odd4), dict(znorm=odd2), dict(dtype=1, am=ctypes.c_void_p(257)), dict(dtype=2, lm=ctypes.c_void_p(257))]
    for kw in shared:
        assert fwd(**kw) == INVALID, kw
        assert bwd(**kw) == INVALID, kw
        if "N" not in kw:                    # a refused argument is not answered as an empty batch
            assert fwd(N=0, **kw) == INVALID and bwd(N=0, **kw) == INVALID, kw
    for kw in (dict(costs=None), dict(costs=odd2), dict(znorm=None)):                    # (pair_grads without znorm)
        assert fwd(**kw) == INVALID, kw
    for kw in (dict(grads=None), dict(znorm=None), dict(dam=None), dict(dlm=None), dict(dam=odd2), dict(dlm=odd2),
               dict(go=odd2), dict(dq=odd2)):
        assert bwd(**kw) == INVALID, kw
    assert L.rnnt_amd_simple_workspace_size(2, 0, 4) == 0 and L.rnnt_amd_simple_workspace_size(70000, 3, 4) == 0
    assert L.rnnt_amd_simple_workspace_size(2, 65535 * 64 + 1, 1) == 0
    # the loss's own size entry answers what it answered; this one says what lies behind it
    for dims in ((2, 3, 4), (16, 1500, 300), (1, 1, 1)):
        assert L.rnnt_amd_simple_workspace_size(*dims) > L.rnnt_amd_workspace_size(*dims) > 0
    assert L.rnnt_amd_simple_workspace_size(0, 3, 4) == L.rnnt_amd_workspace_size(0, 3, 4)
    for dtype in (0, 1, 2):
        # no utterances: success without a launch; halves on 2-byte addresses; scales on the edge; optional pointers
        assert fwd(dtype=dtype, N=0) == SUCCESS and bwd(dtype=dtype, N=0) == SUCCESS
        assert fwd(dtype=dtype, N=0, grads=None, znorm=None) == SUCCESS and fwd(dtype=dtype, N=0, grads=None) == SUCCESS
        assert fwd(dtype=dtype, N=0, q=None) == SUCCESS and bwd(dtype=dtype, N=0, q=None, dq=None, go=None) == SUCCESS
        assert fwd(dtype=dtype, N=0, c1=0.6, c2=0.4) == SUCCESS and bwd(dtype=dtype, N=0, c1=0.6, c2=0.4) == SUCCESS
        assert fwd(dtype=dtype, N=0, c1=1.0) == SUCCESS and fwd(dtype=dtype, N=0, c1=0.0, c2=1.0) == SUCCESS
        assert fwd(dtype=dtype, N=0, U=1, labels=None) == SUCCESS and bwd(dtype=dtype, N=0, U=1, labels=None) == SUCCESS
    assert fwd(dtype=1, N=0, am=odd2, lm=odd2) == SUCCESS and bwd(dtype=2, N=0, am=odd2, lm=odd2, dam=odd2, dlm=odd2) == SUCCESS


def test_header_declares_what_the_table_binds_and_the_library_exports(monkeypatch):
    import warp_rnnt_amd
    from warp_rnnt_amd import _build, _lib as lib
    L = _lib()
    table = lib.SIMPLE_SYMBOLS
    assert set(table) == ENTRIES and lib.ADDITIVE_SIMPLE == ((table, HEADER),)
    vp, i, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    assert table["rnnt_amd_simple_workspace_size"] == (ctypes.c_size_t, [i, i, i])
    assert table["rnnt_amd_simple_loss"] == (i, [vp, vp, i] + [vp] * 9 + [i] * 5 + [f] * 3)
    assert table["rnnt_amd_simple_backward"] == (i, [vp, vp, i] + [vp] * 12 + [i] * 5 + [f] * 2)
    text = open(os.path.join(ROOT, "include", HEADER)).read()
    declared = set(re.findall(r"\b(run_[a-z_]+|rnnt_amd_[a-z_]+)\s*\(", text))
    assert declared == set(table)
    assert '#include "warp_rnnt_amd.h"' in text
    # the argument names of the two calls, in the header's order
    for name, count in (("rnnt_amd_simple_loss", 20), ("rnnt_amd_simple_backward", 22)):
        body = re.search(name + r"\((.*?)\);", text, re.S).group(1)
        assert len(re.sub(r"/\*.*?\*/", "", body, flags=re.S).split(",")) == count == len(table[name][1]), name
    main = open(os.path.join(ROOT, "include", "warp_rnnt_amd.h")).read()
    earlier = lib.ADDITIVE + lib.ADDITIVE_NEXT + lib.ADDITIVE_TDT_JOINT + lib.ADDITIVE_PRUNED
    others = [lib.SYMBOLS] + [t for t, _ in earlier]
    syms = subprocess.check_output(["nm", "-D", "--defined-only", warp_rnnt_amd.lib_path()]).decode()
    for name in declared:
        assert name + "(" not in main.replace(" (", "(")                   # a header of their own
        assert not any(name in other for other in others)                 # ... and a table of their own
        assert re.search(r"\bT " + name + r"\b", syms), name
        fn = getattr(L, name)
        res, args = table[name]
        assert fn.restype is res and list(fn.argtypes) == list(args)      # bound by load()
    assert L.rnnt_amd_version() == lib.ABI_VERSION == 110                 # the version did not move
    assert any(os.path.basename(h) == HEADER for h in _build.HEADERS)      # part of the build's fingerprint
    assert "simple.hip" in _build.SOURCES and "simple.h" in _build.HEADERS
    assert "simple.hip" not in _build.HAZARD_CHECKED and "simple.hip" not in _build.RELOAD_CHECKED
    assert "asm" not in open(os.path.join(_build.CSRC, "simple.hip")).read()
    # the older tuples are what they were
    assert [h for _, h in lib.ADDITIVE] == ["warp_rnnt_amd_clamp.h", "warp_rnnt_amd_joint_dropout.h", "warp_rnnt_amd_hat.h",
                                            "warp_rnnt_amd_align.h", "warp_rnnt_amd_tdt.h"]
    assert lib.ADDITIVE_NEXT == ((lib.TDT_ALIGN_SYMBOLS, "warp_rnnt_amd_tdt_align.h"),)
    assert lib.ADDITIVE_TDT_JOINT == ((lib.TDT_JOINT_SYMBOLS, "warp_rnnt_amd_tdt_joint.h"),)
    assert lib.ADDITIVE_PRUNED == ((lib.PRUNED_SYMBOLS, "warp_rnnt_amd_pruned.h"),)
    # a stale library (same version, built before the entries existed) is refused with the rebuild message
    monkeypatch.setattr(lib, "_lib", None)
    monkeypatch.setitem(table, "rnnt_amd_no_such_entry", (ctypes.c_int, [ctypes.c_float]))
    with pytest.raises(RuntimeError, match=r"rnnt_amd_no_such_entry \(include/" + re.escape(HEADER) + r"\).*rebuild it"):
        lib.load()


def test_public_signature_and_argument_errors_on_cpu_tensors():
    from warp_rnnt_amd import ops, pruned, simple
    params = inspect.signature(simple.simple_rnnt_loss).parameters
    assert list(params) == ["am", "lm", "labels", "frames_lengths", "labels_lengths", "blank", "lm_only_scale",
                            "am_only_scale", "fastemit_lambda", "average_frames", "reduction", "return_grad"]
    assert [params[k].default for k in list(params)[5:]] == [0, 0.0, 0.0, 0.0, False, "none", False]
    assert list(inspect.signature(ops.simple_loss).parameters) == ["am", "lm", "q", "labels", "xn", "yn", "blank",
                                                                    "lm_only_scale", "am_only_scale", "fastemit_lambda",
                                                                    "with_grads"]
    assert list(inspect.signature(ops.simple_backward).parameters) == ["am", "lm", "q", "labels", "xn", "yn", "grads",
                                                                        "znorm", "grad_costs", "blank", "lm_only_scale",
                                                                        "am_only_scale"]
    assert list(inspect.signature(simple.batch_log_unigram).parameters) == ["lm"]
    assert list(inspect.signature(pruned.simple_pairs).parameters) == ["am", "lm", "labels", "blank"]       # stays as it is
    N, T, U, V = 2, 3, 4, 7
    batch = (torch.zeros((N, T, V)), torch.zeros((N, U, V)), torch.ones((N, U - 1), dtype=torch.int32),
             torch.tensor([3, 2], dtype=torch.int32), torch.tensor([3, 1], dtype=torch.int32))
    with pytest.raises(AssertionError):
        simple.simple_rnnt_loss(*batch, reduction="avg")
    with pytest.raises(AssertionError):
        simple.simple_rnnt_loss(*batch, blank=1.0)
    with pytest.raises(RuntimeError, match="must be located in the CUDA"):
        simple.simple_rnnt_loss(*batch)
    with pytest.raises(RuntimeError, match="must be located in the CUDA"):
        simple.simple_rnnt_loss(*batch, am_only_scale=0.1, return_grad=True)
    with pytest.raises(RuntimeError, match="ys must be a Int tensor"):
        simple.simple_rnnt_loss(batch[0], batch[1], batch[2].long(), *batch[3:])
    with pytest.raises(RuntimeError, match="am must be a float32, bfloat16 or float16 tensor"):
        simple.simple_rnnt_loss(batch[0].double(), *batch[1:])
    with pytest.raises(RuntimeError, match="lm must have the dtype of am"):
        simple.simple_rnnt_loss(batch[0], batch[1].bfloat16(), *batch[2:])
    with pytest.raises(RuntimeError, match="am must be contiguous"):
        simple.simple_rnnt_loss(torch.zeros((N, V, T)).transpose(1, 2), *batch[1:])
    # the values the C entries would refuse, with their reasons, before anything is loaded or launched
    for kw, text in ((dict(V=1, blank=0), "V >= 2"), (dict(V=5, blank=5), "vocabulary index"),
                     (dict(V=5, blank=0, lm_only_scale=-0.1), "finite scales"),
                     (dict(V=5, blank=0, lm_only_scale=0.7, am_only_scale=0.4, q=batch[0]), "finite scales"),
                     (dict(V=5, blank=0, am_only_scale=float("nan"), q=batch[0]), "finite scales"),
                     (dict(V=5, blank=0, am_only_scale=0.1), "needs the log unigram")):
        args = dict(lm_only_scale=0.0, am_only_scale=0.0, q=None)
        args.update(kw)
        with pytest.raises(RuntimeError, match="status 5.*" + text):
            ops._simple_check(args["V"], args["blank"], args["lm_only_scale"], args["am_only_scale"], args["q"])
    assert ops._simple_check(5, 0, 0.6, 0.4, batch[0]) == (ctypes.c_float(0.6).value, ctypes.c_float(0.4).value)
    module = simple.SimpleRNNTLoss(blank=3, lm_only_scale=0.25, am_only_scale=0.1, fastemit_lambda=0.01, reduction="sum")
    assert isinstance(module, torch.nn.Module)
    assert (module.blank, module.lm_only_scale, module.am_only_scale, module.fastemit_lambda, module.reduction) == \
        (3, 0.25, 0.1, 0.01, "sum")
    assert "return_grad=True" in pruned.__doc__ and "simple_rnnt_loss" in pruned.__doc__ and "Out of scope" in simple.__doc__
