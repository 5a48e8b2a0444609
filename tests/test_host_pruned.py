"""The pruned transducer loss without a GPU: the fp64 reference (tests/pruned_reference.py) against brute-force enumeration,
central differences and the full lattice; the fp32 oracle on the gathered layout with the floor the kernels use; the
plain-torch helpers of the recipe (prune_ranges, simple_pairs, prune_joint_inputs); the C entries' refusals with pointers
that are never dereferenced; the additive contract of include/warp_rnnt_amd_pruned.h and its table; the front end's
signature and argument errors."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import pruned_reference as pr
from helpers import np_log_softmax32
from oracle import transduce_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "warp_rnnt_amd_pruned.h"
ENTRIES = {"rnnt_amd_pruned_loss_logits", "rnnt_amd_pruned_logits_backward"}
INVALID, SUCCESS = 5, 0
FLOOR = np.float32(-1e30)


def _lib():
    import warp_rnnt_amd
    from warp_rnnt_amd import _build
    _build.build()          # hipcc cross-compiles for gfx950 without a GPU; no-op when up to date
    return warp_rnnt_amd.load()


# ---- the reference ----

@pytest.mark.parametrize("T,U,S", [(4, 4, 2), (4, 3, 2), (3, 4, 3), (4, 4, 4), (2, 3, 2), (1, 1, 1), (4, 1, 1)])
def test_reference_against_enumeration_of_all_paths(T, U, S):
    N, V, blank = 3, 4, 1
    logits, labels, starts, xn, yn = pr.make_band_case(100 * T + 10 * U + S, N, T, U, S, V, blank=blank)
    ref = pr.pruned_loss64(logits, labels, starts, xn, yn, blank)
    lp = transduce_np.log_softmax(logits)
    for n in range(N):
        want = pr.brute_force_cost(lp[n], labels[n], starts[n], int(xn[n]), int(yn[n]) + 1, blank)
        print(f"T{T} U{U} S{S} utterance {n}: {ref['costs'][n]:.12f} enumeration {want:.12f}")
        assert np.isfinite(want)
        np.testing.assert_allclose(ref["costs"][n], want, rtol=1e-13)
    # a band that leaves (0,0) out holds no path: both say so
    off = starts.copy()
    off[0, 0] = 1
    if U > 1:
        assert np.isinf(pr.pruned_loss64(logits, labels, off, xn, yn, blank)["costs"][0])
        assert np.isinf(pr.brute_force_cost(lp[0], labels[0], off[0], int(xn[0]), int(yn[0]) + 1, blank))


@pytest.mark.parametrize("blank,lam", [(0, 0.0), (2, 0.01), (4, 0.0)])
def test_reference_gradient_against_central_differences(blank, lam):
    """pruned_loss64 is what judges the kernels: its d/d logits against central differences of its own costs."""
    N, T, U, S, V = 2, 5, 4, 2, 5
    logits, labels, starts, xn, yn = pr.make_band_case(11 + blank, N, T, U, S, V, blank=blank)
    z = logits.astype(np.float64)
    go = pr.upstream(N)
    ref = pr.pruned_loss64(z, labels, starts, xn, yn, blank, lam)
    ref0 = pr.pruned_loss64(z, labels, starts, xn, yn, blank, 0.0)
    assert np.isfinite(ref["costs"]).all()
    h = 1e-5
    num = np.zeros_like(z)
    for idx in np.ndindex(*z.shape):
        zp, zm = z.copy(), z.copy()
        zp[idx] += h
        zm[idx] -= h
        cp = pr.pruned_loss64(zp, labels, starts, xn, yn, blank)["costs"]
        cm = pr.pruned_loss64(zm, labels, starts, xn, yn, blank)["costs"]
        num[idx] = go[idx[0]] * (cp[idx[0]] - cm[idx[0]]) / (2 * h)
    # FastEmit scales the label gradient and leaves the cost alone: the lam = 0 gradient is the cost's derivative
    np.testing.assert_allclose(ref0["dlogits"], num, rtol=0, atol=1e-6)
    if lam:
        assert not np.allclose(ref["dlogits"], ref0["dlogits"])
        np.testing.assert_allclose(ref["pair_grads"][..., 1], (1.0 + lam) * ref0["pair_grads"][..., 1], rtol=1e-14)
        np.testing.assert_array_equal(ref["pair_grads"][..., 0], ref0["pair_grads"][..., 0])
    assert (ref["pair_grads"][~ref["inband"]] == 0).all() and (ref["dlogits"] != 0).any()


@pytest.mark.parametrize("lam", [0.0, 0.01])
def test_the_full_band_is_the_standard_loss(lam):
    N, T, U, V, blank = 3, 7, 5, 6, 2
    logits, labels, _, xn, yn = pr.make_band_case(5, N, T, U, U, V, blank=blank)
    starts = np.zeros((N, T), np.int32)
    go = pr.upstream(N)
    ref = pr.pruned_loss64(logits, labels, starts, xn, yn, blank, lam)
    lp = transduce_np.log_softmax(logits)                 # (N,T,S = U,V): the same tensor is the dense lattice's
    costs, glp = transduce_np.transduce_batch(lp, labels, xn, yn, blank=blank, fastemit_lambda=lam, fast=True)
    dz = (glp - np.exp(lp) * glp.sum(-1, keepdims=True)) * go[:, None, None, None]
    np.testing.assert_allclose(ref["costs"], costs, rtol=1e-13)
    np.testing.assert_allclose(ref["dlogits"], dz, rtol=0, atol=1e-13)


# ---- the fp32 oracle with the floor the kernels use ----

def _floored_pairs(logits, labels, starts, U, blank):
    """(N,T,U,2) fp32: the band's pairs from the fp32 log-softmax, FLOOR in both channels everywhere else; the last
    column's label is the blank."""
    N, T, S, V = logits.shape
    lp = np_log_softmax32(logits)
    pairs = np.full((N, T, U, 2), FLOOR, np.float32)
    for n in range(N):
        for t in range(T):
            for s in range(S):
                u = int(starts[n, t]) + s
                if 0 <= u < U:
                    lab = labels[n, u] if u < U - 1 else blank
                    pairs[n, t, u] = (lp[n, t, s, blank], lp[n, t, s, lab])
    return pairs


def test_fp32_oracle_with_the_floor_on_thirty_random_bands():
    """The gathered-layout fp32 oracle -- the sweeps' arithmetic on the CPU -- on pair planes with -1e30 outside the band,
    against the fp64 band recursion with true -inf: costs and gradient pairs inside the fp32 bars of BASELINE.json (costs
    1e-5 relative, gradients 1e-4 absolute), exactly zero gradients outside the band, everything finite, the
    forward/backward guard silent."""
    import oracle
    rng = np.random.RandomState(2024)
    worst_cost = worst_grad = 0.0
    lowest = 0.0
    for k in range(30):
        N = 2
        S = int(rng.randint(2, 7))
        T = int(rng.randint(6, 59))
        U = int(rng.randint(S, 29))
        V, blank, lam = 7, int(rng.randint(0, 7)), (0.0, 0.01)[k % 2]
        logits, labels, starts, xn, yn = pr.make_band_case(3000 + k, N, T, U, S, V, blank=blank)
        ref = pr.pruned_loss64(logits, labels, starts, xn, yn, blank, lam)
        assert np.isfinite(ref["costs"]).all()
        pairs = _floored_pairs(logits, labels, starts, U, blank)
        o = oracle.rnnt_loss_f32(pairs, None, xn, yn, blank=-1, fastemit_lambda=lam)
        assert np.isfinite(o["costs"]).all() and np.isfinite(o["grads"]).all()
        assert np.isfinite(o["alphas"]).all() and np.isfinite(o["betas"]).all()
        assert not o["mismatch"].any()
        cost = float((np.abs(o["costs"] - ref["costs"]) / np.abs(ref["costs"])).max())
        grad = float(np.abs(o["grads"] - ref["pair_grads"]).max())
        worst_cost, worst_grad = max(worst_cost, cost), max(worst_grad, grad)
        lowest = min(lowest, float(o["alphas"].min()), float(o["betas"].min()))
        assert (o["grads"][~ref["inband"]] == 0).all(), k
        assert cost <= 1e-5 and grad <= 1e-4, (k, cost, grad)
    print(f"30 bands: cost rel {worst_cost:.3e}, gradient pairs abs {worst_grad:.3e}, lowest lattice value {lowest:.3e}")
    assert lowest > -3e38


# ---- the helpers of the recipe ----

def _prune_ranges_loop(occ, xn, yn, S):
    """prune_ranges as its docstring says it, with loops."""
    N, T, U = occ.shape
    out = np.zeros((N, T), np.int64)
    if S >= U:
        return out
    for n in range(N):
        Tn, hi = int(xn[n]), max(int(yn[n]) + 1 - S, 0)
        s = np.zeros(T, np.int64)
        for t in range(Tn):
            sums = [occ[n, t, u0:u0 + S].sum() for u0 in range(hi + 1)]
            s[t] = int(np.argmax(sums))                       # (numpy: the first of equal maxima)
        s[Tn - 1:] = hi
        for t in range(T - 2, -1, -1):
            s[t] = min(s[t], s[t + 1])
        for t in range(T - 2, -1, -1):
            s[t] = max(s[t], s[t + 1] - (S - 1))
        out[n] = s
    return out


@pytest.mark.parametrize("S", [2, 3, 5, 6])
def test_prune_ranges_properties_on_random_occupancies(S):
    from warp_rnnt_amd.pruned import prune_ranges
    rng = np.random.RandomState(40 + S)
    N, T, U = 4, 23, 11
    # occupancies on a grid of 1/64: window sums are exact in fp32, so ties are ties on both sides
    occ = np.round(rng.rand(N, T, U) * 64) / 64
    occ[0, 3] = 0.25                                          # a frame of equal sums: the lowest argmax
    xn = np.array([T, T - 4, 9, T], np.int32)
    yn = np.array([U - 1, U - 3, 4, 1], np.int32)
    grads = np.zeros((N, T, U, 2), np.float32)
    grads[..., 0] = -0.25 * occ
    grads[..., 1] = -0.75 * occ
    got = prune_ranges(torch.tensor(grads), torch.tensor(xn), torch.tensor(yn), S)
    assert got.dtype == torch.int32 and tuple(got.shape) == (N, T)
    got = got.numpy().astype(np.int64)
    np.testing.assert_array_equal(got, _prune_ranges_loop(occ, xn, yn, S))
    for n in range(N):
        Tn, hi = int(xn[n]), max(int(yn[n]) + 1 - S, 0)
        assert (got[n] >= 0).all() and (got[n] <= hi).all()               # within bounds
        assert got[n, Tn - 1] == hi and (got[n, Tn:] == hi).all()         # the last live start forced, repeated behind it
        d = np.diff(got[n])
        assert (d >= 0).all() and (d <= S - 1).all()
    with pytest.raises(ValueError, match="s_range"):
        prune_ranges(torch.tensor(grads), torch.tensor(xn), torch.tensor(yn), 1)


def test_prune_ranges_the_full_band_and_the_infeasible_case():
    from warp_rnnt_amd.pruned import prune_ranges
    N, T, U = 2, 4, 12
    grads = torch.zeros(N, T, U, 2)
    grads[:, :, 0, :] = -0.5                  # all the occupancy in column 0: every argmax is 0
    xn, yn = torch.tensor([T, T], dtype=torch.int32), torch.tensor([U - 1, 3], dtype=torch.int32)
    for S in (U, U + 3):
        assert (prune_ranges(grads, xn, yn, S) == 0).all()
    # S = 3: utterance 0 has (T_n - 1)(S - 1) = 6 < U_n + 1 - S = 9 -- no band of that width holds a path, and the
    # result says so with start[0] > 0; utterance 1 (hi = 1) is feasible
    got = prune_ranges(grads, xn, yn, 3).numpy()
    assert got[0, -1] == 9 and got[0, 0] == 9 - 3 * 2 > 0 and (np.diff(got[0]) == 2).all()
    assert got[1, -1] == 1 and (np.diff(got[1]) >= 0).all() and (np.diff(got[1]) <= 2).all()
    # ... and the reference answers +inf for exactly that utterance
    logits, labels, _, _, _ = pr.make_band_case(1, N, T, U, 3, 5)
    costs = pr.pruned_loss64(logits, labels, got, xn.numpy(), yn.numpy(), 0)["costs"]
    assert np.isinf(costs[0]) and np.isfinite(costs[1])


@pytest.mark.parametrize("blank", [0, 3])
def test_simple_pairs_against_the_dense_log_softmax(blank):
    from warp_rnnt_amd.pruned import simple_pairs
    gen = torch.Generator().manual_seed(3)
    N, T, U, V = 2, 6, 4, 7
    am = torch.randn(N, T, V, generator=gen, dtype=torch.float64) * 3 + 40.0      # (the maxima are taken out)
    lm = torch.randn(N, U, V, generator=gen, dtype=torch.float64) * 3 - 25.0
    labels = torch.randint(0, V, (N, U - 1), generator=gen, dtype=torch.int32)
    labels[0, 1] = -7                                                          # outside [0,V): the blank
    got = simple_pairs(am, lm, labels, blank)
    assert tuple(got.shape) == (N, T, U, 2) and got.dtype == torch.float64
    dense = torch.log_softmax(am[:, :, None, :] + lm[:, None, :, :], dim=-1)
    lab = labels.long()
    lab = torch.where((lab >= 0) & (lab < V), lab, torch.full_like(lab, blank))
    lab = torch.cat([lab, torch.full((N, 1), blank, dtype=torch.long)], 1)
    want = torch.stack([dense[..., blank], dense.gather(3, lab[:, None, :, None].expand(N, T, U, 1))[..., 0]], -1)
    np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=0, atol=1e-12)
    assert torch.equal(got[:, :, U - 1, 1], got[:, :, U - 1, 0])               # the last column's label is the blank
    am.requires_grad_(True)
    simple_pairs(am, lm, labels, blank).sum().backward()                        # differentiable: the first pass trains
    assert torch.isfinite(am.grad).all() and (am.grad != 0).any()
    with pytest.raises(ValueError, match="simple_pairs needs"):
        simple_pairs(am, lm[:, :, :-1], labels, blank)


def test_prune_joint_inputs_against_indexing():
    from warp_rnnt_amd.pruned import prune_joint_inputs
    gen = torch.Generator().manual_seed(4)
    N, T, U, H, S = 2, 5, 6, 3, 4
    f, g = torch.randn(N, T, H, generator=gen), torch.randn(N, U, H, generator=gen)
    starts = torch.randint(-2, U, (N, T), generator=gen, dtype=torch.int32)      # (some bands reach outside: clamped)
    fp, gp = prune_joint_inputs(f, g, starts, S)
    assert tuple(fp.shape) == tuple(gp.shape) == (N, T, S, H)
    for n in range(N):
        for t in range(T):
            for s in range(S):
                u = min(max(int(starts[n, t]) + s, 0), U - 1)
                assert torch.equal(fp[n, t, s], f[n, t]) and torch.equal(gp[n, t, s], g[n, u])
    ranges = starts.long()[..., None] + torch.arange(S)                          # k2's form
    fp3, gp3 = prune_joint_inputs(f, g, ranges)
    assert torch.equal(fp3, fp) and torch.equal(gp3, gp)
    with pytest.raises(ValueError, match="s_range"):
        prune_joint_inputs(f, g, starts)


# ---- the C entries ----

def test_entries_refuse_before_any_hip_call():
    """Dummy device pointers that are never dereferenced: each call is refused by the host-side check it names."""
    if torch.cuda.is_available():
        pytest.skip("host-only table: replayed where no GPU is visible (its pointers are made up)")
    L = _lib()
    p = ctypes.c_void_p(256)                 # aligned, non-null, never dereferenced

    def fwd(ws=p, dtype=0, logits=p, labels=p, starts=p, xn=p, yn=p, costs=p, grads=p, N=2, T=3, U=4, S=2, V=5, blank=0):
        return L.rnnt_amd_pruned_loss_logits(None, ws, dtype, logits, labels, starts, xn, yn, costs, grads, N, T, U, S, V,
                                             blank, 0.0)

    def bwd(dtype=0, logits=p, labels=p, starts=p, grads=p, go=p, out=p, N=2, T=3, U=4, S=2, V=5, blank=0):
        return L.rnnt_amd_pruned_logits_backward(None, dtype, logits, labels, starts, grads, go, out, N, T, U, S, V, blank)

    # everything HAT's entries refuse (tests/test_host_hat.py), S = 1 where U is 0 so that it is U that is refused ...
    shared = [dict(dtype=-1), dict(dtype=3), dict(V=1), dict(V=0), dict(blank=5), dict(blank=-1), dict(logits=None),
              dict(labels=None), dict(N=-1), dict(N=70000), dict(T=0), dict(U=0, S=1), dict(T=1 << 15, U=1 << 14),
              dict(N=65535, T=1 << 10, U=1 << 7),
              # ... and the band's own: S < 1, S > U, a null starts (N*T*S >= 2^32 cannot be reached alone: S <= U, and
              # the lattice's N*T*U is refused first)
              dict(S=0), dict(S=-1), dict(S=5), dict(starts=None), dict(N=65535, T=1 << 10, U=1 << 7, S=1 << 7)]
    for kw in shared:
        assert fwd(**kw) == INVALID, kw
        assert bwd(**kw) == INVALID, kw
        if "N" not in kw:                    # a refused argument is not answered as an empty batch
            assert fwd(N=0, **kw) == INVALID and bwd(N=0, **kw) == INVALID, kw
    for kw in (dict(ws=None), dict(ws=ctypes.c_void_p(264)), dict(costs=None), dict(xn=None), dict(yn=None)):
        assert fwd(**kw) == INVALID, kw
    for kw in (dict(grads=None), dict(out=None), dict(grads=ctypes.c_void_p(260))):
        assert bwd(**kw) == INVALID, kw
    for dtype in (0, 1, 2):
        # no utterances: success without a launch; a column of blanks needs no labels; S = U is the full band
        assert fwd(dtype=dtype, N=0) == SUCCESS and bwd(dtype=dtype, N=0) == SUCCESS
        assert fwd(dtype=dtype, N=0, grads=None) == SUCCESS and fwd(dtype=dtype, N=0, S=4) == SUCCESS
        assert fwd(dtype=dtype, N=0, U=1, S=1, labels=None) == SUCCESS
        assert bwd(dtype=dtype, N=0, U=1, S=1, labels=None) == SUCCESS
        assert bwd(dtype=dtype, N=0, go=None) == SUCCESS


def test_header_declares_what_the_table_binds_and_the_library_exports(monkeypatch):
    import warp_rnnt_amd
    from warp_rnnt_amd import _build, _lib as lib
    L = _lib()
    table = lib.PRUNED_SYMBOLS
    assert set(table) == ENTRIES and lib.ADDITIVE_PRUNED == ((table, HEADER),)
    # HAT's argument lists with `starts` behind the labels and S between U and V
    hat_f, hat_b = lib.HAT_SYMBOLS["rnnt_amd_hat_loss_logits"][1], lib.HAT_SYMBOLS["rnnt_amd_hat_logits_backward"][1]
    assert table["rnnt_amd_pruned_loss_logits"][1] == hat_f[:5] + [ctypes.c_void_p] + hat_f[5:12] + [ctypes.c_int] + hat_f[12:]
    assert table["rnnt_amd_pruned_logits_backward"][1] == hat_b[:4] + [ctypes.c_void_p] + hat_b[4:10] + [ctypes.c_int] + hat_b[10:]
    text = open(os.path.join(ROOT, "include", HEADER)).read()
    declared = set(re.findall(r"\b(run_[a-z_]+|rnnt_amd_[a-z_]+)\s*\(", text))
    assert declared == set(table)
    assert '#include "warp_rnnt_amd.h"' in text
    main = open(os.path.join(ROOT, "include", "warp_rnnt_amd.h")).read()
    earlier = lib.ADDITIVE + lib.ADDITIVE_NEXT + lib.ADDITIVE_TDT_JOINT
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
    assert "pruned.hip" in _build.SOURCES and "pruned.h" in _build.HEADERS
    assert "pruned.hip" not in _build.HAZARD_CHECKED and "pruned.hip" not in _build.RELOAD_CHECKED
    assert "asm" not in open(os.path.join(_build.CSRC, "pruned.hip")).read()
    # the three older tuples are what they were
    assert [h for _, h in lib.ADDITIVE] == ["warp_rnnt_amd_clamp.h", "warp_rnnt_amd_joint_dropout.h", "warp_rnnt_amd_hat.h",
                                            "warp_rnnt_amd_align.h", "warp_rnnt_amd_tdt.h"]
    assert lib.ADDITIVE_NEXT == ((lib.TDT_ALIGN_SYMBOLS, "warp_rnnt_amd_tdt_align.h"),)
    assert lib.ADDITIVE_TDT_JOINT == ((lib.TDT_JOINT_SYMBOLS, "warp_rnnt_amd_tdt_joint.h"),)
    # a stale library (same version, built before the entries existed) is refused with the rebuild message
    monkeypatch.setattr(lib, "_lib", None)
    monkeypatch.setitem(table, "rnnt_amd_no_such_entry", (ctypes.c_int, [ctypes.c_float]))
    with pytest.raises(RuntimeError, match=r"rnnt_amd_no_such_entry \(include/" + re.escape(HEADER) + r"\).*rebuild it"):
        lib.load()


def test_public_signature_and_argument_errors_on_cpu_tensors():
    from warp_rnnt_amd import ops, pruned
    params = inspect.signature(pruned.pruned_rnnt_loss_from_logits).parameters
    assert list(params) == ["logits", "labels", "ranges", "frames_lengths", "labels_lengths", "average_frames", "reduction",
                            "blank", "fastemit_lambda"]
    assert [params[k].default for k in list(params)[5:]] == [False, "none", 0, 0.0]
    assert list(inspect.signature(ops.pruned_loss).parameters) == ["logits", "labels", "starts", "xn", "yn", "blank",
                                                                    "fastemit_lambda", "with_grads"]
    assert list(inspect.signature(ops.pruned_logits_backward).parameters) == ["logits", "labels", "starts", "grads",
                                                                               "grad_costs", "blank"]
    assert list(inspect.signature(pruned.prune_ranges).parameters) == ["pair_grads", "frames_lengths", "labels_lengths",
                                                                       "s_range"]
    assert list(inspect.signature(pruned.simple_pairs).parameters) == ["am", "lm", "labels", "blank"]
    assert list(inspect.signature(pruned.prune_joint_inputs).parameters)[:3] == ["f", "g", "ranges"]
    N, T, U, S, V = 2, 3, 4, 2, 7
    batch = (torch.zeros((N, T, S, V)), torch.ones((N, U - 1), dtype=torch.int32), torch.zeros((N, T), dtype=torch.int32),
             torch.tensor([3, 2], dtype=torch.int32), torch.tensor([3, 1], dtype=torch.int32))
    with pytest.raises(AssertionError):
        pruned.pruned_rnnt_loss_from_logits(*batch, reduction="avg")
    with pytest.raises(AssertionError):
        pruned.pruned_rnnt_loss_from_logits(*batch, blank=1.0)
    with pytest.raises(RuntimeError, match="must be located in the CUDA"):
        pruned.pruned_rnnt_loss_from_logits(*batch)
    with pytest.raises(RuntimeError, match="ys must be a Int tensor"):
        pruned.pruned_rnnt_loss_from_logits(batch[0], batch[1].long(), *batch[2:])
    with pytest.raises(RuntimeError, match="integer tensor"):
        pruned.pruned_rnnt_loss_from_logits(batch[0], batch[1], batch[2].float(), *batch[3:])
    with pytest.raises(RuntimeError, match="S = 3"):
        pruned.pruned_rnnt_loss_from_logits(batch[0], batch[1], torch.zeros((N, T, 3), dtype=torch.int64), *batch[3:])
    # both forms of the ranges are one tensor of starts
    starts = torch.tensor([[0, 1, 2], [0, 0, 1]])
    k2 = starts[..., None] + torch.arange(S)
    assert torch.equal(pruned.band_starts(k2, S), pruned.band_starts(starts.int(), S))
    assert pruned.band_starts(k2, S).dtype == torch.int32 and pruned.band_starts(k2, S).is_contiguous()
    module = pruned.PrunedRNNTLoss(blank=3, fastemit_lambda=0.01, reduction="sum")
    assert isinstance(module, torch.nn.Module)
    assert (module.blank, module.fastemit_lambda, module.reduction) == (3, 0.01, "sum")
    import warp_rnnt_amd
    assert "pruned.py" in warp_rnnt_amd.__doc__ and "Out of scope" in pruned.__doc__
