"""The multi-blank transducer loss without a GPU: the fp64 reference (tests/multiblank_reference.py) against exhaustive
path enumeration and its gradient against central differences, B = 1 against the standard loss's oracle, the three C
entries of include/warp_rnnt_amd_multiblank.h -- every refusal with pointers that are never dereferenced, the workspace
size -- the additive contract of the header and its table, and the public signatures."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import multiblank_reference as mr
from oracle import transduce_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "warp_rnnt_amd_multiblank.h"
ENTRIES = {"rnnt_amd_multiblank_workspace_size", "rnnt_amd_multiblank_loss_logits", "rnnt_amd_multiblank_logits_backward"}
INVALID, SUCCESS = 5, 0

# (blank durations, T, U, V): lattices of at most 7 x 4 cells; (1, 8) with T_n < 8: the long jump never fits
LATTICES = [((1,), 6, 4, 3), ((1, 2), 7, 4, 4), ((2, 1), 6, 3, 4), ((1, 2, 4), 7, 3, 5), ((1, 8), 7, 3, 4)]
IDS = ["d" + "".join(map(str, d)) for d, *_ in LATTICES]


def _lib():
    import warp_rnnt_amd
    from warp_rnnt_amd import _build
    _build.build()          # hipcc cross-compiles for gfx950 without a GPU; no-op when up to date
    return warp_rnnt_amd.load()


def _lengths(T, U):
    """The batch of test_host_tdt.py: a full utterance, a ragged one, one of a single frame, one without labels."""
    return [(T, U - 1), (T - 1, max(U - 2, 0)), (1, 0), (T, 0), (2, 1)]


def big_blank_ids_for(V, B, standard):
    """The ids of B - 1 big blanks: the lowest vocabulary indices that are not the standard blank's."""
    return [v for v in range(V) if v != standard][:B - 1]


def small_case(seed, T, U, V, ids, lengths):
    """fp64 logits (N,T,U,V) with labels that avoid every blank id; lengths: the (T_n, U_n) of the batch."""
    rng = np.random.RandomState(seed)
    N = len(lengths)
    z = rng.randn(N, T, U, V) * 1.5
    choices = np.array([v for v in range(V) if v not in set(ids)], np.int32)
    labels = choices[rng.randint(0, len(choices), size=(N, U - 1))].astype(np.int32)
    xn = np.array([l[0] for l in lengths], np.int32)
    yn = np.array([l[1] for l in lengths], np.int32)
    return z, labels, xn, yn


def ids_with_standard_at(durations, V, standard):
    """blank_ids in the order of `durations`: the id of duration 1 is `standard`, the big blanks take the lowest others."""
    big = iter(big_blank_ids_for(V, len(durations), standard))
    return tuple(standard if d == 1 else next(big) for d in durations)


# ---- the reference ----

@pytest.mark.parametrize("sigma", [0.0, 0.05])
@pytest.mark.parametrize("durations,T,U,V", LATTICES, ids=IDS)
def test_reference_costs_are_the_sum_over_every_path(durations, T, U, V, sigma):
    for standard in range(V):
        ids = ids_with_standard_at(durations, V, standard)
        z, labels, xn, yn = small_case(10 * V + standard, T, U, V, ids, _lengths(T, U))
        costs, _, _ = mr.multiblank_loss64(z, labels, xn, yn, ids, durations, sigma)
        lp = mr.log_softmax64(z) - sigma
        for n in range(len(xn)):
            want = -mr.enumerate_paths(lp[n], labels[n], int(xn[n]), int(yn[n]), ids, durations)
            assert np.isfinite(want)            # duration 1 is there: every lattice has a path
            assert abs(costs[n] - want) <= 1e-12 * max(1.0, abs(want)), (standard, n, costs[n], want)


@pytest.mark.parametrize("durations,T,U,V", LATTICES, ids=IDS)
def test_reference_gradient_against_central_differences(durations, T, U, V):
    """multiblank_loss64 is what judges the kernels: its d/d z against central differences of its own costs, fp64;
    beta(0,0) is the log-likelihood; FastEmit leaves the costs alone and scales the label edges."""
    sigma = 0.05
    ids = ids_with_standard_at(durations, V, V // 2)
    z, labels, xn, yn = small_case(3 + V, T, U, V, ids, _lengths(T, U)[:3])
    costs, dz, G = mr.multiblank_loss64(z, labels, xn, yn, ids, durations, sigma)
    h = 1e-5
    num = np.zeros_like(z)
    for idx in np.ndindex(*z.shape):
        zp, zm = z.copy(), z.copy()
        zp[idx] += h
        zm[idx] -= h
        cp = mr.multiblank_loss64(zp, labels, xn, yn, ids, durations, sigma)[0]
        cm = mr.multiblank_loss64(zm, labels, xn, yn, ids, durations, sigma)[0]
        num[idx] = (cp[idx[0]] - cm[idx[0]]) / (2 * h)
    np.testing.assert_allclose(dz, num, rtol=0, atol=2e-8)
    lp = mr.log_softmax64(z) - sigma
    for n in range(len(xn)):
        ll, _, beta, _ = mr.utterance(lp[n], labels[n], int(xn[n]), int(yn[n]), ids, durations)
        assert abs(beta[0, 0] - ll) <= 1e-12 * max(1.0, abs(ll))
        assert (dz[n, xn[n]:] == 0).all() and (dz[n, :, yn[n] + 1:] == 0).all()
    costs_l, dz_l, G_l = mr.multiblank_loss64(z, labels, xn, yn, ids, durations, sigma, lam=0.25)
    assert np.array_equal(costs_l, costs)
    np.testing.assert_allclose(G_l[..., 0], 1.25 * G[..., 0], rtol=1e-14)
    assert np.array_equal(G_l[..., 1:], G[..., 1:]) and not np.allclose(dz_l, dz)


@pytest.mark.parametrize("blank", [0, 2, 4])
@pytest.mark.parametrize("sigma", [0.0, 0.05])
def test_one_blank_is_the_standard_loss_plus_sigma_per_step(blank, sigma):
    T, U, V = 7, 4, 5
    z, labels, xn, yn = small_case(blank + 1, T, U, V, (blank,), _lengths(T, U))
    costs, dz, _ = mr.multiblank_loss64(z, labels, xn, yn, (blank,), (1,), sigma)
    lp = transduce_np.log_softmax(z)
    want, glp = transduce_np.transduce_batch(lp, labels, xn, yn, blank=blank, fastemit_lambda=0.0, fast=True)
    np.testing.assert_allclose(costs, want + sigma * (xn + yn), rtol=1e-12, atol=0)
    np.testing.assert_allclose(dz, glp - np.exp(lp) * glp.sum(-1, keepdims=True), rtol=0, atol=1e-12)


def test_reference_refuses_lengths_out_of_range_and_takes_masked_logits():
    ids, durations = (1, 3), (1, 2)
    z, labels, xn, yn = small_case(1, 5, 3, 5, ids, [(5, 2), (6, 1), (3, 3), (0, 0)])
    costs, dz, G = mr.multiblank_loss64(z, labels, xn, yn, ids, durations)
    assert np.isfinite(costs[0]) and np.isnan(costs[1:]).all()
    assert (dz[1:] == 0).all() and (G[1:] == 0).all()
    # a masked token that is no label, and the masked big blank
    unused = [v for v in range(5) if v not in ids and v not in set(labels[0].tolist())]
    z[0, ..., unused[0]] = -np.inf
    z[0, ..., 3] = -np.inf
    costs, dz, _ = mr.multiblank_loss64(z, labels, xn, yn, ids, durations)
    assert np.isfinite(costs[0]) and np.isfinite(dz).all()
    assert (dz[0, ..., unused[0]] == 0).all() and (dz[0, ..., 3] == 0).all() and (dz[0] != 0).any()


# ---- the C entries ----

def _entries():
    L = _lib()
    p = ctypes.c_void_p(256)                 # aligned, non-null, never dereferenced

    def ints(v):
        return None if v is None else (ctypes.c_int * max(len(v), 1))(*v)

    def fwd(ws=p, dtype=0, logits=p, labels=p, xn=p, yn=p, ids=(6, 5, 4, 3), durations=(1, 2, 4, 8), B=None, costs=p,
            grads=p, N=2, T=3, U=2, V=7, sigma=0.0):
        B = (len(ids) if ids is not None else 1) if B is None else B
        return L.rnnt_amd_multiblank_loss_logits(None, ws, dtype, logits, labels, xn, yn, ints(ids), ints(durations), B,
                                                 costs, grads, N, T, U, V, sigma, 0.0)

    def bwd(dtype=0, logits=p, labels=p, grads=p, go=p, out=p, N=2, T=3, U=2, V=7, ids=(6, 5, 4, 3), B=None):
        B = (len(ids) if ids is not None else 1) if B is None else B
        return L.rnnt_amd_multiblank_logits_backward(None, dtype, logits, labels, grads, go, out, N, T, U, V, ints(ids), B)

    return L, fwd, bwd


def test_multiblank_entries_refuse_before_any_hip_call():
    """Dummy device pointers that are never dereferenced: each call is refused by the host-side check it names; what is
    not refused is an empty batch, which succeeds without a launch."""
    if torch.cuda.is_available():
        pytest.skip("host-only table: replayed where no GPU is visible (its pointers are made up)")
    L, fwd, bwd = _entries()
    odd = ctypes.c_void_p(258)
    eight = tuple(range(8))
    shared = [dict(dtype=-1), dict(dtype=3),                                  # a bad dtype
              dict(V=4, ids=(0, 1, 2, 3)), dict(V=4), dict(V=1), dict(V=0),   # V < B + 1
              dict(ids=(6, 5, 4, 7)), dict(ids=(6, 5, 4, -1)), dict(ids=(6, 5, 4, 6)),      # an id out of range, repeated
              dict(ids=None), dict(ids=(), B=0), dict(ids=tuple(range(9)), V=12),           # null, B of 0 and 9
              dict(logits=None), dict(labels=None), dict(N=-1), dict(N=70000), dict(T=0), dict(U=0), dict(U=1025),
              dict(U=1025, T=1), dict(T=1 << 20, U=1 << 10), dict(logits=ctypes.c_void_p(257)), dict(labels=odd)]
    for kw in shared:
        fkw = dict(kw)
        if kw.get("ids") is not None and len(kw["ids"]) != 4:            # (durations of the ids' count)
            fkw["durations"] = tuple(range(1, len(kw["ids"]) + 1)) or (1,)
        assert fwd(**fkw) == INVALID, kw
        assert bwd(**kw) == INVALID, kw
        if "N" not in kw:       # a refused argument is not answered as an empty batch
            assert fwd(N=0, **fkw) == INVALID and bwd(N=0, **kw) == INVALID, kw
    # bad durations: a 0, a 9, a repeat, no 1, a null pointer
    for durations in ((1, 2, 4, 0), (1, 2, 4, 9), (1, 2, 2, 4), (2, 3, 4, 8), (1, 2, 4, -1)):
        assert fwd(durations=durations) == INVALID, durations
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
    for ids, durations, V in (((0,), (1,), 2), ((3, 0), (2, 1), 4), ((1, 2, 3), (4, 1, 2), 4), (eight, (8, 7, 6, 5, 4, 3, 2, 1), 9)):
        assert fwd(ids=ids, durations=durations, V=V, N=0) == SUCCESS, (ids, durations)
        assert bwd(ids=ids, V=V, N=0) == SUCCESS, ids


def test_a_lattice_of_1025_columns_is_refused():
    L, fwd, bwd = _entries()
    size = L.rnnt_amd_multiblank_workspace_size
    assert size(1, 4, 1025, 4) == 0 and size(1, 4, 1024, 4) > 0
    if not torch.cuda.is_available():       # (made-up pointers: only where nothing can be launched)
        assert fwd(N=1, T=4, U=1025) == INVALID and bwd(N=1, T=4, U=1025) == INVALID
        assert fwd(N=0, T=4, U=1024) == SUCCESS
    from warp_rnnt_amd import ops
    with pytest.raises(RuntimeError, match="status 5.*unsupported sizes.*U=1025"):
        ops._workspace("cpu", size, "N T U B", 1, 4, 1025, 4)


def test_workspace_size_is_a_function_of_the_shape_and_monotone():
    L = _lib()
    size = L.rnnt_amd_multiblank_workspace_size
    assert len(size.argtypes) == 4          # (N, T, U, B) and nothing else
    base = (3, 20, 7, 4)
    assert size(*base) == size(*base) > 0
    # at least the planes the header names: 1 + B channels, alpha, beta
    assert size(*base) >= 4 * 3 * 20 * 7 * (1 + 4 + 2)
    for k, hi in enumerate((40, 200, 1024, 8)):
        sizes = [size(*(base[:k] + (v,) + base[k + 1:])) for v in range(1, hi + 1)]
        assert all(s > 0 for s in sizes), k
        assert all(a <= b for a, b in zip(sizes, sizes[1:])), k
        for v, s in zip(range(1, hi + 1), sizes):
            N, T, U, B = base[:k] + (v,) + base[k + 1:]
            assert s >= 4 * N * T * U * (1 + B + 2), (k, v)
    for bad in ((-1, 20, 7, 4), (3, 0, 7, 4), (3, 20, 0, 4), (3, 20, 7, 0), (3, 20, 7, 9), (3, 20, 1025, 4), (70000, 20, 7, 4)):
        assert size(*bad) == 0, bad


# ---- the additive contract ----

def test_header_declares_what_the_table_binds_and_the_library_exports(monkeypatch):
    import warp_rnnt_amd
    from warp_rnnt_amd import _build, _lib as lib
    L = _lib()
    table = lib.MULTIBLANK_SYMBOLS
    assert set(table) == ENTRIES and lib.ADDITIVE_MULTIBLANK == ((table, HEADER),)
    vp, i, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    assert table["rnnt_amd_multiblank_workspace_size"] == (ctypes.c_size_t, [i, i, i, i])
    assert table["rnnt_amd_multiblank_loss_logits"] == (i, [vp, vp, i] + [vp] * 6 + [i, vp, vp] + [i] * 4 + [f, f])
    assert table["rnnt_amd_multiblank_logits_backward"] == (i, [vp, i] + [vp] * 5 + [i] * 4 + [vp, i])
    text = open(os.path.join(ROOT, "include", HEADER)).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(run_[a-z_]+|rnnt_amd_[a-z_]+)\s*\(", code))
    assert declared == set(table)
    assert '#include "warp_rnnt_amd.h"' in text
    # the argument counts of the two calls, in the header's order
    for name, count in (("rnnt_amd_multiblank_loss_logits", 18), ("rnnt_amd_multiblank_logits_backward", 13)):
        body = re.search(name + r"\((.*?)\);", code, re.S).group(1)
        assert len(body.split(",")) == count == len(table[name][1]), name
    main = open(os.path.join(ROOT, "include", "warp_rnnt_amd.h")).read()
    earlier = lib.ADDITIVE + lib.ADDITIVE_NEXT + lib.ADDITIVE_TDT_JOINT + lib.ADDITIVE_PRUNED + lib.ADDITIVE_SIMPLE
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
    assert "multiblank.hip" in _build.SOURCES and "multiblank.h" in _build.HEADERS
    assert "multiblank.hip" not in _build.HAZARD_CHECKED and "multiblank.hip" not in _build.RELOAD_CHECKED
    source = open(os.path.join(_build.CSRC, "multiblank.hip")).read()
    assert "asm" not in re.sub(r"//.*", "", source)
    assert "#pragma clang fp contract(off)" in source
    # the older tuples are what they were
    assert [h for _, h in lib.ADDITIVE] == ["warp_rnnt_amd_clamp.h", "warp_rnnt_amd_joint_dropout.h", "warp_rnnt_amd_hat.h",
                                            "warp_rnnt_amd_align.h", "warp_rnnt_amd_tdt.h"]
    assert lib.ADDITIVE_NEXT == ((lib.TDT_ALIGN_SYMBOLS, "warp_rnnt_amd_tdt_align.h"),)
    assert lib.ADDITIVE_TDT_JOINT == ((lib.TDT_JOINT_SYMBOLS, "warp_rnnt_amd_tdt_joint.h"),)
    assert lib.ADDITIVE_PRUNED == ((lib.PRUNED_SYMBOLS, "warp_rnnt_amd_pruned.h"),)
    assert lib.ADDITIVE_SIMPLE == ((lib.SIMPLE_SYMBOLS, "warp_rnnt_amd_simple.h"),)
    # a stale library (same version, built before the entries existed) is refused with the rebuild message
    monkeypatch.setattr(lib, "_lib", None)
    monkeypatch.setitem(table, "rnnt_amd_no_such_entry", (ctypes.c_int, [ctypes.c_float]))
    with pytest.raises(RuntimeError, match=r"rnnt_amd_no_such_entry \(include/" + re.escape(HEADER) + r"\).*rebuild it"):
        lib.load()


# ---- Python ----

def test_public_signature_and_argument_errors_on_cpu_tensors():
    from warp_rnnt_amd import multiblank, ops
    params = inspect.signature(multiblank.multiblank_loss_from_logits).parameters
    assert list(params) == ["logits", "labels", "frames_lengths", "labels_lengths", "big_blank_durations", "sigma", "blank",
                            "big_blank_ids", "fastemit_lambda", "average_frames", "reduction"]
    assert [params[k].default for k in list(params)[4:]] == [(2, 4, 8), 0.0, 0, None, 0.0, False, "none"]
    assert list(inspect.signature(ops.multiblank_loss).parameters) == ["logits", "labels", "xn", "yn", "blank_ids",
                                                                        "blank_durations", "sigma", "fastemit_lambda",
                                                                        "with_grads"]
    assert list(inspect.signature(ops.multiblank_logits_backward).parameters) == ["logits", "labels", "grads",
                                                                                   "grad_costs", "blank_ids"]
    batch = (torch.zeros((2, 3, 2, 9)), torch.ones((2, 1), dtype=torch.int32), torch.tensor([3, 2], dtype=torch.int32),
             torch.tensor([1, 1], dtype=torch.int32))
    with pytest.raises(AssertionError):
        multiblank.multiblank_loss_from_logits(*batch, blank=8, reduction="avg")
    with pytest.raises(AssertionError):
        multiblank.multiblank_loss_from_logits(*batch, blank=8.0)
    with pytest.raises(RuntimeError, match="must be located in the CUDA"):
        multiblank.multiblank_loss_from_logits(*batch, blank=8)
    with pytest.raises(RuntimeError, match="ys must be a Int tensor"):
        multiblank.multiblank_loss_from_logits(batch[0], batch[1].long(), batch[2], batch[3], blank=8)
    # big_blank_ids=None is NeMo's kernel convention, blank - 1 - i: the standard blank is entry 0 with duration 1
    assert multiblank.blank_set(8, (2, 4, 8)) == ((8, 7, 6, 5), (1, 2, 4, 8))
    assert multiblank.blank_set(0, (4, 2), (5, 6)) == ((0, 5, 6), (1, 4, 2))
    assert multiblank.blank_set(3, ()) == ((3,), (1,))
    with pytest.raises(ValueError, match="one id per big-blank duration"):
        multiblank.blank_set(0, (2, 4), (5,))
    # ... so with the default blank = 0 its ids fall outside [0, V): refused with the reason, on CPU tensors, before anything
    # touches the device
    with pytest.raises(RuntimeError, match=r"status 5.*blank ids.*\[0, V\)"):
        multiblank.multiblank_loss_from_logits(*batch)
    with pytest.raises(RuntimeError, match=r"status 5.*blank ids.*\[0, V\)"):
        multiblank.multiblank_loss_from_logits(*batch, blank=0, big_blank_ids=(7, 8, 9))
    # what depends on values is refused with its reason
    for durations in ((1, 2, 9), (1, 0), (1, 2, 2), (2, 4), (), tuple(range(1, 10))):
        with pytest.raises(RuntimeError, match="status 5.*durations"):
            ops._multiblank_check(20, tuple(range(len(durations))), durations, 0.0)
    for ids in ((0, 0, 1), (0, 1)):
        with pytest.raises(RuntimeError, match="status 5.*one distinct blank id per duration"):
            ops._multiblank_check(9, ids, (1, 2, 4), 0.0)
    for V, ids in ((9, (0, 9, 1)), (9, (-1, 2, 3)), (3, (0, 1, 2))):
        with pytest.raises(RuntimeError, match=r"status 5.*blank ids.*\[0, V\)"):
            ops._multiblank_check(V, ids, (1, 2, 4), 0.0)
    for sigma in (-1.0, float("nan"), float("inf")):
        with pytest.raises(RuntimeError, match="status 5.*sigma"):
            ops._multiblank_check(9, (8, 7), (1, 2), sigma)
    assert ops._multiblank_check(9, (8, 2, 5), (1, 4, 2), 0.05) == ([8, 2, 5], [1, 4, 2])
    module = multiblank.MultiblankLoss(big_blank_durations=[2, 4], sigma=0.05, blank=8, big_blank_ids=[1, 2],
                                       fastemit_lambda=0.01, reduction="sum")
    assert isinstance(module, torch.nn.Module)
    assert (module.big_blank_durations, module.sigma, module.blank, module.big_blank_ids, module.fastemit_lambda,
            module.reduction) == ((2, 4), 0.05, 8, (1, 2), 0.01, "sum")
    for word in ("compact layout", "joint entry", "align entry", "gradient clamp", "mismatch guard", "U > 1024"):
        assert word in multiblank.multiblank_loss_from_logits.__doc__ and word in multiblank.__doc__, word
    import warp_rnnt_amd
    assert "multiblank.py" in warp_rnnt_amd.__doc__ and not hasattr(warp_rnnt_amd, "multiblank_loss_from_logits")
