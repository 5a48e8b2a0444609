"""k2's modified topology and delay penalty for the pruned and the simple loss, without a GPU: the fp64 reference
(tests/modified_reference.py) against brute-force enumeration and central differences; the shear identity the kernels are
built on -- the modified lattice is the regular one on the sheared plane with a virtual terminal cell; the regular form
against tests/pruned_reference.py; the C entries' refusals with pointers that are never dereferenced; the workspace sizes;
the additive contract of include/warp_rnnt_amd_topology.h and its table; the front ends' signatures and argument errors."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import modified_reference as mr
import pruned_reference as pr
import simple_reference as sr
from oracle import transduce_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "warp_rnnt_amd_topology.h"
ENTRIES = {"rnnt_amd_pruned_topology_workspace_size", "rnnt_amd_simple_topology_workspace_size",
           "rnnt_amd_pruned_loss_logits_topology", "rnnt_amd_pruned_logits_backward_topology",
           "rnnt_amd_simple_loss_topology", "rnnt_amd_simple_backward_topology"}
INVALID, SUCCESS = 5, 0
REGULAR, MODIFIED = 0, 1
ALIGN = 256


def _lib():
    import warp_rnnt_amd
    from warp_rnnt_amd import _build
    _build.build()          # hipcc cross-compiles for gfx950 without a GPU; no-op when up to date
    return warp_rnnt_amd.load()


def _window(seed, T, U):
    """A random (T, U + 1) window of log-prob pairs (not normalised: the lattices do not ask for it)."""
    rng = np.random.RandomState(seed)
    return np.log(rng.uniform(0.05, 0.6, size=(T, U + 1))), np.log(rng.uniform(0.05, 0.6, size=(T, U + 1)))


# ---- the reference ----

@pytest.mark.parametrize("dp", [0.0, 0.3])
@pytest.mark.parametrize("rnnt_type", ["regular", "modified"])
@pytest.mark.parametrize("T,U", [(1, 1), (3, 3), (4, 1), (5, 3), (6, 4)])
def test_recurrence_against_enumeration_of_all_paths(T, U, rnnt_type, dp):
    lpb, lpl = _window(10 * T + U, T, U)
    lpl = mr.penalised(lpl, T, dp)
    cost, gb, gl = mr.window64(lpb, lpl, rnnt_type)
    want = mr.brute_force_cost(lpb, lpl, rnnt_type)
    print(f"T{T} U{U} {rnnt_type} dp {dp}: recurrence {cost:.12f} enumeration {want:.12f}")
    assert np.isfinite(want)
    np.testing.assert_allclose(cost, want, rtol=1e-13)
    # every path of the modified lattice takes T edges, U of them labels: the occupancies say so
    if rnnt_type == "modified":
        np.testing.assert_allclose(-(gb + gl).sum(1), np.ones(T), rtol=1e-12)
        np.testing.assert_allclose(-gl.sum(), U, rtol=1e-12)


def test_modified_without_a_path_and_the_single_path():
    lpb, lpl = _window(3, 2, 3)                               # T_n = 2 < U_n = 3
    assert np.isinf(mr.window64(lpb, lpl, "modified")[0]) and np.isinf(mr.brute_force_cost(lpb, lpl, "modified"))
    assert np.isfinite(mr.window64(lpb, lpl, "regular")[0])
    lpb, lpl = _window(4, 3, 3)                               # T_n == U_n: the all-label path
    cost, gb, gl = mr.window64(lpb, lpl, "modified")
    np.testing.assert_allclose(cost, -(lpl[0, 0] + lpl[1, 1] + lpl[2, 2]), rtol=1e-14)
    assert (gb == 0).all() and np.allclose(np.diag(gl[:, :3]), -1.0)
    lpb, lpl = _window(5, 4, 0)                               # no labels: the blanks of every frame, none behind them
    np.testing.assert_allclose(mr.window64(lpb, lpl, "modified")[0], -lpb[:, 0].sum(), rtol=1e-14)


@pytest.mark.parametrize("rnnt_type", ["regular", "modified"])
def test_reference_gradient_against_central_differences(rnnt_type):
    """pruned64 is what judges the kernels: its d/d logits against central differences of its own costs."""
    N, T, U, S, V, blank, dp = 2, 5, 4, 3, 5, 2, 0.3
    logits, labels, starts, xn, yn = pr.make_band_case(17, N, T, U, S, V, blank=blank, lengths=((5, 4), (3, 2)))
    z = logits.astype(np.float64)
    go = mr.upstream(N)
    ref = mr.pruned64(z, labels, starts, xn, yn, blank, 0.0, dp, rnnt_type)
    assert np.isfinite(ref["costs"]).all() and (ref["dlogits"] != 0).any()
    h = 1e-5
    num = np.zeros_like(z)
    for idx in np.ndindex(*z.shape):
        zp, zm = z.copy(), z.copy()
        zp[idx] += h
        zm[idx] -= h
        cp = mr.pruned64(zp, labels, starts, xn, yn, blank, 0.0, dp, rnnt_type)["costs"]
        cm = mr.pruned64(zm, labels, starts, xn, yn, blank, 0.0, dp, rnnt_type)["costs"]
        num[idx] = go[idx[0]] * (cp[idx[0]] - cm[idx[0]]) / (2 * h)
    print(f"{rnnt_type}: largest difference {np.abs(ref['dlogits'] - num).max():.3e}")
    np.testing.assert_allclose(ref["dlogits"], num, rtol=0, atol=1e-6)
    lam = mr.pruned64(z, labels, starts, xn, yn, blank, 0.01, dp, rnnt_type)
    np.testing.assert_allclose(lam["pair_grads"][..., 1], 1.01 * ref["pair_grads"][..., 1], rtol=1e-14)
    np.testing.assert_array_equal(lam["pair_grads"][..., 0], ref["pair_grads"][..., 0])


@pytest.mark.parametrize("dp", [0.0, 0.3])
@pytest.mark.parametrize("T,U", [(1, 1), (3, 3), (4, 1), (5, 3), (6, 4), (7, 0), (1, 0), (9, 5)])
def test_the_modified_lattice_is_the_regular_one_on_the_sheared_plane(T, U, dp):
    """What the kernels run: the regular lattice (the existing references) over the cells (t - u, u) with T - U + 1
    frames and a virtual terminal cell whose blank is 0 -- costs and every cell's gradient pair to 1e-12."""
    lpb, lpl = _window(100 * T + U, T, U)
    lpl = mr.penalised(lpl, T, dp)
    cost, gb, gl = mr.window64(lpb, lpl, "modified", 0.01)
    sb, sl = mr.sheared_window(lpb, lpl)
    Tp, W = sb.shape
    assert (Tp, W) == (T - U + 1, U + 1)
    pairs = np.stack([sb, sl], -1)[None]
    costs, pg = sr.lattice64(pairs, np.array([Tp]), np.array([U]), 0.01)              # (tests/simple_reference.py)
    print(f"T{T} U{U} dp {dp}: modified {cost:.15f} sheared regular {costs[0]:.15f}")
    np.testing.assert_allclose(costs[0], cost, rtol=1e-12)
    tp, u = np.meshgrid(np.arange(Tp), np.arange(W), indexing="ij")
    real = tp + u < T
    np.testing.assert_allclose(pg[0][real][:, 0], gb[(tp + u)[real], u[real]], rtol=0, atol=1e-12)
    np.testing.assert_allclose(pg[0][real][:, 1], gl[(tp + u)[real], u[real]], rtol=0, atol=1e-12)
    np.testing.assert_allclose(pg[0, Tp - 1, W - 1], (-1.0, 0.0), rtol=0, atol=1e-12)   # the terminal cell's pair
    # ... and the window is exactly the set of modified cells on a path: every other cell's gradient is zero
    on_path = np.zeros((T, W), bool)
    on_path[(tp + u)[real], u[real]] = True
    assert (gb[~on_path] == 0).all() and (gl[~on_path] == 0).all()
    # the same through the band recursion of tests/pruned_reference.py: one "logit row" per cell
    al, be = transduce_np._sweeps_fast(sb, np.where(u == W - 1, -np.inf, sl))
    np.testing.assert_allclose(-be[0, 0], cost, rtol=1e-12)


def test_regular_without_a_penalty_is_the_pruned_reference():
    N, T, U, S, V, blank = 3, 7, 5, 3, 6, 2
    logits, labels, starts, xn, yn = pr.make_band_case(5, N, T, U, S, V, blank=blank)
    for lam in (0.0, 0.01):
        got = mr.pruned64(logits, labels, starts, xn, yn, blank, lam, 0.0, "regular")
        want = pr.pruned_loss64(logits, labels, starts, xn, yn, blank, lam)
        for key in ("costs", "dlogits", "pair_grads"):
            np.testing.assert_array_equal(got[key], want[key])
    am, lm, labels, xn, yn = sr.make_case(6, N, T, U, V, blank=blank)
    got = mr.simple64(am, lm, labels, xn, yn, blank, 0.25, 0.01, 0.0, "regular")
    want = sr.simple_loss64(am, lm, labels, xn, yn, blank, 0.25, 0.0, 0.01)
    np.testing.assert_array_equal(got["costs"], want["costs"])
    np.testing.assert_array_equal(got["pair_grads"], want["pair_grads"])
    np.testing.assert_allclose(got["dam"], want["dam"], rtol=0, atol=1e-14)
    np.testing.assert_allclose(got["dlm"], want["dlm"], rtol=0, atol=1e-14)
    # the penalty moves the regular cost too, and by what the label edges of a path carry
    pen = mr.pruned64(logits, labels, starts, xn, yn, blank, 0.0, 0.3, "regular")
    assert (np.abs(pen["costs"] - want["costs"]) > 1e-3).any()


# ---- the C entries ----

def test_entries_refuse_before_any_hip_call():
    """Dummy device pointers that are never dereferenced: each call is refused by the host-side check it names."""
    if torch.cuda.is_available():
        pytest.skip("host-only table: replayed where no GPU is visible (its pointers are made up)")
    L = _lib()
    p = ctypes.c_void_p(256)                 # aligned, non-null, never dereferenced
    inf, nan = float("inf"), float("nan")

    def pf(ws=p, dtype=0, logits=p, labels=p, starts=p, xn=p, yn=p, costs=p, grads=p, N=2, T=3, U=4, S=2, V=5, blank=0,
           topology=MODIFIED, dp=0.1):
        return L.rnnt_amd_pruned_loss_logits_topology(None, ws, dtype, logits, labels, starts, xn, yn, costs, grads, N, T, U,
                                                      S, V, blank, 0.0, topology, dp)

    def pb(dtype=0, logits=p, labels=p, starts=p, xn=p, yn=p, grads=p, go=p, out=p, N=2, T=3, U=4, S=2, V=5, blank=0,
           topology=MODIFIED):
        return L.rnnt_amd_pruned_logits_backward_topology(None, dtype, logits, labels, starts, xn, yn, grads, go, out, N, T,
                                                          U, S, V, blank, topology)

    def sf(ws=p, dtype=0, am=p, lm=p, q=p, labels=p, xn=p, yn=p, costs=p, grads=p, znorm=p, N=2, T=3, U=4, V=5, blank=0,
           topology=MODIFIED, dp=0.1):
        return L.rnnt_amd_simple_loss_topology(None, ws, dtype, am, lm, q, labels, xn, yn, costs, grads, znorm, N, T, U, V,
                                               blank, 0.25, 0.0, 0.0, topology, dp)

    def sb(ws=p, dtype=0, am=p, lm=p, q=p, labels=p, xn=p, yn=p, grads=p, znorm=p, go=p, dam=p, dlm=p, dq=p, N=2, T=3,
           U=4, V=5, blank=0, topology=MODIFIED):
        return L.rnnt_amd_simple_backward_topology(None, ws, dtype, am, lm, q, labels, xn, yn, grads, znorm, go, dam, dlm,
                                                   dq, N, T, U, V, blank, 0.25, 0.0, topology)

    # T * U < 2^29 <= (T + 1) * U: the regular topology takes the shape, the modified plane of T + 1 rows does not
    tips = dict(N=1, T=(1 << 15) - 1, U=1 << 14)
    for topology in (REGULAR, MODIFIED):
        # an unknown topology; what the namesakes refuse
        shared = [dict(topology=-1), dict(topology=2), dict(dtype=3), dict(V=1), dict(blank=5), dict(labels=None),
                  dict(N=-1), dict(N=70000), dict(T=0), dict(U=0), dict(T=1 << 15, U=1 << 14)]
        for kw in shared:
            kw = dict(dict(topology=topology), **kw)
            for fn in (pf, pb, sf, sb):
                args = dict(kw, S=1) if kw.get("U") == 0 and fn in (pf, pb) else kw
                assert fn(**args) == INVALID, (fn.__name__, kw)
                if "N" not in kw:                # a refused argument is not answered as an empty batch
                    assert fn(N=0, **args) == INVALID, (fn.__name__, kw)
        for dp in (-1.0, nan, inf, -inf):
            assert pf(topology=topology, dp=dp) == INVALID and sf(topology=topology, dp=dp) == INVALID, dp
            assert pf(topology=topology, dp=dp, N=0) == INVALID and sf(topology=topology, dp=dp, N=0) == INVALID, dp
        for fn in (pf, pb, sf, sb):
            assert fn(topology=topology, N=0) == SUCCESS, fn.__name__
            assert fn(topology=topology, N=0, **{k: v for k, v in tips.items() if k != "N"}) == \
                (SUCCESS if topology == REGULAR else INVALID), fn.__name__
        for fn in (pf, sf):
            assert fn(topology=topology, N=0, dp=0.0) == SUCCESS
            for kw in (dict(ws=None), dict(ws=ctypes.c_void_p(264)), dict(costs=None), dict(xn=None), dict(yn=None)):
                assert fn(topology=topology, **kw) == INVALID, (fn.__name__, kw)
    assert pf(S=5) == INVALID and pb(S=0) == INVALID and pf(starts=None) == INVALID and pb(starts=None) == INVALID
    # the modified pruned backward reads the lengths; the regular one does not
    assert pb(xn=None) == INVALID and pb(yn=None) == INVALID and pb(xn=None, N=0) == INVALID
    assert pb(topology=REGULAR, xn=None, yn=None, N=0) == SUCCESS
    for kw in (dict(grads=None), dict(out=None), dict(grads=ctypes.c_void_p(260))):
        assert pb(**kw) == INVALID, kw
    for kw in (dict(grads=None), dict(znorm=None), dict(dam=None), dict(dlm=None), dict(xn=None), dict(yn=None)):
        assert sb(**kw) == INVALID, kw


def test_workspace_sizes():
    L = _lib()
    up = lambda b: (b + ALIGN - 1) // ALIGN * ALIGN
    for N, T, U in ((1, 1, 1), (2, 3, 4), (5, 12, 6), (16, 1500, 300), (3, 63, 65), (300, 40, 12)):
        reg, mod = (L.rnnt_amd_pruned_topology_workspace_size(k, N, T, U) for k in (REGULAR, MODIFIED))
        print(f"N{N} T{T} U{U}: pruned {reg} -> {mod} bytes")
        assert reg == L.rnnt_amd_workspace_size(N, T, U) > 0
        assert mod == L.rnnt_amd_workspace_size(N, T + 1, U) + up(4 * N) and mod >= reg
        sreg, smod = (L.rnnt_amd_simple_topology_workspace_size(k, N, T, U) for k in (REGULAR, MODIFIED))
        assert sreg == L.rnnt_amd_simple_workspace_size(N, T, U) > 0
        # the simple entries' statistics lie behind the lattice's layout, sized by (N, T, U) in both topologies
        assert smod - mod == sreg - reg and smod >= sreg
    for size in (L.rnnt_amd_pruned_topology_workspace_size, L.rnnt_amd_simple_topology_workspace_size):
        assert size(2, 2, 3, 4) == 0 and size(-1, 2, 3, 4) == 0 and size(MODIFIED, 2, 0, 4) == 0
        assert size(REGULAR, 1, (1 << 15) - 1, 1 << 14) > 0 and size(MODIFIED, 1, (1 << 15) - 1, 1 << 14) == 0


def test_header_declares_what_the_table_binds_and_the_library_exports(monkeypatch):
    import warp_rnnt_amd
    from warp_rnnt_amd import _build, _lib as lib
    L = _lib()
    table = lib.TOPOLOGY_SYMBOLS
    assert set(table) == ENTRIES and lib.ADDITIVE_TOPOLOGY == ((table, HEADER),)
    assert (lib.TOPOLOGY_REGULAR, lib.TOPOLOGY_MODIFIED) == (REGULAR, MODIFIED)
    i, f, vp = ctypes.c_int, ctypes.c_float, ctypes.c_void_p
    # the namesakes' argument lists with the topology (the forwards: and the penalty) behind them; xn, yn behind the starts
    pruned_b = lib.PRUNED_SYMBOLS["rnnt_amd_pruned_logits_backward"][1]
    assert table["rnnt_amd_pruned_loss_logits_topology"][1] == lib.PRUNED_SYMBOLS["rnnt_amd_pruned_loss_logits"][1] + [i, f]
    assert table["rnnt_amd_pruned_logits_backward_topology"][1] == pruned_b[:5] + [vp, vp] + pruned_b[5:] + [i]
    assert table["rnnt_amd_simple_loss_topology"][1] == lib.SIMPLE_SYMBOLS["rnnt_amd_simple_loss"][1] + [i, f]
    assert table["rnnt_amd_simple_backward_topology"][1] == lib.SIMPLE_SYMBOLS["rnnt_amd_simple_backward"][1] + [i]
    text = open(os.path.join(ROOT, "include", HEADER)).read()
    declared = set(re.findall(r"\b(run_[a-z_]+|rnnt_amd_[a-z_]+)\s*\(", text))
    assert declared == set(table)
    assert '#include "warp_rnnt_amd.h"' in text
    assert re.search(r"#define RNNT_TOPOLOGY_REGULAR 0\b", text) and re.search(r"#define RNNT_TOPOLOGY_MODIFIED 1\b", text)
    for phrase in ("0.5f * (float)(T_n - 1) - (float)t", "t' = t - u", "(n * (T+1) + t) * U + u", "no terminal blank"):
        assert phrase in text, phrase                                      # the definition, the shear, the plane's layout
    main = open(os.path.join(ROOT, "include", "warp_rnnt_amd.h")).read()
    earlier = (lib.ADDITIVE + lib.ADDITIVE_NEXT + lib.ADDITIVE_TDT_JOINT + lib.ADDITIVE_PRUNED + lib.ADDITIVE_SIMPLE +
               lib.ADDITIVE_MULTIBLANK)
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
    # the older tables are what they were
    assert set(lib.PRUNED_SYMBOLS) == {"rnnt_amd_pruned_loss_logits", "rnnt_amd_pruned_logits_backward"}
    assert set(lib.SIMPLE_SYMBOLS) == {"rnnt_amd_simple_workspace_size", "rnnt_amd_simple_loss", "rnnt_amd_simple_backward"}
    # a stale library (same version, built before the entries existed) is refused with the rebuild message
    monkeypatch.setattr(lib, "_lib", None)
    monkeypatch.setitem(table, "rnnt_amd_no_such_entry", (ctypes.c_int, [ctypes.c_float]))
    with pytest.raises(RuntimeError, match=r"rnnt_amd_no_such_entry \(include/" + re.escape(HEADER) + r"\).*rebuild it"):
        lib.load()


def test_public_signatures_and_argument_errors_on_cpu_tensors():
    from warp_rnnt_amd import ops, pruned, simple
    # the two front ends take the keywords behind their positional signatures, which stay what they were (the tests of
    # the two losses pin them): keyword-only, defaults "regular" and 0.0
    for fn in (pruned.pruned_rnnt_loss_from_logits, simple.simple_rnnt_loss):
        own = inspect.signature(fn, follow_wrapped=False).parameters
        assert [k for k, v in own.items() if v.kind is inspect.Parameter.KEYWORD_ONLY] == ["rnnt_type", "delay_penalty"]
        assert (own["rnnt_type"].default, own["delay_penalty"].default) == ("regular", 0.0)
        assert "rnnt_type" in fn.__doc__ and "delay_penalty" in fn.__doc__ and "constrained" in fn.__doc__
    for cls in (pruned.PrunedRNNTLoss, simple.SimpleRNNTLoss):
        params = inspect.signature(cls.__init__).parameters
        assert (params["rnnt_type"].default, params["delay_penalty"].default) == ("regular", 0.0)
        module = cls(rnnt_type="modified", delay_penalty=0.1)
        assert (module.rnnt_type, module.delay_penalty) == ("modified", 0.1)
        with pytest.raises(ValueError, match="constrained"):
            cls(rnnt_type="constrained")
    assert list(inspect.signature(ops.pruned_loss_topology).parameters)[-2:] == ["topology", "delay_penalty"]
    assert list(inspect.signature(ops.pruned_logits_backward_topology).parameters) == [
        "logits", "labels", "starts", "xn", "yn", "grads", "grad_costs", "blank", "topology"]
    assert list(inspect.signature(ops.simple_loss_topology).parameters)[-2:] == ["topology", "delay_penalty"]
    assert list(inspect.signature(ops.simple_backward_topology).parameters)[-1] == "topology"
    assert ops.topology_of("regular", 0.0) == (REGULAR, 0.0) and ops.topology_of("modified", 0.5) == (MODIFIED, 0.5)
    N, T, U, S, V = 2, 3, 4, 2, 7
    labels, xn, yn = (torch.ones((N, U - 1), dtype=torch.int32), torch.tensor([3, 2], dtype=torch.int32),
                      torch.tensor([3, 1], dtype=torch.int32))
    batch = (torch.zeros((N, T, S, V)), labels, torch.zeros((N, T), dtype=torch.int32), xn, yn)
    first = (torch.zeros((N, T, V)), torch.zeros((N, U, V)), labels, xn, yn)
    for fn, args in ((pruned.pruned_rnnt_loss_from_logits, batch), (simple.simple_rnnt_loss, first)):
        for bad in ("constrained", "Modified", "", None):
            with pytest.raises(ValueError, match='"constrained" topology is not covered'):
                fn(*args, rnnt_type=bad)
        for dp in (-0.1, float("nan"), float("inf")):
            with pytest.raises(ValueError, match="delay_penalty"):
                fn(*args, rnnt_type="modified", delay_penalty=dp)
        # the keywords are looked at first, the tensors as ever behind them
        with pytest.raises(RuntimeError, match="must be located in the CUDA"):
            fn(*args, rnnt_type="modified", delay_penalty=0.1)
    assert "modified" in pruned.__doc__ and "constrained" in pruned.__doc__.split("Out of scope")[1]
    assert "modified" not in pruned.__doc__.split("Out of scope")[1]
