"""The factorised-blank loss on the pruned band without a GPU: the fp64 reference (tests/pruned_hat_reference.py) against
the enumeration of all paths, the two C entries' refusals beside their twins' with pointers that are never dereferenced,
and the additive contract of include/warp_rnnt_amd_pruned_hat.h and its table."""
import ctypes
import os
import re

import numpy as np
import pytest

import hat_reference as hr
import modified_reference as mr
import pruned_hat_reference as phr
import pruned_reference as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "warp_rnnt_amd_pruned_hat.h"
INVALID, SUCCESS = 5, 0
REGULAR, MODIFIED = 0, 1


def _lib():
    import warp_rnnt_amd
    from warp_rnnt_amd import _build
    _build.build()          # hipcc cross-compiles for gfx950 without a GPU; no-op when up to date
    return warp_rnnt_amd.load()


@pytest.mark.parametrize("rnnt_type", ["regular", "modified"])
@pytest.mark.parametrize("S", [1, 2, "U"])
@pytest.mark.parametrize("T,U", [(1, 1), (2, 2), (4, 3), (5, 4), (3, 4)])
def test_reference_against_enumeration_of_all_paths(T, U, S, rnnt_type):
    S = U if S == "U" else min(S, U)
    N, V, blank, dp = 2, 4, 1, 0.3
    logits, labels, starts, xn, yn = pr.make_band_case(100 * T + 10 * U + S, N, T, U, S, V, blank=blank)
    if rnnt_type == "modified" and S < U:
        starts = np.zeros((N, T), np.int32)
        for n in range(N):                       # a diagonal band: frame t holds column min(t, hi), the modified path's
            starts[n] = np.minimum(np.arange(T), max(int(yn[n]) + 1 - S, 0))
    ref = phr.pruned_hat64(logits, labels, starts, xn, yn, blank, dp=dp, rnnt_type=rnnt_type)
    plain = phr.pruned_hat64(logits, labels, starts, xn, yn, blank)["costs"]
    for n in range(N):
        Tn, W = int(xn[n]), int(yn[n]) + 1
        lpb, lpl, _ = phr.window_pairs64(logits[n], labels[n], starts[n], Tn, W, blank, dp)
        # ... and the regular lattice without a penalty by the pruned reference's own enumeration
        flat = pr.brute_force_cost(hr.hat_log_probs64(logits[n], blank), labels[n], starts[n], Tn, W, blank)
        for got, want in ((ref["costs"][n], mr.brute_force_cost(lpb, lpl, rnnt_type)), (plain[n], flat)):
            assert np.isinf(want) == np.isinf(got) and (np.isinf(want) or abs(got - want) <= 1e-12 * max(1.0, abs(want))), n
        assert np.isfinite(ref["costs"][n]) or (ref["dlogits"][n] == 0).all()
    assert np.isfinite(ref["costs"]).any() or (rnnt_type == "modified" and T < U), "the case holds no path at all"


def test_entries_refuse_what_their_twins_refuse_before_any_hip_call():
    """Made-up pointers and a null stream: every call is refused by a host-side check or is an empty batch."""
    L = _lib()
    p, nan, inf = ctypes.c_void_p(256), float("nan"), float("inf")

    def fwd(fn, ws=p, dtype=0, logits=p, labels=p, starts=p, xn=p, yn=p, costs=p, grads=p, N=2, T=3, U=4, S=2, V=5, blank=0,
            topology=MODIFIED, dp=0.1):
        return fn(None, ws, dtype, logits, labels, starts, xn, yn, costs, grads, N, T, U, S, V, blank, 0.0, topology, dp)

    def bwd(fn, dtype=0, logits=p, labels=p, starts=p, xn=p, yn=p, grads=p, go=p, out=p, N=2, T=3, U=4, S=2, V=5, blank=0,
            topology=MODIFIED):
        return fn(None, dtype, logits, labels, starts, xn, yn, grads, go, out, N, T, U, S, V, blank, topology)

    both = [dict(topology=-1), dict(topology=2), dict(dtype=3), dict(V=1), dict(blank=5), dict(blank=-1), dict(labels=None),
            dict(N=-1), dict(N=70000), dict(T=0), dict(U=0, S=1), dict(T=1 << 15, U=1 << 14), dict(S=0), dict(S=5),
            dict(logits=None), dict(starts=None)]
    forward = both + [dict(dp=-1.0), dict(dp=nan), dict(dp=inf), dict(ws=None), dict(ws=ctypes.c_void_p(264)),
                      dict(costs=None), dict(xn=None), dict(yn=None)]
    backward = both + [dict(grads=None), dict(grads=ctypes.c_void_p(260)), dict(out=None)]
    pairs = ((fwd, forward, L.rnnt_amd_pruned_hat_loss_logits, L.rnnt_amd_pruned_loss_logits_topology),
             (bwd, backward, L.rnnt_amd_pruned_hat_logits_backward, L.rnnt_amd_pruned_logits_backward_topology))
    for call, refused, mine, twin in pairs:
        for topology in (REGULAR, MODIFIED):
            for kw in refused:
                kw = dict(dict(topology=topology), **kw)
                assert call(mine, **kw) == call(twin, **kw) == INVALID, (mine.__name__, kw)
                if "N" not in kw:                # a refused argument is not answered as an empty batch
                    assert call(mine, N=0, **kw) == call(twin, N=0, **kw) == INVALID, (mine.__name__, kw)
            assert call(mine, topology=topology, N=0) == call(twin, topology=topology, N=0) == SUCCESS
    # the modified backward reads the lengths; the regular one does not
    hb = L.rnnt_amd_pruned_hat_logits_backward
    assert bwd(hb, xn=None) == INVALID and bwd(hb, yn=None) == INVALID and bwd(hb, xn=None, N=0) == INVALID
    assert bwd(hb, topology=REGULAR, xn=None, yn=None, N=0) == SUCCESS


def test_header_declares_what_the_table_binds_and_the_version_did_not_move():
    from warp_rnnt_amd import _build, _lib as lib
    L = _lib()
    table = lib.PRUNED_HAT_SYMBOLS
    assert lib.ADDITIVE_PRUNED_HAT == ((table, HEADER),)
    with open(os.path.join(ROOT, "include", HEADER)) as f:
        declared = set(re.findall(r"\b(rnnt_amd_\w+)\s*\(", f.read().split("#ifndef")[1]))
    assert declared == set(table) == {"rnnt_amd_pruned_hat_loss_logits", "rnnt_amd_pruned_hat_logits_backward"}
    twins = lib.TOPOLOGY_SYMBOLS                 # the argument lists of the two ..._topology pruned entries
    assert table["rnnt_amd_pruned_hat_loss_logits"] == twins["rnnt_amd_pruned_loss_logits_topology"]
    assert table["rnnt_amd_pruned_hat_logits_backward"] == twins["rnnt_amd_pruned_logits_backward_topology"]
    for name, (res, args) in table.items():
        fn = getattr(L, name)
        assert fn.restype is res and list(fn.argtypes) == list(args)
    assert L.rnnt_amd_version() == lib.ABI_VERSION == 110
    assert "pruned_hat.hip" in _build.SOURCES and "pruned_hat.h" in _build.HEADERS
    assert any(os.path.basename(h) == HEADER for h in _build.HEADERS)
    assert len(lib.ADDITIVE) == 5 and lib.ADDITIVE_PRUNE_RANGES == ((lib.PRUNE_RANGES_SYMBOLS, "warp_rnnt_amd_prune_ranges.h"),)
    # the front end: keyword-only, off by default
    from warp_rnnt_amd import pruned
    with pytest.raises(TypeError):
        pruned.pruned_rnnt_loss_from_logits(None, None, None, None, None, False, "none", 0, 0.0, True)
    assert pruned.PrunedRNNTLoss().use_hat_loss is False and pruned.PrunedRNNTLoss(use_hat_loss=True).use_hat_loss is True
