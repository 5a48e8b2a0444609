"""The gather and scatter kernels of the packed (compact=True) layout, bit for bit: every route through csrc/compact.hip
and csrc/expand.hip against the plain statement of tests/compact_reference.py and against each other.  These kernels do no
arithmetic (the scatter: one fp32 multiply), they go wrong by index -- so apart from the two tolerances this path has
always had against the fp32 oracle (rtol 1e-5 on costs, atol 1e-4 on gradient pairs) every comparison here is exact.

Which test reaches which kernel:
    k_gather_compact (32x32 tiles, N > 4096)        test_tiled_gather, test_bounded_tiled_gather
    k_gather_compact_linear (N <= 4096)             test_route_switch, test_linear_gather_seams, the halves of test_tiled_gather
    k_gather_compact_rowmajor                       the reference-named route of all of them
    k_expand_small<CompactRows>                     test_scatter_backward, V <= 1024 on an aligned output
    k_expand_large<4, CompactRows>                  test_scatter_backward, V in {1028}
    k_expand_large<1, CompactRows>                  test_scatter_backward, V in {1025, 2050}; V in {4, 1028} one float off
    k_turn_compact32<true / false>, k_split_pairs_compact32   test_staged_turns_odd_total
"""
import numpy as np
import pytest
import torch

import compact_reference as cr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(autouse=True)
def seen_diagnostics():
    """An utterance without frames is reported through the sticky diagnostics words (warp_rnnt_amd/_mismatch.py), which
    the next loss call turns into a RuntimeWarning: looked at here, so that no report of this file reaches a later test."""
    yield
    import warnings
    import warp_rnnt_amd
    torch.cuda.synchronize()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        warp_rnnt_amd.last_mismatch()


def T(a):
    a = np.asarray(a)
    return torch.tensor(a if a.ndim == 0 else np.ascontiguousarray(a), device=DEV)


def host(results):
    return tuple(None if r is None else r.cpu().numpy() for r in results)


def poison(case):
    """The native entries allocate their results with torch.empty, and the caching allocator likes to hand back the block
    an identical call has just released -- with that call's correct results in it.  Blocks of the results' sizes are
    filled with NaN / -77 and released first, so that a cell no kernel writes does not pass for written (best effort)."""
    junk = [torch.full((case.N,), float("nan"), device=DEV), torch.full((case.STU, 2), float("nan"), device=DEV),
            torch.full((case.STU,), -77, dtype=torch.int64, device=DEV)]
    torch.cuda.synchronize()
    del junk


def native(case, **bounds):
    """(costs, grads2, loc) of _C.rnnt_loss_compact / ops.loss_compact: the tiled gather from 4097 utterances on, the linear
    one below."""
    poison(case)
    if bounds:
        from warp_rnnt_amd import ops
        out = ops.loss_compact(T(case.xs), T(case.ys), T(case.xn), T(case.yn), case.blank, case.lam, **bounds)
    else:
        import warp_rnnt._C as core
        out = core.rnnt_loss_compact(T(case.xs), T(case.ys), T(case.xn), T(case.yn), blank=case.blank,
                                     fastemit_lambda=case.lam)
    torch.cuda.synchronize()
    return host(out)


def reference_named(case):
    """(costs, grads2, loc), pairs of the reference's own call sequence (binding.cpp:139-207) on the reference-named entry
    points: run_gather_for_compact (k_gather_compact_rowmajor) and run_warp_rnnt_compact, 32-bit exclusive prefixes, raw
    pointers, NULL stream."""
    import warp_rnnt_amd
    L = warp_rnnt_amd.load()
    N, V, STU = case.N, case.V, case.STU
    txs, tys, txn, tyn = T(case.xs), T(case.ys), T(case.xn), T(case.yn)
    tmem, tlab = T(case.offs[:-1].astype(np.int32)), T(case.label_offs[:-1].astype(np.int32))
    Tmax, Umax = int(case.xn.max()), int(case.yn.max()) + 1
    pairs = torch.full((STU, 2), float("nan"), device=DEV)
    loc = torch.full((STU,), -77, dtype=torch.int64, device=DEV)
    torch.cuda.synchronize()
    L.run_gather_for_compact(txs.data_ptr(), tys.data_ptr(), txn.data_ptr(), tyn.data_ptr(), pairs.data_ptr(),
                             loc.data_ptr(), tmem.data_ptr(), tlab.data_ptr(), N, Tmax, Umax, V, case.blank)
    torch.cuda.synchronize()
    assert L.rnnt_amd_compact_last_status() == 0
    costs = torch.full((N,), float("nan"), device=DEV)
    counts = torch.zeros((int(case.ys.size) * 2 + 2 * N,), dtype=torch.int32, device=DEV)
    alphas, betas = torch.empty((STU,), device=DEV), torch.empty((STU,), device=DEV)
    grads = torch.full_like(pairs, float("nan"))
    L.run_warp_rnnt_compact(counts.data_ptr(), alphas.data_ptr(), betas.data_ptr(), pairs.data_ptr(), grads.data_ptr(),
                            costs.data_ptr(), txn.data_ptr(), tyn.data_ptr(), tmem.data_ptr(), tlab.data_ptr(), N, Tmax,
                            Umax, case.lam, True)
    torch.cuda.synchronize()
    assert L.rnnt_amd_compact_last_status() == 0
    return host((costs, grads, loc)), pairs.cpu().numpy()


def check_routes(case, got):
    """What every batch of this file is held to: loc exact, the pairs of the reference-named gather exact, its results
    the native route's bits, the oracle within the path's two tolerances."""
    cr.assert_loc(got[2], case)
    named, pairs = reference_named(case)
    cr.assert_pairs(pairs, case)
    cr.assert_same_results(named, got, f"{case.name}: reference-named route against the native one")
    cr.assert_oracle(got[0], got[1], case)


def joined(parts):
    return tuple(np.concatenate([p[i] for p in parts]) for i in range(3))


# ---------------------------------------------------------------------------------------------------------------------
# The tiled gather and the switch between the two
# ---------------------------------------------------------------------------------------------------------------------
TILE_EDGE_PARAMS = [(0, 0.0), (0, 0.01), (4, 0.0), (4, 0.01)]


@pytest.mark.parametrize("blank,lam", TILE_EDGE_PARAMS)
def test_tiled_gather(blank, lam):
    """N = 4097: k_gather_compact with partial tiles, dead tiles, utterances without labels and without frames, labels
    outside the vocabulary.  The same utterances as two calls of 2048 and 2049 (the linear gather) must give the same bits:
    results never depend on the batch."""
    case = cr.tile_edge_case(blank, lam)
    assert case.N == cr.LINEAR_MAX_N + 1 and case.STU < 120000
    got = native(case)
    check_routes(case, got)
    halves = joined([native(case.subset(0, 2048)), native(case.subset(2048, case.N))])
    cr.assert_same_results(halves, got, "two calls of 2048 + 2049 utterances against one of 4097")


@pytest.mark.parametrize("blank,lam", [(0, 0.0), (4, 0.01)])
def test_bounded_tiled_gather(blank, lam):
    """ops.loss_compact with the caller's launch bounds reaches the same kernel with another grid: the true maxima, and
    Tmax = 100, Umax = 70 with more dead tiles.  That entry refuses a batch that holds an utterance without frames (NaN
    costs, zero gradients: rnnt_amd_loss_compact_bounded) -- which is asserted on the batch of test_tiled_gather; the
    bit-equality is asserted on the same batch with one frame in place of none."""
    refused = native(cr.tile_edge_case(blank, lam), max_frames=100, max_labels=69)
    assert np.isnan(refused[0]).all() and not refused[1].any()
    case = cr.tile_edge_case(blank, lam, empties=False)
    assert case.N == cr.LINEAR_MAX_N + 1 and case.live().all()
    got = native(case)
    cr.assert_loc(got[2], case)
    cr.assert_oracle(got[0], got[1], case)
    true_max = native(case, max_frames=int(case.xn.max()), max_labels=int(case.yn.max()))
    cr.assert_same_results(true_max, got, "bounded by the true maxima against unbounded")
    loose = native(case, max_frames=100, max_labels=69)
    cr.assert_same_results(loose, got, "bounded by Tmax = 100, Umax = 70 against unbounded")


@pytest.mark.parametrize("blank,lam", [(0, 0.0), (4, 0.01)])
def test_route_switch(blank, lam):
    """The batch of test_tiled_gather without its last utterance: N = 4096, the last batch of the linear kernel, per
    utterance the bits of the tiled one."""
    full = cr.tile_edge_case(blank, lam)
    case = full.subset(0, cr.LINEAR_MAX_N)
    got = native(case)
    check_routes(case, got)
    tiled = native(full)
    cut = int(case.STU)
    cr.assert_same_results(got, (tiled[0][:case.N], tiled[1][:cut], tiled[2][:cut]), "N = 4096 against N = 4097")


# ---------------------------------------------------------------------------------------------------------------------
# Seams of the linear gather
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cr.SEAM_CASES)
def test_linear_gather_seams(name):
    """k_gather_compact_linear's owner search where utterances meet its 1024-cell chunks (compact_reference.seam_case)."""
    case = cr.seam_case(name)
    assert case.N <= cr.LINEAR_MAX_N
    check_routes(case, native(case))


# ---------------------------------------------------------------------------------------------------------------------
# The scatter backward
# ---------------------------------------------------------------------------------------------------------------------
def expand_rows_per_tile(V):
    """launch_rows (expand.hip): rows per workgroup of k_expand_small."""
    return max(4, 3200 // V // 4 * 4)


def scatter_entries():
    import warp_rnnt_amd
    L = warp_rnnt_amd.load()

    def named(gc, g2, loc, cum, out_ptr, STU, N, V, blank):
        torch.cuda.synchronize()                                     # (NULL stream)
        L.run_scatter_grad_for_compact(gc.data_ptr(), g2.data_ptr(), loc.data_ptr(), cum.data_ptr(), out_ptr, STU, N, V,
                                       blank)
        torch.cuda.synchronize()
        assert L.rnnt_amd_compact_last_status() == 0

    def abi(gc, g2, loc, cum, out_ptr, STU, N, V, blank):
        st = L.rnnt_amd_compact_scatter_grads(torch.cuda.current_stream().cuda_stream, gc.data_ptr(), g2.data_ptr(),
                                              loc.data_ptr(), cum.data_ptr(), out_ptr, STU, N, V, blank)
        assert st == 0

    return (("run_scatter_grad_for_compact", named), ("rnnt_amd_compact_scatter_grads", abi))


@pytest.mark.parametrize("N", [1, 7])
@pytest.mark.parametrize("V", [1, 3, 4, 6, 401, 801, 1023, 1024, 1025, 1028, 2050])
def test_scatter_backward(V, N):
    """_C.rnnt_loss_compact_backward and the two C entries on synthetic inputs, into NaN between two guard rows: every
    written row scatter_reference's bits, nothing unwritten, nothing beyond.  Rows: two whole tiles of k_expand_small and
    three rows more (not a multiple of four, a partial tile), at least one row per vocabulary index; and one row alone.
    V in {4, 1028}: once more with the output one float off 16-byte alignment (k_expand_large<1>)."""
    import warp_rnnt._C as core
    R = expand_rows_per_tile(V)
    rows_many = max(2 * R, (V + 4 + 3) // 4 * 4) + 3
    assert rows_many % 4 == 3 and rows_many % R != 0 and rows_many > R
    for blank in sorted({0, V - 1}):
        for STU in (rows_many, 1):
            gc, g2, loc, cum = cr.scatter_inputs(V, N, STU, blank)
            tgc, tg2, tloc, tcum = T(gc), T(g2), T(loc), T(cum)
            dense = core.rnnt_loss_compact_backward(tgc, tg2, tcum, tloc, V, blank).cpu().numpy()
            cr.assert_same_bits(dense, cr.scatter_reference(gc, g2, loc, cum, V, blank),
                                f"rnnt_loss_compact_backward V={V} N={N} STU={STU} blank={blank}")
            for shift in ((0, 1) if V in (4, 1028) else (0,)):
                size, start = cr.guarded_buffer_layout(V, STU, shift)
                for entry, call in scatter_entries():
                    buf = torch.full((size,), float(cr.GUARD), device=DEV)
                    assert buf.data_ptr() % 16 == 0
                    buf[start:start + STU * V] = float("nan")
                    out_ptr = buf.data_ptr() + 4 * start
                    assert out_ptr % 16 == 4 * shift
                    call(tgc, tg2, tloc, tcum, out_ptr, STU, N, V, blank)
                    torch.cuda.synchronize()
                    cr.assert_scatter(buf.cpu().numpy(), start, gc, g2, loc, cum, V, blank,
                                      f"{entry} V={V} N={N} STU={STU} blank={blank} shift={shift}")


# ---------------------------------------------------------------------------------------------------------------------
# The staged turns
# ---------------------------------------------------------------------------------------------------------------------
def test_staged_turns_odd_total():
    """run_warp_rnnt_compact from 2^20 cells of launch bound on: k_turn_compact32<true>, the sweeps, k_split_pairs_compact32
    and k_turn_compact32<false> -- with an odd number of live cells (the split's lone last cell) and an utterance without
    rows last (xn[N-1] in the split's total).  Bit-equal to the native entry."""
    case = cr.staged_case()
    assert case.N * int(case.xn.max()) * int(case.yn.max() + 1) >= 1 << 20 and case.STU % 2 == 1 and case.xn[-1] == 0
    named, pairs = reference_named(case)
    cr.assert_pairs(pairs, case)
    cr.assert_loc(named[2], case)
    got = native(case)
    cr.assert_same_results(named, got, "staged reference-named route against the native one")
    assert np.isnan(got[0][-1]) and np.isfinite(got[0][:-1]).all()
