"""The gather, turn and expand kernels of the padded (N,T,U,V) layout, bit for bit: every route through csrc/to_diagonal.hip
and the dense row writers of csrc/expand.hip against the plain statement of tests/dense_layout_reference.py (held to loops,
the oracle and torch on the CPU by tests/test_host_dense_layout.py) and against each other.  These kernels do no arithmetic
beyond one fp32 multiply or add, they go wrong by index -- a tile edge, the (t+u) mod T wrap when U > T, an odd last cell,
a tail that is no whole group of rows, a label that equals the blank, a sentinel in the padding, an output one float off
alignment -- so every comparison here is exact: bit for bit, and where dense rows are made from real gradients value for
value (assert_same_values: the sign of a zero aside), with one exception (test_expand_sum: two products added in one slot).

Inputs are pairwise different floats (bit pattern 0x3F800000 + index) wherever no sweep has to run on them; every output
is NaN before the call and sits between two guards of 64 floats that must come back untouched; a workspace is NaN as a
whole, and what no kernel of the call owns must still be NaN afterwards.

Which test reaches which kernel:
    k_to_diagonal<true, 8, false / true>     test_dense_gather_8_frame_tiles; the N = 7 half of ..._the_switch
    k_to_diagonal<true, 32, false / true>    test_dense_gather_32_frame_tiles_and_the_switch, test_dense_gather_wide_lattice
    k_to_diagonal<false, 8, false>           test_relayout_of_pairs_8_frame_tiles; the small shapes of test_the_way_back
    k_to_diagonal<false, 32, false>          test_relayout_of_pairs_32_frame_tiles; the large shapes of test_the_way_back
    k_gather_rowmajor                        test_rowmajor_gather
    k_from_diagonal<false>                   test_the_way_back, >= 2^20 cells, the native GRADS_GATHERED result
    k_split_pairs, k_from_diagonal<true>     test_the_way_back, >= 2^20 cells, run_warp_rnnt_gather (odd cell count: 3 x 611 x 573)
    k_grads' row-major writer                test_the_way_back, the shape below 2^20 cells
    k_expand_small<PaddedRows>               test_expand_sum / test_expand_overwrite, V <= 1024 on an aligned output
    k_expand_large<4, PaddedRows>            the same two, V in {1028, 2052}
    k_expand_large<1, PaddedRows>            the same two, V in {1025, 1030}; V in {4, 50, 1028} one float off alignment
    k_expand_small<GradRows>                 test_one_launch_against_two, V = 50
    k_expand_large<4, GradRows>              test_one_launch_against_two, V = 1028
    k_expand_small<SplitRows>, k_split_pairs test_staged_dense_entry_expands_from_two_planes (run_warp_rnnt, 3 x 611 x 573, V = 3)

Left out on purpose: SplitRows with the large writers (run_warp_rnnt from 2^20 cells on with V > 1024: gigabytes); the ring
preparation folded into the gather's tail (the sweep tests own it: a sweep on unprepared rings does not finish its
lattice); strided inputs (the entries take none).
"""
import numpy as np
import pytest
import torch

import dense_layout_reference as dr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64                   # floats in front of and behind every output
GUARD_VALUE = -77.0
NAN_BITS = 0x7FC00000        # what torch.full(..., nan) writes
STAGED_FROM_CELLS = 1 << 20  # api_common.h: from here on the gathered gradients are turned through LDS tiles
IN_DENSE, IN_GATHERED = 0, 1
GRADS_GATHERED, GRADS_DIAGONAL, GRADS_DENSE = 0, 1, 2


@pytest.fixture(autouse=True)
def seen_diagnostics():
    """A guard that fires in a sweep behind one of these calls (the wide lattice's log-likelihood is in the thousands) is
    reported through the sticky diagnostics words, which the next loss call of the process turns into a RuntimeWarning:
    looked at here, so that no report of this file reaches a later test."""
    yield
    import warnings
    import warp_rnnt_amd
    torch.cuda.synchronize()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        warp_rnnt_amd.last_mismatch()


def lib():
    import warp_rnnt_amd
    return warp_rnnt_amd.load()


def stream():
    return torch.cuda.current_stream().cuda_stream


def dev(a):
    return None if a is None else torch.tensor(np.ascontiguousarray(a), device=DEV)


def ptr(t):
    return 0 if t is None else t.data_ptr()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_same_values(got, want, what):
    """Exact, for dense rows made from REAL gradients: those underflow to -0.0 where a path is improbable enough, and the
    row writers add their two slots into +0.0 (k_expand_small the label slot, k_expand_large both), which the slot writes
    of the plain statement do not -- the sign of a zero is not part of it.  Every non-zero value has all its bits, and
    nothing is left unwritten."""
    assert not np.isnan(got).any(), f"{what}: slots nobody wrote"
    np.testing.assert_array_equal(got, want, err_msg=what)


class Guarded:
    """`size` floats of NaN on the device between two guards, the first of them `shift` floats off 16-byte alignment."""

    def __init__(self, size, shift=0):
        self.size, self.start = int(size), GUARD + shift
        self.buf = torch.full((self.start + self.size + GUARD,), GUARD_VALUE, device=DEV)
        assert self.buf.data_ptr() % 256 == 0
        self.buf[self.start:self.start + self.size] = float("nan")
        self.ptr = self.buf.data_ptr() + 4 * self.start
        assert self.ptr % 16 == 4 * (shift % 4)

    def result(self, what=""):
        torch.cuda.synchronize()
        h = self.buf.cpu().numpy()
        assert (h[:self.start] == GUARD_VALUE).all(), f"{what}: written in front of the output"
        assert (h[self.start + self.size:] == GUARD_VALUE).all(), f"{what}: written behind the output"
        return h[self.start:self.start + self.size]


def workspace(N, T, U):
    size = lib().rnnt_amd_workspace_size(N, T, U)
    off = dr.workspace_offsets(N, T, U)
    assert size % 256 == 0 and size >= off["mismatch"] + 4 * N
    return Guarded(size // 4), off


def tiles32(N, T, U):
    return N * ((T + 31) // 32) * ((U + 31) // 32)


def assert_pair_plane(ws_bits, off, want_diag, what, rest_is_poison):
    """The workspace's pair plane holds want_diag's bits; the slack behind it up to the next plane is still NaN; with
    rest_is_poison everything else of the workspace is too."""
    lo, cells = off["pairs"] // 4, off["cells"]
    np.testing.assert_array_equal(ws_bits[lo:lo + 2 * cells], bits(want_diag).ravel(), err_msg=f"{what}: pair plane")
    assert (ws_bits[lo + 2 * cells:off["ll"] // 4] == NAN_BITS).all(), f"{what}: written behind the pair plane"
    if rest_is_poison:
        assert (ws_bits[:lo] == NAN_BITS).all() and (ws_bits[off["ll"] // 4:] == NAN_BITS).all(), \
            f"{what}: written outside the pair plane"


# ---------------------------------------------------------------------------------------------------------------------
# a, b. The dense gather into the diagonal-major pair plane
# ---------------------------------------------------------------------------------------------------------------------
def dense_gather(lp, labels, blank, with_plane, what):
    """rnnt_amd_debug_gather_only[_blank_plane] on a NaN workspace, everything checked against the reference; returns
    the pair plane's bits.  The plane handed over is NOT the blank column: channel 0 must be the plane's float, channel
    1 the row's -- each from where it should come."""
    N, T, U, V = lp.shape
    L = lib()
    ws, off = workspace(N, T, U)
    tlp, tlab = dev(lp), dev(labels)
    want = dr.gather(lp, labels, blank)
    if with_plane:
        plane = dr.distinct_floats((N, T, U), first=0x40000000)
        tplane = dev(plane)
        want[..., 0] = plane
        st = L.rnnt_amd_debug_gather_only_blank_plane(stream(), ws.ptr, tlp.data_ptr(), tplane.data_ptr(), ptr(tlab), N, T,
                                                      U, V, blank)
    else:
        st = L.rnnt_amd_debug_gather_only(stream(), ws.ptr, tlp.data_ptr(), ptr(tlab), N, T, U, V, blank)
    assert st == 0, what
    got = bits(ws.result(what))
    assert_pair_plane(got, off, dr.to_diagonal(want), what, rest_is_poison=True)
    np.testing.assert_array_equal(bits(tlp.cpu().numpy()), bits(lp), err_msg=f"{what}: the log-probs changed")
    if with_plane:
        np.testing.assert_array_equal(bits(tplane.cpu().numpy()), bits(plane), err_msg=f"{what}: the plane changed")
    return got[off["pairs"] // 4:off["pairs"] // 4 + 2 * off["cells"]].reshape(N, T, U, 2)


def vocabularies():
    for V in (1, 2, 33, 130):
        for blank in sorted({0, V - 1, V // 2}):
            yield V, blank


T_EDGES = [1, 7, 8, 9, 31, 32, 33]
U_EDGES = [1, 2, 31, 32, 33, 65]


@pytest.mark.parametrize("U", U_EDGES)
@pytest.mark.parametrize("T", T_EDGES)
def test_dense_gather_8_frame_tiles(T, U):
    """Both axes around the edges of the 8 x 32 tiles, T < U (the wrap), one frame, one column (labels NULL), labels that
    are the blank, -1 / V+7 / INT_MIN in the padding; every vocabulary with the blank first, last and in the middle."""
    N = 3
    assert tiles32(N, T, U) < 512
    for V, blank in vocabularies():
        lp = dr.distinct_floats((N, T, U, V))
        labels = dr.sentinel_labels(N, U, V, blank, seed=T * 100 + U)
        for with_plane in (False, True):
            dense_gather(lp, labels, blank, with_plane, f"T={T} U={U} V={V} blank={blank} plane={with_plane}")


def test_dense_gather_32_frame_tiles_and_the_switch():
    """(8,225,225,5): 512 tiles of 32 x 32, the first batch of the 32-frame form, both axes ending one cell into a tile;
    its first seven utterances alone: 448 tiles, the 8-frame form, the same bits."""
    T, U, V, blank = 225, 225, 5, 2
    assert tiles32(8, T, U) == 512 and tiles32(7, T, U) == 448
    lp = dr.distinct_floats((8, T, U, V))
    labels = dr.sentinel_labels(8, U, V, blank, seed=1)
    for with_plane in (False, True):
        big = dense_gather(lp, labels, blank, with_plane, f"N=8 plane={with_plane}")
        small = dense_gather(lp[:7], labels[:7], blank, with_plane, f"N=7 plane={with_plane}")
        if not with_plane:                  # (with it, channel 0 is the test's plane, numbered per batch)
            np.testing.assert_array_equal(big[:7], small, err_msg="utterances 0..6: 32-frame tiles against 8-frame tiles")
        else:
            np.testing.assert_array_equal(big[:7, ..., 1], small[..., 1])


def test_dense_gather_wide_lattice():
    """(2,33,4097,3): 516 tiles, the 32-frame form with T < U: a second tile row of one frame, the last tile column of one
    lattice column, and (t+u) mod T taken up to 124 times round."""
    N, T, U, V, blank = 2, 33, 4097, 3, 2
    assert tiles32(N, T, U) == 516
    lp = dr.distinct_floats((N, T, U, V))
    labels = dr.sentinel_labels(N, U, V, blank, seed=2)
    for with_plane in (False, True):
        dense_gather(lp, labels, blank, with_plane, f"wide plane={with_plane}")


# ---------------------------------------------------------------------------------------------------------------------
# The loss entry on the test's own buffers
# ---------------------------------------------------------------------------------------------------------------------
def log_softmax32(x):
    x = np.asarray(x, dtype=np.float32)
    m = x.max(axis=-1, keepdims=True)
    s = np.exp(x - m, dtype=np.float32).sum(axis=-1, keepdims=True, dtype=np.float32)
    return ((x - m) - np.log(s, dtype=np.float32)).astype(np.float32)


def real_pairs(N, T, U, seed):
    """(N,T,U,2) log-prob pairs a sweep behaves on: two of three classes of a log-softmax."""
    rng = np.random.RandomState(seed)
    return np.ascontiguousarray(log_softmax32(rng.randn(N, T, U, 3).astype(np.float32))[..., :2])


def loss(input_kind, grads_kind, x, labels, xn, yn, blank=0, lam=0.0, what=""):
    """rnnt_amd_loss on a NaN workspace, NaN costs and NaN gradients, all guarded: (costs, grads, workspace bits, offsets)."""
    N, T, U, V = x.shape
    L = lib()
    ws, off = workspace(N, T, U)
    costs = Guarded(N)
    grads = Guarded(N * T * U * (V if grads_kind == GRADS_DENSE else 2))
    tx, tlab, txn, tyn = dev(x), dev(labels), dev(np.asarray(xn, np.int32)), dev(np.asarray(yn, np.int32))
    st = L.rnnt_amd_loss(stream(), ws.ptr, input_kind, tx.data_ptr(), ptr(tlab), txn.data_ptr(), tyn.data_ptr(), costs.ptr,
                         grads.ptr, grads_kind, N, T, U, V, blank, float(lam))
    assert st == 0, what
    g = grads.result(what + ": grads").reshape(N, T, U, -1)
    np.testing.assert_array_equal(bits(tx.cpu().numpy()), bits(x), err_msg=f"{what}: the input changed")
    return costs.result(what + ": costs"), g, bits(ws.result(what + ": workspace")), off


def ragged(N, T, U):
    """Lengths that keep utterance n's last n label columns (sentinel_labels' padding) out of the lattice: the first
    utterance full, one without labels, one of a single frame."""
    xn = np.array([T, max(1, T - 5), 1] + [T] * N, dtype=np.int32)[:N]
    yn = np.array([U - 1, 0, (U - 1) // 2] + [max(0, U - 1 - N)] * N, dtype=np.int32)[:N]
    return xn, yn


# ---------------------------------------------------------------------------------------------------------------------
# c. The re-layout of row-major pairs
# ---------------------------------------------------------------------------------------------------------------------
def relayout(N, T, U, seed):
    """RNNT_IN_LOG_PROBS_GATHERED with RNNT_GRADS_GATHERED_DIAGONAL: the only kind whose gradients go straight to the caller
    (api_loss.hip: every other kind of >= 2^20 cells, and NONE and DENSE at any size, produce theirs in the pair plane), so the
    plane k_to_diagonal<false> wrote is still there when the call is over."""
    lp2 = real_pairs(N, T, U, seed)
    xn, yn = ragged(N, T, U)
    what = f"re-layout N={N} T={T} U={U}"
    _, _, ws_bits, off = loss(IN_GATHERED, GRADS_DIAGONAL, lp2, None, xn, yn, what=what)
    assert_pair_plane(ws_bits, off, dr.to_diagonal(lp2), what, rest_is_poison=False)


@pytest.mark.parametrize("U", [1, 2, 33, 65])
@pytest.mark.parametrize("T", [1, 8, 9, 33])
def test_relayout_of_pairs_8_frame_tiles(T, U):
    assert tiles32(3, T, U) < 512
    relayout(3, T, U, seed=T * 100 + U)


@pytest.mark.parametrize("N,T,U", [(8, 225, 225), (2, 33, 4097)])
def test_relayout_of_pairs_32_frame_tiles(N, T, U):
    assert tiles32(N, T, U) >= 512
    relayout(N, T, U, seed=N)


# ---------------------------------------------------------------------------------------------------------------------
# d. The row-major gather
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("U", [1, 2, 33, 65])
@pytest.mark.parametrize("T", [1, 9, 33])
def test_rowmajor_gather(T, U):
    """rnnt_amd_gather (what ops.gather calls) into a guarded buffer: 891 ... 6435 cells, no multiple of its 256-thread
    workgroups; sentinels, blank != 0, labels NULL for one column."""
    from warp_rnnt_amd import ops
    N, L = 3, lib()
    for V, blank in vocabularies():
        what = f"T={T} U={U} V={V} blank={blank}"
        lp = dr.distinct_floats((N, T, U, V))
        labels = dr.sentinel_labels(N, U, V, blank, seed=T + U)
        out = Guarded(N * T * U * 2)
        tlp, tlab = dev(lp), dev(labels)
        assert L.rnnt_amd_gather(stream(), tlp.data_ptr(), ptr(tlab), out.ptr, N, T, U, V, blank) == 0
        want = dr.gather(lp, labels, blank)
        np.testing.assert_array_equal(bits(out.result(what)).reshape(N, T, U, 2), bits(want), err_msg=what)
        np.testing.assert_array_equal(bits(tlp.cpu().numpy()), bits(lp), err_msg=f"{what}: the log-probs changed")
        if V == 33:
            np.testing.assert_array_equal(bits(ops.gather(tlp, tlab, blank).cpu().numpy()), bits(want), err_msg=what)


# ---------------------------------------------------------------------------------------------------------------------
# e. The way back
# ---------------------------------------------------------------------------------------------------------------------
def reference_named_gathered(lp2, xn, yn, lam, what):
    """run_warp_rnnt_gather on the caller's buffers as the reference's binding allocates them (binding.cpp:58-75)."""
    N, T, U, _ = lp2.shape
    L = lib()
    counts = torch.zeros((N, 2 * U), dtype=torch.int32, device=DEV)
    alphas, betas, grads, costs = Guarded(N * T * U), Guarded(N * T * U), Guarded(N * T * U * 2), Guarded(N)
    tx, txn, tyn = dev(lp2), dev(np.asarray(xn, np.int32)), dev(np.asarray(yn, np.int32))
    st = L.run_warp_rnnt_gather(stream(), counts.data_ptr(), alphas.ptr, betas.ptr, tx.data_ptr(), grads.ptr, costs.ptr,
                                txn.data_ptr(), tyn.data_ptr(), N, T, U, float(lam))
    assert st == 0, what
    alphas.result(what + ": alphas")
    betas.result(what + ": betas")
    return costs.result(what + ": costs"), grads.result(what + ": grads").reshape(N, T, U, 2)


def tail_cell_frame(T, U):
    """The frame of the cell that sits last in an utterance's diagonal-major plane: row T-1, column U-1."""
    return (T - U) % T


WAY_BACK = [
    # N, T, U, FastEmit.  1 050 309 cells, odd (k_split_pairs' lone last cell), both axes end mid-tile
    (3, 611, 573, 0.01),
    # T a whole number of tiles, U one column past, T < U
    (1, 1024, 1025, 0.0),
    # below 2^20 cells: the gradient kernel writes row-major itself
    (3, 33, 34, 0.0),
]


@pytest.mark.parametrize("N,T,U,lam", WAY_BACK)
def test_the_way_back(N, T, U, lam):
    """The row-major GRADS_GATHERED result is from_diagonal of the GRADS_GATHERED_DIAGONAL result of the same arguments, and
    run_warp_rnnt_gather's result has the native one's bits.  Ragged; the last utterance ends in the very cell that is
    last in the planes -- its blank gradient is -1 or so, nothing a missing tail could pass for."""
    staged = N * T * U >= STAGED_FROM_CELLS
    lp2 = real_pairs(N, T, U, seed=T)
    xn, yn = ragged(N, T, U)
    xn[N - 1], yn[N - 1] = tail_cell_frame(T, U) + 1, U - 1
    what = f"N={N} T={T} U={U}"
    c_diag, g_diag, _, _ = loss(IN_GATHERED, GRADS_DIAGONAL, lp2, None, xn, yn, lam=lam, what=what + " diagonal")
    c_row, g_row, _, _ = loss(IN_GATHERED, GRADS_GATHERED, lp2, None, xn, yn, lam=lam, what=what + " row-major")
    assert np.isfinite(c_diag).all() and g_row[N - 1, xn[N - 1] - 1, U - 1, 0] < -0.5
    if (N * T * U) % 2:
        assert g_diag.reshape(-1, 2)[-1, 0] < -0.5, "the lone last cell of the split is a live one"
    np.testing.assert_array_equal(bits(c_row), bits(c_diag), err_msg=what)
    np.testing.assert_array_equal(bits(g_row), bits(dr.from_diagonal(g_diag)),
                                  err_msg=f"{what}: GATHERED against from_diagonal(GATHERED_DIAGONAL)")
    if not staged:                          # (below 2^20 cells the reference-named entry turns nothing: it sweeps and writes row-major)
        return
    c_named, g_named = reference_named_gathered(lp2, xn, yn, lam, what + " run_warp_rnnt_gather")
    np.testing.assert_array_equal(bits(c_named), bits(c_row), err_msg=what)
    np.testing.assert_array_equal(bits(g_named), bits(g_row), err_msg=f"{what}: run_warp_rnnt_gather against the native entry")


def test_staged_dense_entry_expands_from_two_planes():
    """run_warp_rnnt from 2^20 cells on stages the pairs in the caller's `grads`, parks the gradient pairs as two planes in
    alphas / betas (k_split_pairs, here with its lone last cell) and lets k_expand_small<SplitRows> write whole dense rows
    over the staging area: expand_overwrite of the native GRADS_GATHERED_DIAGONAL result of the same arguments, value for
    value, on a `grads` full of NaN.  Labels with the blank, sentinels in the padding and -- the last utterance -- inside
    the live range."""
    N, T, U, V, blank, lam = 3, 611, 573, 3, 1, 0.01
    assert N * T * U >= STAGED_FROM_CELLS and (N * T * U) % 2 == 1
    lp = log_softmax32(np.random.RandomState(7).randn(N, T, U, V).astype(np.float32))
    labels = dr.sentinel_labels(N, U, V, blank, seed=7)
    xn, yn = ragged(N, T, U)
    xn[N - 1], yn[N - 1] = tail_cell_frame(T, U) + 1, U - 1
    c_diag, g_diag, _, _ = loss(IN_DENSE, GRADS_DIAGONAL, lp, labels, xn, yn, blank, lam, "native diagonal")
    assert np.isfinite(c_diag).all() and g_diag.reshape(-1, 2)[-1, 0] < -0.5
    L = lib()
    counts = torch.zeros((N, 2 * U), dtype=torch.int32, device=DEV)
    alphas, betas, grads, costs = Guarded(N * T * U), Guarded(N * T * U), Guarded(N * T * U * V), Guarded(N)
    tx, tlab, txn, tyn = dev(lp), dev(labels), dev(xn), dev(yn)
    st = L.run_warp_rnnt(stream(), counts.data_ptr(), alphas.ptr, betas.ptr, tlab.data_ptr(), tx.data_ptr(), grads.ptr,
                         costs.ptr, txn.data_ptr(), tyn.data_ptr(), N, T, U, V, blank, lam)
    assert st == 0
    alphas.result("run_warp_rnnt: alphas")
    betas.result("run_warp_rnnt: betas")
    np.testing.assert_array_equal(bits(costs.result("run_warp_rnnt: costs")), bits(c_diag))
    got = grads.result("run_warp_rnnt: grads").reshape(N, T, U, V)
    assert_same_values(got, dr.expand_overwrite(g_diag, labels, xn, yn, V, blank), "run_warp_rnnt against the native pairs")


# ---------------------------------------------------------------------------------------------------------------------
# f. Expand, called directly
# ---------------------------------------------------------------------------------------------------------------------
def rows_per_tile(V):
    """launch_rows (expand.hip): rows per workgroup of k_expand_small."""
    return max(4, 3200 // V // 4 * 4)


# (N, T, U), V, floats off alignment
EXPAND_CASES = (
    [((3, 9, 34), V, 0) for V in (2, 3, 5, 50, 130, 799, 801, 1024)] +      # k_expand_small
    [((3, 33, 40), V, 0) for V in (1, 2, 3)] +                             # ... with whole tiles for the smallest V too
    [((2, 5, 7), V, 0) for V in (1028, 2052)] +                            # k_expand_large<4>
    [((2, 5, 7), V, 0) for V in (1025, 1030)] +                            # k_expand_large<1>: V no multiple of four
    [((3, 9, 34), 4, 1), ((3, 9, 34), 50, 1), ((2, 5, 7), 1028, 1)])       # k_expand_large<1>: the output misaligned
EXPAND_IDS = [f"{'x'.join(map(str, s))}-V{V}-off{o}" for s, V, o in EXPAND_CASES]


def test_expand_shapes_have_whole_tiles_and_a_tail():
    """k_expand_small serves R rows per workgroup: every small vocabulary above has a shape with a whole tile AND a tail tile
    that is no multiple of four rows -- except where R = 4 leaves a tail of two."""
    for V in sorted({V for _, V, o in EXPAND_CASES if V <= 1024 and o == 0}):
        R = rows_per_tile(V)
        shapes = [s for s, v, o in EXPAND_CASES if v == V and o == 0]
        assert any(np.prod(s) > R and np.prod(s) % R != 0 for s in shapes), (V, R)


def expand_inputs(shape, V, blank):
    """Diagonal pairs whose gL is non-zero EVERYWHERE (padding and column U-1 included), labels with the blank, sentinels in
    the padding and one inside the live range, ragged lengths with yn = 0 and xn = 1."""
    N, T, U = shape
    diag = dr.distinct_floats((N, T, U, 2))
    labels = dr.sentinel_labels(N, U, V, blank, seed=V)
    labels[0, 2] = -1
    xn = np.array([T, max(1, T - 2), 1], dtype=np.int32)[:N]
    yn = np.array([U - 1, 0, (U - 1) // 2], dtype=np.int32)[:N]
    return diag, labels, xn, yn


def expand(diag, labels, xn, yn, scale, V, blank, overwrite, shift, what):
    N, T, U, _ = diag.shape
    out = Guarded(N * T * U * V, shift)
    td, tl, txn, tyn, ts = dev(diag), dev(labels), dev(xn), dev(yn), dev(scale)
    st = lib().rnnt_amd_expand_grads(stream(), td.data_ptr(), ptr(tl), txn.data_ptr(), tyn.data_ptr(), ptr(ts), out.ptr,
                                     N, T, U, V, blank, overwrite)
    assert st == 0, what
    return out.result(what).reshape(N, T, U, V)


ARBITRARY = np.array([0.737, -1.3, 2.9], dtype=np.float32)
POWER_OF_TWO = np.array([0.5, -4.0, 2.0], dtype=np.float32)


@pytest.mark.parametrize("shape,V,shift", EXPAND_CASES, ids=EXPAND_IDS)
def test_expand_sum(shape, V, shift):
    """Sum mode (the gather=True backward): every slot expand_sum's bits with a power-of-two scale and without one.  With an
    arbitrary scale the cells whose label IS the blank (column U-1 included) add two rounded products in one slot, and
    the compiler may contract one product into the add: there, and only there, a result within one fp32 ulp of the fp64
    value gB*sc + gL*sc is accepted.  That bound holds for either evaluation because both products of a cell lie in one
    binade and their sum in the next (asserted): half an ulp of a product is a quarter ulp of the sum, so two rounded
    products and the rounded add are off by at most 1/4 + 1/4 + 1/2, a contracted one by 1/4 + 1/2."""
    N, T, U = shape
    for blank in sorted({0, V - 1}):
        diag, labels, xn, yn = expand_inputs(shape, V, blank)
        dup = dr.label_equals_blank(labels, N, T, U, V, blank)
        assert dup.sum() == T * (int((labels == blank).sum()) + N) and dup[..., U - 1].all()
        for name, scale in (("arbitrary", ARBITRARY[:N]), ("power of two", POWER_OF_TWO[:N]), ("NULL", None)):
            what = f"sum V={V} blank={blank} scale {name} shift={shift}"
            got = expand(diag, labels, xn, yn, scale, V, blank, 0, shift, what)
            want = dr.expand_sum(diag, labels, scale, V, blank)
            if name != "arbitrary":
                np.testing.assert_array_equal(bits(got), bits(want), err_msg=what)
                continue
            exempt = np.zeros(got.shape, dtype=bool)
            exempt[..., blank] = dup
            np.testing.assert_array_equal(bits(got)[~exempt], bits(want)[~exempt], err_msg=what)
            g = dr.from_diagonal(diag).astype(np.float64)
            sc = scale.astype(np.float64).reshape(N, 1, 1)
            pB, pL = g[..., 0] * sc, g[..., 1] * sc
            exact = pB + pL
            assert (np.frexp(pB)[1] == np.frexp(pL)[1]).all() and (np.frexp(exact)[1] == np.frexp(pB)[1] + 1).all()
            ulp = np.spacing(np.abs(exact).astype(np.float32)).astype(np.float64)
            err = np.abs(got[..., blank].astype(np.float64) - exact)
            assert (err[dup] <= ulp[dup]).all(), f"{what}: {np.max(err[dup] / ulp[dup])} ulp where label == blank"


@pytest.mark.parametrize("shape,V,shift", EXPAND_CASES, ids=EXPAND_IDS)
def test_expand_overwrite(shape, V, shift):
    """Overwrite mode (the gather=False forward's rule): the label slot only for t < xn, u < yn and a label inside the
    vocabulary, label == blank leaves gL in the blank slot; every other gL is dropped."""
    for blank in sorted({0, V - 1}):
        diag, labels, xn, yn = expand_inputs(shape, V, blank)
        what = f"overwrite V={V} blank={blank} shift={shift}"
        got = expand(diag, labels, xn, yn, None, V, blank, 1, shift, what)
        np.testing.assert_array_equal(bits(got), bits(dr.expand_overwrite(diag, labels, xn, yn, V, blank)), err_msg=what)


# ---------------------------------------------------------------------------------------------------------------------
# g. One launch against two
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [50, 1028])
def test_one_launch_against_two(V):
    """Up to 2^20 cells the dense gradients come out of ONE launch whose row writer computes its cell's pair itself (GradRows);
    above, out of k_grads and the expansion.  Held to expand_overwrite of the GRADS_GATHERED_DIAGONAL result of the same
    arguments: the non-zero slots exactly, and the values."""
    N, T, U, blank, lam = 3, 33, 34, 3, 0.01
    rng = np.random.RandomState(V)
    lp = log_softmax32(rng.randn(N, T, U, V).astype(np.float32))
    labels = dr.sentinel_labels(N, U, V, blank, seed=V)
    xn, yn = ragged(N, T, U)
    what = f"V={V}"
    c_dense, dense, _, _ = loss(IN_DENSE, GRADS_DENSE, lp, labels, xn, yn, blank, lam, what + " dense")
    c_diag, g_diag, _, _ = loss(IN_DENSE, GRADS_DIAGONAL, lp, labels, xn, yn, blank, lam, what + " diagonal")
    want = dr.expand_overwrite(g_diag, labels, xn, yn, V, blank)
    assert (labels[0, :yn[0]] == blank).any() and np.isfinite(c_diag).all()
    np.testing.assert_array_equal(bits(c_dense), bits(c_diag), err_msg=what)
    assert not np.isnan(dense).any(), f"{what}: slots nobody wrote"
    np.testing.assert_array_equal(dense != 0, want != 0, err_msg=f"{what}: the set of non-zero slots")
    print(f"{what}: largest difference between the one-launch and the two-launch dense gradients "
          f"{np.max(np.abs(dense.astype(np.float64) - want)):.3e}, {int((dense != want).sum())} slots differ")
    assert_same_values(dense, want, what)                       # (equal on the MI355X: one arithmetic, cell_grads)
