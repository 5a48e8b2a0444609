"""The instrument of tests/test_gpu_compact_layout.py checked on the CPU: tests/compact_reference.py against the C oracle,
and its comparison functions against results that are wrong on purpose."""
import numpy as np
import pytest

import compact_reference as cr
import oracle


def all_cases():
    return ([cr.seam_case(name) for name in cr.SEAM_CASES] +
            [cr.tile_edge_case(0, 0.0), cr.tile_edge_case(4, 0.01), cr.tile_edge_case(4, 0.01, empties=False),
             cr.staged_case()])


CASE_IDS = list(cr.SEAM_CASES) + ["tile_edges_blank0", "tile_edges_blank4", "tile_edges_no_empties", "staged_odd"]


def padded(case, ns, T, Y):
    """Utterances ns, all of shape (T, Y + 1), as the oracle's tensors: log-probs (G,T,U,V) and labels (G,U-1).  The oracle
    indexes with the labels as they are, so a label outside the vocabulary is handed over as what it stands for."""
    U = Y + 1
    lp = np.stack([case.xs[case.offs[n]:case.offs[n + 1]].reshape(T, U, case.V) for n in ns])
    labels = np.zeros((len(ns), max(Y, 1)), dtype=np.int32)
    for i, n in enumerate(ns):
        for u in range(Y):
            labels[i, u] = cr.safe_label(case.ys[case.label_offs[n] + u], case.V, case.blank)
    return lp, labels[:, :Y]


def oracle_pairs_and_loc(case):
    """What the kernels must deliver, from the C oracle instead of pack_reference: oracle.gather_f32 on every utterance's
    padded tensors, packed; loc as tests/test_gpu_compact.py restates it."""
    pairs = np.zeros((case.STU, 2), dtype=np.float32)
    loc = np.zeros((case.STU,), dtype=np.int64)
    for (T, Y), ns in case.groups().items():
        lp, labels = padded(case, ns, T, Y)
        got = oracle.gather_f32(lp, labels, case.blank)
        for i, n in enumerate(ns):
            pairs[case.offs[n]:case.offs[n + 1]] = got[i].reshape(-1, 2)
            l = np.full((T, Y + 1), case.blank, dtype=np.int64)
            l[:, :Y] = labels[i][None, :]
            loc[case.offs[n]:case.offs[n + 1]] = l.reshape(-1)
    return pairs, loc


def oracle_dense_rows(case, scales):
    """(STU,V) gradient rows from the oracle's dense gradients: utterance n's (T,U,V) block times scales[n], packed."""
    out = np.zeros((case.STU, case.V), dtype=np.float32)
    for (T, Y), ns in case.groups().items():
        lp, labels = padded(case, ns, T, Y)
        ref = oracle.rnnt_loss_f32(lp, labels, np.full(len(ns), T, np.int32), np.full(len(ns), Y, np.int32),
                                   blank=case.blank, fastemit_lambda=case.lam, scan_mode=1)
        for i, n in enumerate(ns):
            out[case.offs[n]:case.offs[n + 1]] = (ref["grads"][i] * scales[n]).reshape(-1, case.V)
    return out


def scales_of(case):
    return (0.5 + np.random.RandomState(1).rand(case.N)).astype(np.float32)


@pytest.mark.parametrize("case", all_cases(), ids=CASE_IDS)
def test_pack_reference_is_the_oracles_gather(case):
    pairs, loc = oracle_pairs_and_loc(case)
    want_pairs, want_loc = case.packed()
    assert np.array_equal(cr.bits(want_pairs), cr.bits(pairs))
    assert np.array_equal(want_loc, loc)
    assert case.STU == int((case.xn.astype(np.int64) * (case.yn + 1)).sum())


def test_case_builders_hold_what_they_promise():
    full = cr.tile_edge_case(0, 0.0)
    assert full.N == 4097 and not full.live()[list(cr.TILE_EDGE_EMPTY)].any() and full.live().sum() == full.N - 2
    shapes = {(int(t), int(y) + 1) for t, y in zip(full.xn, full.yn)}
    assert set(cr.TILE_EDGE_SHAPES) <= shapes
    assert (full.xn[0], full.yn[0] + 1) == cr.TILE_EDGE_SHAPES[0] and (full.xn[-1], full.yn[-1] + 1) == cr.TILE_EDGE_SHAPES[-1]
    assert ((full.ys < 0).sum(), (full.ys >= full.V).sum()) == (1, 1)
    assert (full.yn == 0).sum() >= 5 and full.STU < 120000
    half = full.subset(2048, full.N)
    assert half.N == 2049 and np.array_equal(half.xs, full.xs[full.offs[2048]:])
    confetti = cr.seam_case("confetti")
    assert (confetti.cells[:1500] == 1).all() and confetti.STU == 1500 + 40 * 30
    assert (cr.seam_case("no_labels").yn == 0).all() and cr.seam_case("lone").N == 1
    for V in (1, 4, 1025):
        for N in (1, 7):
            for STU in (1, 43, V + 11):
                gc, g2, loc, cum = cr.scatter_inputs(V, N, STU, V - 1)
                assert len(set(gc.tolist())) == N and cum[-1] == STU and (np.diff(cum) >= 0).all()
                assert np.array_equal(g2.astype(np.float64)[:, 0], np.arange(STU) + 0.25)
                if STU >= V + 4:
                    assert set(range(V)) | {V, -1, (1 << 31) + 1} <= set(loc.tolist())
                if N == 7:
                    assert cum[0] == 0 and cum[2] == cum[3] == cum[1] and cum[-1] == cum[-2]


@pytest.mark.parametrize("name", ["edge_off_by_one", "empties"])
def test_scatter_reference_is_the_oracles_dense_gradient(name):
    case = cr.seam_case(name)
    scales = scales_of(case)
    _, grads2 = cr.oracle_packed(case)
    _, loc = case.packed()
    got = cr.scatter_reference(scales, grads2, loc, case.offs[1:].astype(np.int32), case.V, case.blank)
    cr.assert_same_bits(got, oracle_dense_rows(case, scales), name)


def guarded(rows, V, shift=0):
    size, start = cr.guarded_buffer_layout(V, rows.shape[0], shift)
    buf = np.full((size,), cr.GUARD, dtype=np.float32)
    buf[start:start + rows.size] = rows.reshape(-1)
    return buf, start


def test_comparisons_have_teeth():
    """The C oracle's results, packed, stand in for the kernels' results; each is then made wrong the way an index bug would
    make it wrong, one at a time, and the comparison named here must fail:

        pairs of the last cell of one utterance and the first of the next swapped     assert_pairs
        the pairs of one 32x32 tile transposed                                        assert_pairs
        loc shifted by one row across an utterance seam                               assert_loc
        owner = the first n with cum_lens[n] >= row (the wrong scale at a seam)       assert_scatter, rows
        one scatter row left unwritten (NaN)                                          assert_scatter, rows
        -0.0 in place of +0.0 in a zero slot                                          assert_scatter, rows (by bits only)
        a write behind the last row                                                   assert_scatter, guard
        one gradient pair delivered to the neighbouring cell                          assert_same_results between routes
    """
    case = cr.seam_case("edge_exact")
    pairs, loc = oracle_pairs_and_loc(case)
    costs, grads2 = cr.oracle_packed(case)
    scales = scales_of(case)
    cum = case.offs[1:].astype(np.int32)
    rows = oracle_dense_rows(case, scales)
    buf, start = guarded(rows, case.V)
    scatter_args = (scales, grads2, loc, cum, case.V, case.blank, "stand-in")
    # as they are, they pass
    cr.assert_pairs(pairs, case)
    cr.assert_loc(loc, case)
    cr.assert_oracle(costs, grads2, case)
    cr.assert_scatter(buf, start, *scatter_args)
    cr.assert_same_results((costs, grads2, loc), (costs.copy(), grads2.copy(), loc.copy()), "stand-in")

    seam = int(case.offs[1])
    bad = pairs.copy()
    bad[[seam - 1, seam]] = bad[[seam, seam - 1]]
    with pytest.raises(AssertionError, match="pairs"):
        cr.assert_pairs(bad, case)

    n = 2
    assert (case.xn[n], case.yn[n] + 1) == (cr.TILE, cr.TILE)
    bad = pairs.copy()
    block = bad[case.offs[n]:case.offs[n + 1]].reshape(cr.TILE, cr.TILE, 2)
    bad[case.offs[n]:case.offs[n + 1]] = block.transpose(1, 0, 2).reshape(-1, 2)
    with pytest.raises(AssertionError, match="pairs"):
        cr.assert_pairs(bad, case)

    bad = loc.copy()
    bad[seam - 2:seam + 3] = loc[seam - 3:seam + 2]
    with pytest.raises(AssertionError, match="loc"):
        cr.assert_loc(bad, case)

    # first n with cum_lens[n] >= row  <=>  first n with cum_lens[n] + 1 > row
    wrong_owner = cr.scatter_reference(scales, grads2, loc, cum + 1, case.V, case.blank)
    assert (wrong_owner != rows).any(axis=1).sum() == (np.diff(case.offs) > 0).sum() - 1     # the first row behind each seam
    with pytest.raises(AssertionError, match="rows"):
        cr.assert_scatter(guarded(wrong_owner, case.V)[0], start, *scatter_args)

    bad = buf.copy()
    bad[start + 17 * case.V:start + 18 * case.V] = np.nan
    with pytest.raises(AssertionError, match="rows"):
        cr.assert_scatter(bad, start, *scatter_args)

    zero_slot = start + int(np.flatnonzero(cr.bits(rows.reshape(-1)) == 0)[0])
    bad = buf.copy()
    bad[zero_slot] = -0.0
    assert np.array_equal(bad, buf)                   # a comparison of values does not see it
    with pytest.raises(AssertionError, match="rows"):
        cr.assert_scatter(bad, start, *scatter_args)

    bad = buf.copy()
    bad[start + rows.size] = 0.0
    with pytest.raises(AssertionError, match="guard behind"):
        cr.assert_scatter(bad, start, *scatter_args)

    bad = grads2.copy()
    bad[[seam - 1, seam]] = bad[[seam, seam - 1]]
    with pytest.raises(AssertionError, match="grads2"):
        cr.assert_same_results((costs, bad, loc), (costs, grads2, loc), "stand-in")
