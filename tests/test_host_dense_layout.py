"""tests/dense_layout_reference.py is the yardstick of tests/test_gpu_dense_layout.py: here it is held, on the CPU, to
literal loops over the cells, to the fp32 oracle's gather, to torch's scatter_add_ and to the library's own host-side
workspace functions (which launch nothing)."""
import numpy as np
import pytest

import dense_layout_reference as dr

SHAPES = [(2, 3, 5), (3, 4, 4), (2, 7, 3), (2, 1, 4), (3, 5, 1), (1, 1, 1)]       # T<U, T=U, T>U, T=1, U=1, one cell


def _pairs(N, T, U, first=0x3F800000):
    return dr.distinct_floats((N, T, U, 2), first)


@pytest.mark.parametrize("N,T,U", SHAPES)
def test_layout_is_a_bijection_and_from_diagonal_its_inverse(N, T, U):
    pairs = _pairs(N, T, U)
    diag = dr.to_diagonal(pairs)
    want = np.full_like(pairs, np.nan)
    for n in range(N):
        for t in range(T):
            for u in range(U):
                assert np.isnan(want[n, (t + u) % T, u]).all(), "two cells in one slot"
                want[n, (t + u) % T, u] = pairs[n, t, u]
    assert not np.isnan(want).any(), "a slot without a cell"
    np.testing.assert_array_equal(diag.view(np.uint32), want.view(np.uint32))
    np.testing.assert_array_equal(dr.from_diagonal(diag).view(np.uint32), pairs.view(np.uint32))
    # single planes (N,T,U) turn the same way, and the two restatements in this directory agree
    np.testing.assert_array_equal(dr.to_diagonal(pairs[..., 0]), diag[..., 0])
    import lattice_values
    import lsm_values
    np.testing.assert_array_equal(lsm_values.to_diagonal(pairs), diag)
    np.testing.assert_array_equal(lattice_values.unskew(diag[..., 1], T, U), pairs[..., 1])


@pytest.mark.parametrize("blank_of", [lambda V: 0, lambda V: V - 1, lambda V: V // 2])
@pytest.mark.parametrize("N,T,U", SHAPES)
def test_gather_against_loops_and_the_oracle(N, T, U, blank_of):
    import oracle
    for V in (1, 2, 7):
        blank = blank_of(V)
        lp = dr.distinct_floats((N, T, U, V))
        labels = dr.sentinel_labels(N, U, V, blank, seed=V)
        got = dr.gather(lp, labels, blank)
        want = np.empty((N, T, U, 2), np.float32)
        for n in range(N):
            for t in range(T):
                for u in range(U):
                    lab = blank if u == U - 1 else int(labels[n, u])
                    if not 0 <= lab < V:
                        lab = blank
                    want[n, t, u] = (lp[n, t, u, blank], lp[n, t, u, lab])
        np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
        if U > 1:                                   # (the oracle indexes with the label as it is: in-range labels only)
            clean = np.where((labels >= 0) & (labels < V), labels, blank).astype(np.int32)
            np.testing.assert_array_equal(dr.gather(lp, clean, blank), oracle.gather_f32(lp, clean, blank))
            np.testing.assert_array_equal(got, oracle.gather_f32(lp, clean, blank))
        else:
            np.testing.assert_array_equal(got, oracle.gather_f32(lp, np.zeros((N, 0), np.int32), blank))


def _lengths(N, T, U):
    xn = np.array([T, max(1, T - 2), 1], dtype=np.int32)[:N]
    yn = np.array([U - 1, 0, (U - 1) // 2], dtype=np.int32)[:N]
    return xn, yn


@pytest.mark.parametrize("N,T,U", SHAPES)
def test_expand_against_loops(N, T, U):
    for V in (1, 2, 5):
        for blank in sorted({0, V - 1}):
            pairs = _pairs(N, T, U)
            diag = dr.to_diagonal(pairs)
            labels = dr.sentinel_labels(N, U, V, blank, seed=3)
            if U > 3:
                labels[0, 2] = -1                                # a sentinel inside the live range
            xn, yn = _lengths(N, T, U)
            scale = np.array([0.737, -1.3, 2.9], dtype=np.float32)[:N]
            dup = 0
            for sc in (None, scale):
                want_sum = np.zeros((N, T, U, V), np.float32)
                want_ovr = np.zeros((N, T, U, V), np.float32)
                for n in range(N):
                    s = np.float32(1.0) if sc is None else sc[n]
                    for t in range(T):
                        for u in range(U):
                            gB, gL = diag[n, (t + u) % T, u]
                            lab = blank if u == U - 1 else int(labels[n, u])
                            want_sum[n, t, u, blank] = np.float32(gB * s)
                            want_ovr[n, t, u, blank] = gB
                            if 0 <= lab < V:
                                want_sum[n, t, u, lab] = np.float32(want_sum[n, t, u, lab] + np.float32(gL * s))
                                dup += lab == blank
                                if t < xn[n] and u < yn[n]:
                                    want_ovr[n, t, u, lab] = gL
                got = dr.expand_sum(diag, labels, sc, V, blank)
                np.testing.assert_array_equal(got.view(np.uint32), want_sum.view(np.uint32))
            got = dr.expand_overwrite(diag, labels, xn, yn, V, blank)
            np.testing.assert_array_equal(got.view(np.uint32), want_ovr.view(np.uint32))
            assert dr.label_equals_blank(labels, N, T, U, V, blank).sum() * 2 == dup


def test_expand_sum_is_scatter_add_on_in_range_labels():
    """The gather=True backward of the reference: grads scaled in place (__init__.py:23-24), then the autograd backward of
    torch.gather on the index of __init__.py:118-128 -- scatter_add_ into zeros."""
    import torch
    N, T, U, V, blank = 3, 5, 6, 7, 2
    rng = np.random.RandomState(0)
    labels = rng.randint(0, V, size=(N, U - 1)).astype(np.int32)
    labels[:, 1] = blank
    pairs = _pairs(N, T, U)
    scale = np.array([0.5, 4.0, -2.0], dtype=np.float32)        # powers of two: the sum of two products rounds once
    index = torch.full((N, T, U, 2), blank, dtype=torch.int64)
    index[:, :, :U - 1, 1] = torch.from_numpy(labels.astype(np.int64))[:, None, :]
    src = torch.from_numpy(pairs) * torch.from_numpy(scale).view(N, 1, 1, 1)
    want = torch.zeros((N, T, U, V)).scatter_add_(3, index, src).numpy()
    np.testing.assert_array_equal(dr.expand_sum(dr.to_diagonal(pairs), labels, scale, V, blank), want)


WORKSPACE_SHAPES = [(1, 1, 1), (3, 7, 33), (3, 33, 65), (8, 225, 225), (7, 225, 225), (2, 33, 4097), (3, 611, 573),
                    (1, 1024, 1025), (16, 1500, 300), (65, 1, 1)]


@pytest.mark.parametrize("N,T,U", WORKSPACE_SHAPES)
def test_workspace_offsets_against_the_library(N, T, U):
    """The GPU tests read the pair plane at workspace_offsets()['pairs']: the library's own host functions must put the
    mismatch words -- the second plane behind it -- where this statement of the layout does, and the whole must fit."""
    import warp_rnnt_amd
    L = warp_rnnt_amd.load()
    off = dr.workspace_offsets(N, T, U)
    cells = N * T * U
    assert off["cells"] == cells
    assert off["betas"] >= 4 * cells and off["pairs"] - off["betas"] >= 4 * cells and off["ll"] - off["pairs"] >= 8 * cells
    assert all(off[k] % 256 == 0 for k in ("alphas", "betas", "pairs", "ll", "mismatch"))
    assert off["betas"] - 4 * cells < 256 and off["ll"] - off["pairs"] - 8 * cells < 256
    assert off["mismatch"] == off["ll"] + dr.align256(4 * N)
    assert L.rnnt_amd_workspace_mismatch_offset(N, T, U) == off["mismatch"]
    assert L.rnnt_amd_workspace_size(N, T, U) >= off["mismatch"] + 4 * N


def test_inputs_are_what_they_claim():
    x = dr.distinct_floats((3, 5, 7))
    assert np.isfinite(x).all() and len(np.unique(x)) == x.size and x.min() == 1.0 and x.max() < 1.125
    with pytest.raises(AssertionError):
        dr.distinct_floats((1 << 23,))
    lab = dr.sentinel_labels(3, 34, 5, 4)
    assert (lab == 4).any() and lab[1, -1] == 12 and lab[2, -2] == dr.INT_MIN and lab[2, -1] == -1
    assert ((lab[0] >= 0) & (lab[0] < 5)).all()
    assert dr.sentinel_labels(3, 1, 5, 0) is None
