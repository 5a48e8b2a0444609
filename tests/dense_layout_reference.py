"""The padded (N,T,U,V) layout stated plainly in NumPy: what the gather, turn and expand kernels of csrc/to_diagonal.hip
and csrc/expand.hip must deliver.  Written from the comments of those files and from the reference's call chain
(warp_rnnt/__init__.py:118-128: an index full of `blank` with `labels` in channel 1 of the columns < U-1; __init__.py:23-24
and the autograd backward of torch.gather; core.cu:260-332 for the dense gradient tensor), not from the kernels.  None of
the operations does arithmetic beyond one fp32 multiply or one fp32 add, so every comparison against this file is bit for
bit (tests/test_gpu_dense_layout.py names its one exception).

    to_diagonal / from_diagonal   row-major (N,T,U,...) <-> the diagonal-major planes the sweeps read
    gather                        (N,T,U,V) log-probs -> row-major (blank, label) pairs (N,T,U,2)
    expand_sum                    diagonal-major gradient pairs -> dense rows, scatter_add semantics (gather=True backward)
    expand_overwrite              diagonal-major gradient pairs -> dense rows, slot-write semantics (gather=False forward)
    workspace_offsets             where rnnt_amd_loss keeps its planes in the caller's workspace
"""
import numpy as np

ALIGN = 256           # every plane of the workspace starts on a multiple of this many bytes (api_common.h)
INT_MIN = -2 ** 31


def align256(nbytes):
    return (int(nbytes) + ALIGN - 1) // ALIGN * ALIGN


# ---------------------------------------------------------------------------------------------------------------------
# The layout
# ---------------------------------------------------------------------------------------------------------------------
def to_diagonal(pairs):
    """(N, T, U, ...) row-major -> diagonal-major: cell (t, u) of utterance n sits in row (t + u) mod T, column u
    (as lsm_values.to_diagonal; any trailing axes)."""
    pairs = np.asarray(pairs)
    T, U = pairs.shape[1:3]
    out = np.empty_like(pairs)
    t, u = np.meshgrid(np.arange(T), np.arange(U), indexing="ij")
    out[:, (t + u) % T, u] = pairs[:, t, u]
    return out


def from_diagonal(planes):
    """The inverse of to_diagonal (as lattice_values.unskew)."""
    planes = np.asarray(planes)
    T, U = planes.shape[1:3]
    t, u = np.meshgrid(np.arange(T), np.arange(U), indexing="ij")
    return np.ascontiguousarray(planes[:, (t + u) % T, u])


def cell_labels(labels, N, U, blank):
    """(N, U) int64: the label of every lattice column as the caller gave it -- labels[n, u] for u < U-1, `blank` in
    column U-1.  labels may be None when U == 1."""
    lab = np.full((N, U), int(blank), dtype=np.int64)
    if U > 1:
        lab[:, :U - 1] = np.asarray(labels, dtype=np.int64).reshape(N, U - 1)
    return lab


def in_vocabulary(lab, V):
    return (lab >= 0) & (lab < V)


# ---------------------------------------------------------------------------------------------------------------------
# The operations
# ---------------------------------------------------------------------------------------------------------------------
def gather(lp, labels, blank):
    """Row-major (N,T,U,2): channel 0 = lp[..., blank]; channel 1 = lp[..., label], the label replaced by `blank` in
    column U-1 and wherever it is outside [0, V) (common.h: safe_label)."""
    lp = np.asarray(lp, dtype=np.float32)
    N, T, U, V = lp.shape
    lab = cell_labels(labels, N, U, blank)
    lab = np.where(in_vocabulary(lab, V), lab, int(blank))
    out = np.empty((N, T, U, 2), dtype=np.float32)
    out[..., 0] = lp[..., int(blank)]
    out[..., 1] = np.take_along_axis(lp, np.broadcast_to(lab[:, None, :, None], (N, T, U, 1)), axis=3)[..., 0]
    return out


def _scaled(pairs_diag, scale):
    """Row-major (gB, gL) fp32, each multiplied once in fp32 by its utterance's scale (None: 1)."""
    g = from_diagonal(np.asarray(pairs_diag, dtype=np.float32))
    if scale is None:
        return g[..., 0].copy(), g[..., 1].copy()
    sc = np.asarray(scale, dtype=np.float32).reshape(-1, 1, 1)
    return (g[..., 0] * sc).astype(np.float32), (g[..., 1] * sc).astype(np.float32)


def expand_sum(pairs_diag, labels, scale, V, blank):
    """Dense (N,T,U,V) fp32 from diagonal-major pairs, scatter_add into zeros: row[blank] = fp32(gB*sc); where the cell's
    label (`blank` in column U-1) is inside [0, V): row[label] += fp32(gL*sc) -- one fp32 add, which matters only where
    label == blank; a label outside the vocabulary is dropped.  scale=None means 1."""
    N, T, U = np.asarray(pairs_diag).shape[:3]
    gB, gL = _scaled(pairs_diag, scale)
    out = np.zeros((N, T, U, V), dtype=np.float32)
    out[..., int(blank)] = gB
    lab = np.broadcast_to(cell_labels(labels, N, U, blank)[:, None, :], (N, T, U))
    n, t, u = np.nonzero(in_vocabulary(lab, V))
    out[n, t, u, lab[n, t, u]] += gL[n, t, u]          # (one slot per cell: no index repeats)
    return out


def expand_overwrite(pairs_diag, labels, xn, yn, V, blank):
    """Dense (N,T,U,V) fp32 from diagonal-major pairs, the reference's slot writes into zeros: row[blank] = gB for every
    cell; then row[label] = gL only where t < xn[n], u < yn[n] and the label is inside [0, V) -- written after the blank
    slot, so label == blank leaves gL there."""
    N, T, U = np.asarray(pairs_diag).shape[:3]
    gB, gL = _scaled(pairs_diag, None)
    out = np.zeros((N, T, U, V), dtype=np.float32)
    out[..., int(blank)] = gB
    lab = np.broadcast_to(cell_labels(labels, N, U, blank)[:, None, :], (N, T, U))
    xn = np.asarray(xn, dtype=np.int64).reshape(N, 1, 1)
    yn = np.asarray(yn, dtype=np.int64).reshape(N, 1, 1)
    live = (np.arange(T).reshape(1, T, 1) < xn) & (np.arange(U).reshape(1, 1, U) < yn) & in_vocabulary(lab, V)
    n, t, u = np.nonzero(live)
    out[n, t, u, lab[n, t, u]] = gL[n, t, u]
    return out


def label_equals_blank(labels, N, T, U, V, blank):
    """(N,T,U) bool: the cells whose label slot IS the blank slot (column U-1 included) -- where expand_sum adds two
    products."""
    lab = cell_labels(labels, N, U, blank)
    return np.broadcast_to((lab == int(blank))[:, None, :], (N, T, U)).copy()


# ---------------------------------------------------------------------------------------------------------------------
# The workspace
# ---------------------------------------------------------------------------------------------------------------------
def workspace_offsets(N, T, U):
    """Byte offsets of the planes rnnt_amd_loss carves out of its workspace (include/warp_rnnt_amd.h, api_common.h: loss_layout): alphas,
    betas (4 bytes per cell each), the diagonal-major pair plane (8 per cell), the N log-likelihoods, the N mismatch
    words; every plane on a multiple of 256 bytes."""
    cells = int(N) * int(T) * int(U)
    a = align256(4 * cells)
    pairs = 2 * a
    ll = pairs + align256(8 * cells)
    return {"alphas": 0, "betas": a, "pairs": pairs, "ll": ll, "mismatch": ll + align256(4 * N), "cells": cells}


# ---------------------------------------------------------------------------------------------------------------------
# Inputs
# ---------------------------------------------------------------------------------------------------------------------
def distinct_floats(shape, first=0x3F800000):
    """fp32 tensor whose element i has the bit pattern first + i: finite, pairwise different (1.0, 1.0000001, ... for the
    default), so that a misplaced value cannot coincide with the right one."""
    size = int(np.prod(shape))
    assert size < 1 << 23, "the patterns would leave their binade"
    return (np.arange(size, dtype=np.uint32) + np.uint32(first)).view(np.float32).reshape(shape)


def sentinel_labels(N, U, V, blank, seed=0):
    """(N, U-1) int32 labels drawn from the whole vocabulary, every third column (1, 4, ...) the blank, and behind them
    padding as callers leave it: utterance n ends in min(n, U-1) sentinels out of -1, V+7, INT_MIN.  None when U == 1."""
    if U == 1:
        return None
    rng = np.random.RandomState(seed)
    lab = rng.randint(0, V, size=(N, U - 1)).astype(np.int32)
    lab[:, 1::3] = blank
    sent = (-1, V + 7, INT_MIN)
    for n in range(N):
        pad = min(n, U - 1)
        for j in range(pad):
            lab[n, U - 1 - pad + j] = sent[(n + j) % 3]
    return lab
