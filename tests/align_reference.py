"""The best-path alignment of include/warp_rnnt_amd_align.h stated plainly in NumPy: what csrc/align.hip must deliver.

    viterbi32             the header's definition in fp32, operation for operation: one add per edge, one compare per cell,
                          a tie to the blank predecessor.  The kernels have no other arithmetic, so they give these bits.
    viterbi64             the same in fp64
    best_by_enumeration   every monotone tuple of emit frames, scored in fp64: the path of maximal score whose emit frames
                          are smallest when compared from the last label to the first -- what the tie rule is claimed to pick
    path_score64          the fp64 score of the path with the given emit frames

b, l: (T, U) arrays, row-major: the blank and the label log-probability of cell (t, u).  An utterance is the window
t < T_n, u <= U_n.
"""
import itertools

import numpy as np


def _viterbi(b, l, T_n, U_n, dtype):
    b = np.asarray(b, dtype=dtype)
    l = np.asarray(l, dtype=dtype)
    v = np.zeros((T_n, U_n + 1), dtype=dtype)
    by_label = np.zeros((T_n, U_n + 1), dtype=bool)
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(T_n):
            for u in range(U_n + 1):
                if t == 0 and u == 0:
                    continue
                cb = v[t - 1, u] + b[t - 1, u] if t > 0 else None
                cl = v[t, u - 1] + l[t, u - 1] if u > 0 else None
                by_label[t, u] = u > 0 and (t == 0 or bool(cl > cb))
                v[t, u] = cl if by_label[t, u] else cb
        score = v[T_n - 1, U_n] + b[T_n - 1, U_n]
    emit = np.full((U_n,), -1, dtype=np.int32)
    t, u = T_n - 1, U_n
    while t + u > 0:
        if by_label[t, u]:
            emit[u - 1] = t
            u -= 1
        else:
            t -= 1
    return dtype(score), emit


def viterbi32(b, l, T_n, U_n):
    """(score as np.float32, emit frames (U_n,) int32) by the definition, every operation in fp32."""
    return _viterbi(b, l, int(T_n), int(U_n), np.float32)


def viterbi64(b, l, T_n, U_n):
    """The same with every operation in fp64."""
    return _viterbi(b, l, int(T_n), int(U_n), np.float64)


def path_score64(emit, b, l, T_n=None):
    """fp64 score of the path that emits label u at frame emit[u] (non-decreasing) and ends with the blank of
    (T_n-1, U_n); U_n = len(emit), T_n defaults to the planes' frame count."""
    b = np.asarray(b, dtype=np.float64)
    l = np.asarray(l, dtype=np.float64)
    T_n = b.shape[0] if T_n is None else int(T_n)
    emit = [int(e) for e in emit]
    assert all(0 <= e < T_n for e in emit) and all(x <= y for x, y in zip(emit, emit[1:])), emit
    total, t = 0.0, 0
    with np.errstate(invalid="ignore"):
        for u, e in enumerate(emit):
            total += b[t:e, u].sum()            # blank steps (t,u) -> (t+1,u) up to the emit frame
            total += l[e, u]
            t = e
        U_n = len(emit)
        total += b[t:T_n, U_n].sum()            # ... and in the last column, the final blank included
    return float(total)


def best_by_enumeration(b, l, T_n, U_n):
    """(score, emit frames (U_n,) int32, number of paths with that score) over all monotone emit-frame tuples, fp64; the
    winner minimises (-score, emit frames read from the last label to the first)."""
    best = None
    scores = []
    for emit in itertools.combinations_with_replacement(range(int(T_n)), int(U_n)):
        s = path_score64(emit, b, l, T_n)
        scores.append(s)
        key = (-s, tuple(reversed(emit)))
        if best is None or key < best[0]:
            best = (key, s, emit)
    _, s, emit = best
    return s, np.asarray(emit, dtype=np.int32), sum(1 for x in scores if x == s)
