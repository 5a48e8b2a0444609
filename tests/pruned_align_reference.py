"""The best path on the pruned band (include/warp_rnnt_amd_pruned_align.h) stated plainly in NumPy.

    scatter                 band pairs (T,S,2) and starts (T,) -> the (T,U) planes b, l with -inf off the band, on which
                            align_reference.viterbi32 / viterbi64 / best_by_enumeration serve the regular topology unchanged
    VITERBI32 / VITERBI64   per topology; the modified one is the header's recurrence, operation for operation
    modified_path_score64   the fp64 score of the modified path with the given (strictly increasing) emit frames
    modified_enumeration    every such tuple, scored in fp64: (score, emit frames, number of maximal paths); the winner's emit
                            frames are smallest when compared from the last label to the first
"""
import functools
import itertools

import numpy as np

import align_reference as ar


def scatter(pairs, starts, U):
    T, S, _ = pairs.shape
    b = np.full((T, U), -np.inf, pairs.dtype)
    l = np.full((T, U), -np.inf, pairs.dtype)
    for t in range(T):
        for s in range(S):
            u = int(starts[t]) + s
            if 0 <= u < U:
                b[t, u], l[t, u] = pairs[t, s]
    return b, l


def _modified(dtype, b, l, T_n, U_n):
    b, l, T_n, U_n = np.asarray(b, dtype=dtype), np.asarray(l, dtype=dtype), int(T_n), int(U_n)
    v = np.full((T_n + 1, U_n + 1), -np.inf, dtype=dtype)
    by_label = np.zeros((T_n + 1, U_n + 1), dtype=bool)
    v[0, 0] = 0
    for t in range(T_n):
        for u in range(U_n + 1):
            cb = v[t, u] + b[t, u]
            cl = v[t, u - 1] + l[t, u - 1] if u > 0 else dtype(-np.inf)
            by_label[t + 1, u] = u > 0 and bool(cl > cb)
            v[t + 1, u] = cl if by_label[t + 1, u] else cb
    emit = np.full((U_n,), -1, dtype=np.int32)
    t, u = T_n, U_n
    while t > 0 and np.isfinite(v[T_n, U_n]):
        if by_label[t, u]:
            emit[u - 1] = t - 1
            u -= 1
        t -= 1
    return dtype(v[T_n, U_n]), emit


def modified_path_score64(emit, b, l, T_n):
    b, l = np.asarray(b, dtype=np.float64), np.asarray(l, dtype=np.float64)
    emit = [int(e) for e in emit]
    assert all(0 <= e < T_n for e in emit) and all(x < y for x, y in zip(emit, emit[1:])), emit
    total, u = 0.0, 0
    for t in range(int(T_n)):
        if u < len(emit) and emit[u] == t:
            total += l[t, u]
            u += 1
        else:
            total += b[t, u]
    return float(total)


def modified_enumeration(b, l, T_n, U_n):
    scored = [(modified_path_score64(e, b, l, T_n), e) for e in itertools.combinations(range(int(T_n)), int(U_n))]
    if not scored:
        return -np.inf, np.zeros((0,), np.int32), 0
    s, emit = min(scored, key=lambda x: (-x[0], tuple(reversed(x[1]))))
    return s, np.asarray(emit, dtype=np.int32), sum(1 for x, _ in scored if x == s)


VITERBI32 = {"regular": ar.viterbi32, "modified": functools.partial(_modified, np.float32)}
VITERBI64 = {"regular": ar.viterbi64, "modified": functools.partial(_modified, np.float64)}
PATH_SCORE64 = {"regular": ar.path_score64, "modified": modified_path_score64}
ENUMERATION = {"regular": ar.best_by_enumeration, "modified": modified_enumeration}
