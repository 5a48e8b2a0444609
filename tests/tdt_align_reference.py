"""The best path of the token-and-duration (TDT) lattice, include/warp_rnnt_amd_tdt_align.h, stated plainly in NumPy: what
csrc/tdt_align.hip must deliver -- test infrastructure.

    viterbi32         the header's definition in fp32, operation for operation: the weight first, then v + weight, a candidate
                      taken only when strictly greater.  The kernels have no other arithmetic, so they give these bits.
    viterbi64         the same in fp64
    path_score64      the fp64 score of a path given as its edge list
    enumerate_paths   every path from (0,0) to the end, each walked on its own, with its fp64 score
    best_by_enumeration   the maximal score, the maximal path whose codes read from the last edge to the first are
                      lexicographically smallest, and how many paths are maximal
    trace             the path read back along the codes
    rows_of           emit_frames / emit_durations of an edge list
    workspace_offsets, planes_of_plane, codes_of_dec   the layout of the header's workspace, restated

tb, tl: (T,U) arrays, row-major -- tok[blank] and tok[labels[u]] of cell (t,u), sigma subtracted; dur: (T,U,D).  An
utterance is the window t < T_n, u <= U_n.  An edge is (t, u, i, kind): out of cell (t,u), duration durations[i], kind 0
the blank edge to (t+d, u), kind 1 the label edge to (t+d, u+1); its code is 2i + kind.  A path is the list of its edges
from (0,0) to the end cell (T_n, U_n).
"""
import numpy as np

NO_EDGE = 255
ALIGN = 256


def _viterbi(tb, tl, dur, T_n, U_n, durations, dtype):
    tb = np.asarray(tb, dtype=dtype)
    tl = np.asarray(tl, dtype=dtype)
    dur = np.asarray(dur, dtype=dtype)
    neg = dtype(-np.inf)
    v = np.full((T_n + 1, U_n + 1), neg, dtype=dtype)
    codes = np.full((T_n + 1, U_n + 1), NO_EDGE, dtype=np.uint8)      # row T_n: only [T_n, U_n], the end cell, is a cell
    ties = np.zeros((T_n + 1, U_n + 1), dtype=bool)                   # two candidates equal the (finite) maximum
    v[0, 0] = 0
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(T_n + 1):
            for u in range(U_n + 1):
                if (t == 0 and u == 0) or (t == T_n and u != U_n):
                    continue
                best, code, cands = neg, NO_EDGE, []
                for i, d in enumerate(durations):
                    if d > 0 and t - d >= 0:
                        c = v[t - d, u] + (tb[t - d, u] + dur[t - d, u, i])
                        cands.append(c)
                        if c > best:
                            best, code = c, 2 * i
                    if u > 0 and t - d >= 0 and t < T_n:
                        c = v[t - d, u - 1] + (tl[t - d, u - 1] + dur[t - d, u - 1, i])
                        cands.append(c)
                        if c > best:
                            best, code = c, 2 * i + 1
                v[t, u], codes[t, u] = best, code
                ties[t, u] = best > neg and sum(1 for c in cands if c == best) > 1
    score = v[T_n, U_n]
    return dtype(score), codes, trace(codes, T_n, U_n, durations) if score > neg else None, ties


def trace(codes, T_n, U_n, durations):
    """The path read back from the end cell along the codes, as its edge list from (0,0) on."""
    edges, t, u = [], T_n, U_n
    while t + u > 0:
        k = int(codes[t, u])
        assert k != NO_EDGE and k >> 1 < len(durations), (t, u, k)    # a finite score implies a valid code on the path
        t, u = t - durations[k >> 1], u - (k & 1)
        assert t >= 0 and u >= 0, (t, u, k)
        edges.append((t, u, k >> 1, k & 1))
    edges.reverse()
    return edges


def viterbi32(tb, tl, dur, T_n, U_n, durations):
    """(score as np.float32, codes (T_n+1, U_n+1) uint8 with the end cell at [T_n, U_n], the path's edges or None, the
    cells at which two candidates tie for the maximum) by the definition, every operation in fp32."""
    return _viterbi(tb, tl, dur, int(T_n), int(U_n), tuple(durations), np.float32)


def viterbi64(tb, tl, dur, T_n, U_n, durations):
    """The same with every operation in fp64."""
    return _viterbi(tb, tl, dur, int(T_n), int(U_n), tuple(durations), np.float64)


def path_score64(edges, tb, tl, dur):
    """fp64 score of a path: the sum of its edges' weights, each weight first, in path order."""
    total = 0.0
    for t, u, i, kind in edges:
        total += float(tl[t, u] if kind else tb[t, u]) + float(dur[t, u, i])
    return total


def check_path(edges, T_n, U_n, durations):
    """The edges lead from (0,0) to the end cell (T_n, U_n) by the rules of the lattice."""
    t, u = 0, 0
    for et, eu, i, kind in edges:
        assert (et, eu) == (t, u) and t < T_n and 0 <= i < len(durations), (edges, T_n, U_n)
        d = durations[i]
        assert d > 0 or kind == 1
        t, u = t + d, u + kind
        assert u <= U_n and (t < T_n or (t == T_n and kind == 0 and u == U_n)), (edges, T_n, U_n)
    assert (t, u) == (T_n, U_n) and len(edges) > 0


def codes_from_the_end(edges):
    return tuple(2 * i + kind for _, _, i, kind in reversed(edges))


def rows_of(edges, durations, width):
    """(emit_frames, emit_durations), each (width,) int32: frame and duration of the label edge out of column u, -1 from
    U_n on; all -1 for no path (edges None)."""
    frames = np.full((width,), -1, np.int32)
    lengths = np.full((width,), -1, np.int32)
    for t, u, i, kind in edges or ():
        if kind:
            frames[u], lengths[u] = t, durations[i]
    return frames, lengths


def enumerate_paths(tb, tl, dur, T_n, U_n, durations):
    """[(fp64 score, edges)] of every path from (0,0) to the end, each walked on its own (no dynamic programming); the score
    is accumulated in path order, weight first."""
    out = []

    def walk(t, u, score, edges):
        for i, d in enumerate(durations):
            if d > 0 and (t + d < T_n or (t + d == T_n and u == U_n)):
                e = edges + [(t, u, i, 0)]
                s = score + (float(tb[t, u]) + float(dur[t, u, i]))
                if t + d == T_n:
                    out.append((s, e))
                else:
                    walk(t + d, u, s, e)
            if u < U_n and t + d < T_n:
                walk(t + d, u + 1, score + (float(tl[t, u]) + float(dur[t, u, i])), edges + [(t, u, i, 1)])

    walk(0, 0, 0.0, [])
    return out


def best_by_enumeration(tb, tl, dur, T_n, U_n, durations):
    """(maximal score, the maximal path whose codes from the last edge to the first are lexicographically smallest, number
    of maximal paths); (-inf, None, 0) when no path has a finite score."""
    paths = [(s, e) for s, e in enumerate_paths(tb, tl, dur, T_n, U_n, durations) if s > -np.inf]
    if not paths:
        return -np.inf, None, 0
    top = max(s for s, _ in paths)
    maximal = [e for s, e in paths if s == top]
    return top, min(maximal, key=codes_from_the_end), len(maximal)


# ---- the workspace of rnnt_amd_tdt_align, restated from the header ----

def _up(x):
    return (x + ALIGN - 1) // ALIGN * ALIGN


def workspace_offsets(N, T, U, D):
    """Byte offsets: the plane at 0 -- (2+D) channels of N*T*U fp32 -- then the decision bytes dec[n][d][u], d in [0, T+U)."""
    cells = N * T * U
    dec = _up(4 * (2 + D) * cells)
    return {"cells": cells, "plane": 0, "dec": dec, "size": dec + _up(N * (T + U) * U)}


def planes_of_plane(flat, N, T, U, D):
    """The plane's 2+D channels (a flat fp32 array, diagonal-major: cell (n,t,u) at (n*T + (t+u) mod T)*U + u) turned to
    row-major: tb (N,T,U), tl (N,T,U), dur (N,T,U,D)."""
    ch = np.asarray(flat).reshape(2 + D, N, T, U)
    t = np.arange(T)[:, None]
    u = np.arange(U)[None, :]
    rm = ch[:, :, (t + u) % T, u]                         # (2+D, N, T, U) indexed by (t, u)
    return rm[0], rm[1], np.moveaxis(rm[2:], 0, -1)


def codes_of_dec(dec, n, T, U, T_n, U_n):
    """dec[n][d][u] (a flat uint8 array) inside utterance n's window and at its end cell, as viterbi's codes array
    (T_n+1, U_n+1); the entries of row T_n other than the end cell are NO_EDGE."""
    d3 = np.asarray(dec).reshape(-1, T + U, U)[n]
    codes = np.full((T_n + 1, U_n + 1), NO_EDGE, np.uint8)
    for u in range(U_n + 1):
        codes[:T_n, u] = d3[np.arange(T_n) + u, u]
    codes[T_n, U_n] = d3[T_n + U_n, U_n]
    return codes
