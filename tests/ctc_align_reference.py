"""The CTC best-path alignment restated in NumPy (include/warp_rnnt_amd_ctc_align.h): the fp32 recurrence, one vector
operation per frame, whose bits the kernel must give; and the best score of a plane in float64."""
import numpy as np

FLOOR = np.float32(-1e30)


def tokens_of(labels, Ln, V, blank):
    """token(l): a label that is no index of [0,V) is read as the blank."""
    lab = np.asarray(labels[:Ln], dtype=np.int64)
    return np.where((lab >= 0) & (lab < V), lab, blank)


def repeats(labels, Ln):
    return int((np.asarray(labels[1:Ln]) == np.asarray(labels[:Ln - 1])).sum()) if Ln > 1 else 0


def _lattice(E, tok, Tn, Ln, dtype, floor):
    """v(T_n-1, .) and the decisions d (T_n, 2 L_n + 1) on the emission plane E (T, L+1)."""
    S = 2 * Ln + 1
    col = np.zeros(S, dtype=np.int64)
    col[1::2] = 1 + np.arange(Ln)
    skip_ok = np.zeros(S, dtype=bool)
    skip_ok[3::2] = tok[1:] != tok[:-1]
    e = np.maximum(E[:Tn, col].astype(dtype), floor)
    v = np.full(S, floor, dtype=dtype)
    v[:2] = e[0, :2]
    d = np.zeros((Tn, S), dtype=np.int64)
    for t in range(1, Tn):
        stay = v
        step = np.concatenate(([floor], v))[:S].astype(dtype)
        skip = np.where(skip_ok, np.concatenate(([floor, floor], v))[:S], floor).astype(dtype)
        d[t] = np.where((stay >= step) & (stay >= skip), 0, np.where(step >= skip, 1, 2))
        v = np.maximum(e[t] + np.maximum(np.maximum(stay, step), skip), floor).astype(dtype)
    return v, d


def align_fp32(E, labels, xn, yn, V, blank):
    """(scores (N,) float32, frame_tokens (N,T) int32, emit_frames (N,L) int32) of the emission plane E (N,T,L+1)."""
    N, T, W = E.shape
    L = W - 1
    scores = np.full(N, np.nan, dtype=np.float32)
    frame_tokens = np.full((N, T), -1, dtype=np.int32)
    emit_frames = np.full((N, L), -1, dtype=np.int32)
    for n in range(N):
        Tn, Ln = int(xn[n]), int(yn[n])
        if not (1 <= Tn <= T and 0 <= Ln <= L):
            continue
        tok = tokens_of(labels[n], Ln, V, blank)
        v, d = _lattice(E[n], tok, Tn, Ln, np.float32, FLOOR)
        s = 2 * Ln if Ln == 0 or v[2 * Ln] >= v[2 * Ln - 1] else 2 * Ln - 1
        if v[s] <= np.float32(0.5) * FLOOR:
            scores[n] = -np.inf
            continue
        scores[n] = v[s]
        for t in range(Tn - 1, -1, -1):
            frame_tokens[n, t] = tok[s >> 1] if s & 1 else blank
            if s & 1:
                emit_frames[n, s >> 1] = t      # (walking down: the last one written is the first frame)
            s -= d[t, s]
    return scores, frame_tokens, emit_frames


def best_score64(E64, labels, Tn, Ln, V, blank):
    """The best path's score on the float64 plane E64 (T, L+1); -inf stands for log 0."""
    v, _ = _lattice(E64, tokens_of(labels, Ln, V, blank), Tn, Ln, np.float64, -np.inf)
    return float(max(v[2 * Ln], v[2 * Ln - 1]) if Ln > 0 else v[0])


def path_score64(E64, frame_tokens, labels, Tn, Ln, V, blank):
    """The float64 sum of emissions along frame_tokens[:Tn], which must collapse to the labels (asserted)."""
    tok = tokens_of(labels, Ln, V, blank)
    l, prev, total = -1, blank, 0.0                # l: the label the path is in or has last left
    for t in range(Tn):
        k = int(frame_tokens[t])
        if k == blank:
            total += E64[t, 0]
        else:
            if prev == blank or k != prev:
                l += 1
            assert l < Ln and tok[l] == k, (t, k, l)
            total += E64[t, 1 + l]
        prev = k
    assert l == Ln - 1, (l, Ln)
    return float(total)
