"""fp64 NumPy reference of the pruned transducer loss -- test infrastructure.

    logits (N,T,S,V), row (n,t,s) = lattice cell (t, u = starts[n,t] + s);  lp = log_softmax(row)
    pair of the cell = (lp[blank], lp[labels[n,u]]);  every other cell of the grid: (-inf, -inf)

The band recursion runs with TRUE -inf outside the band (the kernels carry a finite floor there), vectorised by
anti-diagonal (oracle.transduce_np._sweeps_fast), per utterance over its (T_n, U_n + 1) window.  From the gradient pair
(gB, gL) of a row's cell and p = softmax(row):  dz = go[n] * ([v == blank] gB + [v == label] gL - p (gB + gL)).
"""
import numpy as np

from oracle import transduce_np


def upstream(N):
    """The upstream gradient of utterance n: 0.5 + 0.25 n -- not 1, exact in fp32."""
    return np.array([0.5 + 0.25 * n for n in range(N)], np.float64)


def band_pairs64(lp, labels_n, starts_n, Tn, Un, blank):
    """(lpb, lpl, s_of) over the (Tn, Un) window of one utterance: lp (T,S,V) fp64 log-probs; -inf outside the band;
    s_of[t,u] = the band row that maps to the cell, or -1."""
    T, S, V = lp.shape
    lpb = np.full((Tn, Un), -np.inf)
    lpl = np.full((Tn, Un), -np.inf)
    s_of = np.full((Tn, Un), -1, np.int64)
    t, s = np.meshgrid(np.arange(Tn), np.arange(S), indexing="ij")
    u = starts_n[:Tn, None].astype(np.int64) + s
    ok = (u >= 0) & (u < Un)
    t, s, u = t[ok], s[ok], u[ok]
    lpb[t, u] = lp[t, s, blank]
    s_of[t, u] = s
    lab = u < Un - 1                                   # (the window's last column has no label transition)
    lpl[t[lab], u[lab]] = lp[t[lab], s[lab], labels_n[u[lab]]]
    return lpb, lpl, s_of


def pruned_loss64(logits, labels, starts, xn, yn, blank, lam=0.0, go=None):
    """dict(costs (N,), dlogits (N,T,S,V) at the upstream gradient ``go`` (default: upstream(N)), pair_grads (N,T,U,2)
    unscaled and row-major, inband (N,T,U) bool).  An utterance whose band holds no path: cost +inf, zero gradients."""
    z = np.asarray(logits, np.float64)
    N, T, S, V = z.shape
    U = np.asarray(labels).shape[1] + 1
    go = upstream(N) if go is None else np.asarray(go, np.float64)
    lp_all = transduce_np.log_softmax(z)
    costs = np.zeros(N)
    dz = np.zeros_like(z)
    pair_grads = np.zeros((N, T, U, 2))
    inband = np.zeros((N, T, U), bool)
    for n in range(N):
        Tn, Un = int(xn[n]), int(yn[n]) + 1
        lab_n = np.asarray(labels[n], np.int64)
        lpb, lpl, s_of = band_pairs64(lp_all[n], lab_n, np.asarray(starts[n]), Tn, Un, blank)
        st = np.asarray(starts[n], np.int64)
        for t in range(T):                             # the band over the whole padded grid (for the tests' masks)
            lo, hi = max(st[t], 0), min(st[t] + S, U)
            if lo < hi:
                inband[n, t, lo:hi] = True
        with np.errstate(all="ignore"):
            al, be = transduce_np._sweeps_fast(lpb, lpl)
            ll = be[0, 0]
            if not np.isfinite(ll):
                costs[n] = np.inf
                continue
            costs[n] = -ll
            gb = np.zeros((Tn, Un))
            gl = np.zeros((Tn, Un))
            gb[:Tn - 1] = -np.exp(al[:Tn - 1] + be[1:] + lpb[:Tn - 1] - ll)
            gb[Tn - 1, Un - 1] = -np.exp(al[Tn - 1, Un - 1] + lpb[Tn - 1, Un - 1] - ll)
            gl[:, :Un - 1] = -(1.0 + lam) * np.exp(al[:, :Un - 1] + be[:, 1:] + lpl[:, :Un - 1] - ll)
        gb = np.nan_to_num(gb, nan=0.0)                # (-inf - -inf off the band: no path through the cell)
        gl = np.nan_to_num(gl, nan=0.0)
        pair_grads[n, :Tn, :Un, 0] = gb
        pair_grads[n, :Tn, :Un, 1] = gl
        t, u = np.nonzero(s_of >= 0)
        s = s_of[t, u]
        p = np.exp(lp_all[n, t, s])                    # (rows, V)
        gB, gL = gb[t, u], gl[t, u]
        d = -p * (gB + gL)[:, None]
        d[np.arange(len(t)), blank] += gB
        lab = np.where(u < U - 1, lab_n[np.minimum(u, U - 2)] if U > 1 else blank, blank)
        d[np.arange(len(t)), lab] += gL
        dz[n, t, s] = d * go[n]
    return dict(costs=costs, dlogits=dz, pair_grads=pair_grads, inband=inband)


def brute_force_cost(lp, labels_n, starts_n, Tn, Un, blank):
    """-log of the summed probability of every path of one utterance, by enumeration (small lattices only)."""
    lpb, lpl, _ = band_pairs64(np.asarray(lp, np.float64), np.asarray(labels_n, np.int64), np.asarray(starts_n), Tn, Un, blank)
    total = []

    def walk(t, u, acc):
        if t == Tn - 1 and u == Un - 1:
            total.append(acc + lpb[t, u])
            return
        if t < Tn - 1:
            walk(t + 1, u, acc + lpb[t, u])
        if u < Un - 1:
            walk(t, u + 1, acc + lpl[t, u])

    walk(0, 0, 0.0)
    total = np.array(total)
    with np.errstate(all="ignore"):
        m = total.max()
        return np.inf if np.isneginf(m) else -(m + np.log(np.exp(total - m).sum()))


def feasible_starts(rng, T, U, S, xn, yn, dead=None):
    """(N,T) int32 starts of random bands that hold a path: per utterance monotone, start[0] = 0, the last live start
    max(U_n + 1 - S, 0), steps <= S - 1.  Needs (T_n - 1)(S - 1) >= U_n + 1 - S.  Frames t >= T_n repeat the last live
    value, or hold ``dead`` where it is given."""
    N = len(xn)
    out = np.zeros((N, T), np.int32)
    for n in range(N):
        Tn, hi = int(xn[n]), max(int(yn[n]) + 1 - S, 0)
        assert (Tn - 1) * (S - 1) >= hi, "no band of this width holds a path"
        s = np.sort(rng.randint(0, hi + 1, size=Tn))
        s[-1] = hi
        for t in range(Tn - 2, -1, -1):
            s[t] = max(s[t], s[t + 1] - (S - 1))
        s[0] = 0                                       # (T_n = 1: hi = 0)
        for t in range(1, Tn):                         # (start[0] = 0 may have opened a step: close it from the front;
            s[t] = min(s[t], s[t - 1] + S - 1)         #  s[t] = min(s[t], t (S-1)), which still ends at hi)
        assert s[0] == 0 and s[-1] == hi and (np.diff(s) >= 0).all() and (np.diff(s) <= S - 1).all()
        out[n, :Tn] = s
        out[n, Tn:] = hi if dead is None else dead
    return out


def make_band_case(seed, N, T, U, S, V, blank=0, ragged=True, scale=1.0, lengths=None):
    """Seeded inputs of a pruned case: fp32 logits (N,T,S,V), labels (N,U-1) never blank, lengths (full in utterance 0,
    feasible for the band everywhere; ``lengths`` = (xn, yn): these), feasible starts."""
    rng = np.random.RandomState(seed)
    logits = (rng.randn(N, T, S, V) * scale).astype(np.float32)
    choices = np.array([v for v in range(V) if v != blank], np.int32)
    labels = choices[rng.randint(0, len(choices), size=(N, max(U - 1, 0)))].astype(np.int32)
    xn = np.full((N,), T, np.int32)
    yn = np.full((N,), U - 1, np.int32)
    if ragged and N > 1:
        xn[1:] = rng.randint(max(T // 2, 1), T + 1, size=N - 1)
        yn[1:] = rng.randint(U // 2, U, size=N - 1) if U > 1 else 0
    if lengths is not None:
        xn[:], yn[:] = lengths
    for n in range(N):                                # shorten the labels until the band can climb them
        while (int(xn[n]) - 1) * (S - 1) < max(int(yn[n]) + 1 - S, 0):
            yn[n] -= 1
    starts = feasible_starts(rng, T, U, S, xn, yn)
    return logits, labels, starts, xn, yn


def dense_from_band(logits, starts, U, fill_seed=0):
    """Dense (N,T,U,V) logits whose band cells hold the band's rows and whose other cells hold seeded noise: what the
    yardstick (the dense loss) runs on, and the full-lattice comparison."""
    N, T, S, V = logits.shape
    dense = np.random.RandomState(fill_seed).randn(N, T, U, V).astype(logits.dtype)
    n, t, s = np.meshgrid(np.arange(N), np.arange(T), np.arange(S), indexing="ij")
    u = starts[:, :, None].astype(np.int64) + s
    ok = (u >= 0) & (u < U)
    dense[n[ok], t[ok], u[ok]] = logits[n[ok], t[ok], s[ok]]
    return dense
