"""fp64 NumPy reference of the multi-blank transducer loss -- test infrastructure.

Logits (N,T,U,V), one softmax: lp = log_softmax(z) - sigma.  B blanks, blank_ids[i] with duration d = blank_durations[i]
(distinct integers in [1,8], 1 among them).  Edges out of cell (t,u) of an utterance with T_n frames and U_n labels:

    blank i, weight lp[blank_ids[i]]:  to (t+d, u) if t+d < T_n;  to the end if t+d == T_n and u == U_n
    label,   weight lp[labels[u]]:     to (t, u+1) if u < U_n

alpha / beta by log-sum-exp over these edges, costs = -ll; an edge's occupancy is exp(alpha + w + beta(dest) - ll), label
edges times (1 + lam); per cell G_l, G_blank[i] and S = G_l + sum_i G_blank[i], and

    dz[v] = p_v S - [v == labels[u]] G_l - sum_i [v == blank_ids[i]] G_blank[i]
"""
import numpy as np

NEG = -np.inf


def _lse(terms):
    terms = [x for x in terms if x > NEG]
    if not terms:
        return NEG
    m = max(terms)
    return m + np.log(sum(np.exp(x - m) for x in terms))


def log_softmax64(z):
    z = np.asarray(z, dtype=np.float64)
    m = z.max(axis=-1, keepdims=True)
    with np.errstate(divide="ignore"):
        return (z - m) - np.log(np.exp(z - m).sum(axis=-1, keepdims=True))


def utterance(lp, labels, Tn, Un, blank_ids, blank_durations, lam=0.0):
    """One utterance from lp (T,U,V) (sigma already subtracted): (ll, alpha (Tn,Un+1), beta, G (Tn,Un+1,1+B)); G[..., 0] is
    G_l, G[..., 1+i] is G_blank[i]."""
    B = len(blank_ids)
    blanks = list(zip([int(v) for v in blank_ids], [int(d) for d in blank_durations]))
    alpha = np.full((Tn, Un + 1), NEG)
    beta = np.full((Tn, Un + 1), NEG)
    lab = [int(labels[u]) for u in range(Un)]
    for t in range(Tn):
        for u in range(Un + 1):
            if t == 0 and u == 0:
                alpha[0, 0] = 0.0
                continue
            terms = [alpha[t - d, u] + lp[t - d, u, v] for v, d in blanks if t - d >= 0]
            if u > 0:
                terms.append(alpha[t, u - 1] + lp[t, u - 1, lab[u - 1]])
            alpha[t, u] = _lse(terms)
    ll = _lse([alpha[Tn - d, Un] + lp[Tn - d, Un, v] for v, d in blanks if Tn - d >= 0])
    for t in range(Tn - 1, -1, -1):
        for u in range(Un, -1, -1):
            terms = []
            for v, d in blanks:
                if t + d < Tn:
                    terms.append(lp[t, u, v] + beta[t + d, u])
                elif t + d == Tn and u == Un:
                    terms.append(lp[t, u, v])
            if u < Un:
                terms.append(lp[t, u, lab[u]] + beta[t, u + 1])
            beta[t, u] = _lse(terms)
    G = np.zeros((Tn, Un + 1, 1 + B))
    for t in range(Tn):
        for u in range(Un + 1):
            if u < Un:
                G[t, u, 0] = (1.0 + lam) * np.exp(alpha[t, u] + lp[t, u, lab[u]] + beta[t, u + 1] - ll)
            for i, (v, d) in enumerate(blanks):
                if t + d < Tn:
                    G[t, u, 1 + i] = np.exp(alpha[t, u] + lp[t, u, v] + beta[t + d, u] - ll)
                elif t + d == Tn and u == Un:
                    G[t, u, 1 + i] = np.exp(alpha[t, u] + lp[t, u, v] - ll)
    return ll, alpha, beta, G


def multiblank_loss64(z, labels, xn, yn, blank_ids, blank_durations, sigma=0.0, lam=0.0):
    """costs (N,), d costs / d z (N,T,U,V) and the G plane (N,T,U,1+B), fp64; zero outside every utterance's window, NaN
    cost and zeros for an utterance whose lengths are out of range."""
    z = np.asarray(z, dtype=np.float64)
    N, T, U, V = z.shape
    B = len(blank_ids)
    lp = log_softmax64(z)
    p = np.exp(lp)
    lp = lp - sigma
    costs = np.zeros(N)
    dz = np.zeros_like(z)
    G = np.zeros((N, T, U, 1 + B))
    for n in range(N):
        Tn, Un = int(xn[n]), int(yn[n])
        if not (1 <= Tn <= T and 0 <= Un <= U - 1):
            costs[n] = np.nan
            continue
        ll, _, _, g = utterance(lp[n], labels[n], Tn, Un, blank_ids, blank_durations, lam)
        costs[n] = -ll
        G[n, :Tn, :Un + 1] = g
        S = g.sum(-1)
        d = dz[n, :Tn, :Un + 1]
        d[...] = p[n, :Tn, :Un + 1] * S[..., None]
        for u in range(Un):
            d[:, u, int(labels[n, u])] -= g[:, u, 0]
        for i, v in enumerate(blank_ids):
            d[..., int(v)] -= g[..., 1 + i]
    return costs, dz, G


def enumerate_paths(lp, labels, Tn, Un, blank_ids, blank_durations):
    """log of the sum over every path from (0,0) to the end, each path walked on its own (no dynamic programming)."""
    total = []
    blanks = list(zip([int(v) for v in blank_ids], [int(d) for d in blank_durations]))

    def walk(t, u, score):
        for v, d in blanks:
            if t + d < Tn:
                walk(t + d, u, score + lp[t, u, v])
            elif t + d == Tn and u == Un:
                total.append(score + lp[t, u, v])
        if u < Un:
            walk(t, u + 1, score + lp[t, u, int(labels[u])])

    walk(0, 0, 0.0)
    return _lse(total)
