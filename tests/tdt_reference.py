"""fp64 NumPy reference of the token-and-duration transducer (TDT) loss -- test infrastructure.

Logits (N,T,U,V+D): tok = log_softmax(z[:V]) - sigma, dur = log_softmax(z[V:]).  Edges out of cell (t,u) of an utterance
with T_n frames and U_n labels, d = durations[i]:

    blank, d >  0, weight tok[blank] + dur[i]:       to (t+d, u) if t+d < T_n;  to the end if t+d == T_n and u == U_n
    label, d >= 0, weight tok[labels[u]] + dur[i]:   to (t+d, u+1) if u < U_n and t+d < T_n

alpha / beta by log-sum-exp over these edges, costs = -ll; an edge's occupancy is exp(alpha + w + beta(dest) - ll), label
edges times (1 + lam); per cell G_b, G_l, G_dur[i] and S = G_b + G_l, and

    dz[v] = p_v S - [v == blank] G_b - [v == label] G_l,     dz[V+i] = q_i S - G_dur[i]
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


def tdt_log_probs64(z, D):
    """(token log-softmax (..., V), duration log-softmax (..., D)) in fp64; sigma not subtracted."""
    z = np.asarray(z, dtype=np.float64)
    V = z.shape[-1] - D
    return log_softmax64(z[..., :V]), log_softmax64(z[..., V:])


def utterance(tok, dur, labels, Tn, Un, durations, blank, lam=0.0):
    """One utterance from tok (T,U,V) (sigma already subtracted) and dur (T,U,D): (ll, alpha (Tn,Un+1), beta, G (Tn,Un+1,2+D))."""
    D = len(durations)
    alpha = np.full((Tn, Un + 1), NEG)
    beta = np.full((Tn, Un + 1), NEG)
    lab = [int(labels[u]) for u in range(Un)]
    for t in range(Tn):
        for u in range(Un + 1):
            if t == 0 and u == 0:
                alpha[0, 0] = 0.0
                continue
            terms = []
            for i, d in enumerate(durations):
                if d > 0 and t - d >= 0:
                    terms.append(alpha[t - d, u] + tok[t - d, u, blank] + dur[t - d, u, i])
                if u > 0 and t - d >= 0:
                    terms.append(alpha[t - d, u - 1] + tok[t - d, u - 1, lab[u - 1]] + dur[t - d, u - 1, i])
            alpha[t, u] = _lse(terms)
    ll = _lse([alpha[Tn - d, Un] + tok[Tn - d, Un, blank] + dur[Tn - d, Un, i]
               for i, d in enumerate(durations) if d > 0 and Tn - d >= 0])
    for t in range(Tn - 1, -1, -1):
        for u in range(Un, -1, -1):
            terms = []
            for i, d in enumerate(durations):
                if d > 0 and t + d < Tn:
                    terms.append(tok[t, u, blank] + dur[t, u, i] + beta[t + d, u])
                if d > 0 and t + d == Tn and u == Un:
                    terms.append(tok[t, u, blank] + dur[t, u, i])
                if u < Un and t + d < Tn:
                    terms.append(tok[t, u, lab[u]] + dur[t, u, i] + beta[t + d, u + 1])
            beta[t, u] = _lse(terms)
    G = np.zeros((Tn, Un + 1, 2 + D))
    for t in range(Tn):
        for u in range(Un + 1):
            for i, d in enumerate(durations):
                gb = gl = 0.0
                if d > 0 and t + d < Tn:
                    gb = np.exp(alpha[t, u] + tok[t, u, blank] + dur[t, u, i] + beta[t + d, u] - ll)
                elif d > 0 and t + d == Tn and u == Un:
                    gb = np.exp(alpha[t, u] + tok[t, u, blank] + dur[t, u, i] - ll)
                if u < Un and t + d < Tn:
                    gl = (1.0 + lam) * np.exp(alpha[t, u] + tok[t, u, lab[u]] + dur[t, u, i] + beta[t + d, u + 1] - ll)
                G[t, u, 0] += gb
                G[t, u, 1] += gl
                G[t, u, 2 + i] = gb + gl
    return ll, alpha, beta, G


def tdt_loss64(z, labels, xn, yn, durations, blank, sigma=0.0, lam=0.0):
    """costs (N,), d costs / d z (N,T,U,V+D) and the G plane (N,T,U,2+D), fp64; zero outside every utterance's window,
    NaN cost and zeros for an utterance whose lengths are out of range."""
    z = np.asarray(z, dtype=np.float64)
    N, T, U, W = z.shape
    D = len(durations)
    V = W - D
    tok, dur = tdt_log_probs64(z, D)
    p, q = np.exp(tok), np.exp(dur)
    tok = tok - sigma
    costs = np.zeros(N)
    dz = np.zeros_like(z)
    G = np.zeros((N, T, U, 2 + D))
    for n in range(N):
        Tn, Un = int(xn[n]), int(yn[n])
        if not (1 <= Tn <= T and 0 <= Un <= U - 1):
            costs[n] = np.nan
            continue
        ll, _, _, g = utterance(tok[n], dur[n], labels[n], Tn, Un, durations, blank, lam)
        costs[n] = -ll
        G[n, :Tn, :Un + 1] = g
        S = g[..., 0] + g[..., 1]
        d = dz[n, :Tn, :Un + 1]
        d[..., :V] = p[n, :Tn, :Un + 1] * S[..., None]
        d[..., blank] -= g[..., 0]
        for u in range(Un):
            d[:, u, int(labels[n, u])] -= g[:, u, 1]
        d[..., V:] = q[n, :Tn, :Un + 1] * S[..., None] - g[..., 2:]
    return costs, dz, G


def enumerate_paths(tok, dur, labels, Tn, Un, durations, blank):
    """log of the sum over every path from (0,0) to the end, each path walked on its own (no dynamic programming)."""
    total = []

    def walk(t, u, score):
        for i, d in enumerate(durations):
            if d > 0 and t + d < Tn:
                walk(t + d, u, score + tok[t, u, blank] + dur[t, u, i])
            if d > 0 and t + d == Tn and u == Un:
                total.append(score + tok[t, u, blank] + dur[t, u, i])
            if u < Un and t + d < Tn:
                walk(t + d, u + 1, score + tok[t, u, int(labels[u])] + dur[t, u, i])

    walk(0, 0, 0.0)
    return _lse(total)
