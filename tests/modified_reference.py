"""fp64 NumPy reference of k2's two lattice topologies with the delay penalty, for the pruned and the simple loss -- test
infrastructure.

Utterance n: T_n = xn[n] frames, U_n = yn[n] labels, cell (t,u) holds (lpB, lpL); true -inf outside a band.

    delay penalty:  lpL(t,u) += dp * ((T_n - 1) / 2 - t)     (dp: the fp32 value the C entries receive, arithmetic in fp64)
    "regular":      the lattice of tests/pruned_reference.py (oracle.transduce_np._sweeps_fast), a terminal blank
    "modified":     alpha(0,0) = 0;  alpha(t,u) = lse(alpha(t-1,u) + lpB(t-1,u), alpha(t-1,u-1) + lpL(t-1,u-1)),
                    1 <= t <= T_n;  cost = -alpha(T_n, U_n);  no terminal blank

The modified recurrence is written out frame by frame -- NOT as the regular lattice on the sheared plane, which is how
the kernels run it: the tests check that identity (sheared_window builds the sheared plane for them).  Gradients come from
the backward recurrence beta(T_n,U_n) = 0, beta(t,u) = lse(beta(t+1,u) + lpB(t,u), beta(t+1,u+1) + lpL(t,u)).
"""
import numpy as np

import pruned_reference as pr
import simple_reference as sr
from oracle import transduce_np

upstream = pr.upstream


def penalised(lpl, Tn, dp):
    """lpL of a (T_n, .) window with the delay penalty of every frame added."""
    t = np.arange(lpl.shape[0], dtype=np.float64)
    return lpl + float(np.float32(dp)) * ((Tn - 1) / 2.0 - t)[:, None]


def window64(lpb, lpl, rnnt_type, lam=0.0):
    """(cost, gb, gl) of one utterance's (T_n, U_n + 1) window (the last column's label channel is not read): the cost and
    d cost / d (lpB, lpL), the label's scaled by 1 + lam (FastEmit).  No path: (+inf, zeros, zeros)."""
    Tn, W = lpb.shape
    lpl = lpl.copy()
    lpl[:, W - 1] = -np.inf
    zero = np.zeros((Tn, W))
    with np.errstate(all="ignore"):
        if rnnt_type == "regular":
            al, be = transduce_np._sweeps_fast(lpb, lpl)
            ll = be[0, 0]
            if not np.isfinite(ll):
                return np.inf, zero, zero.copy()
            gb, gl = zero, zero.copy()
            gb[:Tn - 1] = -np.exp(al[:Tn - 1] + be[1:] + lpb[:Tn - 1] - ll)
            gb[Tn - 1, W - 1] = -np.exp(al[Tn - 1, W - 1] + lpb[Tn - 1, W - 1] - ll)
            gl[:, :W - 1] = -(1.0 + lam) * np.exp(al[:, :W - 1] + be[:, 1:] + lpl[:, :W - 1] - ll)
        else:
            assert rnnt_type == "modified"
            al = np.full((Tn + 1, W), -np.inf)
            be = np.full((Tn + 1, W + 1), -np.inf)                  # (a column behind the last: absent terms)
            al[0, 0] = 0.0
            for t in range(1, Tn + 1):
                al[t] = al[t - 1] + lpb[t - 1]
                al[t, 1:] = np.logaddexp(al[t, 1:], al[t - 1, :W - 1] + lpl[t - 1, :W - 1])
            be[Tn, W - 1] = 0.0
            for t in range(Tn - 1, -1, -1):
                be[t, :W] = np.logaddexp(be[t + 1, :W] + lpb[t], be[t + 1, 1:] + lpl[t])
            ll = al[Tn, W - 1]
            if not np.isfinite(ll):
                return np.inf, zero, zero.copy()
            gb = -np.exp(al[:Tn] + lpb + be[1:, :W] - ll)
            gl = -(1.0 + lam) * np.exp(al[:Tn] + lpl + be[1:, 1:] - ll)
    return -ll, np.nan_to_num(gb, nan=0.0), np.nan_to_num(gl, nan=0.0)


def brute_force_cost(lpb, lpl, rnnt_type):
    """-log of the summed probability of every path of one window, by enumeration (small lattices only)."""
    Tn, W = lpb.shape
    total = []

    def regular(t, u, acc):
        if t == Tn - 1 and u == W - 1:
            total.append(acc + lpb[t, u])
            return
        if t < Tn - 1:
            regular(t + 1, u, acc + lpb[t, u])
        if u < W - 1:
            regular(t, u + 1, acc + lpl[t, u])

    def modified(t, u, acc):
        if t == Tn:
            if u == W - 1:
                total.append(acc)
            return
        modified(t + 1, u, acc + lpb[t, u])
        if u < W - 1:
            modified(t + 1, u + 1, acc + lpl[t, u])

    (regular if rnnt_type == "regular" else modified)(0, 0, 0.0)
    total = np.array(total if total else [-np.inf])
    with np.errstate(all="ignore"):
        m = total.max()
        return np.inf if np.isneginf(m) else -(m + np.log(np.exp(total - m).sum()))


def sheared_window(lpb, lpl):
    """The (T_n - U_n + 1, U_n + 1) regular window the kernels sweep for a modified (T_n, U_n + 1) window: cell (t',u) holds
    the pair of (t' + u, u); the virtual terminal cell (T_n - U_n, U_n) holds a blank of 0.  None where T_n < U_n."""
    Tn, W = lpb.shape
    if Tn < W - 1:
        return None
    tp, u = np.meshgrid(np.arange(Tn - W + 2), np.arange(W), indexing="ij")
    t = tp + u
    real = t < Tn
    sb = np.full(t.shape, -np.inf)
    sl = np.full(t.shape, -np.inf)
    sb[real] = lpb[t[real], u[real]]
    sl[real] = lpl[t[real], u[real]]
    sb[Tn - W + 1, W - 1] = 0.0
    return sb, sl


def pruned64(logits, labels, starts, xn, yn, blank, lam=0.0, dp=0.0, rnnt_type="regular", go=None):
    """pruned_reference.pruned_loss64 with a topology and a delay penalty: dict(costs, dlogits, pair_grads (N,T,U,2) by
    (t,u), unscaled)."""
    z = np.asarray(logits, np.float64)
    N, T, S, V = z.shape
    U = np.asarray(labels).shape[1] + 1
    go = upstream(N) if go is None else np.asarray(go, np.float64)
    lp_all = transduce_np.log_softmax(z)
    costs = np.zeros(N)
    dz = np.zeros_like(z)
    pair_grads = np.zeros((N, T, U, 2))
    for n in range(N):
        Tn, W = int(xn[n]), int(yn[n]) + 1
        lab_n = np.asarray(labels[n], np.int64)
        lpb, lpl, s_of = pr.band_pairs64(lp_all[n], lab_n, np.asarray(starts[n]), Tn, W, blank)
        costs[n], gb, gl = window64(lpb, penalised(lpl, Tn, dp), rnnt_type, lam)
        pair_grads[n, :Tn, :W, 0] = gb
        pair_grads[n, :Tn, :W, 1] = gl
        t, u = np.nonzero(s_of >= 0)
        s = s_of[t, u]
        p = np.exp(lp_all[n, t, s])
        gB, gL = gb[t, u], gl[t, u]
        d = -p * (gB + gL)[:, None]
        d[np.arange(len(t)), blank] += gB
        lab = np.where(u < U - 1, lab_n[np.minimum(u, U - 2)] if U > 1 else blank, blank)
        d[np.arange(len(t)), lab] += gL
        dz[n, t, s] = d * go[n]
    return dict(costs=costs, dlogits=dz, pair_grads=pair_grads)


def simple64(am, lm, labels, xn, yn, blank, lm_only_scale=0.0, lam=0.0, dp=0.0, rnnt_type="regular", go=None):
    """simple_reference.simple_loss64 (am_only_scale = 0) with a topology and a delay penalty: dict(costs, pair_grads
    (N,T,U,2) unscaled, dam, dlm)."""
    am, lm = np.asarray(am, np.float64), np.asarray(lm, np.float64)
    N, T, V = am.shape
    U = lm.shape[1]
    go = upstream(N) if go is None else np.asarray(go, np.float64)
    c0, c1, _ = sr.scales(lm_only_scale, 0.0)
    pairs = sr.pairs64(am, lm, labels, blank, lm_only_scale, 0.0, None)
    sym = sr.symbols(labels, U, V, blank)
    costs = np.zeros(N)
    pg = np.zeros((N, T, U, 2))
    dam, dlm = np.zeros_like(am), np.zeros_like(lm)
    for n in range(N):
        Tn, W = int(xn[n]), int(yn[n]) + 1
        costs[n], gb, gl = window64(pairs[n, :Tn, :W, 0], penalised(pairs[n, :Tn, :W, 1], Tn, dp), rnnt_type, lam)
        pg[n, :Tn, :W, 0] = gb
        pg[n, :Tn, :W, 1] = gl
        G = go[n] * pg[n]
        Ssum = G[..., 0] + G[..., 1]
        joint = am[n][:, None, :] + lm[n][None, :, :]
        P = np.exp(joint - sr._lse(joint, -1)[..., None])
        PL = np.exp(lm[n] - sr._lse(lm[n], -1)[:, None])
        hot_a, hot_l = np.zeros((T, V)), np.zeros((U, V))
        for ch, s in ((0, np.full(U, blank, np.int64)), (1, sym[n])):
            for u in range(U):
                hot_a[:, s[u]] += G[:, u, ch]
                hot_l[u, s[u]] += G[:, u, ch].sum()
        dam[n] = c0 * hot_a - c0 * np.einsum("tu,tuv->tv", Ssum, P)
        dlm[n] = (c0 + c1) * hot_l - c0 * np.einsum("tu,tuv->uv", Ssum, P) - c1 * PL * Ssum.sum(0)[:, None]
    return dict(costs=costs, pairs=pairs, pair_grads=pg, dam=dam, dlm=dlm)
