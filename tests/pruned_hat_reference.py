"""fp64 NumPy reference of the factorised-blank (HAT) loss on the pruned band -- test infrastructure.

A composition, no recursion of its own: HAT's log-probs (hat_reference.hat_log_probs64) in the band's cells
(pruned_reference.band_pairs64, true -inf outside), the delay penalty and either topology
(modified_reference.penalised / window64), and HAT's chain rule from the gradient pair (gB, gL) of a row's cell:

    u_b = gB (1 - sig) - gL sig,   u_v = gL ([v == label] - q_v),   q = softmax of the non-blank logits
"""
import numpy as np

import hat_reference as hr
import modified_reference as mr
import pruned_reference as pr

upstream = pr.upstream


def window_pairs64(logits_n, labels_n, starts_n, Tn, W, blank, dp=0.0):
    """(lpb, lpl, s_of) of one utterance's (T_n, U_n + 1) window, the penalty added."""
    lpb, lpl, s_of = pr.band_pairs64(hr.hat_log_probs64(logits_n, blank), np.asarray(labels_n, np.int64),
                                     np.asarray(starts_n), Tn, W, blank)
    return lpb, mr.penalised(lpl, Tn, dp), s_of


def pruned_hat64(logits, labels, starts, xn, yn, blank, lam=0.0, dp=0.0, rnnt_type="regular", go=None):
    """dict(costs (N,), dlogits (N,T,S,V) at the upstream gradient ``go`` (default: upstream(N))).  An utterance whose
    band holds no path: cost +inf, zero gradients."""
    z = np.asarray(logits, np.float64)
    N, T, S, V = z.shape
    go = upstream(N) if go is None else np.asarray(go, np.float64)
    costs, dz = np.zeros(N), np.zeros_like(z)
    for n in range(N):
        Tn, W = int(xn[n]), int(yn[n]) + 1
        lab_n = np.asarray(labels[n], np.int64)
        lpb, lpl, s_of = window_pairs64(z[n], lab_n, starts[n], Tn, W, blank, dp)
        costs[n], gb, gl = mr.window64(lpb, lpl, rnnt_type, lam)
        t, u = np.nonzero(s_of >= 0)
        rows = z[n, t, s_of[t, u]]                                     # (rows, V)
        keep, logq, zb = hr._parts(rows, blank)
        e = np.exp(-np.abs(zb))
        sig = np.where(zb >= 0, 1.0 / (1.0 + e), e / (1.0 + e))
        gB, gL = gb[t, u], gl[t, u]                                    # (gL is 0 in the window's last column)
        d = np.zeros_like(rows)
        d[:, keep] = -np.exp(logq) * gL[:, None]
        d[:, blank] = gB * (1.0 - sig) - gL * sig
        has = u < W - 1
        d[np.nonzero(has)[0], lab_n[u[has]]] += gL[has]
        dz[n, t, s_of[t, u]] = d * go[n]
    return dict(costs=costs, dlogits=dz)
