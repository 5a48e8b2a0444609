"""fp64 NumPy reference of the factorised-blank (HAT) loss -- test infrastructure.

    lpB = -sp(-z_b), lnb = -sp(z_b), lp[v] = ((z_v - m) - log s) + lnb for v != b   (m, s over the non-blank logits)

and the chain from d cost / d log-probs (the oracle's transducer in fp64) to d cost / d z:

    u_b = gB (1 - sig) - gL sig,   u_v = gL ([v == label] - q_v),   q = softmax of the non-blank logits
"""
import numpy as np

from oracle import transduce_np


def _sp(x):
    return np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x)))


def _parts(z, blank):
    """(keep mask, log q (..., V-1) of the non-blank softmax, z_b) in fp64; -inf non-blank logits are masked entries."""
    z = np.asarray(z, dtype=np.float64)
    keep = np.arange(z.shape[-1]) != blank
    rest = z[..., keep]
    m = rest.max(axis=-1, keepdims=True)
    with np.errstate(divide="ignore"):
        logq = (rest - m) - np.log(np.exp(rest - m).sum(axis=-1, keepdims=True))
    return keep, logq, z[..., blank]


def hat_log_probs64(z, blank):
    keep, logq, zb = _parts(z, blank)
    out = np.empty(np.shape(z), dtype=np.float64)
    out[..., keep] = logq + (-_sp(zb))[..., None]
    out[..., blank] = -_sp(-zb)
    return out


def shifted_logits64(z, blank):
    """z' of the identity: HAT on z is the standard loss on z', z'_b = z_b + log sum_{v != b} exp z_v."""
    z = np.asarray(z, dtype=np.float64)
    keep = np.arange(z.shape[-1]) != blank
    rest = z[..., keep]
    m = rest.max(axis=-1)
    out = z.copy()
    out[..., blank] = z[..., blank] + (m + np.log(np.exp(rest - m[..., None]).sum(axis=-1)))
    return out


def hat_loss64(z, labels, xn, yn, blank, lam=0.0):
    """costs (N,) and d costs / d z (N,T,U,V), fp64; zero outside every utterance's window."""
    z = np.asarray(z, dtype=np.float64)
    N, T, U, V = z.shape
    costs, glp = transduce_np.transduce_batch(hat_log_probs64(z, blank), labels, xn, yn, blank=blank,
                                              fastemit_lambda=lam, fast=True)
    keep, logq, zb = _parts(z, blank)
    sig = np.where(zb >= 0, 1.0 / (1.0 + np.exp(-np.abs(zb))), np.exp(-np.abs(zb)) / (1.0 + np.exp(-np.abs(zb))))
    gB = glp[..., blank]
    # the label's slot is the only non-blank one the lattice's gradient fills: gL = the sum over the non-blank slots
    gL = glp[..., keep].sum(axis=-1)
    dz = np.empty_like(z)
    dz[..., keep] = glp[..., keep] - np.exp(logq) * gL[..., None]
    dz[..., blank] = gB * (1.0 - sig) - gL * sig
    return costs, dz
