"""fp64 reference of pruned_rnnt_loss_from_joint -- test infrastructure.

joint_reference.py's conventions on the band: h = E(act_fp32(f[n,t] + g[n,u])), u = starts[n,t] + s, E the activations'
dtype; z = h W_E^T + b in fp64; the loss and dz of pruned_reference.pruned_loss64; dz rounded to E in front of the second
products when E is a half type (db from the unrounded dz)."""
import numpy as np
import torch

from joint_reference import _act, _act_grad
from pruned_reference import pruned_loss64


def nrel(got, want):
    """Normwise relative error of a gradient."""
    got, want = got.detach().double().cpu(), want.double()
    return float((got - want).norm() / want.norm().clamp_min(1e-300))


def pruned_joint_reference(f, g, weight, bias, labels, starts, S, xn, yn, act="tanh", blank=0, lam=0.0, go=None):
    """(costs, df, dg, dW, db) in float64 on the CPU: gradients of sum_n go[n] * cost[n] (pruned_loss64's default go)."""
    E, d64 = f.dtype, torch.float64
    N, T, H = f.shape
    U, V = g.shape[1], weight.shape[0]
    W = weight.to(E).to(d64)
    b = bias.to(d64) if bias is not None else torch.zeros(V, dtype=d64)
    u = torch.as_tensor(starts).long()[..., None] + torch.arange(S)                      # (N,T,S)
    idx = u.clamp(0, U - 1).reshape(N, T * S, 1).expand(N, T * S, H)
    h = _act(act, f.float()[:, :, None, :] + g.float().gather(1, idx).reshape(N, T, S, H)).to(E).to(d64)
    ref = pruned_loss64((h @ W.T + b).numpy(), np.asarray(labels), np.asarray(starts), np.asarray(xn), np.asarray(yn),
                        blank, lam, go)
    dz = torch.from_numpy(ref["dlogits"])                                                # zero off the lattice
    dzr = dz.to(E).to(d64) if E != torch.float32 else dz
    dx = (dzr @ W) * _act_grad(act, h)
    dg = torch.zeros(N, U, H, dtype=d64).scatter_add_(1, idx, dx.reshape(N, T * S, H))
    return (torch.from_numpy(ref["costs"]), dx.sum(2), dg, dzr.reshape(-1, V).T @ h.reshape(-1, H),
            dz.sum((0, 1, 2)))
