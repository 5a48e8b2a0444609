"""fp64 reference of the joint network fused into the TDT loss -- test infrastructure (a helper, not a test file).

The joint in torch on the CPU, ``z = linear(act(f[:, :, None] + g[:, None]), W, b)`` in float64; tests/tdt_reference.py's
``tdt_loss64`` on z gives the costs and dz = d cost / d z; the gradients to f, g, W and b are autograd's of
``(z * dz * weights[:, None, None, None]).sum()`` -- the chain rule through the joint with dz held constant.  With dropout
the keep mask is the host definition of tests/joint_dropout_mask.py, multiplied into act(f+g) with the scale 1/(1-p).
"""
import numpy as np
import torch

import joint_dropout_mask
from tdt_reference import tdt_loss64

ACTS = {"tanh": torch.tanh, "relu": torch.relu}


def joint_logits64(f, g, weight, bias, act, keep=None, p=0.0):
    """z (N,T,U+1,V+D) float64 of f (N,T,H), g (N,U+1,H), weight (V+D,H), bias (V+D,) or None; keep: (N,T,U+1,H) bool."""
    h = ACTS[act](f[:, :, None] + g[:, None])
    if keep is not None:
        h = h * torch.as_tensor(keep, dtype=torch.float64) * joint_dropout_mask.scale(p)
    return torch.nn.functional.linear(h, weight, bias)


def tdt_joint_reference(f, g, weight, bias, labels, xn, yn, durations, act="tanh", blank=0, sigma=0.0, lam=0.0,
                        weights=None, dropout=0.0, seed=None, want_grads=True):
    """costs (N,) float64 tensor (NaN for an utterance whose lengths are out of range) and, want_grads, d(sum_n weights[n]
    costs[n]) / d (f, g, weight, bias) as float64 tensors (bias None: None); weights None: ones.  dropout > 0: the mask of
    (seed, dropout)."""
    leaves = [x.detach().double().clone().requires_grad_(True) if x is not None else None for x in (f, g, weight, bias)]
    fd, gd, wd, bd = leaves
    N, T, H = fd.shape
    U1 = gd.shape[1]
    keep = joint_dropout_mask.keep_mask(int(seed), dropout, N, T, U1, H) if dropout > 0 else None
    z = joint_logits64(fd, gd, wd, bd, act, keep, dropout)
    lab, x, y = (np.asarray(t.cpu()) for t in (labels, xn, yn))
    costs, dz, _ = tdt_loss64(z.detach().numpy(), lab, x, y, tuple(durations), blank, sigma, lam)
    costs = torch.from_numpy(costs)
    if not want_grads:
        return costs, None, None, None, None
    dz = torch.from_numpy(dz)
    w = torch.ones(N, dtype=torch.float64) if weights is None else torch.as_tensor(weights, dtype=torch.float64).cpu()
    # (a masked logit is -inf and its dz exactly zero: it is kept out of the product, -inf * 0 is not a number)
    (torch.where(dz != 0, z, torch.zeros_like(z)) * dz * w[:, None, None, None]).sum().backward()
    return (costs,) + tuple(x.grad if x is not None else None for x in leaves)


def nrel(got, ref):
    """Normwise relative error in fp64 (tests/test_gpu_joint.py's)."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((got - ref).norm() / ref.norm().clamp_min(1e-300))
