"""float64 reference of rnnt_loss_from_joint that applies the kernels' operand rounding -- TEST INFRASTRUCTURE ONLY.

The fused joint kernels (csrc/joint.hip) compute, per lattice cell of an utterance,
  h  = E(act_fp32(f + g))                 the activation in fp32, rounded once to E = the activations' dtype
  z  = h W_E^T + b                        W staged in E, fp32 accumulation, bias fp32
  dz = LSM_BWD(z, lse, gB, gL)            fp32
  df/dg = sum (E(dz) W_E) * act'(h)       dz rounded to E as the second product's operand
  dW = sum E(dz)^T h,  db = sum dz        db from the unrounded dz
This module repeats those steps in float64 with the same roundings of the OPERANDS (h and W always; dz when
model_dz_rounding), so what remains between a kernel and it is the kernels' fp32 accumulation and the rounding of the
outputs.  With E = fp32 and model_dz_rounding off it is the plain fp64 joint (the autograd reference of
tests/test_gpu_joint.py, up to act evaluated in fp32).

It runs per utterance, in chunks of frames, on the device of its inputs (CPU for small cases, the GPU for large ones),
with plain torch float64 arithmetic; alpha / beta come from oracle.transduce_np._sweeps_fast on the utterance's
(T_n, U_n) log-prob planes only -- no (N,T,U,V) tensor is formed.
"""
import numpy as np
import torch

from oracle.transduce_np import _sweeps_fast


def _act(name, x):
    return torch.tanh(x) if name == "tanh" else torch.clamp_min(x, 0.0)


def _act_grad(name, y):
    """act' from the activation's output, as the kernels (and autograd's tanh / relu backward) take it."""
    return 1.0 - y * y if name == "tanh" else (y > 0).to(y.dtype)


def valid_length(x, y, T, U1):
    """The library's test for an utterance's lengths (common.h utt_lens): 1 <= x <= T, 0 <= y < U+1."""
    return 1 <= x <= T and 0 <= y < U1


def joint_reference(f, g, weight, bias, labels, xn, yn, act="tanh", blank=0, fastemit_lambda=0.0, upstream=None,
                    model_dz_rounding=False, act_dtype=torch.float32, chunk_elems=1 << 25):
    """costs (N,), df (N,T,H), dg (N,U+1,H), dW (V,H), db (V,), all float64 on f's device: gradients of
    sum_n upstream[n] * cost[n] (upstream defaults to ones).  E = f.dtype.  An utterance whose lengths are invalid gets
    a NaN cost and contributes nothing.  act_dtype is the precision act(f+g) is evaluated in (the kernels': fp32); with
    float64 inputs and act_dtype=float64 nothing is rounded anywhere."""
    E, dev = f.dtype, f.device
    N, T, H = f.shape
    U1 = g.shape[1]
    V = weight.shape[0]
    d64 = torch.float64
    W = weight.to(E).to(d64)                                   # W_E
    b = bias.to(d64) if bias is not None else torch.zeros(V, dtype=d64, device=dev)
    up = upstream.to(d64).cpu() if upstream is not None else torch.ones(N, dtype=d64)
    xs, ys = [int(v) for v in xn.cpu()], [int(v) for v in yn.cpu()]
    lab_all = labels.cpu().long()
    costs = torch.full((N,), float("nan"), dtype=d64)
    df = torch.zeros(N, T, H, dtype=d64, device=dev)
    dg = torch.zeros(N, U1, H, dtype=d64, device=dev)
    dW = torch.zeros(V, H, dtype=d64, device=dev)
    db = torch.zeros(V, dtype=d64, device=dev)

    for n in range(N):
        Tn, yl = xs[n], ys[n]
        if not valid_length(Tn, yl, T, U1):
            continue
        Un = yl + 1
        lab = lab_all[n, :yl].to(dev)
        fn, gn = f[n, :Tn], g[n, :Un]
        tc = max(1, chunk_elems // max(1, Un * max(H, V)))   # frames per chunk

        def h_of(t0, t1):
            x = fn[t0:t1, None, :].to(act_dtype) + gn[None, :, :].to(act_dtype)
            return _act(act, x).to(E).to(d64)                 # (tc, Un, H)

        # pass 1: log-normaliser, blank and label log-probs per cell
        lse = torch.empty(Tn, Un, dtype=d64, device=dev)
        lpb = torch.empty(Tn, Un, dtype=d64, device=dev)
        lpl = torch.zeros(Tn, Un, dtype=d64, device=dev)
        for t0 in range(0, Tn, tc):
            t1 = min(Tn, t0 + tc)
            z = h_of(t0, t1) @ W.T + b
            m = z.max(-1, keepdim=True).values
            ls = m[..., 0] + torch.log(torch.exp(z - m).sum(-1))
            lse[t0:t1] = ls
            lpb[t0:t1] = z[..., blank] - ls
            if yl > 0:
                lpl[t0:t1, :yl] = torch.gather(z[:, :yl], 2, lab.view(1, yl, 1).expand(t1 - t0, yl, 1))[..., 0] \
                    - ls[:, :yl]

        # alpha / beta on the (Tn, Un) planes; d cost / d log-probs of blank and label (compute_gradient's formulas)
        pb, pl = lpb.cpu().numpy(), lpl.cpu().numpy()
        al, be = _sweeps_fast(pb, pl)
        ll = be[0, 0]
        costs[n] = -ll
        gB = np.zeros((Tn, Un))
        gB[:Tn - 1] = -np.exp(al[:Tn - 1] + be[1:] + pb[:Tn - 1] - ll)
        gB[Tn - 1, Un - 1] = -np.exp(al[Tn - 1, Un - 1] + pb[Tn - 1, Un - 1] - ll)
        gL = np.zeros((Tn, Un))
        if Un > 1:
            gL[:, :Un - 1] = -(1.0 + fastemit_lambda) * np.exp(al[:, :Un - 1] + be[:, 1:] + pl[:, :Un - 1] - ll)
        w = float(up[n])
        gB = torch.from_numpy(gB * w).to(dev)
        gL = torch.from_numpy(gL * w).to(dev)

        # pass 2: dz by the LSM_BWD formula, the second products
        for t0 in range(0, Tn, tc):
            t1 = min(Tn, t0 + tc)
            h = h_of(t0, t1)
            z = h @ W.T + b
            dz = -torch.exp(z - lse[t0:t1, :, None]) * (gB[t0:t1] + gL[t0:t1])[..., None]
            dz[..., blank] += gB[t0:t1]
            if yl > 0:
                dz[:, :yl].scatter_add_(2, lab.view(1, yl, 1).expand(t1 - t0, yl, 1), gL[t0:t1, :yl, None])
            db += dz.sum((0, 1))
            dzr = dz.to(E).to(d64) if model_dz_rounding else dz
            dx = (dzr @ W) * _act_grad(act, h)
            df[n, t0:t1] += dx.sum(1)
            dg[n, :Un] += dx.sum(0)
            dW += dzr.reshape(-1, V).T @ h.reshape(-1, H)
    return costs.to(dev), df, dg, dW, db
