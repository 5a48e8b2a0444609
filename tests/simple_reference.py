"""The smoothed simple transducer loss, twice -- test infrastructure.

Per utterance (include/warp_rnnt_amd_simple.h), c1 = lm_only_scale, c2 = am_only_scale, c0 = 1 - c1 - c2 (not below 0, from
the fp32 values of the two scales, as the C entries form it), b = blank, q the log of a unigram distribution:

    sym(u,0) = b,  sym(u,1) = y_u for u < U-1 and 0 <= y_u < V, else b
    Z(t,u) = log sum_v exp(am[t,v] + lm[u,v]),  ZL(u) = log sum_v exp(lm[u,v]),  ZA(t) = log sum_v exp(am[t,v] + q[v])
    pair(t,u,c) = c0 (am[t,s] + lm[u,s] - Z(t,u)) + c1 (lm[u,s] - ZL(u)) + c2 (am[t,s] + q[s] - ZA(t)),  s = sym(u,c)

simple_loss64: NumPy fp64 -- the pairs, the lattice of tests/pruned_reference.py (oracle.transduce_np._sweeps_fast over the
utterance's window) and the analytic gradients to am, lm and q.
chain32: the same definition in plain fp32 torch on any device, warp_rnnt.rnnt_loss(blank=-1) and autograd behind it --
the unfused chain, the yardstick of the GPU tests.
"""
import numpy as np
import torch

from oracle import transduce_np

TINY = float(np.finfo(np.float32).tiny)


def upstream(N):
    """The upstream gradient of utterance n: 0.5 + 0.25 n -- not 1, exact in fp32."""
    return np.array([0.5 + 0.25 * n for n in range(N)], np.float64)


def scales(lm_only_scale, am_only_scale):
    """(c0, c1, c2) as the C entries form them: the fp32 values of the two scales, c0 = max((1 - c1) - c2, 0) in fp32."""
    c1, c2 = np.float32(lm_only_scale), np.float32(am_only_scale)
    c0 = max(np.float32(np.float32(1.0) - c1) - c2, np.float32(0.0))
    return float(c0), float(c1), float(c2)


def symbols(labels, U, V, blank):
    """(N,U) int64: sym(u,1) of every column."""
    lab = np.asarray(labels, np.int64).reshape(len(labels), -1)
    lab = np.where((lab >= 0) & (lab < V), lab, blank)
    return np.concatenate([lab, np.full((lab.shape[0], 1), blank, np.int64)], axis=1)[:, :U]


def _lse(x, axis):
    m = x.max(axis=axis, keepdims=True)
    return (m + np.log(np.exp(x - m).sum(axis=axis, keepdims=True))).squeeze(axis)


def log_unigram64(lm):
    """k2's batch unigram in fp64: log(mean over all (n,u) rows of softmax(lm[n,u,:]) + tiny)."""
    lm = np.asarray(lm, np.float64)
    p = np.exp(lm - _lse(lm, -1)[..., None])
    return np.log(p.mean(axis=(0, 1)) + TINY)


def pairs64(am, lm, labels, blank, lm_only_scale=0.0, am_only_scale=0.0, q=None):
    """(N,T,U,2) fp64 pairs as defined above."""
    am, lm = np.asarray(am, np.float64), np.asarray(lm, np.float64)
    N, T, V = am.shape
    U = lm.shape[1]
    c0, c1, c2 = scales(lm_only_scale, am_only_scale)
    sym = symbols(labels, U, V, blank)
    out = np.zeros((N, T, U, 2))
    for n in range(N):
        Z = _lse(am[n][:, None, :] + lm[n][None, :, :], -1)                  # (T,U)
        ZL = _lse(lm[n], -1)                                                  # (U,)
        qq = np.zeros(V) if q is None else np.asarray(q, np.float64)
        ZA = _lse(am[n] + qq[None, :], -1)                                    # (T,)
        for ch, s in ((0, np.full(U, blank, np.int64)), (1, sym[n])):
            a, l = am[n][:, s], lm[n][np.arange(U), s]                        # (T,U), (U,)
            out[n, :, :, ch] = c0 * (a + l[None, :] - Z) + c1 * (l - ZL)[None, :] + c2 * (a + qq[s][None, :] - ZA[:, None])
    return out


def lattice64(pairs, xn, yn, lam=0.0):
    """(costs (N,), pair_grads (N,T,U,2)) of an fp64 pair plane: zero gradients outside the (T_n, U_n + 1) windows."""
    N, T, U, _ = pairs.shape
    costs = np.zeros(N)
    grads = np.zeros((N, T, U, 2))
    for n in range(N):
        Tn, Un = int(xn[n]), int(yn[n]) + 1
        lpb, lpl = pairs[n, :Tn, :Un, 0], pairs[n, :Tn, :Un, 1].copy()
        lpl[:, Un - 1] = -np.inf                                              # (the window's last column emits nothing)
        with np.errstate(all="ignore"):
            al, be = transduce_np._sweeps_fast(lpb, lpl)
            ll = be[0, 0]
            costs[n] = -ll
            gb = np.zeros((Tn, Un))
            gl = np.zeros((Tn, Un))
            gb[:Tn - 1] = -np.exp(al[:Tn - 1] + be[1:] + lpb[:Tn - 1] - ll)
            gb[Tn - 1, Un - 1] = -np.exp(al[Tn - 1, Un - 1] + lpb[Tn - 1, Un - 1] - ll)
            gl[:, :Un - 1] = -(1.0 + lam) * np.exp(al[:, :Un - 1] + be[:, 1:] + lpl[:, :Un - 1] - ll)
        grads[n, :Tn, :Un, 0] = gb
        grads[n, :Tn, :Un, 1] = gl
    return costs, grads


def simple_loss64(am, lm, labels, xn, yn, blank, lm_only_scale=0.0, am_only_scale=0.0, lam=0.0, q=None, go=None):
    """dict(costs (N,), pairs, pair_grads (N,T,U,2) unscaled, dam (N,T,V), dlm (N,U,V) with q held fixed, dq (V,), and
    dlm_total = dlm plus the path through q = log_unigram64(lm)), the gradients at the upstream ``go`` (default:
    upstream(N)).  q: the log unigram (default with am_only_scale != 0: log_unigram64(lm))."""
    am, lm = np.asarray(am, np.float64), np.asarray(lm, np.float64)
    N, T, V = am.shape
    U = lm.shape[1]
    go = upstream(N) if go is None else np.asarray(go, np.float64)
    c0, c1, c2 = scales(lm_only_scale, am_only_scale)
    if c2 != 0.0 and q is None:
        q = log_unigram64(lm)
    qq = np.zeros(V) if q is None else np.asarray(q, np.float64)
    pairs = pairs64(am, lm, labels, blank, lm_only_scale, am_only_scale, q)
    costs, pg = lattice64(pairs, xn, yn, lam)
    sym = symbols(labels, U, V, blank)
    dam, dlm, dq = np.zeros_like(am), np.zeros_like(lm), np.zeros(V)
    for n in range(N):
        G = go[n] * pg[n]                                                     # (T,U,2)
        S = G[..., 0] + G[..., 1]
        P = np.exp(am[n][:, None, :] + lm[n][None, :, :] - _lse(am[n][:, None, :] + lm[n][None, :, :], -1)[..., None])
        PA = np.exp(am[n] + qq - _lse(am[n] + qq, -1)[:, None])
        PL = np.exp(lm[n] - _lse(lm[n], -1)[:, None])
        hot_a, hot_l = np.zeros((T, V)), np.zeros((U, V))
        for ch, s in ((0, np.full(U, blank, np.int64)), (1, sym[n])):
            for u in range(U):
                hot_a[:, s[u]] += G[:, u, ch]
                hot_l[u, s[u]] += G[:, u, ch].sum()
        dam[n] = (c0 + c2) * hot_a - c0 * np.einsum("tu,tuv->tv", S, P) - c2 * PA * S.sum(1)[:, None]
        dlm[n] = (c0 + c1) * hot_l - c0 * np.einsum("tu,tuv->uv", S, P) - c1 * PL * S.sum(0)[:, None]
        dq += c2 * (hot_a.sum(0) - (PA * S.sum(1)[:, None]).sum(0))
    # the path through q = log(mean_rows softmax(lm) + tiny): d q[v] / d lm[n,u,w] = p[n,u,v] ([v == w] - p[n,u,w]) / (R mean_v)
    dlm_total = dlm.copy()
    if c2 != 0.0:
        p = np.exp(lm - _lse(lm, -1)[..., None])
        a = dq / (N * U * (p.mean(axis=(0, 1)) + TINY))
        dlm_total += p * (a[None, None, :] - (p * a).sum(-1, keepdims=True))
    return dict(costs=costs, pairs=pairs, pair_grads=pg, dam=dam, dlm=dlm, dq=dq, dlm_total=dlm_total)


def brute_force_cost(pairs_n, Tn, Un):
    """-log of the summed probability of every path of one utterance's (T,U,2) pair plane, by enumeration."""
    total = []

    def walk(t, u, acc):
        if t == Tn - 1 and u == Un - 1:
            total.append(acc + pairs_n[t, u, 0])
            return
        if t < Tn - 1:
            walk(t + 1, u, acc + pairs_n[t, u, 0])
        if u < Un - 1:
            walk(t, u + 1, acc + pairs_n[t, u, 1])

    walk(0, 0, 0.0)
    total = np.array(total)
    m = total.max()
    return -(m + np.log(np.exp(total - m).sum()))


def make_case(seed, N, T, U, V, blank=0, scale=2.0, lengths=None, repeats=True):
    """Seeded inputs: am (N,T,V), lm (N,U,V) fp32 normal with the given scale, labels (N,U-1) never blank -- with runs of a
    repeated label where ``repeats`` -- and ragged lengths (full in utterance 0; ``lengths`` = (xn, yn): these)."""
    rng = np.random.RandomState(seed)
    am = (rng.randn(N, T, V) * scale).astype(np.float32)
    lm = (rng.randn(N, U, V) * scale).astype(np.float32)
    choices = np.array([v for v in range(V) if v != blank], np.int32)
    labels = choices[rng.randint(0, len(choices), size=(N, max(U - 1, 0)))].astype(np.int32)
    if repeats and U > 3:
        labels[:, 1::3] = labels[:, 0:1]                                      # the same label in many columns
    xn = np.full((N,), T, np.int32)
    yn = np.full((N,), U - 1, np.int32)
    if N > 1:
        xn[1:] = rng.randint(max(T // 2, 1), T + 1, size=N - 1)
        yn[1:] = rng.randint(U // 2, U, size=N - 1) if U > 1 else 0
    if lengths is not None:
        xn[:], yn[:] = lengths
    return am, lm, labels, xn, yn


def log_unigram32(lm):
    """The front end's batch unigram in fp32 torch (warp_rnnt_amd.simple.batch_log_unigram without the import)."""
    return (torch.softmax(lm.float(), dim=-1).mean(dim=(0, 1)) + TINY).log()


def pairs32(am, lm, labels, blank, lm_only_scale=0.0, am_only_scale=0.0, q=None):
    """The definition in plain torch in the dtype of am (fp32 on the yardstick's path), differentiable: the normaliser as
    pruned.simple_pairs forms it, log(exp(am - max) @ exp(lm - max)^T) plus the two maxima."""
    N, T, V = am.shape
    U = lm.shape[1]
    c0, c1, c2 = scales(lm_only_scale, am_only_scale)
    am_max = am.max(dim=2, keepdim=True).values
    lm_max = lm.max(dim=2, keepdim=True).values
    prod = torch.matmul((am - am_max).exp(), (lm - lm_max).exp().transpose(1, 2))
    Z = prod.clamp(min=TINY).log() + am_max + lm_max.transpose(1, 2)                                   # (N,T,U)
    lab = labels.long()
    lab = torch.where((lab >= 0) & (lab < V), lab, torch.full_like(lab, blank))
    lab = torch.cat([lab, torch.full((N, 1), blank, dtype=torch.long, device=lab.device)], dim=1)     # (N,U)
    out = []
    for s in (torch.full_like(lab, blank), lab):
        a = am.gather(2, s[:, None, :].expand(N, T, U))                                                # (N,T,U)
        l = lm.gather(2, s[:, :, None]).transpose(1, 2)                                                # (N,1,U)
        pair = c0 * (a + l - Z)
        if c1 != 0.0:
            pair = pair + c1 * (l - torch.logsumexp(lm, dim=2)[:, None, :])
        if c2 != 0.0:
            pair = pair + c2 * (a + q[s][:, None, :] - torch.logsumexp(am + q, dim=2)[:, :, None])
        out.append(pair)
    return torch.stack(out, dim=-1)


def chain32(am, lm, labels, xn, yn, blank, lm_only_scale=0.0, am_only_scale=0.0, lam=0.0, go=None, q_from_lm=True):
    """The unfused chain on the tensors' device: fp32 pairs32 -> warp_rnnt.rnnt_loss(blank=-1) -> autograd.  Returns
    dict(costs, pair_grads (unscaled), dam, dlm) -- dlm through q as well when q_from_lm -- at the upstream ``go`` (a
    tensor; default ones)."""
    import warp_rnnt
    a = am.detach().float().clone().requires_grad_(True)
    l = lm.detach().float().clone().requires_grad_(True)
    q = None
    if scales(lm_only_scale, am_only_scale)[2] != 0.0:
        q = log_unigram32(l if q_from_lm else l.detach())
    pairs = pairs32(a, l, labels, blank, lm_only_scale, am_only_scale, q).contiguous()
    costs = warp_rnnt.rnnt_loss(pairs, labels, xn, yn, blank=-1, fastemit_lambda=lam)
    g = torch.ones_like(costs) if go is None else go
    (pg,) = torch.autograd.grad(costs.sum(), pairs, retain_graph=True)
    (costs * g).sum().backward()
    return dict(costs=costs.detach(), pair_grads=pg, dam=a.grad, dlm=l.grad)
