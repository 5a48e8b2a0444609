"""The factorised-blank (HAT) transducer loss on the fused path: logits -> costs -> d/d logits.

HAT is the Hybrid Autoregressive Transducer of Variani et al. 2020.  The blank probability of a lattice cell is a
Bernoulli, ``sigmoid(z[blank])``; the labels share ``1 - sigmoid(z[blank])`` through a softmax over the non-blank logits
only.  With ``b = blank`` and ``sp(x) = max(x,0) + log1p(exp(-|x|))``::

    lpB   = -sp(-z_b)                        log sigmoid(z_b)
    lnb   = -sp( z_b)                        log(1 - sigmoid(z_b))
    m     = max_{v != b} z_v ,  s = sum_{v != b} exp(z_v - m)
    lp[v] = ((z_v - m) - log s) + lnb        v != b

The loss is the ordinary transducer lattice over these log-probabilities -- the sweeps and the gradient kernel of
``rnnt_loss_from_logits`` -- between two streaming kernels of its own (csrc/hat.hip), so the (N,T,U,V) log-probabilities
never exist in memory: the forward reads the logits once, the backward reads them once more and writes d/d logits.

In exact arithmetic HAT on ``z`` is the standard loss on ``z'``, ``z'_v = z_v`` for ``v != b`` and
``z'_b = z_b + log sum_{v != b} exp z_v``.
"""
from typing import Optional

import torch

from . import ops
from .fused import check_logits_inputs, finish_costs


def _softplus(x):
    """max(x,0) + log1p(exp(-|x|)): exact to rounding at every x (torch's softplus goes linear above its threshold)."""
    return x.clamp(min=0) + torch.log1p(torch.exp(-x.abs()))


def hat_log_probs(logits: torch.Tensor, blank: int = 0) -> torch.Tensor:
    """The dense ``(..., V)`` HAT log-probabilities as defined above, in plain torch on any device and dtype (the stable
    softplus form): for decoding, internal-LM scoring and tests -- not the hot path.  A non-blank logit of ``-inf`` is a
    masked entry (log-probability ``-inf``); a row needs one finite non-blank logit."""
    V = logits.shape[-1]
    if V < 2 or not 0 <= blank < V:
        raise ValueError(f"hat_log_probs needs V >= 2 and 0 <= blank < V (V={V}, blank={blank})")
    zb = logits[..., blank]
    keep = torch.arange(V, device=logits.device) != blank
    rest = logits[..., keep]
    m = rest.max(dim=-1, keepdim=True).values
    d = rest - m
    lnb = -_softplus(zb)
    out = torch.empty_like(logits)
    out[..., keep] = (d - d.exp().sum(dim=-1, keepdim=True).log()) + lnb.unsqueeze(-1)
    out[..., blank] = -_softplus(-zb)
    return out


class HATLossFromLogits(torch.autograd.Function):

    @staticmethod
    def forward(ctx, logits, labels, frames_lengths, labels_lengths, blank=0, fastemit_lambda=0.0):
        check_logits_inputs(logits, labels, frames_lengths, labels_lengths)
        V = logits.shape[-1]
        if V < 2 or not 0 <= blank < V:
            raise RuntimeError(f"rnnt_loss status 5 (RNNT_STATUS_INVALID_ARGUMENT): the HAT loss needs V >= 2 and a "
                               f"blank that is a vocabulary index (V={V}, blank={blank})")
        wants_grad = ctx.needs_input_grad[0]          # (nothing requires grad: no pairs are produced or kept)
        costs, grads = ops.hat_loss(logits, labels, frames_lengths, labels_lengths, blank, fastemit_lambda, wants_grad)
        if wants_grad:
            ctx.save_for_backward(logits, labels, grads)
        ctx.blank = blank
        return costs

    @staticmethod
    def backward(ctx, grads_output):
        logits, labels, grads = ctx.saved_tensors
        go = grads_output.reshape(-1).to(torch.float32).contiguous()
        return (ops.hat_logits_backward(logits, labels, grads, go, ctx.blank),) + (None,) * 5


def hat_loss_from_logits(logits: torch.Tensor, labels: torch.Tensor, frames_lengths: torch.Tensor,
                         labels_lengths: torch.Tensor, average_frames: bool = False,
                         reduction: Optional[str] = "none", blank: int = 0,
                         fastemit_lambda: float = 0.0) -> torch.Tensor:
    """The HAT loss of logits ``(N,T,U,V)`` (fp32, bf16 or fp16; ``V >= 2``), arguments as ``rnnt_loss_from_logits``:
    the value and gradients of ``warp_rnnt.rnnt_loss(hat_log_probs(logits, blank), ..., gather=False)`` without the
    log-probabilities in memory.  Costs are fp32 at every dtype, d/d logits comes in the logits' dtype.  Enqueue-only:
    the call can be captured into a graph."""
    assert reduction is None or reduction in ("none", "mean", "sum")
    assert isinstance(blank, int)
    costs = HATLossFromLogits.apply(logits, labels, frames_lengths, labels_lengths, blank, fastemit_lambda)
    return finish_costs(costs, frames_lengths, average_frames, reduction)


class HATLoss(torch.nn.Module):
    """:func:`hat_loss_from_logits` as a module: stores ``blank``, ``fastemit_lambda`` and ``reduction``."""

    def __init__(self, blank: int = 0, fastemit_lambda: float = 0.0, reduction: Optional[str] = "mean"):
        super().__init__()
        self.blank = blank
        self.fastemit_lambda = fastemit_lambda
        self.reduction = reduction

    def forward(self, logits, labels, frames_lengths, labels_lengths):
        return hat_loss_from_logits(logits, labels, frames_lengths, labels_lengths, reduction=self.reduction,
                                    blank=self.blank, fastemit_lambda=self.fastemit_lambda)
