"""Fused logits -> RNN-T loss (additive API).

The reference's callers compute ``rnnt_loss(F.log_softmax(logits, -1), ..., gather=True)``
(pytorch_binding/benchmark.py:65-70): the dense (N,T,U,V) log-probabilities are written and re-read in
forward, and backward materialises a dense gradient w.r.t. them before the log-softmax backward
turns it into a gradient w.r.t. the logits -- about 28V bytes of HBM traffic per lattice cell.
Here forward reads the logits once (log-softmax + gather fused, 4V+8 B/cell) and backward reads them
once more and writes d(logits) (8V B/cell); log-probabilities never exist in HBM.

The logits may be fp32, bf16 or fp16 (what a joint network under ``torch.autocast`` produces): half-precision logits are
converted to fp32 as the kernels load them, so the costs (fp32 at every dtype) are bit-equal to those of ``logits.float()``
and d(logits) comes back in the logits' dtype, the fp32 result rounded once -- at half the bytes (2V+8 / 4V+8 B/cell).
"""
from typing import Optional

import torch

from . import _mismatch, ops
from warp_rnnt import _C as _core


def check_logits_inputs(xs, ys, xn, yn):
    """The reference's checks, in its order and with its texts (binding.cpp:32-51, warp_rnnt._C.check_inputs) -- except
    that the logits may be fp32, bf16 or fp16.  (Without ``xs_dtypes`` check_inputs keeps asking for a Float tensor: the
    reference-shaped op takes fp32 log-probs only.)"""
    _core.check_inputs(xs, ys, xn, yn, xs_dtypes=tuple(ops.LOGITS_DTYPES))


def finish_costs(costs, frames_lengths, average_frames, reduction):
    """The tail of every ``*_loss_from_*`` function: the per-utterance costs divided by the frame counts where
    ``average_frames`` asks for it, then ``reduction`` ("none" / None, "sum", "mean")."""
    if average_frames:
        costs = costs / frames_lengths.to(costs)      # (fp32 costs: T_n rounded to bf16 would be 1499 -> 1496)
    if reduction == "none" or reduction is None:
        return costs
    if reduction == "sum":
        return costs.sum()
    return costs.mean()


class RNNTLossFromLogits(torch.autograd.Function):

    @staticmethod
    def forward(ctx, logits, labels, frames_lengths, labels_lengths, blank=0, fastemit_lambda=0.0, clamp=0.0):
        check_logits_inputs(logits, labels, frames_lengths, labels_lengths)
        costs, grads = ops.loss(logits, labels, frames_lengths, labels_lengths, ops.IN_LOGITS_DENSE,
                                ops.GRADS_GATHERED_DIAGONAL, blank, fastemit_lambda)
        ctx.save_for_backward(logits, labels, grads)
        ctx.blank = blank
        ctx.clamp = clamp
        return costs

    @staticmethod
    def backward(ctx, grads_output):
        logits, labels, grads = ctx.saved_tensors
        go = grads_output.reshape(-1).to(torch.float32).contiguous()
        return (ops.logits_backward(logits, labels, grads, go, ctx.blank, clamp=ctx.clamp),) + (None,) * 6


def check_compact_logits_inputs(xs, ys, xn, yn):
    """The checks of ``rnnt_loss(compact=True)`` (warp_rnnt._C.rnnt_loss_compact), in its order and with its texts --
    except that the logits may be fp32, bf16 or fp16."""
    for x, name in ((xs, "xs"), (ys, "ys"), (xn, "xn"), (yn, "yn")):
        _core._check_contiguous(x, name)
    if xs.dtype not in ops.LOGITS_DTYPES:
        raise RuntimeError(f"xs (logits) must be a float32, bfloat16 or float16 tensor, not {xs.dtype}")
    for x, name in ((ys, "ys"), (xn, "xn"), (yn, "yn")):
        _core._check_int(x, name)
    for x, name in ((xs, "xs"), (ys, "ys"), (xn, "xn"), (yn, "yn")):
        _core._check_cuda(x, name)
    if xs.dim() != 2:
        raise RuntimeError("xs must have 2 dimensions")
    if xn.size(0) != yn.size(0):
        raise RuntimeError("xn and yn shape must be equal (N,)")


class RNNTLossCompactFromLogits(torch.autograd.Function):
    """Packed logits (sum_n T_n*(U_n+1), V) -> costs; backward writes d/d logits in the logits' dtype, out of place."""

    @staticmethod
    def forward(ctx, logits, labels, frames_lengths, labels_lengths, blank=0, fastemit_lambda=0.0,
                enable_grad: bool = True, max_frames=None, max_labels=None, clamp=0.0):
        costs, grads, offs, loffs = ops.loss_compact_logits(logits, labels, frames_lengths, labels_lengths, blank,
                                                            fastemit_lambda, enable_grad, max_frames, max_labels)
        if enable_grad:
            ctx.save_for_backward(logits, labels, frames_lengths, labels_lengths, offs, loffs, grads)
        ctx.blank = blank
        ctx.clamp = clamp
        return costs

    @staticmethod
    def backward(ctx, grads_output):
        logits, labels, xn, yn, offs, loffs, grads = ctx.saved_tensors
        _mismatch.poll(grads.device)
        go = grads_output.reshape(-1).to(torch.float32).contiguous()
        dlogits = ops.compact_logits_backward(logits, labels, xn, yn, offs, loffs, grads, go, ctx.blank, clamp=ctx.clamp)
        return (dlogits,) + (None,) * 9


def rnnt_loss_from_logits(logits: torch.Tensor, labels: torch.Tensor, frames_lengths: torch.Tensor,
                          labels_lengths: torch.Tensor, average_frames: bool = False,
                          reduction: Optional[str] = "none", blank: int = 0,
                          fastemit_lambda: float = 0.0, compact: bool = False,
                          max_frames: Optional[int] = None, max_labels: Optional[int] = None,
                          clamp: float = 0.0) -> torch.Tensor:
    """Same value and gradients as ``warp_rnnt.rnnt_loss(F.log_softmax(logits, -1), ..., gather=True)``
    (arguments as there), without materialising the log-probabilities.

    ``compact=True``: the ragged packed layout of ``rnnt_loss(compact=True)`` -- logits ``(sum_n T_n*(U_n+1), V)``,
    labels ``(sum_n U_n,)`` -- with that call's checks and ``max_frames`` / ``max_labels`` (launch bounds: no host
    synchronisation, capturable; a batch that does not fit comes back with NaN costs and zero gradients).  Without them
    one host synchronisation.  The log-probabilities and their (STU,V) gradient never exist.

    ``clamp`` > 0: the gradient clamp of torchaudio's and warp-transducer's rnnt_loss -- d/d logits of every utterance's
    cost are limited to [-clamp, +clamp] elementwise and only then multiplied by the upstream gradient (which carries the
    ``reduction`` and ``average_frames``).  It sits inside the backward kernel (the unscaled gradient never exists in
    memory); the costs do not depend on it.  0.0: no clamp, the kernels and bits there have always been."""
    assert reduction is None or reduction in ("none", "mean", "sum")
    assert isinstance(blank, int)
    clamp = float(clamp)
    if not 0.0 <= clamp < float("inf"):
        raise ValueError(f"clamp must be a finite number >= 0 (0 = off), not {clamp}")
    if not compact and (max_frames is not None or max_labels is not None):
        raise ValueError("max_frames / max_labels are launch bounds of the compact layout: pass compact=True with them")
    if compact:
        check_compact_logits_inputs(logits, labels, frames_lengths, labels_lengths)
        wants_grad = logits.requires_grad and torch.is_grad_enabled()
        costs = RNNTLossCompactFromLogits.apply(logits, labels, frames_lengths, labels_lengths, blank, fastemit_lambda,
                                                wants_grad, max_frames, max_labels, clamp)
    else:
        costs = RNNTLossFromLogits.apply(logits, labels, frames_lengths, labels_lengths, blank, fastemit_lambda, clamp)
    return finish_costs(costs, frames_lengths, average_frames, reduction)
