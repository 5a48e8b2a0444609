"""The multi-blank transducer loss on the fused path: logits -> costs -> d/d logits.

The multi-blank transducer is the one of Xu et al. 2022, "Multi-blank Transducers for Speech Recognition" (NeMo's
``MultiblankRNNTLossNumba``), TDT's predecessor: beside the standard blank the vocabulary holds "big blanks" that consume
2, 4, 8 ... frames at once.  Logits are ``(N,T,U,V)`` with one softmax over all ``V`` columns.  Per cell, with
``sigma >= 0``::

    lp = log_softmax(z) - sigma

and the edges out of cell (t,u) of an utterance with T_n frames and U_n labels are, for the B blanks (the standard one,
duration 1, among them)::

    blank i, d = duration of blank i, weight lp[blank_ids[i]]:  to (t+d, u) if t+d < T_n;  to the end if t+d == T_n and u == U_n
    label,                            weight lp[labels[u]]:     to (t, u+1) if u < U_n

This is NeMo's lattice: a big blank reaches the end only when it lands exactly on T_n.  The cost is minus the log of the
sum over all paths from (0,0) to the end; with no big blanks it is the standard loss plus ``sigma (T_n + U_n)``.  The
lattice is neither the standard one nor TDT's, so the kernels are the feature's own (csrc/multiblank.hip): a producer that
reads the logits once, the two sweeps, a gradient kernel, and a backward that reads the logits once more and writes
d/d logits.  The ``(N,T,U,V)`` log-probabilities never exist in memory.

Out of scope: the compact layout, a joint entry (the joint network fused in front), an align entry (best paths), a
gradient clamp, the forward/backward mismatch guard, and lattices of more than 1024 columns (``U > 1024`` is refused).
"""
from typing import Optional, Sequence

import torch

from . import ops
from .fused import check_logits_inputs, finish_costs


def blank_set(blank: int, big_blank_durations: Sequence[int], big_blank_ids: Optional[Sequence[int]] = None):
    """``(ids, durations)`` as the C entry takes them: the standard blank with duration 1 is entry 0, the big blanks
    follow in the order given.  ``big_blank_ids=None``: NeMo's kernel convention, ``blank - 1 - i`` for big blank ``i``
    (meant for ``blank = V - 1``)."""
    durations = tuple(int(d) for d in big_blank_durations)
    if big_blank_ids is None:
        big_blank_ids = tuple(blank - 1 - i for i in range(len(durations)))
    big_blank_ids = tuple(int(v) for v in big_blank_ids)
    if len(big_blank_ids) != len(durations):
        raise ValueError(f"big_blank_ids must name one id per big-blank duration (ids={big_blank_ids}, "
                         f"durations={durations})")
    return (blank,) + big_blank_ids, (1,) + durations


class MultiblankLossFromLogits(torch.autograd.Function):

    @staticmethod
    def forward(ctx, logits, labels, frames_lengths, labels_lengths, ids, durations, sigma, fastemit_lambda, wants_grad):
        check_logits_inputs(logits, labels, frames_lengths, labels_lengths)
        costs, grads = ops.multiblank_loss(logits, labels, frames_lengths, labels_lengths, ids, durations, sigma,
                                           fastemit_lambda, wants_grad)
        if wants_grad:
            ctx.save_for_backward(logits, labels, grads)
        ctx.ids = ids
        return costs

    @staticmethod
    def backward(ctx, grads_output):
        logits, labels, grads = ctx.saved_tensors
        go = grads_output.reshape(-1).to(torch.float32).contiguous()
        return (ops.multiblank_logits_backward(logits, labels, grads, go, ctx.ids),) + (None,) * 8


def multiblank_loss_from_logits(logits: torch.Tensor, labels: torch.Tensor, frames_lengths: torch.Tensor,
                                labels_lengths: torch.Tensor, big_blank_durations: Sequence[int] = (2, 4, 8),
                                sigma: float = 0.0, blank: int = 0, big_blank_ids: Optional[Sequence[int]] = None,
                                fastemit_lambda: float = 0.0, average_frames: bool = False,
                                reduction: Optional[str] = "none") -> torch.Tensor:
    """The multi-blank loss of logits ``(N,T,U,V)`` (fp32, bf16 or fp16); labels and lengths as ``rnnt_loss_from_logits``.
    ``blank`` is the standard blank (one frame); ``big_blank_durations``: distinct integers in [2, 8] in any order, at
    most seven; ``big_blank_ids``: the vocabulary index of each big blank -- ``None`` means NeMo's kernel convention,
    ``blank - 1 - i``, which is meant for ``blank = V - 1``.  All ids are distinct and lie in ``[0, V)``: one outside is
    refused with its reason before anything touches the device.  ``sigma``: the logit under-normalisation constant
    subtracted from every log-probability; ``fastemit_lambda`` scales the label edges' gradients and leaves the costs
    alone.  Costs are fp32 at every dtype, d/d logits comes in the logits' dtype.  Enqueue-only: the call can be captured
    into a graph.  When nothing requires grad, neither the beta sweep nor the gradient kernel runs.  Not part of it: the
    compact layout, a joint entry, an align entry, a gradient clamp, the mismatch guard, ``U > 1024``."""
    assert reduction is None or reduction in ("none", "mean", "sum")
    assert isinstance(blank, int)
    ids, durations = blank_set(blank, big_blank_durations, big_blank_ids)
    if isinstance(logits, torch.Tensor) and logits.dim() == 4:         # (what depends on values first, with its reasons)
        ops._multiblank_check(logits.size(3), ids, durations, float(sigma))
    # (nothing requires grad, or no_grad: no beta sweep, no G plane -- asked here, where the caller's grad mode is visible)
    wants_grad = torch.is_grad_enabled() and isinstance(logits, torch.Tensor) and logits.requires_grad
    costs = MultiblankLossFromLogits.apply(logits, labels, frames_lengths, labels_lengths, ids, durations, float(sigma),
                                           float(fastemit_lambda), wants_grad)
    return finish_costs(costs, frames_lengths, average_frames, reduction)


class MultiblankLoss(torch.nn.Module):
    """:func:`multiblank_loss_from_logits` as a module: stores ``big_blank_durations``, ``sigma``, ``blank``,
    ``big_blank_ids``, ``fastemit_lambda`` and ``reduction``."""

    def __init__(self, big_blank_durations: Sequence[int] = (2, 4, 8), sigma: float = 0.0, blank: int = 0,
                 big_blank_ids: Optional[Sequence[int]] = None, fastemit_lambda: float = 0.0,
                 reduction: Optional[str] = "mean"):
        super().__init__()
        self.big_blank_durations = tuple(big_blank_durations)
        self.sigma = sigma
        self.blank = blank
        self.big_blank_ids = None if big_blank_ids is None else tuple(big_blank_ids)
        self.fastemit_lambda = fastemit_lambda
        self.reduction = reduction

    def forward(self, logits, labels, frames_lengths, labels_lengths):
        return multiblank_loss_from_logits(logits, labels, frames_lengths, labels_lengths,
                                           big_blank_durations=self.big_blank_durations, sigma=self.sigma,
                                           blank=self.blank, big_blank_ids=self.big_blank_ids,
                                           fastemit_lambda=self.fastemit_lambda, reduction=self.reduction)
