"""The token-and-duration transducer (TDT) loss on the fused path: logits -> costs -> d/d logits.

TDT is the transducer of Xu et al. 2023 (NeMo's ``TDTLossNumba``; Parakeet-style models train with it): beside the token
the model predicts how many frames the step consumes.  Logits are ``(N,T,U,V+D)``: columns ``[0,V)`` are token logits, the
blank among them, column ``V+i`` is the logit of ``durations[i]``.  Per cell, with ``sigma >= 0``::

    tok = log_softmax(z[:V]) - sigma          dur = log_softmax(z[V:])

and the edges out of cell (t,u) of an utterance with T_n frames and U_n labels are, for d = durations[i]::

    blank, d >  0, weight tok[blank] + dur[i]:       to (t+d, u) if t+d < T_n;  to the end if t+d == T_n and u == U_n
    label, d >= 0, weight tok[labels[u]] + dur[i]:   to (t+d, u+1) if u < U_n and t+d < T_n

The cost is minus the log of the sum over all paths from (0,0) to the end.  The lattice is not the standard one -- a cell
has up to 2D-1 incoming edges from up to max(durations)+1 earlier anti-diagonals -- so the kernels are the feature's own
(csrc/tdt.hip): a producer that reads the logits once, the two sweeps, a gradient kernel, and a backward that reads the
logits once more and writes d/d logits.  The ``(N,T,U,V+D)`` log-probabilities never exist in memory.

Out of scope: NeMo's ``omega`` mix with the standard loss (add ``rnnt_loss_from_logits(logits[..., :V])`` yourself), the
gradient clamp, the forward/backward mismatch guard, the compact layout, the joint entry, and lattices of more than
1024 columns (``U > 1024`` is refused).
"""
from typing import Optional, Sequence, Tuple

import torch

from . import ops
from .fused import check_logits_inputs, finish_costs


def tdt_log_probs(logits: torch.Tensor, num_durations: int, blank: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(token_lp (..., V), duration_lp (..., D))`` of logits ``(..., V+D)``: the two log-softmaxes as defined above
    (sigma not subtracted), in plain torch on any device and dtype: for decoding and tests -- not the hot path.  A logit
    of ``-inf`` is a masked entry (log-probability ``-inf``)."""
    V = logits.shape[-1] - num_durations
    if num_durations < 1 or V < 2 or not 0 <= blank < V:
        raise ValueError(f"tdt_log_probs needs num_durations >= 1, V >= 2 and 0 <= blank < V (V={V}, "
                         f"num_durations={num_durations}, blank={blank})")
    return torch.log_softmax(logits[..., :V], dim=-1), torch.log_softmax(logits[..., V:], dim=-1)


class TDTLossFromLogits(torch.autograd.Function):

    @staticmethod
    def forward(ctx, logits, labels, frames_lengths, labels_lengths, durations, sigma, blank, fastemit_lambda):
        check_logits_inputs(logits, labels, frames_lengths, labels_lengths)
        wants_grad = ctx.needs_input_grad[0]          # (nothing requires grad: no beta sweep, no G plane)
        costs, grads = ops.tdt_loss(logits, labels, frames_lengths, labels_lengths, durations, blank, sigma,
                                    fastemit_lambda, wants_grad)
        if wants_grad:
            ctx.save_for_backward(logits, labels, grads)
        ctx.blank = blank
        ctx.num_durations = len(durations)
        return costs

    @staticmethod
    def backward(ctx, grads_output):
        logits, labels, grads = ctx.saved_tensors
        go = grads_output.reshape(-1).to(torch.float32).contiguous()
        return (ops.tdt_logits_backward(logits, labels, grads, go, ctx.num_durations, ctx.blank),) + (None,) * 7


def tdt_loss_from_logits(logits: torch.Tensor, labels: torch.Tensor, frames_lengths: torch.Tensor,
                         labels_lengths: torch.Tensor, durations: Sequence[int] = (0, 1, 2, 3, 4), sigma: float = 0.0,
                         blank: int = 0, fastemit_lambda: float = 0.0, average_frames: bool = False,
                         reduction: Optional[str] = "none") -> torch.Tensor:
    """The TDT loss of logits ``(N,T,U,V+D)`` (fp32, bf16 or fp16; ``V >= 2``, ``D = len(durations)``); labels and lengths
    as ``rnnt_loss_from_logits``.  ``durations``: distinct integers in [0, 8] in any order, 1 among them; ``blank``: any
    token index (NeMo's convention is ``V-1``); ``sigma``: the logit under-normalisation constant subtracted from every
    token log-probability; ``fastemit_lambda`` scales the label edges' gradients and leaves the costs alone.  Costs are
    fp32 at every dtype, d/d logits comes in the logits' dtype.  Enqueue-only: the call can be captured into a graph.
    When nothing requires grad, neither the beta sweep nor the gradient kernel runs.  Not part of it: NeMo's ``omega``
    mix, a gradient clamp, the mismatch guard, the compact layout, the joint entry, ``U > 1024``."""
    assert reduction is None or reduction in ("none", "mean", "sum")
    assert isinstance(blank, int)
    costs = TDTLossFromLogits.apply(logits, labels, frames_lengths, labels_lengths, tuple(durations), float(sigma), blank,
                                    float(fastemit_lambda))
    return finish_costs(costs, frames_lengths, average_frames, reduction)


def tdt_align(logits: torch.Tensor, labels: torch.Tensor, frames_lengths: torch.Tensor, labels_lengths: torch.Tensor,
              durations: Sequence[int] = (0, 1, 2, 3, 4), sigma: float = 0.0,
              blank: int = 0) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The best path of every utterance through the TDT lattice: ``(scores, emit_frames, emit_durations)``.

    The loss sums over every path; this asks the same lattice -- same logits, ``durations``, ``sigma`` and ``blank`` as
    :func:`tdt_loss_from_logits`, same producer -- for its single best one (csrc/tdt_align.hip: a max-plus sweep that
    records one decision byte per cell, and a trace).  All arithmetic is fp32, one add for an edge's weight
    ``tok[.] + dur[i]``, one for ``v(source) + weight``, one compare; of equal candidates the earlier one in the order
    ``i = 0..D-1``, blank before label, is kept.

    ``scores`` (N,) fp32 is the log-probability of the best path, ``-inf`` where the lattice has none (``T_n <= U_n``
    without a duration 0, masked logits).  ``emit_frames`` (N,U-1) int32 holds the frame ``t`` at which label ``u`` is
    emitted and ``emit_durations`` (N,U-1) int32 the duration ``d`` emitted with it -- the label edge
    ``(t,u) -> (t+d,u+1)`` of the path.  ``emit_frames + emit_durations`` is the frame the token ends on: it is ``<=``
    the next token's emit frame and ``< T_n``.  Both rows hold -1 in the columns from ``labels_lengths[n]`` on, and
    throughout for an utterance without a path.  An utterance whose lengths are outside ``[1,T]`` x ``[0,U-1]`` gets a
    NaN score and -1 rows.  Token timestamps, alignment-restricted training masks, emission-delay statistics (what
    ``fastemit_lambda`` and ``sigma`` are tuned against) and the diagnostic ``score + cost <= 0`` come from here.

    Results are detached and computed under ``no_grad``.  Enqueue-only: the call can be captured into a graph.
    ``U > 1024`` is refused."""
    assert isinstance(blank, int)
    with torch.no_grad():
        logits = logits.detach()
        check_logits_inputs(logits, labels, frames_lengths, labels_lengths)
        return ops.tdt_align(logits, labels, frames_lengths, labels_lengths, tuple(durations), blank, float(sigma))


class TDTLoss(torch.nn.Module):
    """:func:`tdt_loss_from_logits` as a module: stores ``durations``, ``sigma``, ``blank``, ``fastemit_lambda`` and
    ``reduction``."""

    def __init__(self, durations: Sequence[int] = (0, 1, 2, 3, 4), sigma: float = 0.0, blank: int = 0,
                 fastemit_lambda: float = 0.0, reduction: Optional[str] = "mean"):
        super().__init__()
        self.durations = tuple(durations)
        self.sigma = sigma
        self.blank = blank
        self.fastemit_lambda = fastemit_lambda
        self.reduction = reduction

    def forward(self, logits, labels, frames_lengths, labels_lengths):
        return tdt_loss_from_logits(logits, labels, frames_lengths, labels_lengths, durations=self.durations,
                                    sigma=self.sigma, blank=self.blank, fastemit_lambda=self.fastemit_lambda,
                                    reduction=self.reduction)
