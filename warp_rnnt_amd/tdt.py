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

:func:`tdt_loss_from_joint` takes the joint network's inputs instead of its logits -- ``z = W act(f_t + g_u) + b`` is
formed tile by tile inside the kernels (csrc/tdt_joint.hip, include/warp_rnnt_amd_tdt_joint.h), so the ``(N,T,U,V+D)``
logits and their gradient, the largest tensors of a TDT training step, never exist either.

Out of scope: NeMo's ``omega`` mix with the standard loss (add ``rnnt_loss_from_logits(logits[..., :V])`` yourself), the
gradient clamp, the forward/backward mismatch guard, the compact layout, a joint entry for :func:`tdt_align`, and lattices
of more than 1024 columns (``U > 1024`` is refused).
"""
import math
from typing import Optional, Sequence, Tuple

import torch

from . import ops
from .fused import check_logits_inputs, finish_costs
from .joint import _aligned, check_dropout, check_joint_inputs, resolve_dropout_seed


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
    mix, a gradient clamp, the mismatch guard, the compact layout, ``U > 1024``; the joint network in front of the
    logits is :func:`tdt_loss_from_joint`."""
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


class TDTLossFromJoint(torch.autograd.Function):

    @staticmethod
    def forward(ctx, f, g, weight, bias, labels, frames_lengths, labels_lengths, durations, sigma, blank, activation,
                fastemit_lambda, with_grads, dropout, seed):
        fc, gc = _aligned(f), _aligned(g)
        w = _aligned(weight.to(fc.dtype))                        # W staged in the activations' dtype
        b = bias.to(torch.float32).contiguous() if bias is not None else None
        labels, xn, yn = labels.contiguous(), frames_lengths.contiguous(), labels_lengths.contiguous()
        costs, stats, grads = ops.tdt_joint_loss(fc, gc, w, b, labels, xn, yn, durations, activation, blank, sigma,
                                                 fastemit_lambda, with_grads, dropout, seed)
        if with_grads:
            ctx.save_for_backward(fc, gc, w, b, labels, xn, yn, stats, grads, seed)   # (the backward reads the same word)
        ctx.activation, ctx.blank, ctx.dropout, ctx.num_durations = activation, blank, dropout, len(durations)
        ctx.weight_dtype = weight.dtype
        ctx.bias_dtype = bias.dtype if bias is not None else None
        return costs

    @staticmethod
    def backward(ctx, grads_output):
        f, g, w, b, labels, xn, yn, stats, grads, seed = ctx.saved_tensors
        go = grads_output.reshape(-1).to(torch.float32).contiguous()
        need = ctx.needs_input_grad
        df, dg, dw, db = ops.tdt_joint_backward(f, g, w, b, labels, xn, yn, stats, grads, go, ctx.num_durations,
                                                ctx.activation, ctx.blank, need[0], need[1], need[2],
                                                need[3] and b is not None, ctx.dropout, seed)
        if dw is not None:
            dw = dw.to(ctx.weight_dtype)
        if db is not None:
            db = db.to(ctx.bias_dtype)
        return (df, dg, dw, db) + (None,) * 11


def tdt_loss_from_joint(f: torch.Tensor, g: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor],
                        labels: torch.Tensor, frames_lengths: torch.Tensor, labels_lengths: torch.Tensor,
                        durations: Sequence[int] = (0, 1, 2, 3, 4), sigma: float = 0.0, blank: int = 0,
                        activation: str = "tanh", fastemit_lambda: float = 0.0, average_frames: bool = False,
                        reduction: Optional[str] = "none", *, dropout: float = 0.0, training: bool = True,
                        dropout_seed: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The value of ``tdt_loss_from_logits(z, labels, frames_lengths, labels_lengths, durations, sigma, blank, ...)`` with
    ``z[n,t,u] = weight @ act(f[n,t] + g[n,u]) + bias`` -- f (N,T,H), g (N,U+1,H), weight (V+D,H) (``nn.Linear.weight``:
    rows ``[0,V)`` the tokens, row ``V+i`` ``durations[i]``, NeMo's joint output order), bias (V+D,) or None, act
    ``"tanh"`` or ``"relu"`` -- and gradients to f, g, weight and bias, without materialising an (N,T,U+1,H) or
    (N,T,U+1,V+D) tensor.

    f and g share one dtype (fp32, bf16 or fp16); weight and bias may be fp32 or that dtype and are staged in the
    activations' dtype; their gradients come back in their own dtype, d f and d g in the activations'.  Costs are fp32.
    Supported: H % 32 == 0, 32 <= H <= 1024, V >= 2, ``blank < V``, up to 1024 lattice columns.  Enqueue-only: the call can
    be captured into a graph.  When nothing requires grad, no beta sweep runs and neither the G plane nor the per-cell
    statistics are produced; only the gradients that are needed are computed.  Saved for the backward: the inputs, 16 B of
    statistics and ``4 (2 + D)`` B of the G plane per lattice cell.

    ``dropout``, ``training``, ``dropout_seed``: Dropout(p) between the activation and the projection inside the kernels,
    exactly as :func:`warp_rnnt_amd.joint.rnnt_loss_from_joint` defines it (same mask, same rules under graph capture).
    Not part of it: NeMo's ``omega`` mix, a gradient clamp, the compact layout, ``U > 1024``."""
    p = check_dropout(dropout)
    if not training:
        p = 0.0
    assert reduction is None or reduction in ("none", "mean", "sum")
    assert isinstance(blank, int)
    durations = tuple(durations)
    if isinstance(weight, torch.Tensor) and weight.dim() == 2:       # (what depends on values first, with its reasons;
        ops._tdt_check(weight.size(0) - len(durations), len(durations), blank, durations, float(sigma))  # a weight of
    check_joint_inputs(f, g, weight, bias, labels, frames_lengths, labels_lengths, activation, blank)   # another form: here)
    with_grads = torch.is_grad_enabled() and any(x is not None and x.requires_grad for x in (f, g, weight, bias))
    seed = None
    if p > 0:
        seed = resolve_dropout_seed(dropout_seed, f.device, torch.cuda.is_current_stream_capturing())
    costs = TDTLossFromJoint.apply(f, g, weight, bias, labels, frames_lengths, labels_lengths, durations, float(sigma),
                                   blank, activation, float(fastemit_lambda), with_grads, p, seed)
    return finish_costs(costs, frames_lengths, average_frames, reduction)


class TDTJointLoss(torch.nn.Module):
    """The joint's projection and the TDT loss as one module -- ``activation -> Dropout(dropout) -> Linear(hidden,
    vocab + D) -> loss`` on :func:`tdt_loss_from_joint`: it owns ``weight`` (vocab + D, hidden) and ``bias``, initialised
    as ``nn.Linear`` initialises them; ``self.training`` switches the dropout (``.eval()`` is the call without)."""

    def __init__(self, hidden: int, vocab: int, durations: Sequence[int] = (0, 1, 2, 3, 4), sigma: float = 0.0,
                 blank: int = 0, activation: str = "tanh", dropout: float = 0.0, bias: bool = True,
                 fastemit_lambda: float = 0.0, average_frames: bool = False, reduction: Optional[str] = "mean"):
        super().__init__()
        if activation not in ops.ACTIVATIONS:
            raise ValueError(f"activation must be one of {tuple(ops.ACTIVATIONS)}, not {activation!r}")
        self.hidden, self.vocab, self.durations = hidden, vocab, tuple(durations)
        self.sigma, self.blank, self.activation, self.dropout = sigma, blank, activation, check_dropout(dropout)
        self.fastemit_lambda, self.average_frames, self.reduction = fastemit_lambda, average_frames, reduction
        rows = vocab + len(self.durations)
        self.weight = torch.nn.Parameter(torch.empty(rows, hidden))
        self.bias = torch.nn.Parameter(torch.empty(rows)) if bias else None
        self.reset_parameters()

    def reset_parameters(self):
        torch.nn.init.kaiming_uniform_(self.weight, a=math.sqrt(5))      # (nn.Linear.reset_parameters)
        if self.bias is not None:
            bound = 1 / math.sqrt(self.hidden) if self.hidden > 0 else 0
            torch.nn.init.uniform_(self.bias, -bound, bound)

    def forward(self, f, g, labels, frames_lengths, labels_lengths, dropout_seed=None):
        return tdt_loss_from_joint(f, g, self.weight, self.bias, labels, frames_lengths, labels_lengths,
                                   durations=self.durations, sigma=self.sigma, blank=self.blank,
                                   activation=self.activation, fastemit_lambda=self.fastemit_lambda,
                                   average_frames=self.average_frames, reduction=self.reduction, dropout=self.dropout,
                                   training=self.training, dropout_seed=dropout_seed)

    def extra_repr(self):
        return (f"hidden={self.hidden}, vocab={self.vocab}, durations={self.durations}, sigma={self.sigma}, "
                f"activation={self.activation!r}, dropout={self.dropout}, bias={self.bias is not None}, "
                f"blank={self.blank}, reduction={self.reduction!r}")
