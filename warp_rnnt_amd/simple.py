"""The "simple" transducer loss on the fused path: ``am`` ``(N,T,V)``, ``lm`` ``(N,U,V)`` -> costs -> d/d am, d/d lm.

This is the first pass of the pruned recipe of Kuang et al. 2022 -- in exact arithmetic k2's ``rnnt_loss_smoothed(lm, am,
symbols, termination_symbol=blank, lm_only_scale, am_only_scale, boundary)`` with the regular topology, what the icefall /
Zipformer recipes add to their objective as ``simple_loss_scale * simple_loss`` (with ``lm_only_scale=0.25``).  The joiner
is trivial, ``am[n,t,:] + lm[n,u,:]``, and the loss is smoothed towards the two marginal models.  With ``c1 =
lm_only_scale``, ``c2 = am_only_scale``, ``c0 = 1 - c1 - c2``, ``b = blank`` and ``q`` the log of the batch's unigram
(:func:`batch_log_unigram`; only with ``c2 != 0``)::

    sym(u,0) = b,   sym(u,1) = labels[n,u] for u < U-1 and a label inside [0,V), else b
    Z(t,u) = log sum_v exp(am[t,v] + lm[u,v]),   ZL(u) = log sum_v exp(lm[u,v]),   ZA(t) = log sum_v exp(am[t,v] + q[v])
    pair(t,u,c) = c0 (am[t,s] + lm[u,s] - Z(t,u)) + c1 (lm[u,s] - ZL(u)) + c2 (am[t,s] + q[s] - ZA(t)),   s = sym(u,c)

and the cost is the standard transducer cost of that ``(T,U,2)`` pair plane: ``warp_rnnt.rnnt_loss(pairs, ..., blank=-1)``
on ``pruned.simple_pairs(am, lm, labels, blank)`` when both scales are 0.  No ``(N,T,U,V)`` tensor exists, and no
``exp(am)``, ``exp(lm)`` or ``(N,T,U,2)`` pair tensor either: the normaliser is an exact-fp32 MFMA GEMM per utterance whose
epilogue writes the pairs where the lattice sweeps read them, and the backward is two more such GEMMs (csrc/simple.hip,
DESIGN.md 3.18).  The forward already holds the gradient pairs -- minus the edge occupancies that
:func:`warp_rnnt_amd.pruned.prune_ranges` reads -- and hands them back with ``return_grad=True``.

``am`` and ``lm`` are finite: a ``-inf`` entry is not a masked entry here.  ``rnnt_type="modified"`` and
``delay_penalty`` are those of :func:`warp_rnnt_amd.pruned.pruned_rnnt_loss_from_logits`; the two passes
of the recipe take the same values.  Out of scope: k2's ``constrained`` topology, the compact layout, the gradient clamp.
"""
from typing import Optional

import torch

from . import ops
from .fused import finish_costs
from .pruned import NO_PATH_COST
from warp_rnnt import _C as _core

TINY = torch.finfo(torch.float32).tiny


def check_simple_inputs(am, lm, labels, xn, yn):
    """The checks of the logits entries (warp_rnnt._C.check_inputs: its order, its texts, as
    ``pruned.check_pruned_inputs`` has them) for the two inputs of the trivial joiner."""
    for x, name in ((am, "am"), (lm, "lm"), (labels, "ys"), (xn, "xn"), (yn, "yn")):
        _core._check_contiguous(x, name)
    if am.dtype not in ops.LOGITS_DTYPES:
        raise RuntimeError(f"am must be a float32, bfloat16 or float16 tensor, not {am.dtype}")
    if lm.dtype != am.dtype:
        raise RuntimeError(f"lm must have the dtype of am ({am.dtype}), not {lm.dtype}")
    for x, name in ((labels, "ys"), (xn, "xn"), (yn, "yn")):
        _core._check_int(x, name)
    for x, name in ((am, "am"), (lm, "lm"), (labels, "ys"), (xn, "xn"), (yn, "yn")):
        _core._check_cuda(x, name)
    if am.dim() != 3:
        raise RuntimeError("am must have 3 dimensions")
    if lm.dim() != 3:
        raise RuntimeError("lm must have 3 dimensions")
    N, T, V = am.shape
    if lm.size(0) != N or lm.size(2) != V:
        raise RuntimeError(f"lm shape (N, U, V) mismatched with am (N, T, V) = {tuple(am.shape)}")
    if xn.numel() != N:
        raise RuntimeError("xn shape must be equal (N,)")
    if yn.numel() != N:
        raise RuntimeError("yn shape must be equal (N,)")
    if labels.dim() != 2 or labels.size(0) != N or labels.size(1) != lm.size(1) - 1:
        raise RuntimeError("ys shape (N, U-1) mismatched with lm (N, U, V)")
    for x, name in ((lm, "lm"), (labels, "ys"), (xn, "xn"), (yn, "yn")):
        if x.device != am.device:
            raise RuntimeError(f"{name} must be on the same device as am")


def batch_log_unigram(lm: torch.Tensor) -> torch.Tensor:
    """k2's batch unigram of ``lm`` ``(N,U,V)``: ``log(mean over all (n,u) rows of softmax(lm[n,u,:]) + tiny)``, ``(V,)``
    fp32, in ordinary torch ops (fp32 arithmetic), so autograd carries its gradient back to ``lm``."""
    return (torch.softmax(lm.float(), dim=-1).mean(dim=(0, 1)) + TINY).log()


class SimpleRNNTLossFunction(torch.autograd.Function):

    @staticmethod
    def forward(ctx, am, lm, q, labels, frames_lengths, labels_lengths, blank, lm_only_scale, am_only_scale,
                fastemit_lambda, return_grad, topology=ops.RNNT_TYPES["regular"], delay_penalty=0.0):
        check_simple_inputs(am, lm, labels, frames_lengths, labels_lengths)
        wants_grad = any(ctx.needs_input_grad[:3])
        ctx.args = (blank, lm_only_scale, am_only_scale)
        # the defaults are the entries without a topology: the calls, and so the bits, of every earlier version
        ctx.plain = topology == ops.RNNT_TYPES["regular"] and delay_penalty == 0.0
        ctx.topology = topology
        if ctx.plain:
            costs, grads, znorm = ops.simple_loss(am, lm, q, labels, frames_lengths, labels_lengths, blank, lm_only_scale,
                                                  am_only_scale, fastemit_lambda, wants_grad or return_grad)
            if wants_grad:
                ctx.save_for_backward(am, lm, q, labels, frames_lengths, labels_lengths, grads, znorm)
            if not return_grad:
                return costs
            ctx.mark_non_differentiable(grads)
            return costs, grads
        costs, grads, znorm = ops.simple_loss_topology(am, lm, q, labels, frames_lengths, labels_lengths, blank,
                                                       lm_only_scale, am_only_scale, fastemit_lambda,
                                                       wants_grad or return_grad, topology, delay_penalty)
        # the modified lattice of an utterance with T_n < U_n holds no path: +inf, zero pairs, zero rows (on the device)
        no_path = costs >= NO_PATH_COST
        costs = torch.where(no_path, torch.full_like(costs, float("inf")), costs)
        if wants_grad:
            ctx.save_for_backward(am, lm, q, labels, frames_lengths, labels_lengths, grads, znorm, no_path)
        if not return_grad:
            return costs
        # by frame: the modified pairs are (N,T+1,U,2) and row T is no frame's
        pairs = torch.where(no_path[:, None, None, None], torch.zeros_like(grads), grads)[:, :am.shape[1]]
        ctx.mark_non_differentiable(pairs)
        return costs, pairs

    @staticmethod
    def backward(ctx, grads_output, *_):
        go = grads_output.reshape(-1).to(torch.float32)
        if ctx.plain:
            am, lm, q, labels, xn, yn, grads, znorm = ctx.saved_tensors
            dam, dlm, dq = ops.simple_backward(am, lm, q, labels, xn, yn, grads, znorm, go.contiguous(), *ctx.args)
            return (dam, dlm, dq) + (None,) * 10
        am, lm, q, labels, xn, yn, grads, znorm, no_path = ctx.saved_tensors
        go = torch.where(no_path, torch.zeros_like(go), go).contiguous()       # scale 0: exactly zero rows, pairs unread
        dam, dlm, dq = ops.simple_backward_topology(am, lm, q, labels, xn, yn, grads, znorm, go, *ctx.args, ctx.topology)
        return (dam, dlm, dq) + (None,) * 10


def simple_rnnt_loss(am: torch.Tensor, lm: torch.Tensor, labels: torch.Tensor, frames_lengths: torch.Tensor,
                     labels_lengths: torch.Tensor, blank: int = 0, lm_only_scale: float = 0.0,
                     am_only_scale: float = 0.0, fastemit_lambda: float = 0.0, average_frames: bool = False,
                     reduction: Optional[str] = "none", return_grad: bool = False):
    """The smoothed simple loss of ``am`` ``(N,T,V)`` and ``lm`` ``(N,U,V)`` (fp32, bf16 or fp16, one dtype; ``V >= 2``;
    finite), labels ``(N,U-1)`` int32 and the lengths of ``rnnt_loss_from_logits``; ``lm_only_scale, am_only_scale >= 0``
    with a sum of at most 1.  Costs are fp32 at every dtype; d/d am and d/d lm come in the inputs' dtype, the fp32 result
    rounded once; with ``am_only_scale != 0`` d/d lm includes the path through the batch unigram.  Enqueue-only: the call
    can be captured into a graph.

    ``return_grad=True`` returns ``(loss, pair_grads)``: ``pair_grads`` is the detached ``(N,T,U,2)`` fp32
    ``d cost[n] / d pair`` -- not scaled by the reduction or any upstream gradient, zero outside an utterance's window --
    which is what :func:`warp_rnnt_amd.pruned.prune_ranges` takes.  With ``am_only_scale == 0`` an utterance's cost and
    gradients do not depend on its batch.

    Two more arguments, by keyword only: ``rnnt_type="regular"`` and ``delay_penalty=0.0``.
    ``rnnt_type`` (``"regular"`` or ``"modified"``; another string is a ``ValueError``, ``"constrained"`` is not
    covered) and ``delay_penalty >= 0`` are those of :func:`warp_rnnt_amd.pruned.pruned_rnnt_loss_from_logits`.  With
    ``"modified"`` an utterance with ``T_n < U_n`` has the cost ``+inf``, zero ``pair_grads`` and zero gradient rows, and
    ``pair_grads`` is a ``(N,T,U,2)`` view of the frames of a ``(N,T+1,U,2)`` tensor: index it by ``(t,u)`` as ever."""
    return _simple_loss(am, lm, labels, frames_lengths, labels_lengths, blank, lm_only_scale, am_only_scale,
                        fastemit_lambda, average_frames, reduction, return_grad)


def _simple_loss(am, lm, labels, frames_lengths, labels_lengths, blank, lm_only_scale, am_only_scale, fastemit_lambda,
                 average_frames, reduction, return_grad, rnnt_type="regular", delay_penalty=0.0):
    topology, delay_penalty = ops.topology_of(rnnt_type, delay_penalty)
    assert reduction is None or reduction in ("none", "mean", "sum")
    assert isinstance(blank, int)
    q = batch_log_unigram(lm) if am_only_scale != 0 and lm.dim() == 3 and lm.is_floating_point() else None
    out = SimpleRNNTLossFunction.apply(am, lm, q, labels, frames_lengths, labels_lengths, blank, float(lm_only_scale),
                                       float(am_only_scale), float(fastemit_lambda), bool(return_grad), topology,
                                       delay_penalty)
    if not return_grad:
        return finish_costs(out, frames_lengths, average_frames, reduction)
    return finish_costs(out[0], frames_lengths, average_frames, reduction), out[1]


simple_rnnt_loss = ops.with_topology_keywords(simple_rnnt_loss, _simple_loss)


class SimpleRNNTLoss(torch.nn.Module):
    """:func:`simple_rnnt_loss` as a module: stores ``blank``, the two scales, ``fastemit_lambda``, ``reduction``,
    ``rnnt_type`` and ``delay_penalty``."""

    def __init__(self, blank: int = 0, lm_only_scale: float = 0.0, am_only_scale: float = 0.0,
                 fastemit_lambda: float = 0.0, reduction: Optional[str] = "mean", rnnt_type: str = "regular",
                 delay_penalty: float = 0.0):
        super().__init__()
        ops.topology_of(rnnt_type, delay_penalty)
        self.rnnt_type = rnnt_type
        self.delay_penalty = delay_penalty
        self.blank = blank
        self.lm_only_scale = lm_only_scale
        self.am_only_scale = am_only_scale
        self.fastemit_lambda = fastemit_lambda
        self.reduction = reduction

    def forward(self, am, lm, labels, frames_lengths, labels_lengths, return_grad: bool = False):
        return simple_rnnt_loss(am, lm, labels, frames_lengths, labels_lengths, blank=self.blank,
                                lm_only_scale=self.lm_only_scale, am_only_scale=self.am_only_scale,
                                fastemit_lambda=self.fastemit_lambda, reduction=self.reduction, return_grad=return_grad,
                                rnnt_type=self.rnnt_type, delay_penalty=self.delay_penalty)
