"""The pruned transducer loss on the fused path: logits ``(N,T,S,V)`` -> costs -> d/d logits.

This is the loss of Kuang et al. 2022, "Pruned RNN-T for fast, memory-efficient ASR training" -- k2's
``rnnt_loss_pruned(..., rnnt_type="regular")``, what the icefall / Zipformer recipes train with.  A cheap first pass over
a trivial joiner gives, per frame, a band of ``S`` (typically 5) label positions; the joint network runs on that band only;
the loss is the ordinary transducer lattice restricted to the band::

    row (n,t,s) of the logits  =  lattice cell (t, u = starts[n,t] + s) of utterance n
    lp = log_softmax(logits[n,t,s,:]),   pair of the cell = (lp[blank], lp[labels[n,u]])

and every cell of the ``(N,T,U)`` grid that no row maps to is switched off.  The logits are ``(N,T,S,V)`` instead of
``(N,T,U,V)``: at N=16, T=1500, U=300, V=1025 in bf16 0.25 GB instead of 14.8.  The lattice between the two streaming kernels
of csrc/pruned.hip -- sweeps, costs, gradient pairs -- is the one of ``rnnt_loss_from_logits`` over the full grid, with a
finite floor (-1e30) in the cells outside the band.

The recipe, in three steps (tests/test_gpu_simple.py runs it end to end)::

    simple, pair_grads = simple_rnnt_loss(am, lm, labels, xn, yn, lm_only_scale=0.25, return_grad=True)    # the first pass
    starts = prune_ranges(pair_grads, xn, yn, s_range)                     # (N,T) int32; pair_grads = -occupancies
    fp, gp = prune_joint_inputs(f, g, starts, s_range)                     # (N,T,S,H) twice
    loss   = pruned_rnnt_loss_from_logits(joiner(fp, gp), labels, starts, xn, yn)
    (simple_loss_scale * simple.sum() + loss.sum()).backward()

``simple_rnnt_loss`` (simple.py, csrc/simple.hip) is k2's ``rnnt_loss_smoothed`` on the fused path: its forward already
holds the gradient pairs and hands them back with ``return_grad=True`` -- no ``requires_grad_`` on an intermediate tensor,
no ``autograd.grad(..., retain_graph=True)``.  The plain-torch form of its pairs without the smoothing scales,
``simple_pairs`` below with ``warp_rnnt.rnnt_loss(pairs, labels, xn, yn, blank=-1)`` behind it, stays
(tests/test_gpu_pruned.py runs the recipe on it).

``rnnt_type="modified"`` (k2's second topology: a label consumes a frame, at most one symbol per frame, no terminal blank)
and ``delay_penalty`` (Kang et al. 2022: ``delay_penalty * ((T_n - 1) / 2 - t)`` added to the label log-probs of frame
``t``) are the two knobs of the streaming recipes; both passes take them and must be given the same values.  The modified
lattice is the regular one over the sheared cells ``(t - u, u)``, whose diagonals are the frames: the sweeps, the gradient
kernel, FastEmit and the guard run unchanged on a frame-major plane of ``T + 1`` rows.

Out of scope: k2's ``constrained`` topology; a pruned form of HAT, TDT, the joint entries, the compact
layout or ``rnnt_align``; the gradient clamp; a sweep that visits the band's cells only (the sweeps cost what the dense
loss's do -- DESIGN.md 3.17 prices the alternative).
"""
from typing import Optional

import torch

from . import ops
from .fused import finish_costs
from warp_rnnt import _C as _core

NO_PATH_COST = 1e29      # the C entry's cost of an utterance whose band holds no path is at least this (sums of the floor)


def check_pruned_inputs(logits, labels, starts, xn, yn):
    """The checks of the logits entries (warp_rnnt._C.check_inputs: its order, its texts) for logits ``(N,T,S,V)`` whose
    third dimension is the band, not the lattice's ``U``."""
    for x, name in ((logits, "xs"), (labels, "ys"), (xn, "xn"), (yn, "yn")):
        _core._check_contiguous(x, name)
    if logits.dtype not in ops.LOGITS_DTYPES:
        raise RuntimeError(f"xs (logits) must be a float32, bfloat16 or float16 tensor, not {logits.dtype}")
    for x, name in ((labels, "ys"), (xn, "xn"), (yn, "yn")):
        _core._check_int(x, name)
    for x, name in ((logits, "xs"), (labels, "ys"), (xn, "xn"), (yn, "yn")):
        _core._check_cuda(x, name)
    if logits.dim() != 4:
        raise RuntimeError("xs must have 4 dimensions")
    N, T, S, _ = logits.shape
    if xn.numel() != N:
        raise RuntimeError("xn shape must be equal (N,)")
    if yn.numel() != N:
        raise RuntimeError("yn shape must be equal (N,)")
    if labels.dim() != 2 or labels.size(0) != N:
        raise RuntimeError("ys shape (N, U-1) mismatched with xs (N, T, S, V)")
    if tuple(starts.shape) != (N, T):
        raise RuntimeError(f"ranges must be (N,T,S) or (N,T) for xs (N, T, S, V) = {tuple(logits.shape)}")
    for x, name in ((labels, "ys"), (xn, "xn"), (yn, "yn"), (starts, "ranges")):
        if x.device != logits.device:
            raise RuntimeError(f"{name} must be on the same device as xs")


def band_starts(ranges, S=None):
    """``(N,T)`` int32 contiguous starts of ``ranges``: k2's ``(N,T,S)`` integer tensor (only ``[..., 0]`` is used:
    ``ranges[n,t,s] = starts[n,t] + s``) or the starts themselves."""
    if ranges.dtype.is_floating_point or ranges.dtype == torch.bool:
        raise RuntimeError(f"ranges must be an integer tensor, not {ranges.dtype}")
    if ranges.dim() == 3:
        if S is not None and ranges.size(2) != S:
            raise RuntimeError(f"ranges (N,T,S) has S = {ranges.size(2)}, the logits have S = {S}")
        ranges = ranges[..., 0]
    elif ranges.dim() != 2:
        raise RuntimeError("ranges must be (N,T,S) or (N,T)")
    return ranges.to(torch.int32).contiguous()


class PrunedRNNTLossFromLogits(torch.autograd.Function):

    @staticmethod
    def forward(ctx, logits, labels, starts, frames_lengths, labels_lengths, blank=0, fastemit_lambda=0.0,
                topology=ops.RNNT_TYPES["regular"], delay_penalty=0.0):
        check_pruned_inputs(logits, labels, starts, frames_lengths, labels_lengths)
        wants_grad = ctx.needs_input_grad[0]          # (nothing requires grad: no pairs are produced or kept)
        # the defaults are the entries without a topology: the calls, and so the bits, of every earlier version
        ctx.plain = topology == ops.RNNT_TYPES["regular"] and delay_penalty == 0.0
        if ctx.plain:
            costs, grads = ops.pruned_loss(logits, labels, starts, frames_lengths, labels_lengths, blank, fastemit_lambda,
                                           wants_grad)
        else:
            costs, grads = ops.pruned_loss_topology(logits, labels, starts, frames_lengths, labels_lengths, blank,
                                                    fastemit_lambda, wants_grad, topology, delay_penalty)
        no_path = costs >= NO_PATH_COST               # (on the device: nothing is read back)
        if wants_grad:
            ctx.save_for_backward(logits, labels, starts, frames_lengths, labels_lengths, grads, no_path)
        ctx.blank, ctx.topology = blank, topology
        return torch.where(no_path, torch.full_like(costs, float("inf")), costs)

    @staticmethod
    def backward(ctx, grads_output):
        logits, labels, starts, xn, yn, grads, no_path = ctx.saved_tensors
        go = grads_output.reshape(-1).to(torch.float32)
        go = torch.where(no_path, torch.zeros_like(go), go).contiguous()       # scale 0: exactly zero rows, pairs unread
        if ctx.plain:
            return (ops.pruned_logits_backward(logits, labels, starts, grads, go, ctx.blank),) + (None,) * 8
        return (ops.pruned_logits_backward_topology(logits, labels, starts, xn, yn, grads, go, ctx.blank,
                                                    ctx.topology),) + (None,) * 8


def pruned_rnnt_loss_from_logits(logits: torch.Tensor, labels: torch.Tensor, ranges: torch.Tensor,
                                 frames_lengths: torch.Tensor, labels_lengths: torch.Tensor, average_frames: bool = False,
                                 reduction: Optional[str] = "none", blank: int = 0,
                                 fastemit_lambda: float = 0.0) -> torch.Tensor:
    """The pruned transducer loss of logits ``(N,T,S,V)`` (fp32, bf16 or fp16; ``V >= 2``, ``1 <= S <= U``), labels
    ``(N,U-1)`` int32 and ``ranges``: k2's ``(N,T,S)`` integer tensor -- of which only ``[..., 0]`` is used -- or the starts
    ``(N,T)``; the other arguments as ``rnnt_loss_from_logits``.  In exact arithmetic the value and gradients of k2's
    ``rnnt_loss_pruned(..., rnnt_type="regular")`` with ``ranges[n,t,s] = starts[n,t] + s``.  Costs are fp32 at every
    dtype, d/d logits comes in the logits' dtype.  Enqueue-only: the call can be captured into a graph.

    A row whose ``starts[n,t] + s`` lies outside ``[0,U)`` is not part of the lattice: it is not read and its gradient row
    is exactly zero.  Frames ``t >= frames_lengths[n]`` may hold any start.  A logit of ``-inf`` is a masked entry.

    An utterance whose band holds no path from ``(0,0)`` to ``(T_n - 1, U_n)`` -- ``prune_ranges`` explains when that
    happens -- has the cost ``+inf`` and exactly zero gradient rows; the other utterances of the batch are not affected.
    The forward/backward guard of the lattice (a ``RuntimeWarning`` at a later call, ``warp_rnnt_amd.last_mismatch()``) may
    name such an utterance: its two sweeps are sums of the floor and need not agree.

    Two more arguments, by keyword only: ``rnnt_type="regular"`` and ``delay_penalty=0.0``.
    ``rnnt_type``: ``"regular"`` or ``"modified"`` (k2's: a label consumes a frame; the cost is ``-alpha(T_n, U_n)`` of
    ``alpha(t,u) = lse(alpha(t-1,u) + lpB(t-1,u), alpha(t-1,u-1) + lpL(t-1,u-1))``; an utterance with ``T_n < U_n`` has
    no path); another string is a ``ValueError`` (``"constrained"`` is not covered).  ``delay_penalty >= 0`` adds
    ``delay_penalty * ((T_n - 1) / 2 - t)`` to the label log-prob of every cell of frame ``t`` (fp32), as k2 does.  With
    ``"modified"`` rows of frames ``t >= frames_lengths[n]`` are never read, whatever their starts are."""
    return _pruned_loss(logits, labels, ranges, frames_lengths, labels_lengths, average_frames, reduction, blank,
                        fastemit_lambda)


def _pruned_loss(logits, labels, ranges, frames_lengths, labels_lengths, average_frames, reduction, blank, fastemit_lambda,
                 rnnt_type="regular", delay_penalty=0.0):
    topology, delay_penalty = ops.topology_of(rnnt_type, delay_penalty)
    assert reduction is None or reduction in ("none", "mean", "sum")
    assert isinstance(blank, int)
    starts = band_starts(ranges, logits.shape[2] if logits.dim() == 4 else None)
    costs = PrunedRNNTLossFromLogits.apply(logits, labels, starts, frames_lengths, labels_lengths, blank, fastemit_lambda,
                                           topology, delay_penalty)
    return finish_costs(costs, frames_lengths, average_frames, reduction)


pruned_rnnt_loss_from_logits = ops.with_topology_keywords(pruned_rnnt_loss_from_logits, _pruned_loss)


class PrunedRNNTLoss(torch.nn.Module):
    """:func:`pruned_rnnt_loss_from_logits` as a module: stores ``blank``, ``fastemit_lambda``, ``reduction``,
    ``rnnt_type`` and ``delay_penalty``."""

    def __init__(self, blank: int = 0, fastemit_lambda: float = 0.0, reduction: Optional[str] = "mean",
                 rnnt_type: str = "regular", delay_penalty: float = 0.0):
        super().__init__()
        ops.topology_of(rnnt_type, delay_penalty)
        self.blank = blank
        self.fastemit_lambda = fastemit_lambda
        self.reduction = reduction
        self.rnnt_type = rnnt_type
        self.delay_penalty = delay_penalty

    def forward(self, logits, labels, ranges, frames_lengths, labels_lengths):
        return pruned_rnnt_loss_from_logits(logits, labels, ranges, frames_lengths, labels_lengths,
                                            reduction=self.reduction, blank=self.blank,
                                            fastemit_lambda=self.fastemit_lambda, rnnt_type=self.rnnt_type,
                                            delay_penalty=self.delay_penalty)


# ---- the rest of the recipe: plain torch on any device, not a hot path, no Python loop over N or T, no read-back ----

def simple_pairs(am: torch.Tensor, lm: torch.Tensor, labels: torch.Tensor, blank: int = 0) -> torch.Tensor:
    """The ``(N,T,U,2)`` (blank, label) log-probability pairs of the trivial joiner ``log_softmax(am[n,t,:] + lm[n,u,:])``
    for ``am`` ``(N,T,V)``, ``lm`` ``(N,U,V)`` and labels ``(N,U-1)``, without an ``(N,T,U,V)`` tensor: the normaliser is
    ``log(exp(am - max) @ exp(lm - max)^T)`` plus the two maxima.  The last column's label is the blank, and so is a label
    outside ``[0,V)``.  ``warp_rnnt.rnnt_loss(pairs, labels, xn, yn, blank=-1)`` is the first pass of the recipe; its
    gradient w.r.t. ``pairs`` is minus the edge occupancies, which :func:`prune_ranges` reads."""
    N, T, V = am.shape
    U = lm.shape[1]
    if lm.shape[0] != N or lm.shape[2] != V or tuple(labels.shape) != (N, U - 1) or not 0 <= blank < V:
        raise ValueError(f"simple_pairs needs am (N,T,V), lm (N,U,V), labels (N,U-1) and 0 <= blank < V "
                         f"(am {tuple(am.shape)}, lm {tuple(lm.shape)}, labels {tuple(labels.shape)}, blank={blank})")
    am_max = am.max(dim=2, keepdim=True).values                              # (N,T,1)
    lm_max = lm.max(dim=2, keepdim=True).values                              # (N,U,1)
    norm = torch.matmul((am - am_max).exp(), (lm - lm_max).exp().transpose(1, 2)).log() + am_max + lm_max.transpose(1, 2)
    lab = labels.long()
    lab = torch.where((lab >= 0) & (lab < V), lab, torch.full_like(lab, blank))
    lab = torch.cat([lab, torch.full((N, 1), blank, dtype=torch.long, device=lab.device)], dim=1)       # (N,U)
    label = am.gather(2, lab[:, None, :].expand(N, T, U)) + lm.gather(2, lab[:, :, None]).transpose(1, 2)
    blank_ = am[:, :, blank:blank + 1] + lm[:, :, blank].unsqueeze(1)
    return torch.stack([blank_ - norm, label - norm], dim=-1)


def prune_ranges(pair_grads: torch.Tensor, frames_lengths: torch.Tensor, labels_lengths: torch.Tensor,
                 s_range: int) -> torch.Tensor:
    """The ``(N,T)`` int32 band starts from the first pass's gradient ``pair_grads`` ``(N,T,U,2)``, ``s_range = S >= 2``.

    Per utterance, with ``occ = -(pair_grads[..., 0] + pair_grads[..., 1])`` and ``hi = max(U_n + 1 - S, 0)``: for
    ``t < T_n``, ``start[t]`` is the lowest ``u0`` in ``[0, hi]`` at which ``sum(occ[t, u0 : u0 + S])`` is largest;
    ``start[T_n - 1]`` is then ``hi``; then, from the end backwards, ``start[t] = min(start[t], start[t+1])`` (one scan:
    the starts do not fall), and after it ``start[t] = max(start[t], start[t+1] - (S - 1))`` (a second scan: a band
    reaches the next one).  Frames ``t >= T_n`` repeat ``hi``.  So ``0 <= start[t+1] - start[t] <= S - 1`` and every band
    lies inside ``[0, max(U_n + 1, S))``.  ``s_range >= U``: the band is the lattice, all zeros.

    When ``(T_n - 1) * (S - 1) < U_n + 1 - S`` no band of that width holds a path -- ``T_n`` frames cannot climb ``U_n``
    labels in steps of ``S - 1``.  The second scan then leaves ``start[0] > 0``, cell ``(0,0)`` is outside the band, and
    :func:`pruned_rnnt_loss_from_logits` answers ``+inf`` for that utterance."""
    N, T, U, _ = pair_grads.shape
    S = int(s_range)
    if S < 2:
        raise ValueError(f"s_range must be >= 2, not {s_range}")
    dev = pair_grads.device
    if S >= U:
        return torch.zeros((N, T), dtype=torch.int32, device=dev)
    occ = -(pair_grads[..., 0] + pair_grads[..., 1]).detach()
    cs = torch.cat([occ.new_zeros((N, T, 1)), occ.cumsum(dim=2)], dim=2)          # (N,T,U+1)
    window = cs[..., S:] - cs[..., :U + 1 - S]                                    # (N,T,U-S+1): u0 = 0 .. U-S
    u0 = torch.arange(U + 1 - S, device=dev)
    hi = (labels_lengths.to(dev).long() + 1 - S).clamp(min=0, max=U - S)          # (N,)
    window = window.masked_fill(u0[None, None, :] > hi[:, None, None], float("-inf"))
    best = window.max(dim=2, keepdim=True).values
    start = torch.where(window == best, u0[None, None, :], u0.new_full((), U)).min(dim=2).values      # lowest argmax
    start = torch.minimum(start, hi[:, None])          # (a row of NaN occupancies has no argmax: stays inside the bounds)
    t = torch.arange(T, device=dev)
    live = t[None, :] < (frames_lengths.to(dev).long()[:, None] - 1)
    start = torch.where(live, start, hi[:, None])                                 # start[T_n - 1] and the frames behind it
    # from the end backwards: min(start[t], start[t+1]) -- the running minimum of the reversed sequence
    start = start.flip(1).cummin(dim=1).values.flip(1)
    # ... then max(start[t], start[t+1] - (S-1)): start[t] = t (S-1) + max_{t' >= t} (start[t'] - t' (S-1))
    ramp = t * (S - 1)
    start = (start - ramp).flip(1).cummax(dim=1).values.flip(1) + ramp
    return start.to(torch.int32)


def prune_joint_inputs(f: torch.Tensor, g: torch.Tensor, ranges: torch.Tensor, s_range: Optional[int] = None):
    """The joint network's inputs on the band: ``f`` ``(N,T,H)`` broadcast over ``s`` and ``g`` ``(N,U,H)`` gathered at
    ``start + s`` (the index clamped to ``[0, U-1]``), both ``(N,T,S,H)``.  ``ranges``: k2's ``(N,T,S)`` tensor (only
    ``[..., 0]`` is used) or the ``(N,T)`` starts with ``s_range = S``.  The caller's joiner then produces the
    ``(N,T,S,V)`` logits of :func:`pruned_rnnt_loss_from_logits`."""
    N, T, H = f.shape
    U = g.shape[1]
    if ranges.dim() == 3:
        S = ranges.shape[2] if s_range is None else int(s_range)
        starts = ranges[..., 0]
    else:
        if s_range is None:
            raise ValueError("prune_joint_inputs needs s_range with ranges of shape (N,T)")
        S, starts = int(s_range), ranges
    if tuple(starts.shape) != (N, T) or g.shape[0] != N or g.shape[2] != H or S < 1:
        raise ValueError(f"prune_joint_inputs needs f (N,T,H), g (N,U,H) and ranges (N,T,S) or (N,T) "
                         f"(f {tuple(f.shape)}, g {tuple(g.shape)}, ranges {tuple(ranges.shape)})")
    idx = (starts.long()[..., None] + torch.arange(S, device=starts.device)).clamp(0, U - 1)          # (N,T,S)
    gp = g.gather(1, idx.reshape(N, T * S, 1).expand(N, T * S, H)).reshape(N, T, S, H)
    return f[:, :, None, :].expand(N, T, S, H), gp
