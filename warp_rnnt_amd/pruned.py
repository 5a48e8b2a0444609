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
    starts = prune_ranges_hip(pair_grads, xn, yn, s_range)                 # (N,T) int32; pair_grads = -occupancies
    fp, gp = prune_joint_inputs(f, g, starts, s_range)                     # (N,T,S,H) twice
    loss   = pruned_rnnt_loss_from_logits(joiner(fp, gp), labels, starts, xn, yn)
    (simple_loss_scale * simple.sum() + loss.sum()).backward()

:func:`pruned_joint_hidden` is the third step and the joiner's activation as one HIP unit (csrc/pruned_hidden.hip,
DESIGN.md 3.25): ``h = act(f + g on the band)`` written once, a backward that reads ``dh`` and ``h`` and writes ``df`` and
``dg`` -- no ``(N,T,S,H)`` copy of ``g``, no atomics, nothing saved but ``h``; the output projection stays the vendor's
GEMM.  The recipe is then four calls in a row::

    simple, pair_grads = simple_rnnt_loss(am, lm, labels, xn, yn, lm_only_scale=0.25, return_grad=True)
    starts = prune_ranges_hip(pair_grads, xn, yn, s_range)
    h      = pruned_joint_hidden(f, g, starts, xn, s_range=s_range, activation="tanh")     # (N,T,S,H), once
    loss   = pruned_rnnt_loss_from_logits(joiner.output_linear(h), labels, starts, xn, yn)

``simple_rnnt_loss`` (simple.py, csrc/simple.hip) is k2's ``rnnt_loss_smoothed`` on the fused path: its forward already
holds the gradient pairs and hands them back with ``return_grad=True`` -- no ``requires_grad_`` on an intermediate tensor,
no ``autograd.grad(..., retain_graph=True)``.  The plain-torch form of its pairs without the smoothing scales,
``simple_pairs`` below with ``warp_rnnt.rnnt_loss(pairs, labels, xn, yn, blank=-1)`` behind it, stays
(tests/test_gpu_pruned.py runs the recipe on it).  :func:`prune_ranges_hip` (csrc/prune_ranges.hip) is
:func:`prune_ranges`, the plain-torch definition for any device, in two HIP launches: one pass over the pairs.

``rnnt_type="modified"`` (k2's second topology: a label consumes a frame, at most one symbol per frame, no terminal blank)
and ``delay_penalty`` (Kang et al. 2022: ``delay_penalty * ((T_n - 1) / 2 - t)`` added to the label log-probs of frame
``t``) are the two knobs of the streaming recipes; both passes take them and must be given the same values.  The modified
lattice is the regular one over the sheared cells ``(t - u, u)``, whose diagonals are the frames: the sweeps, the gradient
kernel, FastEmit and the guard run unchanged on a frame-major plane of ``T + 1`` rows.

The joiner itself can be part of the loss: :func:`pruned_rnnt_loss_from_joint` takes ``f``, ``g``, the starts and the
joiner's output projection in place of the last two steps and forms the band's logits tile by tile in HIP (MFMA;
csrc/pruned_joint.hip) -- no ``(N,T,S,V)`` logits, no ``(N,T,S,H)`` gather or activation and no autograd
graph over them; the backward's workspace holds one ``(N,T,S,H)`` buffer::

    loss = pruned_rnnt_loss_from_joint(f, g, joiner.output_linear.weight, joiner.output_linear.bias, labels, starts,
                                       xn, yn, s_range=s_range, activation="tanh")

``use_hat_loss=True`` (k2's argument; icefall's ``zipformer_hat``) puts the factorised-blank (HAT) log-probs of
``hat_loss_from_logits`` into the band's cells: csrc/pruned_hat.hip, DESIGN.md 3.23.

:func:`pruned_rnnt_align` is ``rnnt_align`` for this recipe: the best path through the band -- its score and the frame at
which every label is emitted -- from the band's logits (plain or HAT) or from ready-made pairs, in either topology and
with the delay penalty it is the measure of; a frame-synchronous sweep, one wave per utterance, that never forms an
``(N,T,U)`` plane (csrc/pruned_align.hip).

Out of scope: k2's ``constrained`` topology; a pruned form of TDT or the compact layout; the gradient
clamp; loss sweeps that visit the band's cells only (the loss's alpha/beta sweeps cost what the dense loss's do --
DESIGN.md 3.17 prices the alternative; the alignment's sweep above is such a sweep).  Of the joint form: the two knobs of the streaming recipes above, dropout.
"""
import math
from typing import Optional

import torch

from . import ops
from .fused import finish_costs
from .joint import _aligned, check_joint_inputs
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
                topology=ops.RNNT_TYPES["regular"], delay_penalty=0.0, hat=False):
        check_pruned_inputs(logits, labels, starts, frames_lengths, labels_lengths)
        wants_grad = ctx.needs_input_grad[0]          # (nothing requires grad: no pairs are produced or kept)
        # the defaults are the entries without a topology: the calls, and so the bits, of every earlier version
        ctx.plain = topology == ops.RNNT_TYPES["regular"] and delay_penalty == 0.0 and not hat
        ctx.hat = hat
        if hat:                                       # (one pair of entries: the topology and the penalty are arguments)
            costs, grads = ops.pruned_hat_loss(logits, labels, starts, frames_lengths, labels_lengths, blank,
                                               fastemit_lambda, wants_grad, topology, delay_penalty)
        elif ctx.plain:
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
            return (ops.pruned_logits_backward(logits, labels, starts, grads, go, ctx.blank),) + (None,) * 9
        backward = ops.pruned_hat_logits_backward if ctx.hat else ops.pruned_logits_backward_topology
        return (backward(logits, labels, starts, xn, yn, grads, go, ctx.blank, ctx.topology),) + (None,) * 9


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
    ``"modified"`` rows of frames ``t >= frames_lengths[n]`` are never read, whatever their starts are.

    A third, ``use_hat_loss=False`` (k2's argument of that name; icefall's ``zipformer_hat``): with ``True`` the band's
    cells hold the factorised-blank (HAT) log-probs of ``hat_loss_from_logits`` -- ``log sigmoid(z[blank])`` for the blank,
    ``log_softmax`` over the non-blank logits plus ``log(1 - sigmoid(z[blank]))`` for a label -- and the gradient follows
    HAT's chain rule (csrc/pruned_hat.hip); everything else above holds, both topologies and the delay
    penalty included.  With ``S = U``, zero starts and ``"regular"`` the costs and gradients are ``hat_loss_from_logits``'
    bit for bit.  ``False`` makes exactly the calls it made before the argument existed."""
    return _pruned_loss(logits, labels, ranges, frames_lengths, labels_lengths, average_frames, reduction, blank,
                        fastemit_lambda)


def _pruned_loss(logits, labels, ranges, frames_lengths, labels_lengths, average_frames, reduction, blank, fastemit_lambda,
                 rnnt_type="regular", delay_penalty=0.0, use_hat_loss=False):
    topology, delay_penalty = ops.topology_of(rnnt_type, delay_penalty)
    assert reduction is None or reduction in ("none", "mean", "sum")
    assert isinstance(blank, int)
    starts = band_starts(ranges, logits.shape[2] if logits.dim() == 4 else None)
    costs = PrunedRNNTLossFromLogits.apply(logits, labels, starts, frames_lengths, labels_lengths, blank, fastemit_lambda,
                                           topology, delay_penalty, bool(use_hat_loss))
    return finish_costs(costs, frames_lengths, average_frames, reduction)


pruned_rnnt_loss_from_logits = ops.with_topology_keywords(pruned_rnnt_loss_from_logits, _pruned_loss, use_hat_loss=False)


class PrunedRNNTLoss(torch.nn.Module):
    """:func:`pruned_rnnt_loss_from_logits` as a module: stores ``blank``, ``fastemit_lambda``, ``reduction``,
    ``rnnt_type``, ``delay_penalty`` and ``use_hat_loss``."""

    def __init__(self, blank: int = 0, fastemit_lambda: float = 0.0, reduction: Optional[str] = "mean",
                 rnnt_type: str = "regular", delay_penalty: float = 0.0, use_hat_loss: bool = False):
        super().__init__()
        ops.topology_of(rnnt_type, delay_penalty)
        self.blank = blank
        self.fastemit_lambda = fastemit_lambda
        self.reduction = reduction
        self.rnnt_type = rnnt_type
        self.delay_penalty = delay_penalty
        self.use_hat_loss = use_hat_loss

    def forward(self, logits, labels, ranges, frames_lengths, labels_lengths):
        return pruned_rnnt_loss_from_logits(logits, labels, ranges, frames_lengths, labels_lengths,
                                            reduction=self.reduction, blank=self.blank,
                                            fastemit_lambda=self.fastemit_lambda, rnnt_type=self.rnnt_type,
                                            delay_penalty=self.delay_penalty, use_hat_loss=self.use_hat_loss)


PRUNED_ALIGN_KINDS = tuple(ops.PRUNED_ALIGN_KINDS)


def pruned_rnnt_align(inputs: torch.Tensor, labels: torch.Tensor, ranges: torch.Tensor, frames_lengths: torch.Tensor,
                      labels_lengths: torch.Tensor, blank: int = 0, kind: str = "logits", rnnt_type: str = "regular",
                      delay_penalty: float = 0.0):
    """The best path of every utterance through the band: ``(scores, emit_frames)``.

    ``kind`` says what ``inputs`` holds: ``"logits"`` (N,T,S,V) in fp32, bf16 or fp16, read as
    :func:`pruned_rnnt_loss_from_logits` reads them; ``"hat_logits"`` the same, read as it reads them with
    ``use_hat_loss=True``; ``"pairs"`` (N,T,S,2) fp32, channel 0 the blank's log-probability of row ``(n,t,s)`` and channel 1
    the label's (``labels`` and ``blank`` are then only checked for their shape).  ``ranges``: k2's ``(N,T,S)`` integer
    tensor or the ``(N,T)`` starts; ``1 <= S <= min(U, 64)``.  ``rnnt_type`` and ``delay_penalty`` are the loss's, and the
    penalty is added to the label channel of every kind.

    ``scores`` (N,) fp32 is the log-probability (penalties included) of the best path, ``-inf`` where the band holds none
    -- and, with ``"modified"``, where ``T_n < U_n``; ``emit_frames`` (N,U-1) int32 holds the frame at which label ``u`` is
    emitted (``"modified"``: the frame its edge consumes), -1 in the columns from ``labels_lengths[n]`` on and throughout
    for an utterance without a path.  Lengths outside ``[1,T]`` x ``[0,U-1]`` give a NaN score and a row of -1.  The
    arithmetic is fp32, one add per edge and one compare per cell, a tie goes to the blank.
    ``warp_rnnt_amd.align.alignment_mask`` applies unchanged to the regular topology's frames.  Both outputs are detached
    and computed under ``no_grad``.  Enqueue-only: the call can be captured into a graph."""
    assert isinstance(blank, int)
    if kind not in ops.PRUNED_ALIGN_KINDS:
        raise ValueError(f"kind must be one of {PRUNED_ALIGN_KINDS}, not {kind!r}")
    topology, delay_penalty = ops.topology_of(rnnt_type, delay_penalty)
    with torch.no_grad():
        inputs = inputs.detach()
        starts = band_starts(ranges, inputs.shape[2] if inputs.dim() == 4 else None)
        check_pruned_inputs(inputs, labels, starts, frames_lengths, labels_lengths)
        if kind == "pairs" and (inputs.dtype != torch.float32 or inputs.size(3) != 2):
            raise RuntimeError("xs must be float32 with values only for blank and label")
        return ops.pruned_align(inputs, labels, starts, frames_lengths, labels_lengths, ops.PRUNED_ALIGN_KINDS[kind], blank,
                                topology, delay_penalty)


# ---- the rest of the recipe: plain torch on any device, no Python loop over N or T, no read-back; prune_ranges_hip is the
# ---- band selection on the GPU, prune_ranges its definition ----

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


def prune_ranges_hip(pair_grads: torch.Tensor, frames_lengths: torch.Tensor, labels_lengths: torch.Tensor,
                     s_range: int) -> torch.Tensor:
    """:func:`prune_ranges` in HIP (csrc/prune_ranges.hip): the same arguments, the ``(N,T)`` int32 starts
    from one pass over the pairs and one over the ``(N,T)`` ints instead of about fifteen torch operations over
    ``(N,T,U)`` temporaries.  ``pair_grads`` is fp32 on the GPU, the lengths int32 on its device.  Its last three dimensions
    must be contiguous, its batch stride is free -- the ``(N,T,U,2)`` view of the modified topology's ``(N,T+1,U,2)`` pairs
    is read as it is; any other striding costs one ``.contiguous()``.  ``U <= 4096``.  Enqueue-only: no read-back, no host
    synchronisation, the call can be captured into a graph; no atomics, two runs give the same starts.

    Per utterance, with ``occ = -(pair_grads[..., 0] + pair_grads[..., 1])`` and ``hi = clamp(U_n + 1 - S, 0, U - S)``:
    for ``t < T_n - 1`` the lowest ``u0`` in ``[0, hi]`` at which ``w(t,u0) = occ[t,u0] + ... + occ[t,u0+S-1]`` is largest
    -- ``hi`` if an ``occ[t,u]`` with ``u < hi + S`` is a NaN -- and ``hi`` for ``t >= T_n - 1``, whatever ``T_n`` is; then
    the two backward scans of :func:`prune_ranges`.  ``s_range >= U``: all zeros.  Cells ``u >= hi + S`` and frames
    ``t >= T_n - 1`` are not read.

    ``w`` is added left to right from ``u0``, each sum rounded to fp32 on its own: a function of ``S``, ``u0`` and the
    window's values alone, so an utterance's starts do not depend on ``U``'s padding, on ``T`` or on its place in the batch.
    :func:`prune_ranges` forms ``w`` as a difference of two ``cumsum`` values instead, so on real-valued data the two may
    choose differently between windows whose sums agree to within rounding; where every partial sum is exact in fp32
    (occupancies on a dyadic grid) they return the same starts, ties included."""
    S = int(s_range)
    if S < 2:
        raise ValueError(f"s_range must be >= 2, not {s_range}")
    xn, yn = frames_lengths, labels_lengths
    if pair_grads.dtype != torch.float32:
        raise RuntimeError(f"pair_grads must be a float32 tensor, not {pair_grads.dtype}")
    for x, name in ((xn, "xn"), (yn, "yn")):
        _core._check_int(x, name)
    for x, name in ((pair_grads, "pair_grads"), (xn, "xn"), (yn, "yn")):
        _core._check_cuda(x, name)
    if pair_grads.dim() != 4 or pair_grads.size(3) != 2:
        raise RuntimeError("pair_grads must be (N,T,U,2)")
    N, T, U, _ = pair_grads.shape
    if xn.numel() != N:
        raise RuntimeError("xn shape must be equal (N,)")
    if yn.numel() != N:
        raise RuntimeError("yn shape must be equal (N,)")
    for x, name in ((xn, "xn"), (yn, "yn")):
        if x.device != pair_grads.device:
            raise RuntimeError(f"{name} must be on the same device as pair_grads")
    if S >= U or T == 0:
        return torch.zeros((N, T), dtype=torch.int32, device=pair_grads.device)
    g = pair_grads.detach()
    # the entry reads 8-byte cells at n * pitch + t * U + u: rows and cells contiguous, planes apart and on whole cells
    if (g.stride()[1:] != (2 * U, 2, 1) or g.data_ptr() % 8 or
            (N > 1 and (g.stride(0) < 2 * T * U or g.stride(0) % 2))):
        g = g.contiguous()
    return ops.prune_ranges(g, xn.contiguous(), yn.contiguous(), S)


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


# ---- the joiner's hidden activations on the band (csrc/pruned_hidden.hip) ----

class PrunedJointHidden(torch.autograd.Function):

    @staticmethod
    def forward(ctx, f, g, starts, xn, S, activation):
        h = ops.pruned_hidden(_aligned(f.detach()), _aligned(g.detach()), starts, xn, S, activation)
        ctx.save_for_backward(h, starts, xn)          # h is the output: the Linear behind it keeps it anyway
        ctx.U, ctx.activation = g.shape[1], activation
        return h

    @staticmethod
    def backward(ctx, dh):
        h, starts, xn = ctx.saved_tensors
        df, dg = ops.pruned_hidden_backward(_aligned(dh), h, starts, xn, ctx.U, ctx.activation, ctx.needs_input_grad[0],
                                            ctx.needs_input_grad[1])
        return df, dg, None, None, None, None


def pruned_joint_hidden(f: torch.Tensor, g: torch.Tensor, ranges: torch.Tensor,
                        frames_lengths: Optional[torch.Tensor] = None, *, s_range: Optional[int] = None,
                        activation: str = "tanh") -> torch.Tensor:
    """``act(fp + gp)`` on ``fp, gp = prune_joint_inputs(f, g, ranges, s_range)`` as one HIP launch: f ``(N,T,H)``, g
    ``(N,U,H)`` of one dtype (fp32, bf16 or fp16), ``ranges`` k2's ``(N,T,S)`` integer tensor (only ``[..., 0]`` is used) or
    the ``(N,T)`` starts with ``s_range=S``, ``activation`` one of ``ops.ACTIVATIONS``.  Returns ``h`` ``(N,T,S,H)``,
    contiguous, in that dtype::

        h[n,t,s,:] = act(float(f[n,t,:]) + float(g[n, clamp(starts[n,t] + s, 0, U-1), :]))

    the sum and the activation in fp32, rounded once.  Served: ``H % 8 == 0``, ``8 <= H <= 4096``, ``S >= 1``, ``U >= 1``,
    ``T >= 1``; another shape is a ``ValueError``.  With ``frames_lengths`` (N,) int32, frames ``t >= frames_lengths[n]`` are
    not read: their rows of ``h`` are exactly zero, they add exactly nothing to the gradients and their rows of ``df`` are
    zero.  ``None``: all ``T`` frames are live.

    Gradients go to f and g only, and only where they are needed: with ``p = dh * act'(h)`` (``act'`` from the rounded
    ``h``, the product in fp32) ``df`` is the sum of ``p`` over ``s`` and ``dg[n,u]`` the sum over the live ``(t,s)`` whose
    clamped index is ``u`` -- fp32 sums in ascending ``t``, then ``s``, rounded once; a ``u`` no live row maps to gets an
    exactly zero row.  No atomics and no ``(N,T,S,H)`` temporary: nothing is saved but ``h``, two runs give the same bits.
    Enqueue-only: nothing is read back, the call and its backward can be captured into a graph."""
    if activation not in ops.ACTIVATIONS:
        raise ValueError(f"activation must be one of {tuple(ops.ACTIVATIONS)}, not {activation!r}")
    if not isinstance(f, torch.Tensor) or not isinstance(g, torch.Tensor) or f.dim() != 3 or g.dim() != 3:
        raise RuntimeError("f must be (N,T,H) and g (N,U,H)")
    if f.dtype not in ops.LOGITS_DTYPES or g.dtype != f.dtype:
        raise RuntimeError(f"f and g must share one dtype of float32, bfloat16 and float16 (f is {f.dtype}, g is {g.dtype})")
    if ranges.dim() == 3:
        S = ranges.shape[2] if s_range is None else int(s_range)
    elif s_range is None:
        raise ValueError("pruned_joint_hidden needs s_range with ranges of shape (N,T)")
    else:
        S = int(s_range)
    N, T, H = f.shape
    if g.shape[0] != N or g.shape[2] != H:
        raise RuntimeError(f"g must be (N,U,H) = ({N},U,{H}), not {tuple(g.shape)}")
    ops._pruned_hidden_check(T, g.shape[1], S, H)
    starts = band_starts(ranges, S)
    if tuple(starts.shape) != (N, T):
        raise RuntimeError(f"ranges must be (N,T,S) or (N,T) for f (N,T,H) = {tuple(f.shape)}")
    xn = frames_lengths
    if xn is not None:
        _core._check_int(xn, "frames_lengths")
        if xn.numel() != N:
            raise RuntimeError("frames_lengths shape must be equal (N,)")
        xn = xn.contiguous()
    for x, name in ((f, "f"), (g, "g"), (starts, "ranges"), (xn, "frames_lengths")):
        if x is not None:
            _core._check_cuda(x, name)
            if x.device != f.device:
                raise RuntimeError(f"{name} must be on the device of f ({f.device}), not {x.device}")
    return PrunedJointHidden.apply(f, g, starts, xn, S, activation)


# ---- the joiner fused into the loss (csrc/pruned_joint.hip) ----

class PrunedRNNTLossFromJoint(torch.autograd.Function):

    @staticmethod
    def forward(ctx, f, g, weight, bias, labels, starts, S, frames_lengths, labels_lengths, activation, blank,
                fastemit_lambda, with_grads):
        fc, gc = _aligned(f), _aligned(g)
        w = _aligned(weight.to(fc.dtype))                        # W staged in the activations' dtype
        b = bias.to(torch.float32).contiguous() if bias is not None else None
        labels, xn, yn = labels.contiguous(), frames_lengths.contiguous(), labels_lengths.contiguous()
        costs, stats, grads = ops.pruned_joint_loss(fc, gc, w, b, labels, starts, S, xn, yn, activation, blank,
                                                    fastemit_lambda, with_grads)
        no_path = costs >= NO_PATH_COST               # (on the device: nothing is read back)
        if with_grads:
            ctx.save_for_backward(fc, gc, w, b, labels, starts, xn, yn, stats, grads, no_path)
        ctx.S, ctx.activation, ctx.blank = S, activation, blank
        ctx.weight_dtype = weight.dtype
        ctx.bias_dtype = bias.dtype if bias is not None else None
        return torch.where(no_path, torch.full_like(costs, float("inf")), costs)

    @staticmethod
    def backward(ctx, grads_output):
        f, g, w, b, labels, starts, xn, yn, stats, grads, no_path = ctx.saved_tensors
        go = grads_output.reshape(-1).to(torch.float32)
        go = torch.where(no_path, torch.zeros_like(go), go).contiguous()       # scale 0: the utterance adds exactly nothing
        need = ctx.needs_input_grad
        df, dg, dw, db = ops.pruned_joint_backward(f, g, w, b, labels, starts, ctx.S, xn, yn, stats, grads, go,
                                                   ctx.activation, ctx.blank, need[0], need[1], need[2],
                                                   need[3] and b is not None)
        if dw is not None:
            dw = dw.to(ctx.weight_dtype)
        if db is not None:
            db = db.to(ctx.bias_dtype)
        return (df, dg, dw, db) + (None,) * 9


def pruned_rnnt_loss_from_joint(f: torch.Tensor, g: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor],
                                labels: torch.Tensor, ranges: torch.Tensor, frames_lengths: torch.Tensor,
                                labels_lengths: torch.Tensor, activation: str = "tanh", blank: int = 0,
                                fastemit_lambda: float = 0.0, average_frames: bool = False,
                                reduction: Optional[str] = "none", *, s_range: Optional[int] = None,
                                rnnt_type: str = "regular") -> torch.Tensor:
    """The value of ``pruned_rnnt_loss_from_logits(F.linear(act(fp + gp), weight, bias), labels, ranges, ...)`` on
    ``fp, gp = prune_joint_inputs(f, g, ranges, s_range)`` -- f ``(N,T,H)``, g ``(N,U,H)`` the projected encoder and
    decoder outputs, weight ``(V,H)`` and bias ``(V,)`` or None as ``nn.Linear`` holds them, labels ``(N,U-1)``, act
    ``"tanh"`` or ``"relu"`` -- and gradients to f, g, weight and bias, without an ``(N,T,S,V)`` tensor and without an
    ``(N,T,S,H)`` activation or autograd tensor; the backward's workspace holds one ``(N,T,S,H)`` buffer.  Beyond the inputs
    and the returned gradients a step holds at most the byte count of include/warp_rnnt_amd_pruned_joint.h -- the workspace,
    8 bytes per band row, 8 per lattice cell -- plus the staged copy of a master weight (``V H`` elements of the activations'
    dtype) and 64 KiB for the ``(N,)`` vectors.
    ``ranges``: k2's ``(N,T,S)`` integer tensor (only ``[..., 0]`` is used) or the ``(N,T)`` starts with ``s_range=S``.

    f and g share one dtype (fp32, bf16 or fp16); weight and bias may be fp32 or that dtype (an fp32 master weight is
    staged in the activations' dtype).  act(f+g) is computed in fp32 and rounded once to that dtype as the matrix-core
    operand; the logits stay fp32.  Costs are fp32; every gradient comes back in its parameter's dtype.  Supported:
    H % 32 == 0, 32 <= H <= 1024, V >= 2, 1 <= S <= U.  Enqueue-only: the call can be captured into a graph.

    Rows, masked columns (a bias of ``-inf``), an utterance whose band holds no path (``+inf``, exactly zero gradients,
    the rest of the batch untouched) and the guard are those of :func:`pruned_rnnt_loss_from_logits`; frames
    ``t >= frames_lengths[n]`` and positions behind ``labels_lengths[n]`` are not read.  Two runs give the same bits: no
    atomics anywhere.

    Not covered: ``rnnt_type`` other than ``"regular"`` (a ``ValueError``) and ``delay_penalty``, dropout, the gradient
    clamp, the compact layout, TDT band forms, and ``use_hat_loss``: HAT inside the MFMA joiner is out of scope -- form the
    band's logits and call ``pruned_rnnt_loss_from_logits(..., use_hat_loss=True)``."""
    if rnnt_type != "regular":
        raise ValueError(f"pruned_rnnt_loss_from_joint takes rnnt_type='regular' only, not {rnnt_type!r}: the modified "
                         "topology and the delay penalty are served by pruned_rnnt_loss_from_logits")
    assert reduction is None or reduction in ("none", "mean", "sum")
    assert isinstance(blank, int)
    if not isinstance(labels, torch.Tensor) or not isinstance(g, torch.Tensor) or labels.dim() != 2 or g.dim() != 3:
        raise RuntimeError("labels must be (N,U-1) and g (N,U,H)")
    if ranges.dim() == 3:
        S = ranges.shape[2] if s_range is None else int(s_range)
    elif s_range is None:
        raise ValueError("pruned_rnnt_loss_from_joint needs s_range with ranges of shape (N,T)")
    else:
        S = int(s_range)
    check_joint_inputs(f, g, weight, bias, labels, frames_lengths, labels_lengths, activation, blank)
    starts = band_starts(ranges, S)
    if tuple(starts.shape) != tuple(f.shape[:2]) or starts.device != f.device:
        raise RuntimeError(f"ranges must be (N,T,S) or (N,T) for f (N,T,H) = {tuple(f.shape)}, on its device")
    with_grads = torch.is_grad_enabled() and any(x is not None and x.requires_grad for x in (f, g, weight, bias))
    costs = PrunedRNNTLossFromJoint.apply(f, g, weight, bias, labels, starts, S, frames_lengths, labels_lengths, activation,
                                          blank, fastemit_lambda, with_grads)
    return finish_costs(costs, frames_lengths, average_frames, reduction)


class PrunedJointLoss(torch.nn.Module):
    """The joiner's output projection and the pruned loss as one module -- ``activation -> Linear(hidden, vocab) -> pruned
    loss`` on :func:`pruned_rnnt_loss_from_joint`: it owns ``weight`` (vocab, hidden) and ``bias``, initialised as
    ``nn.Linear`` initialises them."""

    def __init__(self, hidden: int, vocab: int, activation: str = "tanh", bias: bool = True, blank: int = 0,
                 fastemit_lambda: float = 0.0, reduction: Optional[str] = "mean"):
        super().__init__()
        if activation not in ops.ACTIVATIONS:
            raise ValueError(f"activation must be one of {tuple(ops.ACTIVATIONS)}, not {activation!r}")
        self.hidden, self.vocab, self.activation = hidden, vocab, activation
        self.blank, self.fastemit_lambda, self.reduction = blank, fastemit_lambda, reduction
        self.weight = torch.nn.Parameter(torch.empty(vocab, hidden))
        self.bias = torch.nn.Parameter(torch.empty(vocab)) if bias else None
        torch.nn.init.kaiming_uniform_(self.weight, a=math.sqrt(5))      # (nn.Linear.reset_parameters)
        if self.bias is not None:
            torch.nn.init.uniform_(self.bias, -1 / math.sqrt(hidden), 1 / math.sqrt(hidden))

    def forward(self, f, g, labels, ranges, frames_lengths, labels_lengths, s_range=None):
        return pruned_rnnt_loss_from_joint(f, g, self.weight, self.bias, labels, ranges, frames_lengths, labels_lengths,
                                           activation=self.activation, blank=self.blank,
                                           fastemit_lambda=self.fastemit_lambda, reduction=self.reduction, s_range=s_range)
