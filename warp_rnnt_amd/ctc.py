"""The CTC loss (Graves et al. 2006) from logits, fused in HIP: logits -> costs -> d/d logits.

Every recipe this package serves trains a CTC head beside the transducer (icefall's ``--use-ctc``, NeMo's hybrid RNNT-CTC
models, ESPnet's ``ctc_weight``).  Outside the package that term is ``torch.log_softmax(logits.float(), -1).transpose(0, 1)``
followed by ``F.ctc_loss``: an fp32 ``(T,N,V)`` log-prob tensor and its gradient in memory, no half-precision entry, and a
backward that adds up repeated labels with floating-point atomics.  Here (csrc/ctc.hip, include/warp_rnnt_amd_ctc.h) the
logits are read once for the emissions of the ``L_n + 1`` columns the lattice uses, the alpha and beta sweeps run on those,
and the backward reads the logits once more and writes d/d logits in their dtype.  No atomics: the same bits every run, and
an utterance's bits do not depend on the batch it is in.

:func:`ctc_align` is the head's other use: the best path through the same lattice (csrc/ctc_align.hip,
include/warp_rnnt_amd_ctc_align.h) -- its score, the token of every frame and the frame every label starts at -- for a whole
batch in two launches, from logits (the loss's emissions, bit for bit) or from log-probs taken as they are.

Out of scope: torch's ``(T,N,V)`` layout, a ``log_probs`` entry of the loss, the CR-CTC consistency term, label priors, the
compact layout, a gradient clamp, the mismatch guard, a joint / MFMA form; of the alignment: per-frame scores, word-level
merging.
"""
from typing import Optional

import torch

from . import ops
from .compat import REDUCTIONS, resolve_blank
from warp_rnnt import _C as _core


class CTCLossFromLogits(torch.autograd.Function):

    @staticmethod
    def forward(ctx, logits, labels, frames_lengths, labels_lengths, blank):
        costs, workspace = ops.ctc_loss(logits, labels, frames_lengths, labels_lengths, blank)
        if ctx.needs_input_grad[0]:       # (nothing requires grad: the beta sweep and the gradient kernel never run)
            ctx.save_for_backward(logits, labels, frames_lengths, labels_lengths, workspace)
        ctx.blank = blank
        return costs

    @staticmethod
    def backward(ctx, grads_output):
        logits, labels, xn, yn, workspace = ctx.saved_tensors
        go = grads_output.reshape(-1).to(torch.float32).contiguous()
        return ops.ctc_logits_backward(logits, labels, xn, yn, workspace, go, ctx.blank), None, None, None, None


def ctc_loss_from_logits(logits: torch.Tensor, labels: torch.Tensor, frames_lengths: torch.Tensor,
                         labels_lengths: torch.Tensor, blank: int = 0, reduction: Optional[str] = "mean") -> torch.Tensor:
    """The CTC costs ``-log p(labels | logits)`` of ``logits`` ``(N,T,V)`` -- batch-major and contiguous, as the encoder's
    CTC head emits them; fp32, bf16 or fp16 -- with ``labels`` ``(N,L)`` int32, padded, and ``frames_lengths``,
    ``labels_lengths`` ``(N,)`` int32.  ``blank`` is any column of ``[0, V)``; negative counts from the end.

    ``reduction``: ``"none"`` (the ``(N,)`` costs), ``"sum"`` or ``"mean"`` with the meaning the package's other entries
    give them: ``"mean"`` is the batch mean of the costs.  It is NOT torch's ``ctc_loss(reduction="mean")``, which divides
    every cost by its target length first.

    Costs are fp32 at every dtype; d/d logits comes in the logits' dtype, rows ``t >= frames_lengths[n]`` exactly zero.  An
    utterance without labels has the single all-blank path.  An utterance without any path (``T_n < L_n +`` its adjacent
    repeats) costs ``+inf`` and has an all-zero gradient; nothing is ever NaN because of it.  Lengths outside
    ``1 <= T_n <= T``, ``0 <= L_n <= L`` give a NaN cost and a zero gradient, as in the transducer entries.

    Served: ``1 <= L <= 1023``, ``2 <= V <= 16384``, ``N*T*(L+1) < 2^31``; another shape is a ``ValueError``.
    Enqueue-only: nothing is read back, the call and its backward can be captured into a graph.  When nothing requires
    grad only the forward kernels run."""
    if reduction not in REDUCTIONS:
        raise ValueError(f"reduction must be one of {REDUCTIONS}, not {reduction!r}")
    blank = _checked(logits, labels, frames_lengths, labels_lengths, blank)
    costs = CTCLossFromLogits.apply(logits, labels, frames_lengths, labels_lengths, blank)
    if reduction == "none":
        return costs
    return costs.sum() if reduction == "sum" else costs.mean()


def _checked(logits, labels, frames_lengths, labels_lengths, blank):
    """The argument checks of both entries; returns the blank as a column of ``[0, V)``."""
    if not isinstance(logits, torch.Tensor) or logits.dim() != 3:
        raise RuntimeError("logits must be (N,T,V)")
    if logits.dtype not in ops.LOGITS_DTYPES:
        raise RuntimeError(f"logits must be a float32, bfloat16 or float16 tensor, not {logits.dtype}")
    N, T, V = logits.shape
    if labels.dim() != 2 or labels.shape[0] != N:
        raise RuntimeError(f"labels must be (N,L) = ({N},L), not {tuple(labels.shape)}")
    for x, name in ((labels, "labels"), (frames_lengths, "frames_lengths"), (labels_lengths, "labels_lengths")):
        _core._check_int(x, name)
    for x, name in ((frames_lengths, "frames_lengths"), (labels_lengths, "labels_lengths")):
        if tuple(x.shape) != (N,):
            raise RuntimeError(f"{name} shape must be equal (N,)")
    for x, name in ((logits, "logits"), (labels, "labels"), (frames_lengths, "frames_lengths"),
                    (labels_lengths, "labels_lengths")):
        _core._check_contiguous(x, name)
    ops._ctc_check(N, T, labels.shape[1], V, resolve_blank(blank, V))
    for x, name in ((logits, "logits"), (labels, "labels"), (frames_lengths, "frames_lengths"),
                    (labels_lengths, "labels_lengths")):
        _core._check_cuda(x, name)
        if x.device != logits.device:
            raise RuntimeError(f"{name} must be on the device of logits ({logits.device}), not {x.device}")
    return resolve_blank(blank, V)


def ctc_align(inputs: torch.Tensor, labels: torch.Tensor, frames_lengths: torch.Tensor, labels_lengths: torch.Tensor,
              blank: int = 0, kind: str = "logits"):
    """The best path through the CTC lattice of every utterance (forced alignment): ``(scores, frame_tokens, emit_frames)``.

    ``inputs`` ``(N,T,V)``, batch-major and contiguous, fp32, bf16 or fp16: logits (``kind="logits"``: the emissions are the
    log-softmax bits :func:`ctc_loss_from_logits` uses) or log-probs taken as they are, not normalised
    (``kind="log_probs"``: what ``torchaudio.functional.forced_align`` takes, here for a whole ragged batch).  The other
    arguments are :func:`ctc_loss_from_logits`'s, with its checks.

    ``scores`` ``(N,)`` fp32: the log-probability of the best path; ``frame_tokens`` ``(N,T)`` int32: the token of every
    frame on it (``blank`` between labels), -1 from ``frames_lengths[n]`` on; ``emit_frames`` ``(N,L)`` int32: the first
    frame of every label, -1 from ``labels_lengths[n]`` on.  Of equal paths the one that stays in the higher state wins
    (include/warp_rnnt_amd_ctc_align.h has the rule).  An utterance without any path gets ``-inf`` and rows of -1; lengths
    outside ``1 <= T_n <= T``, ``0 <= L_n <= L`` give a NaN score and rows of -1.  Nothing is differentiable: the results are
    detached.  Enqueue-only: the call can be captured into a graph."""
    if kind not in ops.CTC_ALIGN_KINDS:
        raise ValueError(f"kind must be one of {tuple(ops.CTC_ALIGN_KINDS)}, not {kind!r}")
    blank = _checked(inputs, labels, frames_lengths, labels_lengths, blank)
    with torch.no_grad():
        return ops.ctc_align(inputs.detach(), labels, frames_lengths, labels_lengths, ops.CTC_ALIGN_KINDS[kind], blank)[:3]


class CTCLoss(torch.nn.Module):
    """:func:`ctc_loss_from_logits` as a module: stores ``blank`` and ``reduction``."""

    def __init__(self, blank: int = 0, reduction: Optional[str] = "mean"):
        super().__init__()
        self.blank = blank
        self.reduction = reduction

    def forward(self, logits, labels, frames_lengths, labels_lengths):
        return ctc_loss_from_logits(logits, labels, frames_lengths, labels_lengths, blank=self.blank,
                                    reduction=self.reduction)
