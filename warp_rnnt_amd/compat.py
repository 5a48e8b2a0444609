"""The call shapes most transducer training code uses, on the fused path (logits -> loss -> d/d logits).

``rnnt_loss`` has the signature of ``torchaudio.functional.rnnt_loss``; ``RNNTLoss`` is the module form, and built with
``blank=0`` it is the warp-transducer / NeMo call shape too: ``RNNTLoss(blank=0, reduction=...)(acts, labels, act_lens,
label_lens)``.  Coming from either, the import is the one line that changes.

Both take logits -- not log-probabilities -- and a gradient ``clamp``: the d/d logits of every utterance's cost are limited
to ``[-clamp, +clamp]`` elementwise and only then multiplied by the upstream gradient, which carries the reduction.  On
the fused path that clamp sits inside the backward kernel (include/warp_rnnt_amd_clamp.h).

The pure parts -- blank resolution, clamp mapping, the reduction check -- are functions of their own and need no device.
"""
import torch

REDUCTIONS = ("none", "mean", "sum")


def resolve_blank(blank: int, V: int) -> int:
    """``blank < 0`` counts from the end of the vocabulary (``-1``: the last symbol, torchaudio's default); the result must
    lie in ``[0, V)``."""
    b = int(blank)
    if b < 0:
        b += V
    if not 0 <= b < V:
        raise ValueError(f"blank={blank} is outside a vocabulary of {V} symbols")
    return b


def resolve_clamp(clamp: float) -> float:
    """``clamp <= 0`` means off (torchaudio's default is -1): 0.0, what ``rnnt_loss_from_logits`` takes for "no clamp"."""
    c = float(clamp)
    return c if c > 0.0 else 0.0


def check_reduction(reduction: str) -> str:
    if reduction not in REDUCTIONS:
        raise ValueError(f"reduction should be one of {', '.join(REDUCTIONS)}, not {reduction!r}")
    return reduction


def rnnt_loss(logits: torch.Tensor, targets: torch.Tensor, logit_lengths: torch.Tensor, target_lengths: torch.Tensor,
              blank: int = -1, clamp: float = -1.0, reduction: str = "mean",
              fused_log_softmax: bool = True) -> torch.Tensor:
    """RNN-Transducer loss with the arguments of ``torchaudio.functional.rnnt_loss``.

    ``logits``          ``(N, T, U, V)`` joint-network output, fp32, bf16 or fp16, contiguous, on the GPU.
    ``targets``         int32 ``(N, U-1)``, ``logit_lengths`` / ``target_lengths`` int32 ``(N,)``.
    ``blank``           index of the blank; negative counts from the end (``-1`` = ``V - 1``).
    ``clamp``           > 0: every cost's d/d logits are limited to ``[-clamp, +clamp]`` before the upstream gradient (the
                        reduction's ``1/N`` included) multiplies them.  ``<= 0``: off.
    ``reduction``       ``"none"`` -> ``(N,)`` costs, ``"mean"``, ``"sum"``.
    ``fused_log_softmax``  ``False``: the inputs are log-probabilities already; that route has no clamp.

    The costs are fp32 at every logits dtype and d/d logits come back in the logits' dtype (the fp32 result rounded once):
    this is this library's rule, stated rather than compared -- torchaudio returns costs in the logits' dtype.
    The argument checks are those of ``warp_rnnt_amd.fused.check_logits_inputs``."""
    check_reduction(reduction)
    blank = resolve_blank(blank, logits.shape[-1])
    clamp = resolve_clamp(clamp)
    if fused_log_softmax:
        from .fused import rnnt_loss_from_logits
        return rnnt_loss_from_logits(logits, targets, logit_lengths, target_lengths, reduction=reduction, blank=blank,
                                     clamp=clamp)
    if clamp > 0.0:
        raise ValueError("clamp needs fused_log_softmax=True: the gradient clamp lives on the fused path (logits in), "
                         "log-probabilities have no clamped route")
    import warp_rnnt
    return warp_rnnt.rnnt_loss(logits, targets, logit_lengths, target_lengths, reduction=reduction, gather=True,
                               blank=blank)


class RNNTLoss(torch.nn.Module):
    """Module form of :func:`rnnt_loss` (``torchaudio.transforms.RNNTLoss``; with ``blank=0`` the warp-transducer shape)."""

    def __init__(self, blank: int = -1, clamp: float = -1.0, reduction: str = "mean", fused_log_softmax: bool = True):
        super().__init__()
        self.blank = blank
        self.clamp = clamp
        self.reduction = reduction
        self.fused_log_softmax = fused_log_softmax

    def forward(self, logits, targets, logit_lengths, target_lengths):
        return rnnt_loss(logits, targets, logit_lengths, target_lengths, self.blank, self.clamp, self.reduction,
                         self.fused_log_softmax)
