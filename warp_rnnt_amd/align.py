"""Best-path (Viterbi) alignments from the lattice of the fused loss: where each label is emitted.

The loss sums over every path of the transducer lattice; :func:`rnnt_align` asks the same lattice for its single best
path.  The producers are the loss's own -- logits go through the fused log-softmax + gather (or the factorised-blank HAT
form), so the (N,T,U,V) log-probabilities never exist in memory -- and a max-plus sweep over the (blank, label) pair plane
replaces the alpha / beta sweeps (csrc/align.hip).  With ``b(t,u)``, ``l(t,u)`` the two log-probabilities of a cell, in
fp32, one add per edge and one compare per cell::

    v(0,0) = 0
    cb = v(t-1,u) + b(t-1,u)            (t > 0)
    cl = v(t,u-1) + l(t,u-1)            (u > 0)
    by_label(t,u) = u > 0 and (t == 0 or cl > cb)        a tie goes to the blank predecessor
    v(t,u) = cl if by_label(t,u) else cb
    score = v(T_n-1, U_n) + b(T_n-1, U_n)

The path is read back from ``(T_n-1, U_n)`` along ``by_label``; among all paths of maximal score this is the one whose
emit frames are smallest when compared from the last label to the first.  Token timestamps, emission-delay statistics
(what ``fastemit_lambda`` is tuned against), alignment-restricted training (:func:`alignment_mask`) and the "best path
against total likelihood" diagnostic ``score + cost <= 0`` come from here.
"""
import torch

from . import ops
from .fused import check_logits_inputs
from warp_rnnt import _C as _core

KINDS = ("logits", "hat_logits", "log_probs", "gathered")
_INPUT_KIND = {"logits": ops.IN_LOGITS_DENSE, "hat_logits": ops.ALIGN_IN_HAT_LOGITS, "log_probs": ops.IN_LOG_PROBS_DENSE,
               "gathered": ops.IN_LOG_PROBS_GATHERED}


def rnnt_align(inputs: torch.Tensor, labels: torch.Tensor, frames_lengths: torch.Tensor, labels_lengths: torch.Tensor,
               blank: int = 0, kind: str = "logits"):
    """The best path of every utterance: ``(scores, emit_frames)``.

    ``kind`` says what ``inputs`` holds: ``"logits"`` (N,T,U,V) in fp32, bf16 or fp16, read as ``rnnt_loss_from_logits``
    reads them; ``"hat_logits"`` the same, read as ``hat_loss_from_logits`` reads them (``V >= 2``); ``"log_probs"``
    (N,T,U,V) fp32 log-probabilities; ``"gathered"`` (N,T,U,2) fp32 pairs, channel 0 the blank's log-probability and
    channel 1 the label's (``labels`` and ``blank`` are then only checked for their shape).

    ``scores`` (N,) fp32 is the log-probability of the best path; ``emit_frames`` (N,U-1) int32 holds the frame at which
    label ``u`` is emitted, and -1 in the columns from ``labels_lengths[n]`` on.  An utterance whose lengths are outside
    ``[1,T]`` x ``[0,U-1]`` gets a NaN score and a row of -1.  Both are detached -- nothing flows back through an
    alignment.  Enqueue-only: the call can be captured into a graph."""
    assert isinstance(blank, int)
    if kind not in KINDS:
        raise ValueError(f"kind must be one of {KINDS}, not {kind!r}")
    with torch.no_grad():
        inputs = inputs.detach()
        if kind in ("logits", "hat_logits"):
            check_logits_inputs(inputs, labels, frames_lengths, labels_lengths)
        else:
            _core.check_inputs(inputs, labels, frames_lengths, labels_lengths)
            if kind == "gathered" and inputs.size(3) != 2:
                raise RuntimeError("xs must have values only for blank and label")
        return ops.align(inputs, labels, frames_lengths, labels_lengths, _INPUT_KIND[kind], blank)


def alignment_mask(emit_frames: torch.Tensor, frames_lengths: torch.Tensor, labels_lengths: torch.Tensor, T: int,
                   U: int) -> torch.Tensor:
    """The cells of the path as a bool tensor (N,T,U), from what :func:`rnnt_align` returned: column ``u <= U_n`` holds
    the frames from the emission of label ``u-1`` (frame 0 for ``u = 0``) to the emission of label ``u`` (frame ``T_n-1``
    for ``u = U_n``), ``T_n + U_n`` cells per utterance.  Plain torch on any device."""
    N = emit_frames.shape[0]
    dev = emit_frames.device
    frames = emit_frames.to(torch.int64)
    Tn = frames_lengths.to(device=dev, dtype=torch.int64).reshape(N, 1)
    Un = labels_lengths.to(device=dev, dtype=torch.int64).reshape(N, 1)
    edge = torch.zeros((N, 1), dtype=torch.int64, device=dev)
    u = torch.arange(U, device=dev).reshape(1, U)
    first = torch.cat([edge, frames], dim=1)                                  # (N,U): where the path enters column u
    last = torch.where(u < Un, torch.cat([frames, edge], dim=1), Tn - 1)      # (N,U): where it leaves it
    t = torch.arange(T, device=dev).reshape(1, T, 1)
    return (u <= Un).unsqueeze(1) & (t >= first.unsqueeze(1)) & (t <= last.unsqueeze(1))
