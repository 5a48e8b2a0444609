"""The joint network fused into the loss.

A training step of a transducer puts a joint network in front of the loss, ``z = Linear(H, V)(act(f_t + g_u))``.  Run
as written it materialises two (N,T,U,H) tensors -- ``f + g`` and its activation -- plus the (N,T,U,V) logits, and their
gradients.  :func:`rnnt_loss_from_joint` takes the joint's inputs instead and forms z tile by tile in HIP kernels
(MFMA), so none of those tensors ever exists: forward keeps the log-normaliser (two fp32: the row's maximum and the log of
the sum) and one gradient pair per lattice cell, 16 B in all, backward recomputes z (DESIGN.md
section 3.9).

Dropout between the activation and the projection (NeMo's ``RNNTJoint``: activation -> Dropout(p) -> Linear) acts on the
very tensor the fused path never forms, so it is applied inside the kernels (``dropout=``);
:class:`JointLoss` is the joint's projection and the loss as one module.
"""
import math
from typing import Optional

import torch

from . import _mismatch, ops
from .fused import finish_costs
from warp_rnnt import _C as _core


def check_joint_inputs(f, g, weight, bias, labels, xn, yn, activation, blank):
    """Shapes, dtypes and devices of :func:`rnnt_loss_from_joint`'s arguments, with the library's refusals."""
    for x, name in ((f, "f"), (g, "g"), (weight, "weight"), (labels, "labels"), (xn, "frames_lengths"),
                    (yn, "labels_lengths")):
        if not isinstance(x, torch.Tensor):
            raise RuntimeError(f"{name} must be a tensor")
    if activation not in ops.ACTIVATIONS:
        raise RuntimeError(f"activation must be one of {tuple(ops.ACTIVATIONS)}, not {activation!r}")
    if f.dtype not in ops.LOGITS_DTYPES:
        raise RuntimeError(f"f must be a float32, bfloat16 or float16 tensor, not {f.dtype}")
    if g.dtype != f.dtype:
        raise RuntimeError(f"f and g must share one dtype (f is {f.dtype}, g is {g.dtype})")
    for x, name in ((weight, "weight"), (bias, "bias")):
        if x is not None and x.dtype not in (torch.float32, f.dtype):
            raise RuntimeError(f"{name} must be float32 or the activations' dtype {f.dtype}, not {x.dtype}")
    for x, name in ((labels, "labels"), (xn, "frames_lengths"), (yn, "labels_lengths")):
        _core._check_int(x, name)
    if f.dim() != 3 or g.dim() != 3:
        raise RuntimeError("f must be (N,T,H) and g (N,U+1,H)")
    if weight.dim() != 2:
        raise RuntimeError("weight must be (V,H), the nn.Linear layout")
    N, T, H = f.shape
    V = weight.size(0)
    if g.size(0) != N or g.size(2) != H:
        raise RuntimeError(f"g must be (N,U+1,H) = ({N},U+1,{H}), not {tuple(g.shape)}")
    if weight.size(1) != H:
        raise RuntimeError(f"weight must be (V,H) with H={H}, not {tuple(weight.shape)}")
    if bias is not None and (bias.dim() != 1 or bias.size(0) != V):
        raise RuntimeError(f"bias must be (V,) = ({V},), not {tuple(bias.shape)}")
    if labels.dim() != 2 or labels.size(0) != N or labels.size(1) + 1 != g.size(1):
        raise RuntimeError(f"labels must be (N,U) with g of U+1 rows: labels {tuple(labels.shape)}, g {tuple(g.shape)}")
    if xn.dim() != 1 or yn.dim() != 1 or xn.size(0) != N or yn.size(0) != N:
        raise RuntimeError("frames_lengths and labels_lengths must be (N,)")
    if H % 32 != 0 or not 32 <= H <= 1024 or V < 2 or not 0 <= blank < V:
        raise RuntimeError("rnnt_loss status 5 (RNNT_STATUS_INVALID_ARGUMENT): the fused joint takes H % 32 == 0, "
                           f"32 <= H <= 1024, V >= 2 and 0 <= blank < V (H={H}, V={V}, blank={blank})")
    for x, name in ((f, "f"), (g, "g"), (weight, "weight"), (bias, "bias"), (labels, "labels"),
                    (xn, "frames_lengths"), (yn, "labels_lengths")):
        if x is not None:
            _core._check_cuda(x, name)
            if x.device != f.device:
                raise RuntimeError(f"{name} must be on the device of f ({f.device}), not {x.device}")


def _aligned(x):
    """x contiguous at a 16-byte aligned address, as the C entries require of f, g and weight (their kernels read
    16-byte fragments): a contiguous view at another offset (``buf[1:].view(...)``, a slice of a packed parameter) is
    cloned."""
    x = x.contiguous()
    return x if x.data_ptr() % 16 == 0 else x.clone()


def check_dropout(dropout):
    """The dropout probability as a float; outside [0, 1) (a NaN included) it is a ValueError."""
    p = float(dropout)
    if not 0.0 <= p < 1.0:
        raise ValueError(f"dropout must be in [0, 1), not {dropout!r}")
    return p


def draw_dropout_seed(device):
    """One int64 drawn over the whole int64 range by torch's generator of ``device``: torch.manual_seed reproduces it."""
    info = torch.iinfo(torch.int64)
    return torch.randint(info.min, info.max, (1,), dtype=torch.int64, device=device)


def resolve_dropout_seed(dropout_seed, device, capturing, draw=draw_dropout_seed):
    """The seed tensor of a call with dropout on: ``dropout_seed`` if given -- an int64 tensor of one element on
    ``device``; the kernels read it when they run, so under graph replay its contents at replay time decide the mask --
    else one drawn by ``draw(device)``.  A pure function of its arguments: ``capturing`` says whether the stream is being
    captured into a graph, where a drawn seed would be frozen into every replay and is refused."""
    if dropout_seed is None:
        if capturing:
            raise RuntimeError("rnnt_loss_from_joint with dropout under graph capture needs an explicit dropout_seed: a "
                               "seed drawn during capture would not change between replays; pass an int64 tensor of one "
                               "element and refresh it in place between replays")
        return draw(device)
    if not isinstance(dropout_seed, torch.Tensor):
        raise RuntimeError("dropout_seed must be a tensor (int64, one element, on the device of f)")
    if dropout_seed.dtype != torch.int64:
        raise RuntimeError(f"dropout_seed must be an int64 tensor, not {dropout_seed.dtype}")
    if dropout_seed.numel() != 1:
        raise RuntimeError(f"dropout_seed must hold one element, not {dropout_seed.numel()}")
    if dropout_seed.device != torch.device(device):
        raise RuntimeError(f"dropout_seed must be on the device of f ({device}), not {dropout_seed.device}")
    return dropout_seed


class RNNTLossFromJoint(torch.autograd.Function):

    @staticmethod
    def forward(ctx, f, g, weight, bias, labels, frames_lengths, labels_lengths, activation, blank, fastemit_lambda,
                with_grads, dropout=0.0, seed=None):
        fc, gc = _aligned(f), _aligned(g)
        w = _aligned(weight.to(fc.dtype))                        # W staged in the activations' dtype
        b = bias.to(torch.float32).contiguous() if bias is not None else None
        labels, xn, yn = labels.contiguous(), frames_lengths.contiguous(), labels_lengths.contiguous()
        costs, lse, grads = ops.joint_loss(fc, gc, w, b, labels, xn, yn, activation, blank, fastemit_lambda,
                                           with_grads, dropout, seed)
        if with_grads:
            ctx.save_for_backward(fc, gc, w, b, labels, xn, yn, lse, grads, seed)   # (the backward reads the same word)
        ctx.activation, ctx.blank, ctx.dropout = activation, blank, dropout
        ctx.weight_dtype = weight.dtype
        ctx.bias_dtype = bias.dtype if bias is not None else None
        return costs

    @staticmethod
    def backward(ctx, grads_output):
        f, g, w, b, labels, xn, yn, lse, grads, seed = ctx.saved_tensors
        _mismatch.poll(f.device)
        go = grads_output.reshape(-1).to(torch.float32).contiguous()
        need = ctx.needs_input_grad
        df, dg, dw, db = ops.joint_backward(f, g, w, b, labels, xn, yn, lse, grads, go, ctx.activation, ctx.blank,
                                            need[0], need[1], need[2], need[3] and b is not None, ctx.dropout, seed)
        if dw is not None:
            dw = dw.to(ctx.weight_dtype)
        if db is not None:
            db = db.to(ctx.bias_dtype)
        return (df, dg, dw, db) + (None,) * 9


def rnnt_loss_from_joint(f: torch.Tensor, g: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor],
                         labels: torch.Tensor, frames_lengths: torch.Tensor, labels_lengths: torch.Tensor,
                         activation: str = "tanh", average_frames: bool = False, reduction: Optional[str] = "none",
                         blank: int = 0, fastemit_lambda: float = 0.0, *, dropout: float = 0.0, training: bool = True,
                         dropout_seed: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The value of ``rnnt_loss_from_logits(z, labels, frames_lengths, labels_lengths, ...)`` with
    ``z[n,t,u] = weight @ act(f[n,t] + g[n,u]) + bias`` -- f (N,T,H), g (N,U+1,H), weight (V,H) (``nn.Linear.weight``),
    bias (V,) or None, act ``"tanh"`` or ``"relu"`` -- and gradients to f, g, weight and bias, without materialising an
    (N,T,U+1,H) or (N,T,U+1,V) tensor.

    f and g share one dtype (fp32, bf16 or fp16); weight and bias may be fp32 or that dtype (fp32 master weights under
    autocast).  act(f+g) is computed in fp32 and rounded to the activations' dtype as the matrix-core operand; the logits
    stay fp32.  Costs are fp32; d f and d g come back in the activations' dtype, d weight and d bias in their parameters'.
    Supported: H % 32 == 0, 32 <= H <= 1024, V >= 2.  Nothing is read back to the host: the call can be captured into a
    CUDA graph.

    ``dropout`` (in [0, 1); a ValueError otherwise) with ``training`` true puts ``Dropout(p)`` between the activation and
    the projection: z = weight @ (m * act(f + g) / (1 - p)) + bias, the mask m formed inside the kernels (Philox4x32-10
    keyed by the seed, counter (n, t, u, k >> 2): include/warp_rnnt_amd_joint_dropout.h) -- forward and backward see the
    same one.  ``dropout_seed`` is an int64 tensor of one element on f's device; None draws one with ``torch.randint`` on
    that device, which ``torch.manual_seed`` reproduces.  The kernels read the tensor when they run: under graph capture
    it must be given (a RuntimeError otherwise), and a training loop refreshes it in place between replays.  With
    ``training`` false or ``dropout`` 0 the call is the one without these arguments, bit for bit."""
    p = check_dropout(dropout)
    if not training:
        p = 0.0
    assert reduction is None or reduction in ("none", "mean", "sum")
    assert isinstance(blank, int)
    check_joint_inputs(f, g, weight, bias, labels, frames_lengths, labels_lengths, activation, blank)
    with_grads = torch.is_grad_enabled() and any(x is not None and x.requires_grad for x in (f, g, weight, bias))
    seed = None
    if p > 0:
        seed = resolve_dropout_seed(dropout_seed, f.device, torch.cuda.is_current_stream_capturing())
    costs = RNNTLossFromJoint.apply(f, g, weight, bias, labels, frames_lengths, labels_lengths, activation, blank,
                                    fastemit_lambda, with_grads, p, seed)
    return finish_costs(costs, frames_lengths, average_frames, reduction)


class JointLoss(torch.nn.Module):
    """The joint's projection and the transducer loss as one module -- ``activation -> Dropout(dropout) -> Linear(hidden,
    vocab) -> loss`` on :func:`rnnt_loss_from_joint`: it owns ``weight`` (vocab, hidden) and ``bias``, initialised as
    ``nn.Linear`` initialises them; ``self.training`` switches the dropout (``.eval()`` is the call without dropout)."""

    def __init__(self, hidden: int, vocab: int, activation: str = "tanh", dropout: float = 0.0, bias: bool = True,
                 blank: int = 0, fastemit_lambda: float = 0.0, reduction: Optional[str] = "mean"):
        super().__init__()
        if activation not in ops.ACTIVATIONS:
            raise ValueError(f"activation must be one of {tuple(ops.ACTIVATIONS)}, not {activation!r}")
        self.hidden, self.vocab, self.activation, self.dropout = hidden, vocab, activation, check_dropout(dropout)
        self.blank, self.fastemit_lambda, self.reduction = blank, fastemit_lambda, reduction
        self.weight = torch.nn.Parameter(torch.empty(vocab, hidden))
        self.bias = torch.nn.Parameter(torch.empty(vocab)) if bias else None
        self.reset_parameters()

    def reset_parameters(self):
        torch.nn.init.kaiming_uniform_(self.weight, a=math.sqrt(5))      # (nn.Linear.reset_parameters)
        if self.bias is not None:
            bound = 1 / math.sqrt(self.hidden) if self.hidden > 0 else 0
            torch.nn.init.uniform_(self.bias, -bound, bound)

    def forward(self, f, g, labels, frames_lengths, labels_lengths, dropout_seed=None):
        return rnnt_loss_from_joint(f, g, self.weight, self.bias, labels, frames_lengths, labels_lengths,
                                    activation=self.activation, reduction=self.reduction, blank=self.blank,
                                    fastemit_lambda=self.fastemit_lambda, dropout=self.dropout, training=self.training,
                                    dropout_seed=dropout_seed)

    def extra_repr(self):
        return (f"hidden={self.hidden}, vocab={self.vocab}, activation={self.activation!r}, dropout={self.dropout}, "
                f"bias={self.bias is not None}, blank={self.blank}, reduction={self.reduction!r}")
