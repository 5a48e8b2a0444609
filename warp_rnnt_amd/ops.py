"""Torch-tensor front ends of the native entry points (device memory + streams only)."""
import ctypes
import functools
import inspect
import os
import warnings

import torch

from . import _lib, _mismatch
from ._lib import (GRADS_DENSE, GRADS_GATHERED, GRADS_GATHERED_DIAGONAL, GRADS_NONE,  # noqa: F401
                   IN_LOG_PROBS_DENSE, IN_LOG_PROBS_GATHERED, IN_LOGITS_DENSE, STATUS_NAMES)

# element types the logits entries take (C ABI: RNNT_DTYPE_*); every other entry is fp32 only
LOGITS_DTYPES = {torch.float32: _lib.DTYPE_F32, torch.bfloat16: _lib.DTYPE_BF16, torch.float16: _lib.DTYPE_F16}


def _half(t):
    """True for bf16 / fp16 tensors: served by the typed entries (fp32 arithmetic from the load on)."""
    return t.dtype in (torch.bfloat16, torch.float16)


def _ptr(t):
    return 0 if t is None else t.data_ptr()


def _stream(device):
    return torch.cuda.current_stream(device).cuda_stream


def _check(status):
    if status != 0:
        # same text as the reference's TORCH_CHECK (binding.cpp:102-103)
        raise RuntimeError("rnnt_loss status " + str(status) +
                           " (" + STATUS_NAMES.get(status, "?") + ")")


def _workspace(dev, size_fn, names, *dims):
    """The uint8 workspace of ``size_fn(*dims)`` bytes; 0 = sizes the library does not take (``names``: the dims the
    message spells out)."""
    ws_bytes = size_fn(*dims)
    if ws_bytes == 0:
        raise RuntimeError("rnnt_loss status 5 (RNNT_STATUS_INVALID_ARGUMENT): unsupported sizes" +
                           "".join(f" {k}={v}" for k, v in zip(names.split(), dims)))
    return torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)


# ---- the blank column as a plane of its own ----
# log_softmax writes, beside the (N,T,U,V) log-probs, their column 0 -- the blank of every lattice cell -- as a contiguous
# (N*T*U,) plane and leaves a note on the tensor object it returns; a dense loss call that is handed that very object,
# unchanged, passes the plane on and its gather fetches one dword per row instead of two.  The note:
#   (plane, out._version, column, out.data_ptr())
PLANE_ATTR = "_rnnt_blank_plane"
PLANE_COLUMN = 0             # the column log_softmax keeps: the default blank
# Cells from which the plane is produced (DESIGN.md 3.5 has the numbers).  What it costs is fixed -- one more allocation
# and a second native argument, 3-5 us of host time per step -- and what it saves is one 128-byte line per cell at most,
# ~25 us per million cells at the gather's rate: from 2^20 cells on the saving is five times the cost.  Below it the step
# is launch-bound and gains nothing (c3, 96 k cells: within its spread either way).
PLANE_MIN_CELLS = 1 << 20


def wants_blank_plane(cells, V):
    """The one decision when log_softmax produces the plane -- a pure function of the shape (cells = N*T*U).  Never for
    rows that fit one 128-byte line (4V <= 128: blank and label share lines, nothing is saved), never below
    PLANE_MIN_CELLS (the extra store and the host cost would show on launch-bound steps)."""
    return 4 * V > 128 and cells >= PLANE_MIN_CELLS


def plane_note_valid(note, version, data_ptr, shape, dtype, contiguous, blank):
    """Does ``note`` (the PLANE_ATTR of a tensor) describe the tensor with these facts, for a loss with this blank?
    Pure: no tensor is touched."""
    if not (isinstance(note, tuple) and len(note) == 4):
        return False
    plane, note_version, column, note_ptr = note
    if note_version != version or note_ptr != data_ptr or column != blank:
        return False
    if len(shape) != 4 or dtype != torch.float32 or not contiguous:
        return False
    return plane is not None and plane.numel() == shape[0] * shape[1] * shape[2]


def blank_plane_of(log_probs, blank):
    """The blank plane that belongs to ``log_probs`` as it is now, or None: the note must sit on this very object (a view,
    a clone, a detach() carry none), and neither the tensor's version counter nor its storage may have moved."""
    note = getattr(log_probs, PLANE_ATTR, None)
    if note is None:
        return None
    if plane_note_valid(note, log_probs._version, log_probs.data_ptr(), tuple(log_probs.shape), log_probs.dtype,
                        log_probs.is_contiguous(), blank):
        return note[0]
    return None


def _drop_plane(t):
    """Before anything is enqueued that writes into ``t`` through its raw pointer: such a write does not move
    ``t._version``, so a note left on ``t`` would describe values that are gone."""
    if t is not None and getattr(t, PLANE_ATTR, None) is not None:
        delattr(t, PLANE_ATTR)


_LAST_LOSS_PLANE = False     # debug.last_loss_used_blank_plane(): did the last dense loss call of this process take a plane?


def _note_loss_plane(used):
    global _LAST_LOSS_PLANE
    _LAST_LOSS_PLANE = bool(used)


def _mismatch_policy():
    """WARP_RNNT_AMD_CHECK_MISMATCH = warn | raise: read the guard flags back after every loss call
    (one host synchronisation: exact and immediate).  Unset (default): no read-back; the counterpart of the
    reference's device-side WARNING printf (core_gather.cu:345-349) is the sticky per-device word the gradient kernel
    writes and _mismatch.poll() turns into a RuntimeWarning at the next call or backward.  off: neither."""
    return os.environ.get("WARP_RNNT_AMD_CHECK_MISMATCH", "").lower()


def loss(input, labels, xn, yn, input_kind, grads_kind, blank=0, fastemit_lambda=0.0, return_mismatch=False,
         use_blank_plane=True):
    """costs (N,), grads (layout per grads_kind; None for GRADS_NONE) [, mismatch (N,) int32].
    Dense log-probs that came out of :func:`log_softmax` with their blank plane (and are still what they were:
    :func:`blank_plane_of`) are served through it -- same bits, one line less read per cell; ``use_blank_plane=False``
    never looks for one.
    Tensors must be validated by the caller (contiguous, fp32/int32, same GPU; IN_LOGITS_DENSE also takes bf16 / fp16
    logits -- costs and gradient pairs stay fp32).  ``mismatch[n]`` is 1
    where the forward/backward consistency guard zeroed an utterance's gradients (or its lengths were
    out of range); without asking for it the same event surfaces as a RuntimeWarning a little later, with no
    synchronisation (warp_rnnt_amd/_mismatch.py)."""
    L = _lib.load()
    N, T, U, V = input.shape
    dev = input.device
    if input_kind == IN_LOG_PROBS_GATHERED:
        blank = 0          # channel 0 of the 2-channel layout; the caller's blank is -1 by convention
    elif not 0 <= blank < V:
        raise RuntimeError(f"rnnt_loss status 5 (RNNT_STATUS_INVALID_ARGUMENT): blank={blank} is not a "
                           f"vocabulary index of xs (V={V})")
    with torch.cuda.device(dev):
        costs = torch.empty((N,), dtype=torch.float32, device=dev)
        if grads_kind == GRADS_DENSE:
            grads = torch.empty_like(input)
        elif grads_kind == GRADS_NONE:
            grads = None
        else:
            grads = torch.empty((N, T, U, 2), dtype=torch.float32, device=dev)
        if N == 0:
            if return_mismatch:
                return costs, grads, torch.zeros((0,), dtype=torch.int32, device=dev)
            return costs, grads
        ws = _workspace(dev, L.rnnt_amd_workspace_size, "N T U", N, T, U)
        _mismatch.poll(dev)          # (what an EARLIER call's kernels reported; sets the device's words up at first use)
        plane = blank_plane_of(input, blank) if (use_blank_plane and input_kind == IN_LOG_PROBS_DENSE) else None
        if input_kind == IN_LOG_PROBS_DENSE:
            _note_loss_plane(plane is not None)
        if plane is not None:
            st = L.rnnt_amd_loss_blank_plane(_stream(dev), ws.data_ptr(), input.data_ptr(), plane.data_ptr(),
                                             _ptr(labels), xn.data_ptr(), yn.data_ptr(), costs.data_ptr(), _ptr(grads),
                                             grads_kind, N, T, U, V, blank, float(fastemit_lambda))
        elif input_kind == IN_LOGITS_DENSE and _half(input):
            st = L.rnnt_amd_loss_logits(_stream(dev), ws.data_ptr(), LOGITS_DTYPES[input.dtype], input.data_ptr(),
                                        _ptr(labels), xn.data_ptr(), yn.data_ptr(), costs.data_ptr(), _ptr(grads),
                                        grads_kind, N, T, U, V, blank, float(fastemit_lambda))
        else:
            st = L.rnnt_amd_loss(_stream(dev), ws.data_ptr(), input_kind, input.data_ptr(), _ptr(labels),
                                 xn.data_ptr(), yn.data_ptr(), costs.data_ptr(), _ptr(grads), grads_kind,
                                 N, T, U, V, blank, float(fastemit_lambda))
        _check(st)
        policy = _mismatch_policy()
        if policy not in ("warn", "raise", "1", "on"):
            policy = ""
        if return_mismatch or policy:
            off = L.rnnt_amd_workspace_mismatch_offset(N, T, U)
            mismatch = ws[off:off + 4 * N].view(torch.int32).clone()
            if policy:
                bad = mismatch.nonzero().flatten().tolist()      # host synchronisation (opt-in)
                if bad:
                    msg = (f"rnnt_loss: forward/backward mismatch or invalid lengths for utterance(s) {bad}: "
                           "their gradients are zero (core_gather.cu:341-354)")
                    if policy == "raise":
                        raise RuntimeError(msg)
                    warnings.warn(msg, RuntimeWarning, stacklevel=2)
            if return_mismatch:
                return costs, grads, mismatch
    return costs, grads


def expand_grads(grads_diagonal, labels, xn, yn, grad_costs, V, blank, overwrite=False):
    """Dense (N,T,U,V) d/d log_probs from diagonal-major gathered grads, scaled per utterance."""
    L = _lib.load()
    N, T, U, _ = grads_diagonal.shape
    dev = grads_diagonal.device
    with torch.cuda.device(dev):
        out = torch.empty((N, T, U, V), dtype=torch.float32, device=dev)
        if N == 0:
            return out
        st = L.rnnt_amd_expand_grads(_stream(dev), grads_diagonal.data_ptr(), _ptr(labels), xn.data_ptr(),
                                     yn.data_ptr(), _ptr(grad_costs), out.data_ptr(), N, T, U, V, blank,
                                     1 if overwrite else 0)
        _check(st)
    return out


def _native_binding():
    """warp_rnnt._C_native when it has been built (one compiled call instead of ctypes marshalling)."""
    global _NATIVE
    if _NATIVE is False:
        try:
            from warp_rnnt import _C as _wc
            _NATIVE = _wc._native
        except ImportError:
            _NATIVE = None
    return _NATIVE


_NATIVE = False


def log_softmax(x, out=None, blank_plane=None):
    """Row-wise log-softmax over the last axis (contiguous, GPU). ``out`` may be ``x``.  fp32 in, fp32 out; bf16 / fp16
    in, fp32 out (bit-equal to the fp32 call on ``x.float()``; ``out`` must then be a separate fp32 tensor).
    For fp32 (N,T,U,V) input the kernel can keep column 0 of the result as a plane beside it, for the loss to read
    (PLANE_ATTR above): ``blank_plane=None`` where :func:`wants_blank_plane` says so, ``True`` / ``False`` always / never
    (tests, timing runs).  The returned tensor is the same either way."""
    _drop_plane(out)
    if _half(x):
        return _log_softmax_half(x, out)
    planed = x.dim() == 4 and x.numel() > 0 and (
        wants_blank_plane(x.shape[0] * x.shape[1] * x.shape[2], x.shape[3]) if blank_plane is None else bool(blank_plane))
    nb = _native_binding()
    if nb is not None:
        if not planed:
            return nb.log_softmax(x, out)
        res, plane = nb.log_softmax_plane(x, out, PLANE_COLUMN)
        out = res if out is None else out
    else:
        L = _lib.load()
        assert x.is_cuda and x.dtype == torch.float32 and x.is_contiguous()
        if out is None:
            out = torch.empty_like(x)
        V = x.shape[-1]
        rows = x.numel() // max(V, 1)
        with torch.cuda.device(x.device):
            if not planed:
                _check(L.rnnt_amd_log_softmax(_stream(x.device), x.data_ptr(), out.data_ptr(), rows, V))
                return out
            plane = torch.empty((rows,), dtype=torch.float32, device=x.device)
            _check(L.rnnt_amd_log_softmax_plane(_stream(x.device), x.data_ptr(), out.data_ptr(), plane.data_ptr(), rows,
                                                V, PLANE_COLUMN))
    setattr(out, PLANE_ATTR, (plane, out._version, PLANE_COLUMN, out.data_ptr()))
    return out


def _log_softmax_half(x, out=None):
    L = _lib.load()
    _drop_plane(out)
    if not (x.is_cuda and x.is_contiguous()):
        raise RuntimeError("log_softmax: x must be a contiguous tensor on the GPU")
    if out is None:
        out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    if not (out.is_contiguous() and out.dtype == torch.float32 and out.shape == x.shape and out.device == x.device):
        raise RuntimeError("log_softmax: out must be a contiguous float32 tensor like x (bf16 / fp16 input)")
    V = x.shape[-1] if x.dim() else 1
    rows = x.numel() // max(V, 1)
    with torch.cuda.device(x.device):
        _check(L.rnnt_amd_log_softmax_typed(_stream(x.device), LOGITS_DTYPES[x.dtype], x.data_ptr(), out.data_ptr(),
                                            rows, V))
    return out


def gather(log_probs, labels, blank=0):
    """(N,T,U,V) -> (N,T,U,2) [blank, label] pairs (row-major), as the reference wrapper builds them."""
    L = _lib.load()
    N, T, U, V = log_probs.shape
    out = torch.empty((N, T, U, 2), dtype=torch.float32, device=log_probs.device)
    with torch.cuda.device(log_probs.device):
        _check(L.rnnt_amd_gather(_stream(log_probs.device), log_probs.data_ptr(), _ptr(labels),
                                 out.data_ptr(), N, T, U, V, blank))
    return out


def _bounds_given(max_frames, max_labels):
    if (max_frames is None) != (max_labels is None):
        raise ValueError("max_frames and max_labels go together")
    return max_frames is not None


def _bounded_workspace(L, dev, N, STU, max_frames, max_labels):
    """(workspace, Tmax, Umax) of a compact call with the caller's bounds."""
    tmax, umax = int(max_frames), int(max_labels) + 1
    if tmax < 1 or umax < 1:
        raise ValueError("max_frames >= 1 and max_labels >= 0 expected")
    return _workspace(dev, L.rnnt_amd_workspace_size_compact_bounded, "", N, STU, tmax, umax), tmax, umax


def _compact_offsets(L, dev, xn, yn, N, offs, loffs):
    """Enqueues the offsets of a compact batch into offs (N+1 offsets + the 4 stats) and loffs."""
    _check(L.rnnt_amd_compact_offsets(_stream(dev), xn.data_ptr(), yn.data_ptr(), N, offs.data_ptr(),
                                      loffs.data_ptr(), offs[N + 1:].data_ptr()))


def _sized_workspace(L, dev, ys, xn, yn, N, STU, offs, loffs):
    """(workspace, Tmax, Umax) of a compact call without bounds: the offsets, the one host synchronisation for the
    maxima and sums, the shape checks of the reference's binding."""
    _compact_offsets(L, dev, xn, yn, N, offs, loffs)
    stats = offs[N + 1:].tolist()                                       # the one host sync
    stu_chk, su, tmax, umax = int(stats[0]), int(stats[1]), int(stats[2]), int(stats[3]) + 1
    if ys.numel() != su:
        raise RuntimeError("ys shape must be equal to (sum(yn), )")
    if STU != stu_chk:
        raise RuntimeError("xs shape mismatch with (\\sum{xn*(yn+1)}, )")
    return _workspace(dev, L.rnnt_amd_workspace_size_compact, "", N, STU, tmax, umax), tmax, umax


def loss_compact(xs, ys, xn, yn, blank=0, fastemit_lambda=0.0, required_grad=True, max_frames=None, max_labels=None):
    """Compact (ragged packed) layout: xs (STU,V), ys (sum yn,), xn/yn (N,).
    Returns (costs (N,), grads (STU,2) or None, loc (STU,) int64).

    Without bounds: one host synchronisation (the maxima of the lengths size the launches, and the shape checks of the
    reference's binding need the sums; the reference does four).  With ``max_frames >= max(xn)`` and ``max_labels >=
    max(yn)`` supplied by the caller: none -- offsets, maxima and checks stay on the device (``rnnt_amd_loss_compact_
    bounded``), the call can be captured into a HIP graph; a batch that does not fit the bounds or the tensors' sizes
    comes back with NaN costs and zero gradients instead of an exception."""
    L = _lib.load()
    dev = xs.device
    N = xn.shape[0]
    STU, V = xs.shape
    bounded = _bounds_given(max_frames, max_labels)
    _mismatch.poll(dev)
    with torch.cuda.device(dev):
        costs = torch.empty((N,), dtype=torch.float32, device=dev)
        loc = torch.empty((STU,), dtype=torch.int64, device=dev)
        grads = torch.empty((STU, 2), dtype=torch.float32, device=dev) if required_grad else None
        if N == 0:
            return costs, grads, loc
        if bounded:
            ws, tmax, umax = _bounded_workspace(L, dev, N, STU, max_frames, max_labels)
            _check(L.rnnt_amd_loss_compact_bounded(_stream(dev), ws.data_ptr(), xs.data_ptr(), _ptr(ys), ys.numel(),
                                                   xn.data_ptr(), yn.data_ptr(), costs.data_ptr(), _ptr(grads),
                                                   loc.data_ptr(), N, STU, tmax, umax, V, blank, float(fastemit_lambda)))
            return costs, grads, loc
        offs = torch.empty((N + 1 + 4,), dtype=torch.int64, device=dev)    # offsets + the 4 stats
        loffs = torch.empty((N + 1,), dtype=torch.int32, device=dev)
        ws, tmax, umax = _sized_workspace(L, dev, ys, xn, yn, N, STU, offs, loffs)
        _check(L.rnnt_amd_loss_compact(_stream(dev), ws.data_ptr(), xs.data_ptr(), _ptr(ys), xn.data_ptr(),
                                       yn.data_ptr(), offs.data_ptr(), loffs.data_ptr(), costs.data_ptr(),
                                       _ptr(grads), loc.data_ptr(), N, STU, tmax, umax, V, blank,
                                       float(fastemit_lambda)))
    return costs, grads, loc


def loss_compact_logits(logits, ys, xn, yn, blank=0, fastemit_lambda=0.0, required_grad=True, max_frames=None,
                        max_labels=None):
    """The fused path on the compact layout: logits (STU,V) fp32 / bf16 / fp16, ys (sum yn,), xn/yn (N,).
    Returns (costs (N,) fp32, grads (STU,2) row-major fp32 or None, cell_offsets (N+1,) int64, label_offsets (N+1,)
    int32) -- the offsets are what :func:`compact_logits_backward` needs.  Host synchronisations as
    :func:`loss_compact`: one without bounds, none with them (the offsets for the backward are then enqueued too)."""
    L = _lib.load()
    dev = logits.device
    N = xn.shape[0]
    STU, V = logits.shape
    bounded = _bounds_given(max_frames, max_labels)
    if not 0 <= blank < V:
        raise RuntimeError("rnnt_loss status 5 (RNNT_STATUS_INVALID_ARGUMENT): unsupported sizes or blank")
    dtype = LOGITS_DTYPES[logits.dtype]
    _mismatch.poll(dev)
    with torch.cuda.device(dev):
        costs = torch.empty((N,), dtype=torch.float32, device=dev)
        grads = torch.empty((STU, 2), dtype=torch.float32, device=dev) if required_grad else None
        offs = torch.empty((N + 1 + 4,), dtype=torch.int64, device=dev)    # offsets + the 4 stats
        loffs = torch.empty((N + 1,), dtype=torch.int32, device=dev)
        if N == 0:
            return costs, grads, offs[:N + 1], loffs
        if bounded:
            ws, tmax, umax = _bounded_workspace(L, dev, N, STU, max_frames, max_labels)
            _check(L.rnnt_amd_loss_compact_logits_bounded(
                _stream(dev), ws.data_ptr(), dtype, logits.data_ptr(), _ptr(ys), ys.numel(), xn.data_ptr(),
                yn.data_ptr(), costs.data_ptr(), _ptr(grads), N, STU, tmax, umax, V, blank, float(fastemit_lambda)))
            if required_grad:          # (enqueued only: the backward's offsets)
                _compact_offsets(L, dev, xn, yn, N, offs, loffs)
            return costs, grads, offs[:N + 1], loffs
        ws, tmax, umax = _sized_workspace(L, dev, ys, xn, yn, N, STU, offs, loffs)
        _check(L.rnnt_amd_loss_compact_logits(_stream(dev), ws.data_ptr(), dtype, logits.data_ptr(), _ptr(ys),
                                              xn.data_ptr(), yn.data_ptr(), offs.data_ptr(), loffs.data_ptr(),
                                              costs.data_ptr(), _ptr(grads), N, STU, tmax, umax, V, blank,
                                              float(fastemit_lambda)))
    return costs, grads, offs[:N + 1], loffs


def compact_logits_backward(logits, ys, xn, yn, cell_offsets, label_offsets, grads, grad_costs, blank=0, out=None,
                            clamp=0.0):
    """d(sum_n grad_costs[n]*cost[n]) / d(logits) (STU,V) for the compact fused path, in the logits' dtype; grads and the
    offsets are those :func:`loss_compact_logits` returned.  Rows that belong to no utterance come back zero.
    ``clamp`` > 0: as in :func:`logits_backward`."""
    L = _lib.load()
    STU, V = logits.shape
    N = xn.shape[0]
    dev = logits.device
    with torch.cuda.device(dev):
        if out is None:
            out = torch.empty_like(logits)
        if out.dtype != logits.dtype or out.shape != logits.shape or not out.is_contiguous():
            raise RuntimeError("compact_logits_backward: out must be a contiguous tensor like the logits")
        _drop_plane(out)
        if STU == 0:
            return out
        args = (_stream(dev), LOGITS_DTYPES[logits.dtype], logits.data_ptr(), _ptr(ys), ys.numel(), xn.data_ptr(),
                yn.data_ptr(), cell_offsets.data_ptr(), label_offsets.data_ptr(), grads.data_ptr(), _ptr(grad_costs),
                out.data_ptr(), N, STU, V, blank)
        if clamp == 0.0:
            _check(L.rnnt_amd_compact_logits_backward(*args))
        else:
            _check(L.rnnt_amd_compact_logits_backward_clamped(*args, float(clamp)))
    return out


def compact_scatter_grads(grad_cost, grad_xs, cum_lens, loc, V, blank):
    """(STU,V) gradient rows from the (STU,2) pairs (reference: rnnt_loss_compact_backward)."""
    L = _lib.load()
    dev = grad_xs.device
    STU = grad_xs.shape[0]
    N = grad_cost.shape[0]
    with torch.cuda.device(dev):
        out = torch.empty((STU, V), dtype=torch.float32, device=dev)
        if STU == 0:
            return out
        _check(L.rnnt_amd_compact_scatter_grads(_stream(dev), grad_cost.data_ptr(), grad_xs.data_ptr(),
                                                loc.data_ptr(), cum_lens.data_ptr(), out.data_ptr(), STU, N,
                                                int(V), int(blank)))
    return out


def logits_backward(logits, labels, grads_diagonal, grad_costs, blank=0, out=None, clamp=0.0):
    """d(sum_n grad_costs[n]*cost[n]) / d(logits) for the fused RNNT_IN_LOGITS_DENSE path, in the logits' dtype (fp32,
    bf16 or fp16: the fp32 result rounded once).  ``clamp`` > 0: the gradient of every cost is limited to
    [-clamp, +clamp] elementwise BEFORE it is multiplied by grad_costs (the clamp of torchaudio and warp-transducer;
    include/warp_rnnt_amd_clamp.h); 0.0 calls the unclamped entries."""
    L = _lib.load()
    N, T, U, V = logits.shape
    dev = logits.device
    with torch.cuda.device(dev):
        if out is None:
            out = torch.empty_like(logits)
        _drop_plane(out)
        if N == 0:
            return out
        if clamp != 0.0:
            if out.dtype != logits.dtype:
                raise RuntimeError("logits_backward: out must have the logits' dtype")
            _check(L.rnnt_amd_logits_backward_clamped(_stream(dev), LOGITS_DTYPES[logits.dtype], logits.data_ptr(),
                                                      _ptr(labels), grads_diagonal.data_ptr(), _ptr(grad_costs),
                                                      out.data_ptr(), N, T, U, V, blank, float(clamp)))
        elif _half(logits):
            if out.dtype != logits.dtype:
                raise RuntimeError("logits_backward: out must have the logits' dtype")
            _check(L.rnnt_amd_logits_backward_typed(_stream(dev), LOGITS_DTYPES[logits.dtype], logits.data_ptr(),
                                                    _ptr(labels), grads_diagonal.data_ptr(), _ptr(grad_costs),
                                                    out.data_ptr(), N, T, U, V, blank))
        else:
            _check(L.rnnt_amd_logits_backward(_stream(dev), logits.data_ptr(), _ptr(labels),
                                              grads_diagonal.data_ptr(), _ptr(grad_costs), out.data_ptr(),
                                              N, T, U, V, blank))
    return out


def log_softmax_backward(grad_out, out, grad_in=None):
    """grad_in = grad_out - exp(out) * rowsum(grad_out) (rows = everything but the last axis)."""
    L = _lib.load()
    assert grad_out.is_cuda and grad_out.dtype == torch.float32 and grad_out.is_contiguous()
    assert out.is_contiguous() and out.shape == grad_out.shape and out.dtype == torch.float32
    if grad_in is None:
        grad_in = torch.empty_like(grad_out)
    _drop_plane(grad_in)
    V = out.shape[-1]
    rows = out.numel() // max(V, 1)
    with torch.cuda.device(out.device):
        _check(L.rnnt_amd_log_softmax_backward(_stream(out.device), grad_out.data_ptr(), out.data_ptr(),
                                               grad_in.data_ptr(), rows, V))
    return grad_in


ACTIVATIONS = {"tanh": _lib.ACT_TANH, "relu": _lib.ACT_RELU}


def _dropout_args(dropout, seed):
    """(p, seed pointer) of the *_dropout entries: seed an int64 tensor of one element on the device, read by the kernels
    when they run."""
    if seed is None or seed.dtype != torch.int64 or seed.numel() != 1:
        raise RuntimeError("dropout > 0 needs seed: an int64 tensor of one element on the device of f")
    return float(dropout), seed.data_ptr()


def joint_loss(f, g, weight, bias, labels, xn, yn, activation="tanh", blank=0, fastemit_lambda=0.0, with_grads=True,
               dropout=0.0, seed=None):
    """The joint network fused into the loss: f (N,T,H), g (N,U,H), weight (V,H) of one dtype (fp32 / bf16 / fp16),
    bias (V,) fp32 or None; validated by the caller.  Returns costs (N,) fp32 and, with_grads, lse (N,T,U,2) fp32 -- the
    log-normaliser of every cell as (max, log sum of exp(z - max)), never added up in fp32 -- and the
    gradient pairs (N,T,U,2) in the diagonal-major layout -- what :func:`joint_backward` reads (else None, None).
    dropout > 0: dropout between the activation and the projection, the mask a function of ``seed`` (an int64 tensor of
    one element on the device, read at run time) -- include/warp_rnnt_amd_joint_dropout.h; hand :func:`joint_backward` the
    same two."""
    L = _lib.load()
    N, T, H = f.shape
    U = g.shape[1]
    V = weight.shape[0]
    dev = f.device
    _mismatch.poll(dev)
    with torch.cuda.device(dev):
        costs = torch.empty((N,), dtype=torch.float32, device=dev)
        lse = torch.empty((N, T, U, 2), dtype=torch.float32, device=dev) if with_grads else None
        grads = torch.empty((N, T, U, 2), dtype=torch.float32, device=dev) if with_grads else None
        if N == 0:
            return costs, lse, grads
        ws = _workspace(dev, L.rnnt_amd_joint_workspace_size, "N T U H V", N, T, U, H, V)
        args = (_stream(dev), ws.data_ptr(), LOGITS_DTYPES[f.dtype], ACTIVATIONS[activation], f.data_ptr(), g.data_ptr(),
                weight.data_ptr(), _ptr(bias), _ptr(labels), xn.data_ptr(), yn.data_ptr(), costs.data_ptr(), _ptr(lse),
                _ptr(grads), N, T, U, H, V, blank, float(fastemit_lambda))
        if dropout > 0:
            _check(L.rnnt_amd_joint_loss_dropout(*args, *_dropout_args(dropout, seed)))
        else:
            _check(L.rnnt_amd_joint_loss(*args))
    return costs, lse, grads


def joint_backward(f, g, weight, bias, labels, xn, yn, lse, grads, grad_costs, activation="tanh", blank=0,
                   need_f=True, need_g=True, need_weight=True, need_bias=True, dropout=0.0, seed=None):
    """d(sum_n grad_costs[n]*cost[n]) / d(f, g, weight, bias) of :func:`joint_loss`: df / dg in f's dtype, dweight /
    dbias fp32; None for what is not asked for.  dropout, seed: those of the forward."""
    L = _lib.load()
    N, T, H = f.shape
    U = g.shape[1]
    V = weight.shape[0]
    dev = f.device
    with torch.cuda.device(dev):
        df = torch.empty_like(f) if need_f else None
        dg = torch.empty_like(g) if need_g else None
        dw = torch.empty((V, H), dtype=torch.float32, device=dev) if need_weight else None
        db = torch.empty((V,), dtype=torch.float32, device=dev) if (need_bias and bias is not None) else None
        if N == 0:
            for t in (df, dg, dw, db):
                if t is not None:
                    t.zero_()
            return df, dg, dw, db
        ws = _workspace(dev, L.rnnt_amd_joint_workspace_size, "N T U H V", N, T, U, H, V)
        args = (_stream(dev), ws.data_ptr(), LOGITS_DTYPES[f.dtype], ACTIVATIONS[activation], f.data_ptr(), g.data_ptr(),
                weight.data_ptr(), _ptr(bias), _ptr(labels), xn.data_ptr(), yn.data_ptr(), lse.data_ptr(),
                grads.data_ptr(), _ptr(grad_costs), _ptr(df), _ptr(dg), _ptr(dw), _ptr(db), N, T, U, H, V, blank)
        if dropout > 0:
            _check(L.rnnt_amd_joint_backward_dropout(*args, *_dropout_args(dropout, seed)))
        else:
            _check(L.rnnt_amd_joint_backward(*args))
    return df, dg, dw, db


def hat_loss(logits, labels, xn, yn, blank=0, fastemit_lambda=0.0, with_grads=True):
    """The factorised-blank (HAT) loss on the fused path (include/warp_rnnt_amd_hat.h): logits (N,T,U,V) fp32 / bf16 /
    fp16, validated by the caller.  Returns costs (N,) fp32 and, with_grads, the gradient pairs (N,T,U,2) fp32 in the
    diagonal-major layout -- what :func:`hat_logits_backward` reads (else None)."""
    L = _lib.load()
    N, T, U, V = logits.shape
    dev = logits.device
    if V < 2 or not 0 <= blank < V:
        raise RuntimeError(f"rnnt_loss status 5 (RNNT_STATUS_INVALID_ARGUMENT): the HAT loss needs V >= 2 and a blank "
                           f"that is a vocabulary index (V={V}, blank={blank})")
    _mismatch.poll(dev)
    with torch.cuda.device(dev):
        costs = torch.empty((N,), dtype=torch.float32, device=dev)
        grads = torch.empty((N, T, U, 2), dtype=torch.float32, device=dev) if with_grads else None
        if N == 0:
            return costs, grads
        ws = _workspace(dev, L.rnnt_amd_workspace_size, "N T U", N, T, U)
        _check(L.rnnt_amd_hat_loss_logits(_stream(dev), ws.data_ptr(), LOGITS_DTYPES[logits.dtype], logits.data_ptr(),
                                          _ptr(labels), xn.data_ptr(), yn.data_ptr(), costs.data_ptr(), _ptr(grads),
                                          N, T, U, V, blank, float(fastemit_lambda)))
    return costs, grads


def hat_logits_backward(logits, labels, grads, grad_costs, blank=0):
    """d(sum_n grad_costs[n]*cost[n]) / d(logits) of :func:`hat_loss`, in the logits' dtype (the fp32 result rounded
    once); grads: the pairs the forward returned."""
    L = _lib.load()
    N, T, U, V = logits.shape
    dev = logits.device
    with torch.cuda.device(dev):
        out = torch.empty_like(logits)
        if N == 0:
            return out
        _check(L.rnnt_amd_hat_logits_backward(_stream(dev), LOGITS_DTYPES[logits.dtype], logits.data_ptr(), _ptr(labels),
                                              grads.data_ptr(), _ptr(grad_costs), out.data_ptr(), N, T, U, V, blank))
    return out


def _pruned_check(S, U, V, blank):
    if V < 2 or not 0 <= blank < V or not 1 <= S <= U:
        raise RuntimeError(f"rnnt_loss status 5 (RNNT_STATUS_INVALID_ARGUMENT): the pruned loss needs V >= 2, a blank that "
                           f"is a vocabulary index and a band of 1 <= S <= U positions (V={V}, blank={blank}, S={S}, U={U})")


def pruned_loss(logits, labels, starts, xn, yn, blank=0, fastemit_lambda=0.0, with_grads=True):
    """The pruned transducer loss on the fused path (include/warp_rnnt_amd_pruned.h): logits (N,T,S,V) fp32 / bf16 / fp16,
    labels (N,U-1), starts (N,T) int32 contiguous, validated by the caller.  Returns costs (N,) fp32 -- >= 1e29 for an
    utterance whose band holds no path -- and, with_grads, the gradient pairs (N,T,U,2) fp32 of the whole lattice in the
    diagonal-major layout -- what :func:`pruned_logits_backward` reads (else None)."""
    L = _lib.load()
    N, T, S, V = logits.shape
    U = labels.shape[1] + 1
    dev = logits.device
    _pruned_check(S, U, V, blank)
    _mismatch.poll(dev)
    with torch.cuda.device(dev):
        costs = torch.empty((N,), dtype=torch.float32, device=dev)
        grads = torch.empty((N, T, U, 2), dtype=torch.float32, device=dev) if with_grads else None
        if N == 0:
            return costs, grads
        ws = _workspace(dev, L.rnnt_amd_workspace_size, "N T U", N, T, U)
        _check(L.rnnt_amd_pruned_loss_logits(_stream(dev), ws.data_ptr(), LOGITS_DTYPES[logits.dtype], logits.data_ptr(),
                                             _ptr(labels), starts.data_ptr(), xn.data_ptr(), yn.data_ptr(),
                                             costs.data_ptr(), _ptr(grads), N, T, U, S, V, blank, float(fastemit_lambda)))
    return costs, grads


def pruned_logits_backward(logits, labels, starts, grads, grad_costs, blank=0):
    """d(sum_n grad_costs[n]*cost[n]) / d(logits) of :func:`pruned_loss`, (N,T,S,V) in the logits' dtype (the fp32 result
    rounded once); grads: the pairs the forward returned.  An utterance with grad_costs[n] == 0 gets exactly zero rows
    whatever its pairs hold."""
    L = _lib.load()
    N, T, S, V = logits.shape
    U = labels.shape[1] + 1
    dev = logits.device
    with torch.cuda.device(dev):
        out = torch.empty_like(logits)
        if N == 0:
            return out
        _check(L.rnnt_amd_pruned_logits_backward(_stream(dev), LOGITS_DTYPES[logits.dtype], logits.data_ptr(), _ptr(labels),
                                                 starts.data_ptr(), grads.data_ptr(), _ptr(grad_costs), out.data_ptr(),
                                                 N, T, U, S, V, blank))
    return out


def _simple_check(V, blank, lm_only_scale, am_only_scale, q):
    """The refusals of include/warp_rnnt_amd_simple.h that depend on values, with their reasons spelt out; returns the
    two scales as the fp32 values the C entries receive."""
    if V < 2 or not 0 <= blank < V:
        raise RuntimeError(f"rnnt_loss status 5 (RNNT_STATUS_INVALID_ARGUMENT): the simple loss needs V >= 2 and a blank "
                           f"that is a vocabulary index (V={V}, blank={blank})")
    c1, c2 = ctypes.c_float(lm_only_scale).value, ctypes.c_float(am_only_scale).value
    if not (c1 >= 0.0 and c2 >= 0.0 and ctypes.c_float(c1 + c2).value <= 1.0):          # (false for a NaN)
        raise RuntimeError(f"rnnt_loss status 5 (RNNT_STATUS_INVALID_ARGUMENT): the simple loss needs finite scales "
                           f"lm_only_scale >= 0, am_only_scale >= 0 with a sum of at most 1 "
                           f"(lm_only_scale={lm_only_scale}, am_only_scale={am_only_scale})")
    if c2 != 0.0 and q is None:
        raise RuntimeError("rnnt_loss status 5 (RNNT_STATUS_INVALID_ARGUMENT): am_only_scale != 0 needs the log unigram q")
    return c1, c2


def simple_loss(am, lm, q, labels, xn, yn, blank=0, lm_only_scale=0.0, am_only_scale=0.0, fastemit_lambda=0.0,
                with_grads=True):
    """The smoothed simple loss (include/warp_rnnt_amd_simple.h): am (N,T,V) and lm (N,U,V) fp32 / bf16 / fp16 of one
    dtype, q (V,) fp32 or None, labels (N,U-1), validated by the caller.  Returns costs (N,) fp32 and, with_grads, the
    gradient pairs d cost / d pair (N,T,U,2) fp32 row-major and the normaliser plane (N,T,U) fp32 -- what
    :func:`simple_backward` reads (else None, None)."""
    L = _lib.load()
    N, T, V = am.shape
    U = lm.shape[1]
    dev = am.device
    c1, c2 = _simple_check(V, blank, lm_only_scale, am_only_scale, q)
    _mismatch.poll(dev)
    with torch.cuda.device(dev):
        costs = torch.empty((N,), dtype=torch.float32, device=dev)
        grads = torch.empty((N, T, U, 2), dtype=torch.float32, device=dev) if with_grads else None
        znorm = torch.empty((N, T, U), dtype=torch.float32, device=dev) if with_grads else None
        if N == 0:
            return costs, grads, znorm
        ws = _workspace(dev, L.rnnt_amd_simple_workspace_size, "N T U", N, T, U)
        _check(L.rnnt_amd_simple_loss(_stream(dev), ws.data_ptr(), LOGITS_DTYPES[am.dtype], am.data_ptr(), lm.data_ptr(),
                                      _ptr(q), _ptr(labels), xn.data_ptr(), yn.data_ptr(), costs.data_ptr(), _ptr(grads),
                                      _ptr(znorm), N, T, U, V, blank, c1, c2, float(fastemit_lambda)))
    return costs, grads, znorm


def simple_backward(am, lm, q, labels, xn, yn, grads, znorm, grad_costs, blank=0, lm_only_scale=0.0, am_only_scale=0.0):
    """d(sum_n grad_costs[n]*cost[n]) / d am, / d lm of :func:`simple_loss` in the inputs' dtype (the fp32 result rounded
    once) and, with am_only_scale != 0, / d q (V,) fp32 with lm held fixed (else None); grads, znorm: what the forward
    returned."""
    L = _lib.load()
    N, T, V = am.shape
    U = lm.shape[1]
    dev = am.device
    c1, c2 = _simple_check(V, blank, lm_only_scale, am_only_scale, q)
    with torch.cuda.device(dev):
        dam, dlm = torch.empty_like(am), torch.empty_like(lm)
        parts = torch.empty((N, V), dtype=torch.float32, device=dev) if c2 != 0.0 else None
        if N == 0:
            return dam, dlm, None if parts is None else parts.sum(0)
        ws = _workspace(dev, L.rnnt_amd_simple_workspace_size, "N T U", N, T, U)
        _check(L.rnnt_amd_simple_backward(_stream(dev), ws.data_ptr(), LOGITS_DTYPES[am.dtype], am.data_ptr(),
                                          lm.data_ptr(), _ptr(q), _ptr(labels), xn.data_ptr(), yn.data_ptr(),
                                          grads.data_ptr(), znorm.data_ptr(), _ptr(grad_costs), dam.data_ptr(),
                                          dlm.data_ptr(), _ptr(parts), N, T, U, V, blank, c1, c2))
    return dam, dlm, None if parts is None else parts.sum(0)


RNNT_TYPES = {"regular": _lib.TOPOLOGY_REGULAR, "modified": _lib.TOPOLOGY_MODIFIED}


def topology_of(rnnt_type, delay_penalty):
    """(topology, delay_penalty as the fp32 value the C entries receive) of k2's ``rnnt_type`` and ``delay_penalty``, with
    the refusals of include/warp_rnnt_amd_topology.h spelt out."""
    if rnnt_type not in RNNT_TYPES:
        raise ValueError(f'rnnt_type must be "regular" or "modified", not {rnnt_type!r} (k2\'s "constrained" topology is '
                         f"not covered)")
    dp = ctypes.c_float(delay_penalty).value
    if not 0.0 <= dp < float("inf"):                                                             # (false for a NaN)
        raise ValueError(f"delay_penalty must be finite and >= 0, not {delay_penalty}")
    return RNNT_TYPES[rnnt_type], dp


def with_topology_keywords(positional, full):
    """``positional`` -- a front end as it is documented and introspected, its positional signature unchanged -- taking
    the keyword-only ``rnnt_type`` and ``delay_penalty`` as well: ``full`` is called with ``positional``'s arguments, bound
    and with their defaults, and the two keywords behind them."""
    signature = inspect.signature(positional)

    @functools.wraps(positional)
    def front(*args, rnnt_type="regular", delay_penalty=0.0, **kwargs):
        bound = signature.bind(*args, **kwargs)
        bound.apply_defaults()
        return full(*bound.args, rnnt_type=rnnt_type, delay_penalty=delay_penalty)
    return front


def pruned_loss_topology(logits, labels, starts, xn, yn, blank=0, fastemit_lambda=0.0, with_grads=True,
                         topology=_lib.TOPOLOGY_REGULAR, delay_penalty=0.0):
    """:func:`pruned_loss` with a topology and a delay penalty (include/warp_rnnt_amd_topology.h).  The gradient pairs of
    TOPOLOGY_MODIFIED are (N,T+1,U,2), frame-major -- what :func:`pruned_logits_backward_topology` reads."""
    L = _lib.load()
    N, T, S, V = logits.shape
    U = labels.shape[1] + 1
    dev = logits.device
    _pruned_check(S, U, V, blank)
    _mismatch.poll(dev)
    frames = T + 1 if topology == _lib.TOPOLOGY_MODIFIED else T
    with torch.cuda.device(dev):
        costs = torch.empty((N,), dtype=torch.float32, device=dev)
        grads = torch.empty((N, frames, U, 2), dtype=torch.float32, device=dev) if with_grads else None
        if N == 0:
            return costs, grads
        ws = _workspace(dev, lambda n, t, u: L.rnnt_amd_pruned_topology_workspace_size(topology, n, t, u), "N T U", N, T, U)
        _check(L.rnnt_amd_pruned_loss_logits_topology(
            _stream(dev), ws.data_ptr(), LOGITS_DTYPES[logits.dtype], logits.data_ptr(), _ptr(labels), starts.data_ptr(),
            xn.data_ptr(), yn.data_ptr(), costs.data_ptr(), _ptr(grads), N, T, U, S, V, blank, float(fastemit_lambda),
            topology, float(delay_penalty)))
    return costs, grads


def pruned_logits_backward_topology(logits, labels, starts, xn, yn, grads, grad_costs, blank=0,
                                    topology=_lib.TOPOLOGY_REGULAR):
    """:func:`pruned_logits_backward` of :func:`pruned_loss_topology`; TOPOLOGY_MODIFIED reads the lengths: rows with
    t >= xn[n], t < u or u > yn[n] are exactly zero."""
    L = _lib.load()
    N, T, S, V = logits.shape
    U = labels.shape[1] + 1
    dev = logits.device
    with torch.cuda.device(dev):
        out = torch.empty_like(logits)
        if N == 0:
            return out
        _check(L.rnnt_amd_pruned_logits_backward_topology(
            _stream(dev), LOGITS_DTYPES[logits.dtype], logits.data_ptr(), _ptr(labels), starts.data_ptr(), xn.data_ptr(),
            yn.data_ptr(), grads.data_ptr(), _ptr(grad_costs), out.data_ptr(), N, T, U, S, V, blank, topology))
    return out


def simple_loss_topology(am, lm, q, labels, xn, yn, blank=0, lm_only_scale=0.0, am_only_scale=0.0, fastemit_lambda=0.0,
                         with_grads=True, topology=_lib.TOPOLOGY_REGULAR, delay_penalty=0.0):
    """:func:`simple_loss` with a topology and a delay penalty (include/warp_rnnt_amd_topology.h).  The gradient pairs of
    TOPOLOGY_MODIFIED are (N,T+1,U,2), frame-major: rows 0 .. T-1 are d cost / d pair of cell (t,u), zero outside an
    utterance's window (the terminal cell's pair is cleared); row T is no frame's -- what
    :func:`simple_backward_topology` reads."""
    L = _lib.load()
    N, T, V = am.shape
    U = lm.shape[1]
    dev = am.device
    c1, c2 = _simple_check(V, blank, lm_only_scale, am_only_scale, q)
    _mismatch.poll(dev)
    frames = T + 1 if topology == _lib.TOPOLOGY_MODIFIED else T
    with torch.cuda.device(dev):
        costs = torch.empty((N,), dtype=torch.float32, device=dev)
        grads = torch.empty((N, frames, U, 2), dtype=torch.float32, device=dev) if with_grads else None
        znorm = torch.empty((N, T, U), dtype=torch.float32, device=dev) if with_grads else None
        if N == 0:
            return costs, grads, znorm
        ws = _workspace(dev, lambda n, t, u: L.rnnt_amd_simple_topology_workspace_size(topology, n, t, u), "N T U", N, T, U)
        _check(L.rnnt_amd_simple_loss_topology(
            _stream(dev), ws.data_ptr(), LOGITS_DTYPES[am.dtype], am.data_ptr(), lm.data_ptr(), _ptr(q), _ptr(labels),
            xn.data_ptr(), yn.data_ptr(), costs.data_ptr(), _ptr(grads), _ptr(znorm), N, T, U, V, blank, c1, c2,
            float(fastemit_lambda), topology, float(delay_penalty)))
    return costs, grads, znorm


def simple_backward_topology(am, lm, q, labels, xn, yn, grads, znorm, grad_costs, blank=0, lm_only_scale=0.0,
                             am_only_scale=0.0, topology=_lib.TOPOLOGY_REGULAR):
    """:func:`simple_backward` of :func:`simple_loss_topology`."""
    L = _lib.load()
    N, T, V = am.shape
    U = lm.shape[1]
    dev = am.device
    c1, c2 = _simple_check(V, blank, lm_only_scale, am_only_scale, q)
    with torch.cuda.device(dev):
        dam, dlm = torch.empty_like(am), torch.empty_like(lm)
        parts = torch.empty((N, V), dtype=torch.float32, device=dev) if c2 != 0.0 else None
        if N == 0:
            return dam, dlm, None if parts is None else parts.sum(0)
        ws = _workspace(dev, lambda n, t, u: L.rnnt_amd_simple_topology_workspace_size(topology, n, t, u), "N T U", N, T, U)
        _check(L.rnnt_amd_simple_backward_topology(
            _stream(dev), ws.data_ptr(), LOGITS_DTYPES[am.dtype], am.data_ptr(), lm.data_ptr(), _ptr(q), _ptr(labels),
            xn.data_ptr(), yn.data_ptr(), grads.data_ptr(), znorm.data_ptr(), _ptr(grad_costs), dam.data_ptr(),
            dlm.data_ptr(), _ptr(parts), N, T, U, V, blank, c1, c2, topology))
    return dam, dlm, None if parts is None else parts.sum(0)


def _tdt_check(V, D, blank, durations, sigma):
    """The refusals of include/warp_rnnt_amd_tdt.h that depend on values, with their reasons spelt out."""
    ds = [int(d) for d in durations]
    if not (1 <= len(ds) <= 9 and len(set(ds)) == len(ds) and all(0 <= d <= 8 for d in ds) and 1 in ds):
        raise RuntimeError(f"rnnt_loss status 5 (RNNT_STATUS_INVALID_ARGUMENT): the TDT loss needs durations that are "
                           f"distinct integers in [0, 8] with 1 among them (durations={tuple(durations)})")
    if D != len(ds) or V < 2 or not 0 <= blank < V:
        raise RuntimeError(f"rnnt_loss status 5 (RNNT_STATUS_INVALID_ARGUMENT): the TDT loss needs logits of V + D columns, "
                           f"V >= 2, and a blank that is a token index (V={V}, D={len(ds)}, blank={blank})")
    if not 0.0 <= sigma < float("inf"):
        raise RuntimeError(f"rnnt_loss status 5 (RNNT_STATUS_INVALID_ARGUMENT): the TDT loss needs a finite sigma >= 0 "
                           f"(sigma={sigma})")
    return ds


def tdt_loss(logits, labels, xn, yn, durations, blank=0, sigma=0.0, fastemit_lambda=0.0, with_grads=True):
    """The token-and-duration (TDT) loss on the fused path (include/warp_rnnt_amd_tdt.h): logits (N,T,U,V+D) fp32 / bf16 /
    fp16 with D = len(durations), validated by the caller.  Returns costs (N,) fp32 and, with_grads, the per-cell sums
    (2+D,N,T,U) fp32 -- G_b, G_l, G_dur as planes in the diagonal-major cell order -- what :func:`tdt_logits_backward`
    reads (else None: no beta sweep runs and no such plane is produced)."""
    L = _lib.load()
    N, T, U, W = logits.shape
    D = len(durations)
    dev = logits.device
    ds = _tdt_check(W - D, D, blank, durations, sigma)
    with torch.cuda.device(dev):
        costs = torch.empty((N,), dtype=torch.float32, device=dev)
        grads = torch.empty((2 + D, N, T, U), dtype=torch.float32, device=dev) if with_grads else None
        if N == 0:
            return costs, grads
        ws = _workspace(dev, L.rnnt_amd_tdt_workspace_size, "N T U D", N, T, U, D)
        host_durations = (ctypes.c_int * D)(*ds)          # read during the call: nothing of it is needed afterwards
        _check(L.rnnt_amd_tdt_loss_logits(_stream(dev), ws.data_ptr(), LOGITS_DTYPES[logits.dtype], logits.data_ptr(),
                                          _ptr(labels), xn.data_ptr(), yn.data_ptr(), host_durations, D, costs.data_ptr(),
                                          _ptr(grads), N, T, U, W - D, blank, float(sigma), float(fastemit_lambda)))
    return costs, grads


def tdt_logits_backward(logits, labels, grads, grad_costs, num_durations, blank=0):
    """d(sum_n grad_costs[n]*cost[n]) / d(logits) of :func:`tdt_loss`, in the logits' dtype (the fp32 result rounded
    once); grads: the planes the forward returned."""
    L = _lib.load()
    N, T, U, W = logits.shape
    dev = logits.device
    with torch.cuda.device(dev):
        out = torch.empty_like(logits)
        if N == 0:
            return out
        _check(L.rnnt_amd_tdt_logits_backward(_stream(dev), LOGITS_DTYPES[logits.dtype], logits.data_ptr(), _ptr(labels),
                                              grads.data_ptr(), _ptr(grad_costs), out.data_ptr(), N, T, U,
                                              W - num_durations, num_durations, blank))
    return out


def _multiblank_check(V, blank_ids, blank_durations, sigma):
    """The refusals of include/warp_rnnt_amd_multiblank.h that depend on values, with their reasons spelt out."""
    ids, ds = [int(v) for v in blank_ids], [int(d) for d in blank_durations]
    if not (1 <= len(ds) <= 8 and len(set(ds)) == len(ds) and all(1 <= d <= 8 for d in ds) and 1 in ds):
        raise RuntimeError(f"rnnt_loss status 5 (RNNT_STATUS_INVALID_ARGUMENT): the multi-blank loss needs blank durations "
                           f"that are distinct integers in [1, 8] with 1 among them, the standard blank's "
                           f"(durations={tuple(blank_durations)})")
    if len(ids) != len(ds) or len(set(ids)) != len(ids):
        raise RuntimeError(f"rnnt_loss status 5 (RNNT_STATUS_INVALID_ARGUMENT): the multi-blank loss needs one distinct "
                           f"blank id per duration (ids={tuple(blank_ids)}, durations={tuple(blank_durations)})")
    if V < len(ids) + 1 or not all(0 <= v < V for v in ids):
        raise RuntimeError(f"rnnt_loss status 5 (RNNT_STATUS_INVALID_ARGUMENT): the multi-blank loss needs blank ids that "
                           f"are vocabulary indices in [0, V) and V >= B + 1 (V={V}, ids={tuple(blank_ids)})")
    if not 0.0 <= sigma < float("inf"):
        raise RuntimeError(f"rnnt_loss status 5 (RNNT_STATUS_INVALID_ARGUMENT): the multi-blank loss needs a finite "
                           f"sigma >= 0 (sigma={sigma})")
    return ids, ds


def multiblank_loss(logits, labels, xn, yn, blank_ids, blank_durations, sigma=0.0, fastemit_lambda=0.0, with_grads=True):
    """The multi-blank transducer loss on the fused path (include/warp_rnnt_amd_multiblank.h): logits (N,T,U,V) fp32 /
    bf16 / fp16, validated by the caller; blank_ids[i] consumes blank_durations[i] frames.  Returns costs (N,) fp32 and,
    with_grads, the per-cell sums (1+B,N,T,U) fp32 -- G_l, G_blank as planes in the diagonal-major cell order -- what
    :func:`multiblank_logits_backward` reads (else None: no beta sweep runs and no such plane is produced)."""
    N, T, U, V = logits.shape
    ids, ds = _multiblank_check(V, blank_ids, blank_durations, sigma)
    L = _lib.load()
    B = len(ids)
    dev = logits.device
    with torch.cuda.device(dev):
        costs = torch.empty((N,), dtype=torch.float32, device=dev)
        grads = torch.empty((1 + B, N, T, U), dtype=torch.float32, device=dev) if with_grads else None
        if N == 0:
            return costs, grads
        ws = _workspace(dev, L.rnnt_amd_multiblank_workspace_size, "N T U B", N, T, U, B)
        host_ids, host_durations = (ctypes.c_int * B)(*ids), (ctypes.c_int * B)(*ds)      # read during the call
        _check(L.rnnt_amd_multiblank_loss_logits(_stream(dev), ws.data_ptr(), LOGITS_DTYPES[logits.dtype],
                                                 logits.data_ptr(), _ptr(labels), xn.data_ptr(), yn.data_ptr(), host_ids,
                                                 host_durations, B, costs.data_ptr(), _ptr(grads), N, T, U, V,
                                                 float(sigma), float(fastemit_lambda)))
    return costs, grads


def multiblank_logits_backward(logits, labels, grads, grad_costs, blank_ids):
    """d(sum_n grad_costs[n]*cost[n]) / d(logits) of :func:`multiblank_loss`, in the logits' dtype (the fp32 result
    rounded once); grads: the planes the forward returned; blank_ids: as the forward took them."""
    L = _lib.load()
    N, T, U, V = logits.shape
    ids = [int(v) for v in blank_ids]
    B = len(ids)
    dev = logits.device
    with torch.cuda.device(dev):
        out = torch.empty_like(logits)
        if N == 0:
            return out
        host_ids = (ctypes.c_int * B)(*ids)
        _check(L.rnnt_amd_multiblank_logits_backward(_stream(dev), LOGITS_DTYPES[logits.dtype], logits.data_ptr(),
                                                     _ptr(labels), grads.data_ptr(), _ptr(grad_costs), out.data_ptr(), N,
                                                     T, U, V, host_ids, B))
    return out


def tdt_joint_loss(f, g, weight, bias, labels, xn, yn, durations, activation="tanh", blank=0, sigma=0.0,
                   fastemit_lambda=0.0, with_grads=True, dropout=0.0, seed=None):
    """The joint network fused into the TDT loss (include/warp_rnnt_amd_tdt_joint.h): f (N,T,H), g (N,U,H), weight
    (V+D,H) of one dtype (fp32 / bf16 / fp16) with D = len(durations), bias (V+D,) fp32 or None; validated by the caller.
    Returns costs (N,) fp32 and, with_grads, stats (N,T,U,4) fp32 -- (max, log sum) of the token logits and of the
    duration logits of every cell -- and the per-cell sums (2+D,N,T,U) fp32 of :func:`tdt_loss` -- what
    :func:`tdt_joint_backward` reads (else None, None: no beta sweep, no G plane, no stats).  dropout, seed: as
    :func:`joint_loss`."""
    L = _lib.load()
    N, T, H = f.shape
    U = g.shape[1]
    D = len(durations)
    V = weight.shape[0] - D
    dev = f.device
    ds = _tdt_check(V, D, blank, durations, sigma)
    with torch.cuda.device(dev):
        costs = torch.empty((N,), dtype=torch.float32, device=dev)
        stats = torch.empty((N, T, U, 4), dtype=torch.float32, device=dev) if with_grads else None
        grads = torch.empty((2 + D, N, T, U), dtype=torch.float32, device=dev) if with_grads else None
        if N == 0:
            return costs, stats, grads
        ws = _workspace(dev, L.rnnt_amd_tdt_joint_workspace_size, "N T U H V D", N, T, U, H, V, D)
        host_durations = (ctypes.c_int * D)(*ds)          # read during the call: nothing of it is needed afterwards
        p, seed_ptr = _dropout_args(dropout, seed) if dropout > 0 else (0.0, 0)
        _check(L.rnnt_amd_tdt_joint_loss(_stream(dev), ws.data_ptr(), LOGITS_DTYPES[f.dtype], ACTIVATIONS[activation],
                                         f.data_ptr(), g.data_ptr(), weight.data_ptr(), _ptr(bias), _ptr(labels),
                                         xn.data_ptr(), yn.data_ptr(), host_durations, D, costs.data_ptr(), _ptr(stats),
                                         _ptr(grads), N, T, U, H, V, blank, float(sigma), float(fastemit_lambda), p,
                                         seed_ptr))
    return costs, stats, grads


def tdt_joint_backward(f, g, weight, bias, labels, xn, yn, stats, grads, grad_costs, num_durations, activation="tanh",
                       blank=0, need_f=True, need_g=True, need_weight=True, need_bias=True, dropout=0.0, seed=None):
    """d(sum_n grad_costs[n]*cost[n]) / d(f, g, weight, bias) of :func:`tdt_joint_loss`: df / dg in f's dtype, dweight
    (V+D,H) / dbias (V+D,) fp32; None for what is not asked for.  dropout, seed: those of the forward."""
    L = _lib.load()
    N, T, H = f.shape
    U = g.shape[1]
    D = num_durations
    W = weight.shape[0]
    dev = f.device
    with torch.cuda.device(dev):
        df = torch.empty_like(f) if need_f else None
        dg = torch.empty_like(g) if need_g else None
        dw = torch.empty((W, H), dtype=torch.float32, device=dev) if need_weight else None
        db = torch.empty((W,), dtype=torch.float32, device=dev) if (need_bias and bias is not None) else None
        if N == 0:
            for t in (df, dg, dw, db):
                if t is not None:
                    t.zero_()
            return df, dg, dw, db
        ws = _workspace(dev, L.rnnt_amd_tdt_joint_workspace_size, "N T U H V D", N, T, U, H, W - D, D)
        p, seed_ptr = _dropout_args(dropout, seed) if dropout > 0 else (0.0, 0)
        _check(L.rnnt_amd_tdt_joint_backward(_stream(dev), ws.data_ptr(), LOGITS_DTYPES[f.dtype], ACTIVATIONS[activation],
                                             f.data_ptr(), g.data_ptr(), weight.data_ptr(), _ptr(bias), _ptr(labels),
                                             xn.data_ptr(), yn.data_ptr(), stats.data_ptr(), grads.data_ptr(),
                                             _ptr(grad_costs), _ptr(df), _ptr(dg), _ptr(dw), _ptr(db), N, T, U, H, W - D, D,
                                             blank, p, seed_ptr))
    return df, dg, dw, db


def tdt_align(logits, labels, xn, yn, durations, blank=0, sigma=0.0):
    """Best-path alignments over the TDT lattice (include/warp_rnnt_amd_tdt_align.h): logits (N,T,U,V+D) as
    :func:`tdt_loss` takes them, validated by the caller.  Returns scores (N,) fp32 -- the log-probability of the best path,
    -inf where there is none -- and emit_frames, emit_durations (N,U-1) int32: the frame at which label u is emitted and
    the duration emitted with it, -1 behind yn[n] and for an utterance without a path."""
    L = _lib.load()
    N, T, U, W = logits.shape
    D = len(durations)
    dev = logits.device
    ds = _tdt_check(W - D, D, blank, durations, sigma)
    with torch.cuda.device(dev):
        scores = torch.empty((N,), dtype=torch.float32, device=dev)
        emit_frames = torch.empty((N, U - 1), dtype=torch.int32, device=dev)
        emit_durations = torch.empty((N, U - 1), dtype=torch.int32, device=dev)
        if N == 0:
            return scores, emit_frames, emit_durations
        ws = _workspace(dev, L.rnnt_amd_tdt_align_workspace_size, "N T U D", N, T, U, D)
        host_durations = (ctypes.c_int * D)(*ds)          # read during the call: nothing of it is needed afterwards
        _check(L.rnnt_amd_tdt_align(_stream(dev), ws.data_ptr(), LOGITS_DTYPES[logits.dtype], logits.data_ptr(),
                                    _ptr(labels), xn.data_ptr(), yn.data_ptr(), host_durations, D, scores.data_ptr(),
                                    emit_frames.data_ptr() if U > 1 else 0, emit_durations.data_ptr() if U > 1 else 0,
                                    N, T, U, W - D, blank, float(sigma)))
    return scores, emit_frames, emit_durations


ALIGN_IN_HAT_LOGITS = _lib.ALIGN_IN_HAT_LOGITS


def align(input, labels, xn, yn, input_kind, blank=0):
    """Best-path alignments from the loss lattice (include/warp_rnnt_amd_align.h): ``input`` as :func:`loss` takes it for
    IN_LOG_PROBS_DENSE / IN_LOG_PROBS_GATHERED / IN_LOGITS_DENSE, or logits read the HAT way for ALIGN_IN_HAT_LOGITS;
    validated by the caller.  Returns scores (N,) fp32 -- the log-probability of the best path -- and emit_frames (N,U-1)
    int32: the frame at which label u is emitted, -1 behind yn[n]."""
    L = _lib.load()
    N, T, U, V = input.shape
    dev = input.device
    if input_kind == IN_LOG_PROBS_GATHERED:
        blank = 0          # channel 0 of the 2-channel layout
    elif input_kind == ALIGN_IN_HAT_LOGITS and (V < 2 or not 0 <= blank < V):
        raise RuntimeError(f"rnnt_loss status 5 (RNNT_STATUS_INVALID_ARGUMENT): the HAT loss needs V >= 2 and a blank "
                           f"that is a vocabulary index (V={V}, blank={blank})")
    elif not 0 <= blank < V:
        raise RuntimeError(f"rnnt_loss status 5 (RNNT_STATUS_INVALID_ARGUMENT): blank={blank} is not a "
                           f"vocabulary index of xs (V={V})")
    with torch.cuda.device(dev):
        scores = torch.empty((N,), dtype=torch.float32, device=dev)
        emit_frames = torch.empty((N, U - 1), dtype=torch.int32, device=dev)
        if N == 0:
            return scores, emit_frames
        ws = _workspace(dev, L.rnnt_amd_align_workspace_size, "N T U", N, T, U)
        _check(L.rnnt_amd_align(_stream(dev), ws.data_ptr(), input_kind, LOGITS_DTYPES[input.dtype], input.data_ptr(),
                                _ptr(labels), xn.data_ptr(), yn.data_ptr(), scores.data_ptr(),
                                emit_frames.data_ptr(), N, T, U, V, blank))
    return scores, emit_frames
