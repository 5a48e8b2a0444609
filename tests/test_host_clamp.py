"""The gradient clamp of the fused path, without a GPU: the two C entries of include/warp_rnnt_amd_clamp.h (their twins'
argument lists and a float, refusing bad arguments before any HIP call, answering what their unclamped twins answer without
a launch) and the device-free parts of warp_rnnt_amd.compat."""
import ctypes
import math

import pytest
import torch

ENTRIES = {"rnnt_amd_logits_backward_clamped", "rnnt_amd_compact_logits_backward_clamped"}
INVALID, SUCCESS = 5, 0


def _lib():
    import warp_rnnt_amd
    from warp_rnnt_amd import _build
    _build.build()          # hipcc cross-compiles for gfx950 without a GPU; no-op when up to date
    return warp_rnnt_amd.load()


def test_clamped_entries_take_the_arguments_of_their_twins_and_a_float_behind_them():
    """(What every additive header owes -- declared, bound, exported, a stale library refused: test_host_additive_abi.py.)"""
    from warp_rnnt_amd import _lib as lib
    assert set(lib.CLAMP_SYMBOLS) == ENTRIES
    for name in ENTRIES:
        assert lib.CLAMP_SYMBOLS[name][1][-1] is ctypes.c_float
    assert lib.CLAMP_SYMBOLS["rnnt_amd_logits_backward_clamped"][1][:-1] == lib.SYMBOLS["rnnt_amd_logits_backward_typed"][1]
    assert (lib.CLAMP_SYMBOLS["rnnt_amd_compact_logits_backward_clamped"][1][:-1] ==
            lib.SYMBOLS["rnnt_amd_compact_logits_backward"][1])


def test_clamp_entries_do_not_move_the_abi_version():
    from warp_rnnt_amd import _lib as lib
    assert _lib().rnnt_amd_version() == lib.ABI_VERSION == 110


def test_clamped_entries_refuse_before_any_hip_call():
    """Dummy device pointers that are never dereferenced: each call is refused by the host-side check it names, or is one
    of the twin's answers without a launch."""
    L = _lib()
    p = ctypes.c_void_p(256)                 # aligned, non-null, never dereferenced

    def dense(dtype=0, labels=p, N=2, T=3, U=2, V=5, blank=0, clamp=0.5):
        return L.rnnt_amd_logits_backward_clamped(None, dtype, p, labels, p, p, p, N, T, U, V, blank, clamp)

    def twin_dense(dtype=0, labels=p, N=2, T=3, U=2, V=5, blank=0):
        return L.rnnt_amd_logits_backward_typed(None, dtype, p, labels, p, p, p, N, T, U, V, blank)

    def compact(dtype=0, ys=p, n_labels=2, N=2, STU=12, V=5, blank=0, clamp=0.5):
        return L.rnnt_amd_compact_logits_backward_clamped(None, dtype, p, ys, n_labels, p, p, p, p, p, p, p, N, STU, V,
                                                          blank, clamp)

    def twin_compact(dtype=0, ys=p, n_labels=2, N=2, STU=12, V=5, blank=0):
        return L.rnnt_amd_compact_logits_backward(None, dtype, p, ys, n_labels, p, p, p, p, p, p, p, N, STU, V, blank)

    # the clamp itself: negative, NaN, infinite -- whatever else is asked, an early success included
    for clamp in (-1.0, math.nan, math.inf):
        assert dense(clamp=clamp) == INVALID and compact(clamp=clamp) == INVALID
        assert dense(clamp=clamp, N=0) == INVALID and compact(clamp=clamp, STU=0) == INVALID
    for dtype in (-1, 3):
        assert dense(dtype=dtype) == INVALID and compact(dtype=dtype) == INVALID
    # every refusal of the unclamped twin, one at a time, with the clamp on and with clamp == 0 (which is the twin)
    dense_refusals = [dict(N=-1), dict(N=70000), dict(T=0), dict(U=0), dict(T=1 << 15, U=1 << 14),
                      dict(N=65535, T=1 << 10, U=1 << 7), dict(V=0), dict(blank=5), dict(blank=-1), dict(labels=None)]
    compact_refusals = [dict(N=-1), dict(N=70000), dict(STU=-1), dict(STU=1 << 32), dict(V=0), dict(blank=5),
                        dict(blank=-1), dict(n_labels=-1), dict(ys=None)]
    for dtype in (0, 1, 2):
        for kw in dense_refusals:
            assert twin_dense(dtype=dtype, **kw) == INVALID, kw
            assert dense(dtype=dtype, **kw) == INVALID and dense(dtype=dtype, clamp=0.0, **kw) == INVALID, kw
        for kw in compact_refusals:
            assert twin_compact(dtype=dtype, **kw) == INVALID, kw
            assert compact(dtype=dtype, **kw) == INVALID and compact(dtype=dtype, clamp=0.0, **kw) == INVALID, kw
        # the twin's early successes: no utterances (dense), no rows (compact); a column of blanks needs no labels
        assert twin_dense(dtype=dtype, N=0) == SUCCESS and twin_compact(dtype=dtype, STU=0) == SUCCESS
        for clamp in (0.0, 0.5, 3e38):
            assert dense(dtype=dtype, N=0, clamp=clamp) == SUCCESS
            assert dense(dtype=dtype, N=0, U=1, labels=None, clamp=clamp) == SUCCESS
            assert compact(dtype=dtype, STU=0, clamp=clamp) == SUCCESS
            assert compact(dtype=dtype, STU=0, n_labels=0, ys=None, clamp=clamp) == SUCCESS


def test_compat_blank_resolution():
    from warp_rnnt_amd import compat
    V = 29
    assert compat.resolve_blank(-1, V) == V - 1
    assert compat.resolve_blank(0, V) == 0
    assert compat.resolve_blank(V - 1, V) == V - 1
    assert compat.resolve_blank(-V, V) == 0
    for bad in (V, -V - 1):
        with pytest.raises(ValueError, match="blank"):
            compat.resolve_blank(bad, V)


def test_compat_clamp_mapping_and_reduction_check():
    from warp_rnnt_amd import compat
    for off in (-1, 0, -0.5, -1.0, 0.0):
        assert compat.resolve_clamp(off) == 0.0
    assert compat.resolve_clamp(1.0) == 1.0
    assert compat.resolve_clamp(1) == 1.0 and isinstance(compat.resolve_clamp(1), float)
    for ok in ("none", "mean", "sum"):
        assert compat.check_reduction(ok) == ok
    for bad in ("avg", None, ""):
        with pytest.raises(ValueError, match="reduction"):
            compat.check_reduction(bad)


def _cpu_batch(V=7):
    return (torch.zeros((2, 3, 2, V)), torch.ones((2, 1), dtype=torch.int32), torch.tensor([3, 2], dtype=torch.int32),
            torch.tensor([1, 1], dtype=torch.int32))


def test_compat_value_errors_come_before_any_device_work():
    from warp_rnnt_amd import compat
    batch = _cpu_batch()
    with pytest.raises(ValueError, match="reduction"):
        compat.rnnt_loss(*batch, reduction="avg")
    with pytest.raises(ValueError, match="fused path"):
        compat.rnnt_loss(*batch, clamp=1.0, fused_log_softmax=False)
    for bad in (7, -8):
        with pytest.raises(ValueError, match="blank"):
            compat.rnnt_loss(*batch, blank=bad)
    # behind them the checks of check_logits_inputs, with their texts: these tensors are not on the GPU
    with pytest.raises(RuntimeError, match="must be located in the CUDA"):
        compat.rnnt_loss(*batch)
    with pytest.raises(ValueError, match="clamp"):
        from warp_rnnt_amd.fused import rnnt_loss_from_logits
        rnnt_loss_from_logits(*batch, clamp=-1.0)


def test_compat_routes_and_module_share_one_implementation(monkeypatch):
    """What compat.rnnt_loss hands on, recorded instead of run; RNNTLoss stores its arguments and calls the function."""
    import warp_rnnt
    from warp_rnnt_amd import compat, fused
    calls = []
    monkeypatch.setattr(fused, "rnnt_loss_from_logits", lambda *a, **kw: calls.append(("fused", a, kw)) or "F")
    monkeypatch.setattr(warp_rnnt, "rnnt_loss", lambda *a, **kw: calls.append(("log_probs", a, kw)) or "L")
    batch = _cpu_batch()
    assert compat.rnnt_loss(*batch) == "F"                                   # torchaudio's defaults
    assert calls.pop() == ("fused", batch, dict(reduction="mean", blank=6, clamp=0.0))
    assert compat.rnnt_loss(*batch, blank=0, clamp=1.0, reduction="sum") == "F"
    assert calls.pop() == ("fused", batch, dict(reduction="sum", blank=0, clamp=1.0))
    assert compat.rnnt_loss(*batch, blank=-7, clamp=-0.5, reduction="none", fused_log_softmax=False) == "L"
    assert calls.pop() == ("log_probs", batch, dict(reduction="none", gather=True, blank=0))

    module = compat.RNNTLoss(blank=0, clamp=0.25, reduction="sum")
    assert isinstance(module, torch.nn.Module)
    assert (module.blank, module.clamp, module.reduction, module.fused_log_softmax) == (0, 0.25, "sum", True)
    defaults = compat.RNNTLoss()
    assert (defaults.blank, defaults.clamp, defaults.reduction, defaults.fused_log_softmax) == (-1, -1.0, "mean", True)
    assert module(*batch) == "F"
    assert calls.pop() == ("fused", batch, dict(reduction="sum", blank=0, clamp=0.25))
    # one implementation: the module's forward is a call of the function
    seen = []
    monkeypatch.setattr(compat, "rnnt_loss", lambda *a: seen.append(a) or "X")
    assert module(*batch) == "X" and seen == [batch + (0, 0.25, "sum", True)]
    assert not calls


def test_clamp_keyword_goes_last_and_defaults_to_off():
    import inspect
    from warp_rnnt_amd import fused, ops
    for fn in (ops.logits_backward, ops.compact_logits_backward, fused.rnnt_loss_from_logits):
        params = list(inspect.signature(fn).parameters.values())
        assert params[-1].name == "clamp" and params[-1].default == 0.0, fn
    import warp_rnnt_amd
    assert warp_rnnt_amd.compat.rnnt_loss is not None
