"""The fused path on the compact layout, without a GPU: the three C entries (exported, declared, refusing bad arguments
before any HIP call) and the Python argument errors of rnnt_loss_from_logits(compact=True)."""
import ctypes
import os
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rnnt_amd_loss_compact_logits", "rnnt_amd_loss_compact_logits_bounded", "rnnt_amd_compact_logits_backward")


def _lib():
    import warp_rnnt_amd
    from warp_rnnt_amd import _build
    _build.build()
    return warp_rnnt_amd.load()


def test_compact_logits_entries_exported_and_declared():
    from warp_rnnt_amd import _lib as lib
    L = _lib()
    assert L.rnnt_amd_version() == 110
    hdr = open(os.path.join(ROOT, "include", "warp_rnnt_amd.h")).read().replace(" (", "(")
    syms = subprocess.check_output(["nm", "-D", "--defined-only", lib.lib_path()]).decode()
    for name in NEW:
        assert name + "(" in hdr and name in lib.SYMBOLS
        assert f" T {name}\n" in syms, name


def test_compact_logits_entries_refuse_before_any_hip_call():
    """Dummy device pointers that are never dereferenced: each call is refused by the host-side check it names."""
    L = _lib()
    p = ctypes.c_void_p(256)                 # aligned, non-null, never dereferenced
    odd = ctypes.c_void_p(256 + 4)           # a misaligned workspace

    def fwd(ws=p, dtype=0, ys=p, N=2, STU=12, Tmax=3, Umax=2, V=5, blank=0):
        return L.rnnt_amd_loss_compact_logits(None, ws, dtype, p, ys, p, p, p, p, p, p, N, STU, Tmax, Umax, V, blank, 0.0)

    def bnd(ws=p, dtype=0, ys=p, n_labels=2, N=2, STU=12, Tmax=3, Umax=2, V=5, blank=0):
        return L.rnnt_amd_loss_compact_logits_bounded(None, ws, dtype, p, ys, n_labels, p, p, p, p, N, STU, Tmax, Umax,
                                                      V, blank, 0.0)

    def bwd(dtype=0, ys=p, n_labels=2, N=2, STU=12, V=5, blank=0):
        return L.rnnt_amd_compact_logits_backward(None, dtype, p, ys, n_labels, p, p, p, p, p, p, p, N, STU, V, blank)

    for dtype in (-1, 3, 7):
        assert fwd(dtype=dtype) == 5 and bnd(dtype=dtype) == 5 and bwd(dtype=dtype) == 5
    for dtype in (0, 1, 2):
        # sizes compact_dims_ok refuses: N < 0, N > 65535, STU < 0, STU >= 2^32
        for N, STU in ((-1, 12), (70000, 12), (2, -1), (2, 1 << 32)):
            assert fwd(dtype=dtype, N=N, STU=STU) == 5
            assert bnd(dtype=dtype, N=N, STU=STU) == 5
            assert bwd(dtype=dtype, N=N, STU=STU) == 5
        # launch bounds whose plane is too large (Tmax*Umax >= 2^29)
        assert fwd(dtype=dtype, Tmax=1 << 15, Umax=1 << 14) == 5
        assert bnd(dtype=dtype, Tmax=1 << 15, Umax=1 << 14) == 5
        # V < 1, blank outside [0, V)
        for V, blank in ((0, 0), (5, 5), (5, -1)):
            assert fwd(dtype=dtype, V=V, blank=blank) == 5
            assert bnd(dtype=dtype, V=V, blank=blank) == 5
            assert bwd(dtype=dtype, V=V, blank=blank) == 5
        # no workspace, a misaligned one
        for ws in (None, odd):
            assert fwd(dtype=dtype, ws=ws) == 5 and bnd(dtype=dtype, ws=ws) == 5
        # no labels while labels exist
        assert fwd(dtype=dtype, ys=None) == 5
        assert bnd(dtype=dtype, ys=None) == 5
        assert bwd(dtype=dtype, ys=None) == 5
        # the bounded form's own: bounds < 1, a negative label count
        assert bnd(dtype=dtype, Tmax=0) == 5 and bnd(dtype=dtype, Umax=0) == 5 and bnd(dtype=dtype, n_labels=-1) == 5
        assert bwd(dtype=dtype, n_labels=-1) == 5
        # nothing to do is not an error: no utterances, no rows (nothing is launched)
        assert fwd(dtype=dtype, N=0) == 0 and bwd(dtype=dtype, STU=0) == 0
        assert bnd(dtype=dtype, N=0) == 0


def test_compact_from_logits_python_errors():
    from warp_rnnt_amd.fused import rnnt_loss_from_logits
    xn = torch.tensor([2], dtype=torch.int32)
    yn = torch.tensor([1], dtype=torch.int32)
    ys = torch.tensor([1], dtype=torch.int32)
    for dt in (torch.float32, torch.bfloat16, torch.float16):
        with pytest.raises(RuntimeError, match="xs must be located in the CUDA"):
            rnnt_loss_from_logits(torch.zeros((4, 3), dtype=dt), ys, xn, yn, compact=True)
    for dt in (torch.float64, torch.int32, torch.int64):
        with pytest.raises(RuntimeError, match="float32, bfloat16 or float16"):
            rnnt_loss_from_logits(torch.zeros((4, 3), dtype=dt), ys, xn, yn, compact=True)
    with pytest.raises(RuntimeError, match="ys must be a Int tensor"):
        rnnt_loss_from_logits(torch.zeros((4, 3)), ys.long(), xn, yn, compact=True)
    with pytest.raises(RuntimeError, match="xn must be a Int tensor"):
        rnnt_loss_from_logits(torch.zeros((4, 3)), ys, xn.long(), yn, compact=True)
    nc = torch.zeros((3, 4)).t()
    with pytest.raises(RuntimeError, match="xs must be contiguous"):
        rnnt_loss_from_logits(nc, ys, xn, yn, compact=True)
    # launch bounds without the compact layout
    for kw in ({"max_frames": 2}, {"max_labels": 1}, {"max_frames": 2, "max_labels": 1}):
        with pytest.raises(ValueError, match="compact=True"):
            rnnt_loss_from_logits(torch.zeros((1, 2, 2, 3)), torch.zeros((1, 1), dtype=torch.int32), xn, yn, **kw)
