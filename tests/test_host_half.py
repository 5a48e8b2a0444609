"""bf16 / fp16 logits: what can be checked without a GPU -- the typed C entries (exported, refusing an unknown dtype and
bad sizes before any HIP call), the Python checks, and the lazy handle's mechanics with the kernels stubbed."""
import ctypes
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rnnt_amd_loss_logits", "rnnt_amd_logits_backward_typed", "rnnt_amd_log_softmax_typed")


def _lib():
    import warp_rnnt_amd
    from warp_rnnt_amd import _build
    _build.build()          # hipcc cross-compiles for gfx950 without a GPU; no-op when up to date
    return warp_rnnt_amd.load()


def test_typed_entries_exported_and_version():
    import subprocess
    from warp_rnnt_amd import _lib as lib
    L = _lib()
    assert L.rnnt_amd_version() == 110 == lib.ABI_VERSION
    hdr = open(os.path.join(ROOT, "include", "warp_rnnt_amd.h")).read()
    syms = subprocess.check_output(["nm", "-D", "--defined-only", lib.lib_path()]).decode()
    for name in NEW:
        assert name + "(" in hdr.replace(" (", "(") and name in lib.SYMBOLS
        assert f" T {name}\n" in syms, name
    for name, value in (("RNNT_DTYPE_F32", 0), ("RNNT_DTYPE_BF16", 1), ("RNNT_DTYPE_F16", 2)):
        assert f"{name} = {value}" in hdr
    assert (lib.DTYPE_F32, lib.DTYPE_BF16, lib.DTYPE_F16) == (0, 1, 2)


def test_typed_entries_refuse_before_any_hip_call():
    """Dummy device pointers that are never dereferenced: every call below is refused by exactly the host-side check it
    names (a launch would fault), and every other argument would pass its own check."""
    L = _lib()
    p = ctypes.c_void_p(256)       # (aligned, non-null, never dereferenced: the checks come first)
    DIAG, NONE = 1, 3
    for dtype in (-1, 3, 7):
        assert L.rnnt_amd_loss_logits(None, p, dtype, p, p, p, p, p, p, DIAG, 2, 3, 4, 5, 0, 0.0) == 5
        assert L.rnnt_amd_logits_backward_typed(None, dtype, p, p, p, p, p, 2, 3, 4, 5, 0) == 5
        assert L.rnnt_amd_log_softmax_typed(None, dtype, p, p, 10, 5) == 5
    for dtype in (0, 1, 2):
        # sizes the fp32 entries refuse: N > 65535, T < 1, N*T*U >= 2^32, V < 1, blank outside [0, V)
        for N, T, U, V, blank in ((70000, 2, 2, 5, 0), (2, 0, 2, 5, 0), (65535, 65536, 2, 5, 0), (2, 2, 2, 0, 0),
                                  (2, 2, 2, 5, 5), (2, 2, 2, 5, -1)):
            assert L.rnnt_amd_loss_logits(None, p, dtype, p, p, p, p, p, p, DIAG, N, T, U, V, blank, 0.0) == 5
            assert L.rnnt_amd_logits_backward_typed(None, dtype, p, p, p, p, p, N, T, U, V, blank) == 5
        assert L.rnnt_amd_log_softmax_typed(None, dtype, p, p, -1, 5) == 5
        assert L.rnnt_amd_log_softmax_typed(None, dtype, p, p, 10, 0) == 5
        # no workspace; a gradient kind the logits entry does not have (dense d/d log-probs); an unknown kind;
        # no labels with U > 1; no gradient buffer for a kind that writes one
        assert L.rnnt_amd_loss_logits(None, None, dtype, p, p, p, p, p, p, DIAG, 2, 2, 2, 5, 0, 0.0) == 5
        assert L.rnnt_amd_loss_logits(None, p, dtype, p, p, p, p, p, p, 2, 2, 2, 2, 5, 0, 0.0) == 5
        assert L.rnnt_amd_loss_logits(None, p, dtype, p, p, p, p, p, p, 9, 2, 2, 2, 5, 0, 0.0) == 5
        assert L.rnnt_amd_loss_logits(None, p, dtype, p, None, p, p, p, p, NONE, 2, 2, 2, 5, 0, 0.0) == 5
        assert L.rnnt_amd_loss_logits(None, p, dtype, p, p, p, p, p, None, DIAG, 2, 2, 2, 5, 0, 0.0) == 5
        assert L.rnnt_amd_logits_backward_typed(None, dtype, p, None, p, p, p, 2, 2, 2, 5, 0) == 5


def test_from_logits_rejects_other_dtypes_and_cpu_tensors():
    from warp_rnnt_amd.fused import rnnt_loss_from_logits
    e = torch.zeros((1,), dtype=torch.int32)
    ys = torch.zeros((1, 1), dtype=torch.int32)
    for dt in (torch.float64, torch.int32):
        with pytest.raises(RuntimeError, match="float32, bfloat16 or float16"):
            rnnt_loss_from_logits(torch.zeros((1, 2, 2, 3), dtype=dt), ys, e, e)
    for dt in (torch.float32, torch.bfloat16, torch.float16):
        with pytest.raises(RuntimeError, match="xs must be located in the CUDA"):
            rnnt_loss_from_logits(torch.zeros((1, 2, 2, 3), dtype=dt), ys, e, e)
    # the reference's order: contiguity before the dtype, ints before the device
    nc = torch.zeros((1, 2, 3, 2), dtype=torch.float64).transpose(2, 3)
    with pytest.raises(RuntimeError, match="xs must be contiguous"):
        rnnt_loss_from_logits(nc, ys, e, e)
    with pytest.raises(RuntimeError, match="ys must be a Int tensor"):
        rnnt_loss_from_logits(torch.zeros((1, 2, 2, 3), dtype=torch.bfloat16), ys.long(), e, e)


def test_log_softmax_rejects_other_dtypes_and_cpu_tensors():
    from warp_rnnt_amd import functional
    for x in (torch.randn(2, 3, dtype=torch.float64), torch.randn(2, 3), torch.randn(2, 3).bfloat16(),
              torch.randn(2, 3).half()):
        with pytest.raises(RuntimeError, match=r"fp32 tensor on the GPU \(or a bf16 / fp16 one\)"):
            functional.log_softmax(x)


def test_reference_op_still_rejects_half_log_probs():
    import warp_rnnt
    import warp_rnnt._C as core
    e = torch.tensor([], dtype=torch.int)
    for dt in (torch.bfloat16, torch.float16):
        with pytest.raises(RuntimeError, match="xs must be a Float tensor"):
            core.rnnt_loss(torch.tensor([], dtype=dt), e, e, e)
    lp = torch.zeros((1, 2, 2, 3), dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="xs must be a Float tensor"):
        warp_rnnt.rnnt_loss(lp, torch.zeros((1, 1), dtype=torch.int32), torch.ones(1, dtype=torch.int32),
                            torch.ones(1, dtype=torch.int32), gather=True)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_lazy_handle_of_half_logits_is_fp32_and_returns_half_gradients(dtype, monkeypatch):
    """As test_host_cpu's handle test, with the kernels stubbed: fp32 log-probs of the upcast, gradient in x.dtype."""
    import warp_rnnt_amd.functional as F2
    calls = {"fwd": 0, "bwd": 0}

    def fake_fwd(x, out=None):
        calls["fwd"] += 1
        return torch.log_softmax(x.float(), -1)

    def fake_bwd(g, y, grad_in=None):
        calls["bwd"] += 1
        assert g.dtype == y.dtype == torch.float32
        return g - torch.exp(y) * g.sum(-1, keepdim=True)
    monkeypatch.setattr(F2.ops, "log_softmax", fake_fwd)
    monkeypatch.setattr(F2.ops, "log_softmax_backward", fake_bwd)
    x = torch.randn(2, 3, 4, 5).to(dtype).requires_grad_(True)
    h = F2._LazyLogSoftmaxFn.apply(x)
    h._src = x
    assert h.dtype == torch.float32 and h.shape == x.shape and h.fusable() and calls["fwd"] == 0
    s = (h * 2).sum()
    assert calls["fwd"] == 1 and h.materialised and s.dtype == torch.float32
    s.backward()
    assert calls["bwd"] == 1 and x.grad.dtype == dtype
    y32 = torch.log_softmax(x.detach().float(), -1)
    g2 = torch.full_like(y32, 2.0)
    assert torch.equal(x.grad, (g2 - torch.exp(y32) * g2.sum(-1, keepdim=True)).to(dtype))   # one rounding of the fp32 result
    # the eager form: fp32 out, gradient in x.dtype
    x3 = x.detach().clone().requires_grad_(True)
    y = F2._LogSoftmax.apply(x3)
    assert y.dtype == torch.float32
    y.sum().backward()
    assert x3.grad.dtype == dtype
