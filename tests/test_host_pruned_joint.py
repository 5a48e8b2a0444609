"""The joint network fused into the pruned loss without a GPU: the additive contract of
include/warp_rnnt_amd_pruned_joint.h and its table, the workspace size, the C entries' refusals with pointers that are never
dereferenced, and the front end's argument errors."""
import ctypes
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "warp_rnnt_amd_pruned_joint.h"
INVALID, SUCCESS = 5, 0


def _lib():
    import warp_rnnt_amd
    from warp_rnnt_amd import _build
    _build.build()          # hipcc cross-compiles for gfx950 without a GPU; no-op when up to date
    return warp_rnnt_amd.load()


def test_header_declares_what_the_table_binds_and_the_version_did_not_move():
    from warp_rnnt_amd import _build, _lib as lib
    L = _lib()
    table = lib.PRUNED_JOINT_SYMBOLS
    assert lib.ADDITIVE_PRUNED_JOINT == ((table, HEADER),)
    assert os.path.exists(os.path.join(ROOT, "include", HEADER))
    for name, (res, args) in table.items():
        fn = getattr(L, name)
        assert fn.restype is res and list(fn.argtypes) == list(args)
    assert L.rnnt_amd_version() == lib.ABI_VERSION == 110
    assert any(os.path.basename(h) == HEADER for h in _build.HEADERS) and "pruned_joint.h" in _build.HEADERS
    assert "pruned_joint.hip" in _build.SOURCES and "pruned_joint.hip" not in _build.HAZARD_CHECKED


def test_workspace_size_and_refusals_before_any_hip_call():
    L = _lib()
    size = L.rnnt_amd_pruned_joint_workspace_size
    base = dict(dtype=1, N=4, T=300, U=60, S=5, H=256, V=1025)
    of = lambda **kw: size(*dict(base, **kw).values())  # noqa: E731
    assert of() == of() > L.rnnt_amd_workspace_size(4, 300, 60) and of() % 256 == 0
    assert of() + 8 * 4 * 300 * 5 + 8 * 4 * 300 * 60 < 4 * 300 * 5 * 1025 * 2          # the memory contract's count < the logits
    assert of(dtype=0) > of()                                                        # the fp32 dpre and W^T are twice the size
    for bad in (dict(H=48), dict(H=16), dict(H=1056), dict(V=1), dict(S=0), dict(S=61), dict(dtype=3), dict(T=0), dict(N=-1)):
        assert of(**bad) == 0, bad
    p, odd = ctypes.c_void_p(256), ctypes.c_void_p(260)

    def fwd(ws=p, dtype=0, act=0, f=p, w=p, starts=p, stats=p, N=2, T=3, U=4, S=2, H=64, V=5, blank=0):
        return L.rnnt_amd_pruned_joint_loss(None, ws, dtype, act, f, p, w, p, p, starts, p, p, p, stats, p, N, T, U, S, H,
                                            V, blank, 0.0)

    def bwd(ws=p, dtype=0, act=0, f=p, w=p, starts=p, stats=p, N=2, T=3, U=4, S=2, H=64, V=5, blank=0):
        return L.rnnt_amd_pruned_joint_backward(None, ws, dtype, act, f, p, w, p, p, starts, p, p, stats, p, p, p, p, p, p,
                                                N, T, U, S, H, V, blank)

    for call in (fwd, bwd):
        for kw in (dict(ws=None), dict(ws=odd), dict(f=None), dict(f=odd), dict(w=odd), dict(starts=None), dict(stats=None),
                   dict(dtype=3), dict(act=2), dict(H=48), dict(H=1056), dict(V=1), dict(blank=5), dict(S=0), dict(S=5),
                   dict(T=0), dict(N=70000)):
            assert call(**kw) == INVALID, (call.__name__, kw)
        assert call(N=0) == SUCCESS


def test_front_end_argument_errors():
    from warp_rnnt_amd import pruned
    N, T, U, S, V, H = 2, 5, 4, 3, 11, 64
    args = [torch.zeros(N, T, H), torch.zeros(N, U, H), torch.zeros(V, H), torch.zeros(V), torch.ones(N, U - 1, dtype=torch.int32),
            torch.zeros(N, T, dtype=torch.int32), torch.full((N,), T, dtype=torch.int32), torch.full((N,), U - 1, dtype=torch.int32)]
    fn = pruned.pruned_rnnt_loss_from_joint
    with pytest.raises(ValueError, match="regular"):
        fn(*args, s_range=S, rnnt_type="modified")
    with pytest.raises(ValueError, match="s_range"):
        fn(*args)
    with pytest.raises(RuntimeError, match="activation"):
        fn(*args, s_range=S, activation="gelu")
    with pytest.raises(RuntimeError, match="status 5"):
        fn(torch.zeros(N, T, 48), torch.zeros(N, U, 48), torch.zeros(V, 48), *args[3:], s_range=S)
    with pytest.raises(RuntimeError, match="CUDA"):          # well-formed, but no GPU tensors
        fn(*args, s_range=S)
    assert pruned.PrunedJointLoss(64, 11, bias=False).bias is None and pruned.PrunedJointLoss(64, 11).weight.shape == (11, 64)
    for word in ("delay_penalty", "dropout", "clamp", "compact layout"):
        assert word in fn.__doc__, word
