"""The joint network fused into the loss, without a GPU: the C entries (exported, declared, refusing bad arguments
before any HIP call) and the Python argument errors of rnnt_loss_from_joint."""
import ctypes
import os
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rnnt_amd_joint_workspace_size", "rnnt_amd_joint_loss", "rnnt_amd_joint_backward")


def _lib():
    import warp_rnnt_amd
    from warp_rnnt_amd import _build
    _build.build()
    return warp_rnnt_amd.load()


def test_joint_entries_exported_and_declared():
    from warp_rnnt_amd import _lib as lib
    L = _lib()
    assert L.rnnt_amd_version() == 110
    hdr = open(os.path.join(ROOT, "include", "warp_rnnt_amd.h")).read().replace(" (", "(")
    syms = subprocess.check_output(["nm", "-D", "--defined-only", lib.lib_path()]).decode()
    for name in NEW:
        assert name + "(" in hdr and name in lib.SYMBOLS
        assert f" T {name}\n" in syms, name
    assert "RNNT_ACT_TANH = 0" in hdr and "RNNT_ACT_RELU = 1" in hdr
    assert lib.ACT_TANH == 0 and lib.ACT_RELU == 1


def test_joint_workspace_size():
    L = _lib()
    assert L.rnnt_amd_joint_workspace_size(2, 10, 5, 64, 50) >= L.rnnt_amd_workspace_size(2, 10, 5)
    assert L.rnnt_amd_joint_workspace_size(2, 10, 5, 64, 50) % 256 == 0
    for H, V in ((48, 50), (16, 50), (1056, 50), (64, 1), (0, 50)):
        assert L.rnnt_amd_joint_workspace_size(2, 10, 5, H, V) == 0, (H, V)
    assert L.rnnt_amd_joint_workspace_size(2, 0, 5, 64, 50) == 0
    # the weight kernel's partials are bounded by the shape of W, not by the number of cells
    a = L.rnnt_amd_joint_workspace_size(16, 1500, 301, 512, 50) - L.rnnt_amd_workspace_size(16, 1500, 301)
    assert a < 64 << 20, a


def test_joint_entries_refuse_before_any_hip_call():
    """Dummy device pointers that are never dereferenced: each call is refused by the host-side check it names."""
    L = _lib()
    p = ctypes.c_void_p(256)
    odd = ctypes.c_void_p(256 + 4)

    def fwd(ws=p, dtype=0, act=0, f=p, g=p, w=p, labels=p, xn=p, yn=p, costs=p, lse=p, grads=p,
            N=2, T=3, U=2, H=64, V=5, blank=0):
        return L.rnnt_amd_joint_loss(None, ws, dtype, act, f, g, w, p, labels, xn, yn, costs, lse, grads,
                                     N, T, U, H, V, blank, 0.0)

    def bwd(ws=p, dtype=0, act=0, f=p, g=p, w=p, labels=p, xn=p, yn=p, lse=p, grads=p,
            N=2, T=3, U=2, H=64, V=5, blank=0):
        return L.rnnt_amd_joint_backward(None, ws, dtype, act, f, g, w, p, labels, xn, yn, lse, grads, p,
                                         p, p, p, p, N, T, U, H, V, blank)

    for call in (fwd, bwd):
        for kw in (dict(ws=None), dict(f=None), dict(g=None), dict(w=None), dict(xn=None), dict(yn=None),
                   dict(labels=None), dict(ws=odd), dict(f=odd), dict(w=odd),
                   dict(dtype=-1), dict(dtype=3), dict(act=2), dict(act=-1),
                   dict(H=48), dict(H=16), dict(H=1056), dict(H=0),
                   dict(V=1), dict(V=0), dict(blank=5), dict(blank=-1),
                   dict(N=-1), dict(N=70000), dict(T=0), dict(U=0), dict(T=1 << 15, U=1 << 14)):
            assert call(**kw) == 5, (call.__name__, kw)
    assert fwd(costs=None) == 5
    assert fwd(lse=None) == 5                 # grads asked for without lse
    assert bwd(lse=None) == 5 and bwd(grads=None) == 5
    # N == 0 is a valid empty batch: nothing to launch
    assert fwd(N=0) == 0 and bwd(N=0) == 0


def _args(N=2, T=5, U=3, H=64, V=11, dtype=torch.float32):
    f = torch.zeros(N, T, H, dtype=dtype)
    g = torch.zeros(N, U + 1, H, dtype=dtype)
    w = torch.zeros(V, H)
    b = torch.zeros(V)
    labels = torch.ones(N, U, dtype=torch.int32)
    xn = torch.full((N,), T, dtype=torch.int32)
    yn = torch.full((N,), U, dtype=torch.int32)
    return [f, g, w, b, labels, xn, yn]


@pytest.mark.parametrize("i,bad,msg", [
    (1, torch.zeros(2, 4, 64, dtype=torch.bfloat16), "share one dtype"),
    (0, torch.zeros(2, 5, 64, dtype=torch.float64), "float32, bfloat16 or float16"),
    (1, torch.zeros(2, 5, 64), "U\\+1 rows"),
    (1, torch.zeros(2, 4, 32), "g must be"),
    (2, torch.zeros(11, 32), "weight must be"),
    (2, torch.zeros(11, 64, dtype=torch.float16), "weight must be float32"),
    (3, torch.zeros(12), "bias must be"),
    (4, torch.ones(2, 4, dtype=torch.int32), "labels must be"),
    (4, torch.ones(2, 3, dtype=torch.int64), "Int tensor"),
    (5, torch.full((3,), 5, dtype=torch.int32), "frames_lengths"),
])
def test_joint_front_end_rejects_mismatches(i, bad, msg):
    from warp_rnnt_amd.joint import rnnt_loss_from_joint
    a = _args()
    a[i] = bad
    with pytest.raises(RuntimeError, match=msg):
        rnnt_loss_from_joint(*a)


def test_joint_front_end_refuses_sizes_and_activation():
    from warp_rnnt_amd.joint import rnnt_loss_from_joint
    with pytest.raises(RuntimeError, match="status 5"):
        rnnt_loss_from_joint(*_args(H=48))
    with pytest.raises(RuntimeError, match="status 5"):
        rnnt_loss_from_joint(*_args(V=1))
    with pytest.raises(RuntimeError, match="status 5"):
        rnnt_loss_from_joint(*_args(), blank=11)
    with pytest.raises(RuntimeError, match="activation"):
        rnnt_loss_from_joint(*_args(), activation="gelu")
    with pytest.raises(RuntimeError, match="CUDA"):          # well-formed, but no GPU tensors
        rnnt_loss_from_joint(*_args())


@pytest.mark.parametrize("case", [
    # N, T, U (labels), V, H, act, blank, bias, lam
    (3, 5, 3, 7, 32, "relu", 0, True, 0.0),
    (2, 4, 2, 18, 64, "relu", 16, False, 0.05),
    (3, 5, 3, 7, 32, "tanh", 6, False, 0.05),
    (2, 4, 2, 18, 64, "tanh", 16, True, 0.0),
], ids=lambda c: f"V{c[3]}_H{c[4]}_{c[5]}_bias{int(c[7])}_lam{c[8]}")
def test_joint_reference_matches_autograd_fp64(case):
    """tests/joint_reference.py (the fp64 comparator of tests/test_gpu_joint_edges.py) against the autograd fp64 joint of
    tests/test_gpu_joint.py, without a GPU.  relu on inputs whose sums are exact in fp32 runs the reference as the
    kernels do (E = fp32, act in fp32); tanh runs it in float64 throughout (act in fp32 would differ by its rounding)."""
    from joint_reference import joint_reference
    from test_gpu_joint import reference as autograd_reference
    N, T, U, V, H, act, blank, with_bias, lam = case
    gen = torch.Generator().manual_seed(N * 1000 + V)
    # values on a grid of 1/64 below 4 in magnitude: f + g and relu(f + g) are exact in fp32
    f = torch.randint(-128, 129, (N, T, H), generator=gen).double() / 64
    g = torch.randint(-128, 129, (N, U + 1, H), generator=gen).double() / 64
    w = torch.randn(V, H, generator=gen, dtype=torch.float64) / H ** 0.5
    b = torch.randn(V, generator=gen, dtype=torch.float64) * 0.1 if with_bias else torch.zeros(V, dtype=torch.float64)
    labels = ((blank + 1 + torch.randint(0, V - 1, (N, U), generator=gen)) % V).to(torch.int32)
    labels[0, 0] = V - 1 if blank != V - 1 else 0
    xn = torch.tensor([T] + [T - 1 - i % 2 for i in range(N - 1)], dtype=torch.int32)
    yn = torch.tensor([U] + [i % (U + 1) for i in range(N - 1)], dtype=torch.int32)
    up = torch.linspace(0.5, 2.0, N, dtype=torch.float64)
    if act == "relu":
        # the reference stages W in E = fp32: the autograd joint gets the same fp32-valued weight and bias
        w, b = w.float().double(), b.float().double()
        ins = dict(f=f.float(), g=g.float(), weight=w.float(), bias=b.float() if with_bias else None)
        kw = {}
    else:
        ins = dict(f=f, g=g, weight=w, bias=b if with_bias else None)
        kw = dict(act_dtype=torch.float64)
    rc, rf, rg, rw, rb = autograd_reference(f, g, w, b, labels, xn, yn, act, blank, lam, up)
    c, df, dg, dw, db = joint_reference(**ins, labels=labels, xn=xn, yn=yn, act=act, blank=blank,
                                        fastemit_lambda=lam, upstream=up, **kw)
    for got, ref, name in ((c, rc, "costs"), (df, rf, "f"), (dg, rg, "g"), (dw, rw, "weight"), (db, rb, "bias")):
        err = float((got - ref).abs().max() / ref.abs().max())
        assert err < 1e-10, (name, err)
