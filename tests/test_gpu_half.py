"""bf16 / fp16 logits on the fused path (rnnt_loss_from_logits, the lazy log_softmax handle, the typed C entries).

The contract: the logits are converted to fp32 as the kernels load them, so the costs are bit-equal to the fp32 fused path
on ``xh.float()``, d/d logits bit-equal to the fp32 d/d logits rounded once to the logits' dtype, and the library's
log-softmax of ``xh`` bit-equal to its log-softmax of ``xh.float()`` -- over every kernel the dispatcher can choose."""
import numpy as np
import pytest
import torch

import oracle
from helpers import make_case, np_log_softmax32

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HALF = [torch.bfloat16, torch.float16]


def T(a):
    a = np.asarray(a)
    return torch.tensor(a if a.ndim == 0 else np.ascontiguousarray(a), device=DEV)


def fused(x, labels, xn, yn, up, blank=0, lam=0.01, reduction="none", average_frames=False):
    from warp_rnnt_amd.fused import rnnt_loss_from_logits
    z = x.detach().clone().requires_grad_(True)
    loss = rnnt_loss_from_logits(z, labels, xn, yn, blank=blank, fastemit_lambda=lam, reduction=reduction,
                                 average_frames=average_frames)
    loss.backward(up if reduction == "none" else None)
    return loss.detach(), z.grad


# the V grid of test_gpu_wrapper.test_fused_from_logits_forward_backward, plus V = 2 and 1024, and T < 16 at V = 64
# (k_lsm_rows_diag's fallback); every kernel dispatch_lsm chooses for the fused modes
CASES = [(3, 30, 12, 50), (2, 9, 5, 5000), (2, 11, 70, 7), (2, 6, 4, 1030), (3, 40, 21, 128), (2, 33, 9, 64),
         (2, 21, 12, 32), (2, 17, 14, 80), (2, 17, 14, 96), (2, 19, 8, 160), (2, 19, 8, 192), (2, 19, 8, 256),
         (2, 13, 8, 200), (2, 9, 20, 128), (2, 30, 35, 64), (2, 21, 9, 34), (2, 21, 9, 66), (2, 15, 9, 130),
         (2, 11, 7, 258), (2, 9, 5, 510), (2, 9, 5, 514), (2, 9, 5, 1000), (3, 12, 6, 2), (2, 9, 5, 1024),
         (2, 9, 11, 64)]


@pytest.mark.parametrize("dtype", HALF, ids=["bf16", "fp16"])
@pytest.mark.parametrize("N,Tm,Um,V", CASES)
def test_half_logits_bit_equal_to_fp32_of_the_upcast(dtype, N, Tm, Um, V):
    blank = 0 if V % 2 else V - 1
    logits, labels, xn, yn = make_case(7 + V, N, Tm, Um, V, ragged=True, blank=blank)
    xh = (T(logits) * 2).to(dtype)
    up = T(np.random.RandomState(V).rand(N).astype(np.float32) + 0.5)
    tl, txn, tyn = T(labels), T(xn), T(yn)
    c32, g32 = fused(xh.float(), tl, txn, tyn, up, blank)
    ch, gh = fused(xh, tl, txn, tyn, up, blank)
    assert ch.dtype == torch.float32 and gh.dtype == dtype
    assert torch.equal(ch, c32)
    assert torch.equal(gh, g32.to(dtype))
    # the gradient pairs of the forward, and the library's log-softmax (fp32 out)
    from warp_rnnt_amd import ops
    _, p32 = ops.loss(xh.float(), tl, txn, tyn, ops.IN_LOGITS_DENSE, ops.GRADS_GATHERED_DIAGONAL, blank, 0.01)
    _, ph = ops.loss(xh, tl, txn, tyn, ops.IN_LOGITS_DENSE, ops.GRADS_GATHERED_DIAGONAL, blank, 0.01)
    assert torch.equal(ph, p32)
    lh = ops.log_softmax(xh)
    assert lh.dtype == torch.float32 and torch.equal(lh, ops.log_softmax(xh.float()))


@pytest.mark.parametrize("dtype", HALF, ids=["bf16", "fp16"])
@pytest.mark.parametrize("shape", [(1000, 50), (37, 5000), (64, 1030), (300, 17), (300, 36), (300, 100), (300, 128),
                                   (300, 200), (300, 500), (70, 1000), (21, 5124), (9, 10000), (5, 16384), (3, 17000),
                                   (11, 2)])
def test_half_log_softmax_bit_equal(dtype, shape):
    """LSM_NORM: k_lsm_regs (with its tail rows), the mid-V and large-V k_lsm_large covers, the LDS tiles, the generic
    kernel."""
    from warp_rnnt_amd import ops
    xh = (torch.randn(*shape, device=DEV) * 3).to(dtype)
    y = ops.log_softmax(xh)
    assert y.dtype == torch.float32 and torch.equal(y, ops.log_softmax(xh.float()))


@pytest.mark.parametrize("dtype", HALF, ids=["bf16", "fp16"])
def test_lazy_handle_fuses_and_materialises(dtype):
    import warp_rnnt
    from warp_rnnt_amd import ops
    from warp_rnnt_amd.functional import log_softmax
    N, Tm, Um, V = 3, 40, 12, 50
    logits, labels, xn, yn = make_case(11, N, Tm, Um, V, ragged=True)
    xh = T(logits).to(dtype)
    tl, txn, tyn = T(labels), T(xn), T(yn)
    for reduction, avg in (("none", False), ("mean", True), ("sum", False)):
        up = T(np.arange(1, N + 1, dtype=np.float32)) if reduction == "none" else None
        c_ref, g_ref = fused(xh, tl, txn, tyn, up, 0, 0.01, reduction, avg)
        z = xh.detach().clone().requires_grad_(True)
        h = log_softmax(z)
        assert h.dtype == torch.float32
        loss = warp_rnnt.rnnt_loss(h, tl, txn, tyn, gather=True, fastemit_lambda=0.01, reduction=reduction,
                                   average_frames=avg)
        loss.backward(up)
        assert not h.materialised
        assert torch.equal(loss.detach(), c_ref) and z.grad.dtype == dtype and torch.equal(z.grad, g_ref)
    # consumed elsewhere: the log-probs of the upcast, and the gradient back in the logits' dtype
    z = xh.detach().clone().requires_grad_(True)
    h = log_softmax(z)
    w = torch.randn(h.shape, device=DEV)
    (h * w).sum().backward()
    assert h.materialised
    lp = ops.log_softmax(xh.float())
    assert torch.equal(h._cell.y, lp)
    assert z.grad.dtype == dtype
    g32 = ops.log_softmax_backward(w.contiguous(), lp)
    assert torch.equal(z.grad, g32.to(dtype))


def test_autocast_joint_end_to_end():
    from warp_rnnt_amd.fused import rnnt_loss_from_logits
    torch.manual_seed(0)
    N, Tm, Um, H, V = 2, 30, 9, 64, 50
    _, labels, xn, yn = make_case(5, N, Tm, Um, V, ragged=True)
    enc = torch.randn(N, Tm, 1, H, device=DEV)
    dec = torch.randn(N, 1, Um, H, device=DEV)
    joint = torch.nn.Linear(H, V).to(DEV)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        logits = joint(torch.tanh(enc + dec))
    assert logits.dtype == torch.bfloat16
    logits.retain_grad()
    costs = rnnt_loss_from_logits(logits, T(labels), T(xn), T(yn))
    costs.sum().backward()
    assert costs.dtype == torch.float32 and logits.grad.dtype == torch.bfloat16
    assert all(torch.isfinite(p.grad).all() for p in joint.parameters())
    c32, _ = fused(logits.detach().float(), T(labels), T(xn), T(yn), torch.ones(N, device=DEV), lam=0.0)
    assert torch.equal(costs.detach(), c32)


def test_bf16_costs_against_the_oracle():
    from warp_rnnt_amd.fused import rnnt_loss_from_logits
    N, Tm, Um, V = 4, 150, 20, 5000
    logits, labels, xn, yn = make_case(3, N, Tm, Um, V, ragged=True)
    xh = T(logits).to(torch.bfloat16)
    costs = rnnt_loss_from_logits(xh, T(labels), T(xn), T(yn))
    lp = np_log_softmax32(xh.float().cpu().numpy())
    ref = oracle.rnnt_loss_f32(lp, labels, xn, yn, scan_mode=1)
    np.testing.assert_allclose(costs.cpu().numpy(), ref["costs"], rtol=1e-5)


def test_no_hidden_fp32_copy():
    from warp_rnnt_amd.fused import rnnt_loss_from_logits
    N, Tm, Um, V = 8, 512, 256, 50               # 2^20 cells
    logits, labels, xn, yn = make_case(1, N, Tm, Um, V)
    xh = T(logits).to(torch.bfloat16).requires_grad_(True)
    tl, txn, tyn = T(labels), T(xn), T(yn)
    del logits
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    rnnt_loss_from_logits(xh, tl, txn, tyn).sum().backward()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    assert xh.grad.dtype == torch.bfloat16
    assert peak < xh.numel() * 4, (peak, xh.numel() * 4)


@pytest.mark.parametrize("dtype", HALF, ids=["bf16", "fp16"])
def test_unaligned_view(dtype):
    N, Tm, Um, V = 2, 20, 9, 64
    logits, labels, xn, yn = make_case(9, N, Tm, Um, V, ragged=True)
    base = torch.empty(N * Tm * Um * V + 1, dtype=dtype, device=DEV)
    xv = base[1:].view(N, Tm, Um, V)
    xv.copy_(T(logits))
    assert xv.data_ptr() % 16 == 2
    xa = xv.clone()
    up = torch.ones(N, device=DEV)
    ca, ga = fused(xa, T(labels), T(xn), T(yn), up)
    from warp_rnnt_amd.fused import rnnt_loss_from_logits
    z = xv.detach()           # the view itself (a clone would realign it)
    z.requires_grad_(True)
    cv = rnnt_loss_from_logits(z, T(labels), T(xn), T(yn), fastemit_lambda=0.01)
    cv.backward(up)
    torch.testing.assert_close(cv.detach(), ca, rtol=1e-6, atol=0)
    ulp = (ga.float().abs() * (2.0 ** -7 if dtype == torch.bfloat16 else 2.0 ** -10)).clamp_min(
        torch.finfo(dtype).tiny)
    assert ((z.grad.float() - ga.float()).abs() <= ulp * 1.0001 + torch.finfo(dtype).smallest_normal).all()
    from warp_rnnt_amd import ops
    torch.testing.assert_close(ops.log_softmax(xv), ops.log_softmax(xa), rtol=1e-6, atol=1e-6)


def test_hip_graph_bf16_replays_the_eager_bits():
    from warp_rnnt_amd.fused import rnnt_loss_from_logits
    N, Tm, Um, V = 4, 60, 20, 50
    logits, labels, xn, yn = make_case(13, N, Tm, Um, V, ragged=True)
    x = T(logits).to(torch.bfloat16).requires_grad_(True)
    tl, txn, tyn = T(labels), T(xn), T(yn)

    def step():
        loss = rnnt_loss_from_logits(x, tl, txn, tyn, fastemit_lambda=0.01, reduction="sum")
        g, = torch.autograd.grad(loss, x)
        return loss, g

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):
            step()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss, g = step()
    with torch.no_grad():
        x.copy_(T(logits * 0.5).to(torch.bfloat16))
    graph.replay()
    torch.cuda.synchronize()
    le, ge = step()
    torch.cuda.synchronize()
    assert torch.equal(loss, le) and torch.equal(g, ge)


def test_invalid_lengths_nan_cost_and_zero_bf16_gradient():
    from warp_rnnt_amd.fused import rnnt_loss_from_logits
    N, Tm, Um, V = 3, 20, 8, 50
    logits, labels, xn, yn = make_case(17, N, Tm, Um, V)
    xn[1] = Tm + 5                                 # out of range
    xh = T(logits).to(torch.bfloat16)
    z = xh.clone().requires_grad_(True)
    c = rnnt_loss_from_logits(z, T(labels), T(xn), T(yn))
    c.backward(torch.ones(N, device=DEV))
    assert torch.isnan(c[1]) and torch.isfinite(c[[0, 2]]).all()
    assert z.grad.dtype == torch.bfloat16 and (z.grad[1] == 0).all() and (z.grad[[0, 2]] != 0).any()
    c32, g32 = fused(xh.float(), T(labels), T(xn), T(yn), torch.ones(N, device=DEV), lam=0.0)
    assert torch.equal(c.detach()[[0, 2]], c32[[0, 2]]) and torch.equal(z.grad, g32.to(torch.bfloat16))
