"""Every family the log-softmax planner can name (csrc/lsm_plan.h), launched: the launcher is a switch on the plan, so each
case first asks debug.lsm_plan that it reaches the family it is meant to reach, then runs the plain log-softmax and the
fused logits -> loss -> d/d logits path through the Python entries at fp32, bf16 and fp16 -- against torch's fp64
log-softmax and fp64 autograd through it (the lattice gradient from the fp64 oracle), at the tolerances of
test_gpu_parity.test_log_softmax_kernel and test_gpu_wrapper.test_fused_from_logits_forward_backward, and half-precision
logits against the bits of their fp32 upcast (test_gpu_half).

85 rows (N=1, T=17, U=5: odd, so the register kernel's groups of two and four leave a row over, and T >= 16 for the diagonal
walk); the largest case is V = 16388, 5.6 MB."""
import numpy as np
import pytest
import torch

from helpers import make_case
from oracle import transduce_np

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, TM, UM = 1, 17, 5
ROWS = N * TM * UM
LAM = 0.01
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}

# V, aligned -> the family of the plain log-softmax (and of the rows behind the register kernel's groups), of the fused
# gather and of the fused d/d logits
CASES = [
    (28, True, ("small", None), "small", "small"),            # wave-private tiles / whole-workgroup tiles
    (32, True, ("regs", "small"), "rows_diag", "small"),      # four rows per group + one left over; along the diagonals
    (50, True, ("regs", "small"), "small", "small"),          # c4's V: head + tail
    (100, True, ("regs", None), "small", "small"),            # one row per group: nothing left over
    (128, True, ("regs", None), "rows", "small"),
    (256, True, ("lgr", None), "rows", "small"),
    (600, True, ("small", None), "rows", "small"),            # tiles of the whole workgroup (L = 64)
    (1030, True, ("generic", None), "generic", "generic"),
    (5000, True, ("large", None), "large", "large"),
    (16388, True, ("generic", None), "generic", "generic"),
    (50, False, ("generic", None), "generic", "generic"),     # a view one element off the vector grid
]


def _place(t, aligned):
    """t on the device, contiguous, on a 16-byte boundary or exactly one element past one."""
    if aligned:
        out = t.to(DEV).contiguous()
        assert out.data_ptr() % 16 == 0
        return out
    base = torch.empty(t.numel() + 1, dtype=t.dtype, device=DEV)
    view = base[1:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % (4 * t.element_size()) == t.element_size()
    return view


def _reference(x32, labels, xn, yn, up):
    """fp64: log-probs, costs, d/d logits by autograd through torch.log_softmax."""
    x64 = x32.double().cpu().requires_grad_(True)
    lp64 = torch.log_softmax(x64, -1)
    c64, g64 = transduce_np.transduce_batch(lp64.detach().numpy(), labels, xn, yn, fastemit_lambda=LAM, fast=True)
    lp64.backward(torch.from_numpy(g64 * up[:, None, None, None]))
    return lp64.detach(), c64, x64.grad


def _fused(x, labels, xn, yn, up):
    from warp_rnnt_amd.fused import rnnt_loss_from_logits
    z = x.detach().requires_grad_(True)          # (the tensor itself: a clone would realign a view)
    costs = rnnt_loss_from_logits(z, labels, xn, yn, fastemit_lambda=LAM)
    costs.backward(up)
    return costs.detach(), z.grad


@pytest.mark.parametrize("V,aligned,norm,gather,bwd", CASES, ids=[f"V{c[0]}{'' if c[1] else '-unaligned'}" for c in CASES])
def test_every_planned_family_computes_the_log_softmax_and_the_fused_loss(V, aligned, norm, gather, bwd):
    from warp_rnnt_amd import debug, ops
    for name in DTYPES:
        facts = dict(dtype=name, rows=ROWS, V=V, aligned=aligned)
        plan = debug.lsm_plan("norm", **facts)
        assert (plan["family"], plan["tail"]) == norm, (name, plan)
        assert debug.lsm_plan("gather", T=TM, U=UM, **facts)["family"] == gather, name
        assert debug.lsm_plan("bwd", T=TM, U=UM, **facts)["family"] == bwd, name
    logits, labels, xn, yn = make_case(900 + V, N, TM, UM, V, ragged=True)
    up = np.random.RandomState(V).rand(N).astype(np.float32) + 0.5
    tl, txn, tyn, tup = (torch.tensor(a, device=DEV) for a in (labels, xn, yn, up))
    for name, dtype in DTYPES.items():
        xh = _place(torch.tensor(logits).to(dtype), aligned)
        x32 = _place(xh.float(), aligned)                       # the upcast, at the same alignment (the same plan)
        lp64, c64, dz64 = _reference(x32, labels, xn, yn, up)
        lp = ops.log_softmax(x32)
        err = (lp.double().cpu() - lp64).abs().max().item()
        assert err < 2e-6 * max(1.0, float(np.log(V))), (name, err)
        c32, g32 = _fused(x32, tl, txn, tyn, tup)
        np.testing.assert_allclose(c32.cpu().numpy(), c64, rtol=1e-5, err_msg=name)
        np.testing.assert_allclose(g32.cpu().numpy(), dz64.numpy(), atol=1e-4, err_msg=name)
        if dtype is not torch.float32:
            lh = ops.log_softmax(xh)
            assert lh.dtype == torch.float32 and torch.equal(lh, lp), name
            ch, gh = _fused(xh, tl, txn, tyn, tup)
            assert ch.dtype == torch.float32 and gh.dtype == dtype
            assert torch.equal(ch, c32), name
            assert torch.equal(gh, g32.to(dtype)), name
