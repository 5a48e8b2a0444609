"""The lattice sweeps (csrc/lattice_step.h, lattice_ws.hip, lattice_wd.hip, lattice.hip, lattice_single.h) and the gradient
kernel (grads.hip, grads_cell.h) held to an fp64 reference over the VALUE range of their log-prob pairs: the profiles, the
derived per-cell bound and the ratios are lattice_values.py's, the shapes the smallest that reach each kernel.

Per profile x shape x ragged setting:
  * the reference-named C entry (run_warp_rnnt_gather, called as test_gpu_parity._call_ref_abi does, the scratch kept): its
    alphas and betas -- un-skewed from the diagonal-major order include/warp_rnnt_amd.h documents -- its alpha-side
    log-likelihoods (the first N words of `counts`), costs and gradients.  Below 2^20 cells this entry sweeps the caller's
    row-major pairs with the single-role kernel whatever the pin says (csrc/lattice_plan.h: only the diagonal-major loader
    reaches the column-block kernels), so
  * the pinned legs -- auto, ws, wd, wl -- go through the native entry on a workspace of the test's own (what ops.loss
    does), which keeps the lattices of the kernel that ran: alphas at offset 0 of the workspace, betas behind them;
  * every leg: error / bound <= 1 for every quantity (a derived bound), the rms of error / bound of alphas, betas and
    gradients at most 2 x the C oracle's on the same input + 0.01 (two fp32 implementations of one operation order, which
    differ in how exp and log1p are evaluated -- about an ulp of l each -- sit at one distance from fp64;
    test_gpu_baseline_sizes.py notes the same at the BASELINE shapes), dead gradient cells exactly 0, the guard silent;
  * costs, gradients and the live cells of both lattices bit-equal across the four pins and the C entry, and ops.loss
    gives the same costs and gradients.
Then every profile once through the compact entry and once through the dense one."""
import numpy as np
import pytest
import torch

import lattice_values as lv
from warp_rnnt_amd import debug, ops

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
PINS = ("auto", "ws", "wd", "wl")
RMS_FACTOR, RMS_SLACK = 2.0, 0.01
CASES = [(name, shape, ragged) for name in lv.PROFILES for shape in lv.SHAPES for ragged in (False, True)]
IDS = [f"{name}-{'x'.join(map(str, shape))}-{'ragged' if ragged else 'full'}" for name, shape, ragged in CASES]


def _t(a):
    return torch.tensor(np.ascontiguousarray(a), device=DEV)


def c_entry(pairs, xn, yn, lam=lv.LAMBDA):
    """run_warp_rnnt_gather with the reference binding's buffers: dict(costs, grads, alphas, betas (row-major), ll_a)."""
    import warp_rnnt_amd
    L = warp_rnnt_amd.load()
    N, T, U, _ = pairs.shape
    xs, txn, tyn = _t(pairs), _t(xn), _t(yn)
    grads = torch.zeros_like(xs)
    counts = torch.zeros((N, 2 * U), dtype=torch.int32, device=DEV)
    alphas = torch.empty((N, T, U), dtype=torch.float32, device=DEV)
    betas = torch.empty((N, T, U), dtype=torch.float32, device=DEV)
    costs = torch.empty((N,), dtype=torch.float32, device=DEV)
    st = L.run_warp_rnnt_gather(torch.cuda.current_stream().cuda_stream, counts.data_ptr(), alphas.data_ptr(),
                                betas.data_ptr(), xs.data_ptr(), grads.data_ptr(), costs.data_ptr(), txn.data_ptr(),
                                tyn.data_ptr(), N, T, U, lam)
    torch.cuda.synchronize()
    assert st == 0
    return dict(costs=costs.cpu().numpy(), grads=grads.cpu().numpy(), alphas=lv.unskew(alphas.cpu().numpy(), T, U),
                betas=lv.unskew(betas.cpu().numpy(), T, U), ll_a=counts.view(-1)[:N].view(torch.float32).cpu().numpy(),
                kernel=debug.last_lattice_kernel())


def native(xs, txn, tyn, lam=lv.LAMBDA):
    """rnnt_amd_loss on row-major pairs (tensors), as ops.loss calls it, on a workspace that is kept: the same dict, ll_a
    left out, and the guard's flags."""
    import warp_rnnt_amd
    L = warp_rnnt_amd.load()
    N, T, U, _ = xs.shape
    cells = N * T * U
    ws = torch.empty((L.rnnt_amd_workspace_size(N, T, U),), dtype=torch.uint8, device=DEV)
    costs = torch.empty((N,), dtype=torch.float32, device=DEV)
    grads = torch.empty((N, T, U, 2), dtype=torch.float32, device=DEV)
    st = L.rnnt_amd_loss(torch.cuda.current_stream().cuda_stream, ws.data_ptr(), ops.IN_LOG_PROBS_GATHERED, xs.data_ptr(),
                         None, txn.data_ptr(), tyn.data_ptr(), costs.data_ptr(), grads.data_ptr(), ops.GRADS_GATHERED,
                         N, T, U, 2, 0, lam)
    torch.cuda.synchronize()
    assert st == 0
    behind = (4 * cells + 255) // 256 * 256                       # every part of the workspace is 256-byte aligned
    planes = [ws[o:o + 4 * cells].view(torch.float32).cpu().numpy() for o in (0, behind)]
    off = L.rnnt_amd_workspace_mismatch_offset(N, T, U)
    return dict(costs=costs.cpu().numpy(), grads=grads.cpu().numpy(), alphas=lv.unskew(planes[0], T, U),
                betas=lv.unskew(planes[1], T, U), mismatch=ws[off:off + 4 * N].view(torch.int32).cpu().numpy(),
                kernel=debug.last_lattice_kernel())


def ratios_of(c, got, what):
    return lv.batch_ratios(c["refs"], c["xn"], c["yn"], got.get("alphas"), got.get("betas"), got["costs"], got.get("ll_a"),
                           got["grads"], what=what)


def hold(c, got, what):
    """The two assertions of a leg: the derived bound, and the oracle's distance from fp64 with its stated margin."""
    r = ratios_of(c, got, what)
    o = c["oracle_ratios"]
    print(f"{what}: worst/rms " + ", ".join(f"{k} {w:.3f}" + ("" if rms is None else f"/{rms:.4f} (oracle {o[k][1]:.4f})")
                                            for k, (w, rms) in r.items()))
    for k, (worst, rms) in r.items():
        assert worst <= 1.0, (what, k, worst)
        if rms is not None:
            assert rms <= RMS_FACTOR * o[k][1] + RMS_SLACK, (what, k, rms, o[k][1])
    return r


@pytest.mark.parametrize("name,shape,ragged", CASES, ids=IDS)
def test_every_kernel_holds_the_bound_and_gives_the_same_bits(name, shape, ragged):
    c = lv.case(name, shape, ragged)
    assert not c["oracle"]["mismatch"].any()
    xs, txn, tyn = _t(c["pairs"]), _t(c["xn"]), _t(c["yn"])
    ref_abi = c_entry(c["pairs"], c["xn"], c["yn"])
    hold(c, ref_abi, f"{name} {shape} C entry ({ref_abi['kernel']})")
    ran = {}
    for pin in PINS:
        with debug.lattice_kernel(pin):
            got = native(xs, txn, tyn)
        ran[pin] = got["kernel"]
        what = f"{name} {shape} pin {pin} ({got['kernel']})"
        assert not got["mismatch"].any(), what
        hold(c, got, what)
        np.testing.assert_array_equal(got["costs"], ref_abi["costs"], err_msg=what + f" against the C entry ({ref_abi['kernel']})")
        np.testing.assert_array_equal(got["grads"], ref_abi["grads"], err_msg=what + f" against the C entry ({ref_abi['kernel']})")
        for n in range(shape[0]):                                  # the lattices too, where they are defined: live cells
            Tn, Un = int(c["xn"][n]), int(c["yn"][n]) + 1
            for plane in ("alphas", "betas"):
                np.testing.assert_array_equal(got[plane][n, :Tn, :Un], ref_abi[plane][n, :Tn, :Un],
                                              err_msg=f"{what}: {plane}[{n}] against the C entry ({ref_abi['kernel']})")
    costs, grads = ops.loss(xs, None, txn, tyn, ops.IN_LOG_PROBS_GATHERED, ops.GRADS_GATHERED, fastemit_lambda=lv.LAMBDA)
    assert np.array_equal(costs.cpu().numpy(), ref_abi["costs"]) and np.array_equal(grads.cpu().numpy(), ref_abi["grads"])
    if torch.cuda.get_device_properties(DEV).multi_processor_count == 256:      # (MI355X: the kernel each shape is here for)
        want = {(2, 40, 33): ("auto", "lattice_wd"), (2, 40, 130): ("auto", "lattice_wl"), (2, 130, 400): ("wd", "lattice_wd"),
                (2, 60, 700): ("ws", "lattice (single role)"), (2, 1100, 70): ("auto", "lattice_wd"),
                (3, 1030, 129): ("wd", "lattice_wd")}[shape]
        assert ran[want[0]] == want[1], ran


def _dense_case(name):
    """Every profile at (3, 40, 130) ragged as dense log-probs of V = 6 (the other columns -1e30) with their labels."""
    c = lv.case(name, (3, 40, 130), True)
    dense, labels = lv.dense_from_pairs(c["pairs"])
    return c, dense, labels


@pytest.mark.parametrize("name", lv.PROFILES)
def test_compact_entry_holds_the_bound(name):
    c, dense, labels = _dense_case(name)
    xn, yn = c["xn"], c["yn"]
    N = len(xn)
    rows = np.concatenate([dense[n, :xn[n], :yn[n] + 1].reshape(-1, lv.V) for n in range(N)])
    ys = np.concatenate([labels[n, :yn[n]] for n in range(N)]).astype(np.int32)
    costs, grads, _ = ops.loss_compact(_t(rows), _t(ys), _t(xn), _t(yn), blank=0, fastemit_lambda=lv.LAMBDA)
    torch.cuda.synchronize()
    costs, grads = costs.cpu().numpy(), grads.cpu().numpy()
    padded = np.zeros(c["pairs"].shape, np.float32)
    at = 0
    for n in range(N):
        Tn, Un = int(xn[n]), int(yn[n]) + 1
        padded[n, :Tn, :Un] = grads[at:at + Tn * Un].reshape(Tn, Un, 2)
        at += Tn * Un
    assert at == len(grads)
    hold(c, dict(costs=costs, grads=padded), f"{name} compact ({debug.last_lattice_kernel()})")


@pytest.mark.parametrize("name", lv.PROFILES)
def test_dense_entry_gives_the_gathered_entrys_cost_bits(name):
    """The two loaders feed the same sweeps on these values."""
    c, dense, labels = _dense_case(name)
    txn, tyn = _t(c["xn"]), _t(c["yn"])
    cg, _ = ops.loss(_t(c["pairs"]), None, txn, tyn, ops.IN_LOG_PROBS_GATHERED, ops.GRADS_GATHERED, fastemit_lambda=lv.LAMBDA)
    cd, gd = ops.loss(_t(dense), _t(labels), txn, tyn, ops.IN_LOG_PROBS_DENSE, ops.GRADS_DENSE, fastemit_lambda=lv.LAMBDA)
    torch.cuda.synchronize()
    assert torch.equal(cd, cg), (cd, cg)
    assert torch.isfinite(gd).all()
