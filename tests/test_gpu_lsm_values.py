"""The log-softmax kernels across the logit VALUE range (lsm_values.py: profiles, fp64 reference, bound), over every family
the planner can name: the eleven (V, aligned) cases of test_gpu_lsm_routes.py -- 85 rows, the route assertions repeated
here -- times eight profiles times fp32, bf16 and fp16.

Per case, profile and dtype: (a) ops.log_softmax under the bound, -inf exactly where the reference has it, in place / the
blank plane / half inputs bit-equal; (b) ops.logits_backward with synthetic gradient pairs on EVERY row under the gradient
bound; (c) rnnt_loss_from_logits forward and backward against transduce_np on the fp64 log-probs and fp64 autograd, at the
project's tolerances; and at V = 50 and 1030 (d) the compact fused path against the dense one and the standalone
log_softmax_backward.  Every figure is printed before it is asserted (pytest -s)."""
import numpy as np
import pytest
import torch

import lsm_values as lv
from helpers import make_case
from test_gpu_lsm_routes import CASES, DEV, DTYPES, LAM, N, ROWS, TM, UM, _fused, _place, _reference

pytestmark = pytest.mark.gpu
# atol of d/d logits through the fused loss.  The project's 1e-4 everywhere but on the two peaked profiles, where it is the
# fp32 LATTICE that loses the digits, not the log-softmax: costs of 1e3 (spread10) to 6e4 (spread300) put an ulp of 6e-5 to
# 4e-3 on alpha + beta - log-likelihood, the exponent of every gradient pair.  Measured on the MI355X over the eleven cases
# and three dtypes (tools/lsm_value_range.py, profiles/lsm_value_range.txt), torch.log_softmax in fp32 followed by this
# library's loss on log-probs -- no kernel of this family in it -- is off fp64 autograd by 4.68e-4 at most on spread10 and by
# 8.49e-3 on spread300 (every other profile: under 6e-5); the tolerance there is 4x that chain's error, never anything
# the fused path itself reached (which was the same 4.68e-4 and 8.49e-3).
GRAD_ATOL = {"spread10": 4 * 4.68e-4, "spread300": 4 * 8.49e-3}
IDS = [f"V{c[0]}{'' if c[1] else '-unaligned'}" for c in CASES]


def _setup(V):
    _, labels, xn, yn = make_case(900 + V, N, TM, UM, V, ragged=True)
    z = lv.base(ROWS, V, 900 + V)
    up = np.random.RandomState(V).rand(N).astype(np.float32) + 0.5
    return z, labels, xn, yn, up


def _dev(*arrays):
    return tuple(torch.tensor(a, device=DEV) for a in arrays)


@pytest.mark.parametrize("name", lv.PROFILES)
@pytest.mark.parametrize("V,aligned,norm,gather,bwd", CASES, ids=IDS)
def test_every_family_over_the_value_range(V, aligned, norm, gather, bwd, name):
    from warp_rnnt_amd import debug, ops
    for dname in DTYPES:
        facts = dict(dtype=dname, rows=ROWS, V=V, aligned=aligned)
        plan = debug.lsm_plan("norm", **facts)
        assert (plan["family"], plan["tail"]) == norm, (dname, plan)
        assert debug.lsm_plan("gather", T=TM, U=UM, **facts)["family"] == gather, dname
        assert debug.lsm_plan("bwd", T=TM, U=UM, **facts)["family"] == bwd, dname
    z, labels, xn, yn, up = _setup(V)
    tl, txn, tyn, tup = _dev(labels, xn, yn, up)
    gB, gL, go = lv.pair_gradients(ROWS, V)
    lab = lv.cell_labels(labels[0], TM, UM)
    pairs = np.stack([gB, gL], -1).reshape(N, TM, UM, 2)
    diag, tgo = _dev(lv.to_diagonal(pairs), np.array([go], np.float32))
    shape = (N, TM, UM, V)
    for dname, dtype in DTYPES.items():
        tag = f"{name} {dname} V={V}{'' if aligned else ' unaligned'}"
        # (a) the plain log-softmax; the masked profile with its row of one finite entry
        xa = lv.profile(name, z, dtype, keep=np.unique(labels), single=True).view(shape)
        xa32 = _place(xa.float(), aligned)
        x64, lp64 = lv.reference(xa.reshape(ROWS, V))
        lp = ops.log_softmax(xa32)
        r = lv.log_prob_ratio(lp, x64, lp64)
        print(f"{tag}: log_softmax error / bound {r:.3f}")
        assert r <= 1.0, (tag, r)
        inplace = _place(xa.float(), aligned)
        ops.log_softmax(inplace, out=inplace)
        assert torch.equal(inplace, lp), tag
        planed = ops.log_softmax(xa32, blank_plane=True)
        plane = ops.blank_plane_of(planed, 0)
        assert plane is not None and torch.equal(planed, lp), tag
        assert torch.equal(plane, planed.reshape(ROWS, V)[:, 0].contiguous()), tag
        if dtype is not torch.float32:
            lh = ops.log_softmax(_place(xa, aligned))
            assert lh.dtype == torch.float32 and torch.equal(lh, lp), tag
        # (b) d/d logits from synthetic pairs on every row
        xh = _place(lv.profile(name, z, dtype, keep=np.unique(labels)).view(shape), aligned)
        x32 = _place(xh.float(), aligned)
        x64, lp64 = lv.reference(xh.reshape(ROWS, V))
        ref, bound = lv.gradient_reference(x64, lp64, gB, gL, go, lab)
        dz32 = ops.logits_backward(x32, tl, diag, tgo)
        r = lv.gradient_ratio(dz32, ref, bound, lp64)
        print(f"{tag}: logits_backward error / bound {r:.3f}")
        assert r <= 1.0, (tag, r)
        if dtype is not torch.float32:
            dzh = ops.logits_backward(xh, tl, diag, tgo)
            assert dzh.dtype == dtype and torch.equal(dzh, dz32.to(dtype)), tag
        # (c) logits -> loss -> d/d logits
        _, c64, dz64 = _reference(x32, labels, xn, yn, up)
        c32, g32 = _fused(x32, tl, txn, tyn, tup)
        cerr = np.abs(c32.cpu().numpy() / c64 - 1).max()
        gerr = (g32.double().cpu() - dz64).abs().max().item()
        print(f"{tag}: fused costs {c64}, relative error {cerr:.2e}; d/d logits error {gerr:.2e}")
        np.testing.assert_allclose(c32.cpu().numpy(), c64, rtol=1e-5, err_msg=tag)
        np.testing.assert_allclose(g32.cpu().numpy(), dz64.numpy(), atol=GRAD_ATOL.get(name, 1e-4), err_msg=tag)
        if dtype is not torch.float32:
            ch, gh = _fused(xh, tl, txn, tyn, tup)
            assert ch.dtype == torch.float32 and gh.dtype == dtype
            assert torch.equal(ch, c32) and torch.equal(gh, g32.to(dtype)), tag


@pytest.mark.parametrize("name", lv.PROFILES)
@pytest.mark.parametrize("V", [50, 1030])
def test_compact_fused_path_and_standalone_backward(V, name):
    from warp_rnnt_amd import ops
    z, labels, xn, yn, up = _setup(V)
    assert xn[0] == TM and yn[0] == UM - 1         # one utterance, full lengths: its packed rows are the dense ones
    tl, txn, tyn, tup = _dev(labels, xn, yn, up)
    tys = tl.reshape(-1).contiguous()
    gB, gL, _ = lv.pair_gradients(ROWS, V)
    lab = lv.cell_labels(labels[0], TM, UM)
    dy = np.zeros((ROWS, V), np.float32)
    dy[:, 0] += gB
    np.add.at(dy, (np.arange(ROWS), lab), gL)
    for dname, dtype in DTYPES.items():
        tag = f"{name} {dname} V={V}"
        xh = lv.profile(name, z, dtype, keep=np.unique(labels)).to(DEV)
        # compact fused = dense fused, at the tolerances of test_gpu_compact_logits (fused against the chain)
        cd, gd = _fused(xh.view(N, TM, UM, V), tl, txn, tyn, tup)
        cc, pairs, offs, loffs = ops.loss_compact_logits(xh, tys, txn, tyn, 0, LAM)
        gc = ops.compact_logits_backward(xh, tys, txn, tyn, offs, loffs, pairs, tup)
        assert gc.dtype == dtype
        np.testing.assert_allclose(cc.cpu().numpy(), cd.cpu().numpy(), rtol=2e-6, err_msg=tag)
        np.testing.assert_allclose(gc.float().cpu().numpy(), gd.float().reshape(ROWS, V).cpu().numpy(), rtol=1e-4, atol=2e-6,
                                   err_msg=tag)
        # log_softmax_backward(dy, y), y the fp64 log-probs rounded to fp32, dy the pairs a loss would send: gs = rowsum(dy)
        x64, lp64 = lv.reference(xh)
        ref, bound = lv.gradient_reference(x64, lp64, gB, gL, 1.0, lab)
        y = torch.tensor(lp64.astype(np.float32), device=DEV)
        dx = ops.log_softmax_backward(torch.tensor(dy, device=DEV), y)
        r = lv.gradient_ratio(dx, ref, bound, lp64)
        print(f"{tag}: log_softmax_backward error / bound {r:.3f}")
        assert r <= 1.0, (tag, r)
