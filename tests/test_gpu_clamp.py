"""The gradient clamp of the fused path on the GPU (include/warp_rnnt_amd_clamp.h, warp_rnnt_amd.compat):

    u[v]  = [v==blank] gB + [v==label] gL - softmax(z)[v] (gB + gL)        (unit upstream)
    dz[v] = s_n * min(max(u[v], -c), +c)

(a) ops.logits_backward(clamp=c) in every family the backward's planner names, against fp64, with synthetic gradient pairs
on every row and one upstream scale per utterance; (b) nothing that was there moved; (c) the compact layout; (d) end to
end through compat.rnnt_loss / compat.RNNTLoss; (e) one graph capture.

Reference and bound of (a) and (c), per utterance with scale go: ref1, bound1 = lsm_values.gradient_reference at unit
upstream, ref = go * clip(ref1, +-c), tol = go * bound1 + 2 * 2^-24 |ref| -- clip is 1-Lipschitz, so the unclamped bound
carries over, and the added term is the rounding of the final product (and of c itself).  Nothing in it is a measured
number.  Every figure is printed before it is asserted (pytest -s)."""
import numpy as np
import pytest
import torch

import lsm_values as lv
from helpers import make_case
from oracle import transduce_np
from test_gpu_lsm_routes import _place

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, T, U = 3, 16, 12
PER = T * U
ROWS = N * PER                          # 576: more than one LDS tile at every V <= 1024 but V = 5
GO = np.array([0.5, 1.0, 1.5], np.float32)
CLAMPS = (0.25, 0.01)
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
EPS = 2.0 ** -24

# V, aligned, family of the fused d/d logits -- and what the V reaches inside it
CASES = [
    (5, True, "small"), (16, True, "small"),                              # L = 1; the run-time and the 16-column loop
    (28, True, "small"), (32, True, "small"), (37, True, "small"), (50, True, "small"),   # ... L = 4, q = 10 / 13
    (100, True, "small"), (128, True, "small"), (130, True, "small"),     # ... L = 16, q = 9
    (256, True, "small"), (600, True, "small"), (1000, True, "small"), (1024, True, "small"),   # L = 64, q = 16
    (1028, True, "large"), (5000, True, "large"), (8196, True, "large"),  # 256 x 4, 256 x 8, 512 x 8
    (1030, True, "generic"), (16388, True, "generic"),
    (50, False, "generic"),                                               # a view one element off the vector grid
]
IDS = [f"V{v}{'' if a else '-unaligned'}" for v, a, _ in CASES]


def _dev(a, dtype=None):
    return torch.tensor(a, device=DEV, dtype=dtype)


def _labels(V, blank, shape):
    """Drawn with RandomState(V), never the blank."""
    choices = np.array([v for v in range(V) if v != blank], np.int32)
    return choices[np.random.RandomState(V).randint(0, len(choices), size=shape)].astype(np.int32)


def _unit_reference(xh, gB, gL, lab, blank):
    """fp64, rows of ONE utterance: (ref1, bound1) of d/d logits at unit upstream, and where the logits are masked."""
    x64, lp64 = lv.reference(xh)
    ref1, bound1 = lv.gradient_reference(x64, lp64, gB, gL, 1.0, lab, blank)
    return ref1, bound1, np.isneginf(lp64)


def _check_clamped(got, unit, go, c, tag):
    """got (rows, V) fp32 on the host against ref = go * clip(ref1, +-c) under tol (module docstring): the bound
    everywhere, the saturated elements EXACTLY fp32(+-c) * fp32(go) -- the clamp in front of the scale, with the right
    sign -- and exact zeros at masked logits.  Returns error / bound and the elements saturated at each sign and inside."""
    ref1, bound1, masked = unit
    ref = float(go) * np.clip(ref1, -c, c)
    tol = float(go) * bound1 + 2 * EPS * np.abs(ref)
    got = got.astype(np.float64)
    assert np.isfinite(got).all(), tag
    ratio = float((np.abs(got - ref) / tol)[~masked].max())
    assert (got[masked] == 0).all(), f"{tag}: non-zero gradient at a masked logit"
    hi, lo = ref1 > c + bound1, ref1 < -c - bound1
    sat = float(np.float32(c) * np.float32(go))
    assert (got[hi] == sat).all() and (got[lo] == -sat).all(), f"{tag}: a saturated element is not exactly +-c * go"
    return ratio, int(hi.sum()), int(lo.sum()), int((np.abs(ref1) < c - bound1).sum())


# plain at the three storage types; masked and spread10 at fp32 (the arithmetic behind the load is the same code).  Two
# groups, so that the fp64 reference of a case stays at a few seconds at V = 16388.
PROFILE_GROUPS = {"plain": [("plain", d) for d in DTYPES], "masked-spread10": [("masked", "f32"), ("spread10", "f32")]}


@pytest.mark.parametrize("group", list(PROFILE_GROUPS))
@pytest.mark.parametrize("blank_last", [False, True], ids=["blank0", "blankV-1"])
@pytest.mark.parametrize("V,aligned,family", CASES, ids=IDS)
def test_clamped_backward_in_every_family(V, aligned, family, blank_last, group):
    from warp_rnnt_amd import debug, ops
    for dname in DTYPES:
        plan = debug.lsm_plan("bwd", dtype=dname, rows=ROWS, V=V, T=T, U=U, aligned=aligned)
        assert plan["family"] == family, (dname, plan)
    blank = V - 1 if blank_last else 0
    labels = _labels(V, blank, (N, U - 1))
    keep = np.unique(np.concatenate([labels.reshape(-1), [blank]]))
    z = lv.base(ROWS, V, 7 + V)
    gB, gL, _ = lv.pair_gradients(ROWS, 7 + V)
    diag = _dev(lv.to_diagonal(np.stack([gB, gL], -1).reshape(N, T, U, 2)))
    tl, tgo, ones = _dev(labels), _dev(GO), _dev(np.ones(N, np.float32))
    shape = (N, T, U, V)
    for name, dname in PROFILE_GROUPS[group]:
        dtype = DTYPES[dname]
        xh = lv.profile(name, z, dtype, keep=keep)
        dxh = _place(xh.view(shape), aligned)
        dx32 = dxh if dtype is torch.float32 else _place(xh.float().view(shape), aligned)
        base = ops.logits_backward(dx32, tl, diag, tgo, blank)
        # (b) nothing that was there moved: clamp=0.0 is the call without the keyword, and a clamp nothing reaches at
        # unit upstream gives the unclamped bits
        assert torch.equal(ops.logits_backward(dx32, tl, diag, tgo, blank, clamp=0.0), base)
        unit = ops.logits_backward(dx32, tl, diag, ones, blank)
        assert torch.equal(ops.logits_backward(dx32, tl, diag, ones, blank, clamp=1e30), unit), (name, dname)
        if dtype is not torch.float32:
            assert torch.equal(ops.logits_backward(dxh, tl, diag, tgo, blank, clamp=0.0),
                               ops.logits_backward(dxh, tl, diag, tgo, blank))
            assert torch.equal(ops.logits_backward(dxh, tl, diag, ones, blank, clamp=1e30),
                               ops.logits_backward(dxh, tl, diag, ones, blank)), (name, dname)
        units = [_unit_reference(xh[n * PER:(n + 1) * PER], gB[n * PER:(n + 1) * PER], gL[n * PER:(n + 1) * PER],
                                 lv.cell_labels(labels[n], T, U, blank), blank) for n in range(N)]
        for c in CLAMPS:
            tag = f"{name} {dname} V={V}{'' if aligned else ' unaligned'} blank={blank} clamp={c}"
            dz32 = ops.logits_backward(dx32, tl, diag, tgo, blank, clamp=c)
            assert dz32.dtype == torch.float32 and dz32.shape == shape
            got = dz32.cpu().numpy().reshape(N, PER, V)
            worst, hi, lo, inside = 0.0, 0, 0, 0
            for n in range(N):
                r, h, l, i = _check_clamped(got[n], units[n], GO[n], c, f"{tag} n={n}")
                worst, hi, lo, inside = max(worst, r), hi + h, lo + l, inside + i
            print(f"{tag}: error / bound {worst:.3f}; saturated +{hi} -{lo}, inside {inside}")
            assert worst <= 1.0, (tag, worst)
            if name == "plain":       # the case exercises the clamp at both signs and leaves elements alone
                assert hi >= 256 and lo >= 256 and inside >= 256, (tag, hi, lo, inside)
            if dtype is not torch.float32:
                dzh = ops.logits_backward(dxh, tl, diag, tgo, blank, clamp=c)
                assert dzh.dtype == dtype and torch.equal(dzh, dz32.to(dtype)), tag


def test_from_logits_without_clamp_is_the_direct_calls():
    """rnnt_loss_from_logits(...) without the keyword: the bits of ops.loss + ops.logits_backward called directly."""
    from warp_rnnt_amd import ops
    from warp_rnnt_amd.fused import rnnt_loss_from_logits
    for V in (50, 1030, 5000):
        logits, labels, xn, yn = make_case(1200 + V, 3, 17, 5, V, ragged=True)
        tl, txn, tyn, up = _dev(labels), _dev(xn), _dev(yn), _dev(GO)
        for dtype in DTYPES.values():
            x = _dev(logits).to(dtype)
            costs, grads = ops.loss(x, tl, txn, tyn, ops.IN_LOGITS_DENSE, ops.GRADS_GATHERED_DIAGONAL, 0, 0.0)
            direct = ops.logits_backward(x, tl, grads, up, 0)
            z = x.clone().requires_grad_(True)
            c = rnnt_loss_from_logits(z, tl, txn, tyn)
            c.backward(up)
            assert torch.equal(c.detach(), costs) and torch.equal(z.grad, direct), (V, dtype)
            z0 = x.clone().requires_grad_(True)
            rnnt_loss_from_logits(z0, tl, txn, tyn, clamp=0.0).backward(up)
            assert torch.equal(z0.grad, direct), (V, dtype)


# ---- (c) compact ----
XN, YN = np.array([16, 9, 1], np.int32), np.array([11, 4, 0], np.int32)
CELLS = XN.astype(np.int64) * (YN + 1)
STU = int(CELLS.sum())                   # 238
EXTRA = 5                                # appended rows that belong to no utterance


@pytest.mark.parametrize("V,family", [(50, "small"), (1030, "generic"), (5000, "large")])
def test_clamped_compact_backward(V, family):
    from warp_rnnt_amd import debug, ops
    blank = 0
    offs = np.concatenate([[0], np.cumsum(CELLS)]).astype(np.int64)
    loffs = np.concatenate([[0], np.cumsum(YN)]).astype(np.int32)
    ys = _labels(V, blank, (int(YN.sum()),))
    keep = np.unique(np.concatenate([ys, [blank]]))
    rows = STU + EXTRA
    z = lv.base(rows, V, 7 + V)
    gB, gL, _ = lv.pair_gradients(rows, 7 + V)
    pairs = _dev(np.stack([gB, gL], -1))
    tys, txn, tyn, toffs, tloffs, tgo = _dev(ys), _dev(XN), _dev(YN), _dev(offs), _dev(loffs), _dev(GO)
    for dname in ("f32", "bf16"):
        dtype = DTYPES[dname]
        assert debug.lsm_plan("bwd", dtype=dname, rows=rows, V=V, compact=True)["family"] == family
        xh = lv.profile("plain", z, dtype, keep=keep)
        dxh, dx32 = xh.to(DEV), xh.float().to(DEV)
        args = (tys, txn, tyn, toffs, tloffs, pairs, tgo, blank)
        base = ops.compact_logits_backward(dx32, *args)
        assert torch.equal(ops.compact_logits_backward(dx32, *args, clamp=0.0), base)
        for c in CLAMPS:
            tag = f"compact {dname} V={V} clamp={c}"
            dz32 = ops.compact_logits_backward(dx32, *args, clamp=c)
            got = dz32.cpu().numpy()
            assert (got[STU:] == 0).all(), f"{tag}: rows that belong to no utterance must come back zero"
            worst = 0.0
            for n in range(N):
                r0, r1 = int(offs[n]), int(offs[n + 1])
                lab = lv.cell_labels(ys[loffs[n]:loffs[n + 1]], int(XN[n]), int(YN[n]) + 1, blank)
                unit = _unit_reference(xh[r0:r1], gB[r0:r1], gL[r0:r1], lab, blank)
                worst = max(worst, _check_clamped(got[r0:r1], unit, GO[n], c, f"{tag} n={n}")[0])
            print(f"{tag}: error / bound {worst:.3f}")
            assert worst <= 1.0, (tag, worst)
            if dtype is not torch.float32:
                dzh = ops.compact_logits_backward(dxh, *args, clamp=c)
                assert dzh.dtype == dtype and torch.equal(dzh, dz32.to(dtype)), tag


def _fp64_unit_gradients(x32, labels, xn, yn, blank):
    """fp64 costs and d cost_n / d logits (unit upstream) of dense (N,T,U,V) logits: transduce_np on fp64 log-probs, fp64
    autograd through torch.log_softmax."""
    x64 = x32.double().cpu().requires_grad_(True)
    lp64 = torch.log_softmax(x64, -1)
    c64, g64 = transduce_np.transduce_batch(lp64.detach().numpy(), labels, xn, yn, blank=blank, fast=True)
    lp64.backward(torch.from_numpy(g64))
    return c64, x64.grad.numpy()


@pytest.mark.parametrize("V", [50, 1030, 5000])
def test_clamped_compact_from_logits(V):
    """rnnt_loss_from_logits(compact=True, clamp=c), with and without the launch bounds, against fp64: every utterance's
    block of packed rows is a dense (1, T_n, U_n, V) case."""
    from warp_rnnt_amd.fused import rnnt_loss_from_logits
    blank = 0
    offs = np.concatenate([[0], np.cumsum(CELLS)])
    loffs = np.concatenate([[0], np.cumsum(YN)])
    ys = _labels(V, blank, (int(YN.sum()),))
    packed = np.random.RandomState(1200 + V).randn(STU, V).astype(np.float32)
    c64, d64 = np.zeros(N), np.zeros((STU, V))
    for n in range(N):
        Tn, Un = int(XN[n]), int(YN[n]) + 1
        block = torch.tensor(packed[offs[n]:offs[n + 1]].reshape(1, Tn, Un, V))
        lab = ys[loffs[n]:loffs[n + 1]].reshape(1, Un - 1)
        c, d = _fp64_unit_gradients(block, lab, XN[n:n + 1], YN[n:n + 1], blank)
        c64[n], d64[offs[n]:offs[n + 1]] = c[0], d.reshape(-1, V)
    tys, txn, tyn, tgo = _dev(ys), _dev(XN), _dev(YN), _dev(GO)
    for dname in ("f32", "bf16"):
        x = _dev(packed).to(DTYPES[dname])
        for c in CLAMPS:
            results = []
            for bounds in ({}, dict(max_frames=16, max_labels=11)):
                zc = x.clone().requires_grad_(True)
                costs = rnnt_loss_from_logits(zc, tys, txn, tyn, blank=blank, compact=True, clamp=c, **bounds)
                costs.backward(tgo)
                results.append((costs.detach(), zc.grad))
            assert torch.equal(results[0][0], results[1][0]) and torch.equal(results[0][1], results[1][1]), (V, dname, c)
            costs, grad = results[0]
            assert costs.dtype == torch.float32 and grad.dtype == DTYPES[dname]
            if dname == "f32":
                ref = np.repeat(GO, CELLS)[:, None] * np.clip(d64, -c, c)
                err = np.abs(grad.cpu().numpy() - ref).max()
                print(f"compact from logits V={V} clamp={c}: costs {costs.tolist()}, d/d logits error {err:.2e}")
                np.testing.assert_allclose(costs.cpu().numpy(), c64, rtol=1e-5)
                np.testing.assert_allclose(grad.cpu().numpy(), ref, atol=1e-4)
            else:                 # bf16 logits: the bits of the run on their upcast, its gradients rounded once
                z32 = x.float().requires_grad_(True)
                c32 = rnnt_loss_from_logits(z32, tys, txn, tyn, blank=blank, compact=True, clamp=c)
                c32.backward(tgo)
                assert torch.equal(costs, c32.detach()) and torch.equal(grad, z32.grad.to(torch.bfloat16)), (V, c)


# ---- (d) end to end through compat ----
COMPAT_CLAMP = 0.002


@pytest.fixture(scope="module")
def compat_reference():
    """fp64 costs and unit-upstream d/d logits of make_case(1200 + V, 3, 17, 5, V, ragged, blank), computed once per case."""
    cache = {}

    def get(V, blank):
        if (V, blank) not in cache:
            logits, labels, xn, yn = make_case(1200 + V, 3, 17, 5, V, ragged=True, blank=blank)
            c64, d64 = _fp64_unit_gradients(torch.tensor(logits), labels, xn, yn, blank)
            cache[V, blank] = (logits, labels, xn, yn, c64, d64)
        return cache[V, blank]
    return get


@pytest.mark.parametrize("reduction", ["sum", "mean"])
@pytest.mark.parametrize("blank_arg", [0, -1])
@pytest.mark.parametrize("V", [28, 1030, 5000])
def test_compat_rnnt_loss_end_to_end(V, blank_arg, reduction, compat_reference):
    from warp_rnnt_amd import compat
    from warp_rnnt_amd.fused import rnnt_loss_from_logits
    blank = blank_arg % V
    logits, labels, xn, yn, c64, d64 = compat_reference(V, blank)
    c, scale = COMPAT_CLAMP, {"sum": 1.0, "mean": 1.0 / 3}[reduction]
    ref = scale * np.clip(d64, -c, c)
    hi, lo, inside = int((d64 > c + 1e-4).sum()), int((d64 < -c - 1e-4).sum()), int((np.abs(d64) < c - 1e-4).sum())
    assert hi >= 128 and lo >= 128 and inside >= 1024, (hi, lo, inside)
    tl, txn, tyn = _dev(labels), _dev(xn), _dev(yn)
    z = _dev(logits).requires_grad_(True)
    loss = compat.rnnt_loss(z, tl, txn, tyn, blank=blank_arg, clamp=c, reduction=reduction)
    loss.backward()
    want = c64.sum() if reduction == "sum" else c64.mean()
    got = z.grad.cpu().numpy()
    print(f"V={V} blank={blank} {reduction}: loss {loss.item():.6f} (fp64 {want:.6f}), d/d logits error "
          f"{np.abs(got - ref).max():.2e}; saturated +{hi} -{lo}, inside {inside}")
    np.testing.assert_allclose(loss.item(), want, rtol=1e-5)
    np.testing.assert_allclose(got, ref, atol=1e-4)
    np.testing.assert_allclose(got[d64 > c + 1e-4], c * scale, rtol=1e-6)
    np.testing.assert_allclose(got[d64 < -c - 1e-4], -c * scale, rtol=1e-6)
    # the per-utterance costs too
    none = compat.rnnt_loss(z.detach(), tl, txn, tyn, blank=blank_arg, clamp=c, reduction="none")
    np.testing.assert_allclose(none.cpu().numpy(), c64, rtol=1e-5)
    # the module is the function
    zm = _dev(logits).requires_grad_(True)
    lm = compat.RNNTLoss(blank=blank_arg, clamp=c, reduction=reduction)(zm, tl, txn, tyn)
    lm.backward()
    assert torch.equal(lm.detach(), loss.detach()) and torch.equal(zm.grad, z.grad)
    # bf16 logits: fp32 costs, the bits of the run on the upcast; its gradients rounded once
    zh = _dev(logits).to(torch.bfloat16).requires_grad_(True)
    zu = zh.detach().float().requires_grad_(True)
    lh = compat.rnnt_loss(zh, tl, txn, tyn, blank=blank_arg, clamp=c, reduction=reduction)
    lu = compat.rnnt_loss(zu, tl, txn, tyn, blank=blank_arg, clamp=c, reduction=reduction)
    lh.backward()
    lu.backward()
    assert lh.dtype == torch.float32 and zh.grad.dtype == torch.bfloat16
    assert torch.equal(lh.detach(), lu.detach()) and torch.equal(zh.grad, zu.grad.to(torch.bfloat16))
    # clamp=-1 (off) is rnnt_loss_from_logits without a clamp, bit for bit
    z1 = _dev(logits).requires_grad_(True)
    z2 = _dev(logits).requires_grad_(True)
    l1 = compat.rnnt_loss(z1, tl, txn, tyn, blank=blank_arg, clamp=-1, reduction=reduction)
    l2 = rnnt_loss_from_logits(z2, tl, txn, tyn, reduction=reduction, blank=blank)
    l1.backward()
    l2.backward()
    assert torch.equal(l1.detach(), l2.detach()) and torch.equal(z1.grad, z2.grad)


def test_compat_log_probs_route():
    """fused_log_softmax=False with the clamp off: the inputs are log-probs, the existing gathered route."""
    import warp_rnnt
    from warp_rnnt_amd import compat
    V = 28
    logits, labels, xn, yn = make_case(1200 + V, 3, 17, 5, V, ragged=True, blank=V - 1)
    tl, txn, tyn = _dev(labels), _dev(xn), _dev(yn)
    lp1 = torch.log_softmax(_dev(logits), -1).requires_grad_(True)
    lp2 = lp1.detach().clone().requires_grad_(True)
    a = compat.rnnt_loss(lp1, tl, txn, tyn, fused_log_softmax=False)
    b = warp_rnnt.rnnt_loss(lp2, tl, txn, tyn, reduction="mean", gather=True, blank=V - 1)
    a.backward()
    b.backward()
    assert torch.equal(a.detach(), b.detach()) and torch.equal(lp1.grad, lp2.grad)


# ---- (e) capture ----
def test_compat_rnnt_loss_captures():
    from warp_rnnt_amd import compat
    V = 50
    logits, labels, xn, yn = make_case(1200 + V, 2, 17, 5, V, ragged=True)
    tl, txn, tyn = _dev(labels), _dev(xn), _dev(yn)
    x = _dev(logits)
    z = x.clone().requires_grad_(True)
    eager = compat.rnnt_loss(z, tl, txn, tyn, blank=0, clamp=COMPAT_CLAMP)
    eager.backward()
    assert (z.grad.abs() == COMPAT_CLAMP / 2).sum() >= 16        # (mean over two utterances; the clamp is reached)
    static = x.clone().requires_grad_(True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                 # warm-up off the capture, as torch's notes ask
        compat.rnnt_loss(static, tl, txn, tyn, blank=0, clamp=COMPAT_CLAMP).backward()
    torch.cuda.current_stream().wait_stream(side)
    static.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss = compat.rnnt_loss(static, tl, txn, tyn, blank=0, clamp=COMPAT_CLAMP)
        loss.backward()
    loss.zero_()
    static.grad.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(loss.detach(), eager.detach()) and torch.equal(static.grad, z.grad)
