"""The smoothed simple transducer loss on the GPU: warp_rnnt_amd.simple.simple_rnnt_loss, am (N,T,V), lm (N,U,V) -> costs,
gradient pairs -> d/d am, d/d lm.

Against fp64 (tests/simple_reference.py: simple_loss64) over a grid of shapes that crosses every edge of the kernels'
tiles -- 64 x 64 result tiles in steps of 32 along K, where K is V (the producer), U (d am) and T (d lm) -- with ragged
lengths, three blank positions, five pairs of smoothing scales, FastEmit, upstream gradients that are not 1, repeated
labels, an utterance of one frame and one without labels, and each of the three sweep kernels.  The bars are not taken from
the code under test: they are four times the largest error of the UNFUSED chain (simple_reference.chain32: the same
definition in plain fp32 torch, warp_rnnt.rnnt_loss(blank=-1) and autograd) on the same inputs, measured once by
tools/simple_loss_values.py -- profiles/simple_loss_values.txt holds every figure, the fused entry's beside the
yardstick's.  4x is the project's margin between two fp32 orders of summation of one formula.  Then what holds bit for
bit, the zeros, reductions, graph capture and the pruned recipe end to end on this first pass.

Every figure is printed before it is asserted (pytest -s)."""
import functools

import numpy as np
import pytest
import torch

import simple_reference as sr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 2.0 ** -24

# (N, T, U, V)
GRID = [(3, 12, 6, 2),           # an utterance of one frame and one without labels
        (2, 21, 9, 63), (2, 21, 9, 64), (2, 21, 9, 65), (2, 70, 35, 130), (2, 130, 67, 257), (2, 33, 17, 1025),
        # one shape per sweep kernel, chosen with the pure planner of lattice_plan.h (KERNEL_OF below)
        (2, 40, 130, 8), (2, 60, 400, 8), (2, 2048, 260, 8)]
KERNEL_OF = {(2, 40, 130, 8): "lattice_wl", (2, 60, 400, 8): "lattice_ws", (2, 2048, 260, 8): "lattice_wd"}
SCALES = [(0.0, 0.0), (0.25, 0.0), (0.25, 0.1), (0.6, 0.4), (0.0, 0.3)]
LAMS = (0.0, 0.01)
FIGURES = ("cost rel", "pair_grads abs", "d am abs", "d lm abs", "d lm through q abs")

# profiles/simple_loss_values.txt (tools/simple_loss_values.py on an MI355X): the unfused chain, chain32, per shape of GRID
# over its blanks x SCALES with the lambdas of lam_of() -- largest |cost - fp64| / |fp64|, largest |pair_grads - fp64|, and the
# largest |d am - fp64|, |d lm - fp64| (q held fixed) and |d lm - fp64| (through q) at the upstream gradients 0.5 + 0.25 n.
# (The gradients' errors are the lattice's: one ulp of a lattice value is 1.2e-4 to 4.9e-4 at costs of 1e3 to 5e3, and d lm
#  sums the occupancies of up to 2048 frames.  The fused entry's largest figure is at most 1.51x the yardstick's, at
#  (3, 12, 6, 2); the file holds every one.)
YARDSTICK = {
    (3, 12, 6, 2): (2.982e-07, 1.907e-06, 5.049e-07, 6.610e-07, 6.831e-07),
    (2, 21, 9, 63): (2.086e-07, 6.104e-05, 2.987e-05, 2.161e-04, 2.161e-04),
    (2, 21, 9, 64): (2.347e-07, 4.818e-05, 3.828e-05, 2.046e-04, 2.058e-04),
    (2, 21, 9, 65): (2.662e-07, 5.204e-05, 3.302e-05, 2.154e-04, 2.154e-04),
    (2, 70, 35, 130): (2.460e-07, 2.246e-04, 3.226e-04, 1.577e-03, 1.597e-03),
    (2, 130, 67, 257): (4.970e-07, 9.770e-04, 2.418e-03, 4.205e-02, 4.205e-02),
    (2, 33, 17, 1025): (2.418e-07, 1.329e-04, 1.208e-04, 1.159e-03, 1.159e-03),
    (2, 40, 130, 8): (4.761e-07, 2.441e-04, 5.804e-04, 4.215e-04, 4.215e-04),
    (2, 60, 400, 8): (5.359e-07, 1.016e-03, 8.757e-03, 7.795e-03, 7.800e-03),
    (2, 2048, 260, 8): (1.790e-06, 8.309e-03, 2.634e-02, 4.745e-01, 4.753e-01),
}


def bars_of(shape):
    """The five bars of a shape: four times the yardstick's largest errors there (costs: not below four fp32 epsilons)."""
    bars = {name: 4 * v for name, v in zip(FIGURES, YARDSTICK[tuple(shape)])}
    bars["cost rel"] = max(bars["cost rel"], 4 * EPS)        # relative to the fp64 cost
    return bars


def blanks_of(V):
    return (0, V - 1) if V == 2 else (0, V // 2, V - 1)


def lam_of(k, blank_index):
    """FastEmit of scale pair k at the blank_index-th blank: both values at every pair of scales, half the runs."""
    return LAMS[(k + blank_index) % 2]


GRID_CASES = [(shape, b) for shape in GRID for b in blanks_of(shape[3])]
GRID_IDS = ["N%d-T%d-U%d-V%d-b%d" % (*shape, b) for shape, b in GRID_CASES]


def _go(N):
    return sr.upstream(N).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _case(shape, blank, seed):
    N, T, U, V = shape
    lengths = ((T, 1, T // 2), (U - 1, 1, 0)) if shape == GRID[0] else None
    out = sr.make_case(1000 * V + 10 * T + blank + seed, N, T, U, V, blank=blank, lengths=lengths)
    for a in out:
        a.setflags(write=False)
    return out


def case(shape, blank, seed=0):
    """The inputs of a grid case on the host (read-only): am (N,T,V), lm (N,U,V) fp32 of scale 2, labels, xn, yn."""
    return _case(tuple(shape), blank, seed)


@functools.lru_cache(maxsize=None)
def reference(shape, blank, scales, lam):
    """fp64, computed once per case and shared (read-only)."""
    am, lm, labels, xn, yn = case(shape, blank)
    ref = sr.simple_loss64(am, lm, labels, xn, yn, blank, scales[0], scales[1], lam)
    for a in ref.values():
        a.setflags(write=False)
    return ref


def dev(a, dtype=None):
    return torch.tensor(np.asarray(a), device=DEV, dtype=dtype)


def fused_run(am, lm, labels, xn, yn, blank, scales=(0.0, 0.0), lam=0.0, go=None, grad=True):
    """costs (N,), pair_grads (N,T,U,2), d (sum_n go[n] cost[n]) / d am, / d lm (through q) for device tensors."""
    from warp_rnnt_amd.simple import simple_rnnt_loss
    a, l = am.detach().clone().requires_grad_(grad), lm.detach().clone().requires_grad_(grad)
    costs, pg = simple_rnnt_loss(a, l, labels, xn, yn, blank=blank, lm_only_scale=scales[0], am_only_scale=scales[1],
                                 fastemit_lambda=lam, return_grad=True)
    assert not pg.requires_grad and pg.dtype == torch.float32 and tuple(pg.shape) == (*am.shape[:2], lm.shape[1], 2)
    if not grad:
        return costs, pg, None, None
    g = torch.ones_like(costs) if go is None else go
    (costs * g).sum().backward()
    return costs.detach(), pg, a.grad, l.grad


def fused_fixed_q(am, lm, labels, xn, yn, blank, scales, lam, go):
    """d lm with q held fixed and d q, from the two functions of ops.py."""
    from warp_rnnt_amd import ops
    from warp_rnnt_amd.simple import batch_log_unigram
    q = batch_log_unigram(lm) if scales[1] != 0 else None
    _, pg, zn = ops.simple_loss(am, lm, q, labels, xn, yn, blank, scales[0], scales[1], lam)
    return ops.simple_backward(am, lm, q, labels, xn, yn, pg, zn, go, blank, scales[0], scales[1])


def _abs(got, want):
    return float(np.abs(got.detach().double().cpu().numpy() - want).max())


def errors(shape, blank, scales, lam):
    """One case on the GPU: (the fused entry's five figures, the yardstick's five, the sweep kernel the fused call ran)."""
    from warp_rnnt_amd import debug
    am, lm, labels, xn, yn = case(shape, blank)
    ref = reference(shape, blank, scales, lam)
    ta, tl, ty, txn, tyn, go = dev(am), dev(lm), dev(labels), dev(xn), dev(yn), dev(_go(shape[0]))
    costs, pg, dam, dlm = fused_run(ta, tl, ty, txn, tyn, blank, scales, lam, go)
    kernel = debug.last_lattice_kernel()
    _, dlm_fixed, _ = fused_fixed_q(ta, tl, ty, txn, tyn, blank, scales, lam, go)
    y = sr.chain32(ta, tl, ty, txn, tyn, blank, scales[0], scales[1], lam, go)
    y_fixed = sr.chain32(ta, tl, ty, txn, tyn, blank, scales[0], scales[1], lam, go, q_from_lm=False) if scales[1] else y
    for t in (costs, pg, dam, dlm, dlm_fixed):
        assert torch.isfinite(t).all()

    def five(c, p, da, dl_fixed, dl):
        c = c.double().cpu().numpy()
        return (float((np.abs(c - ref["costs"]) / np.abs(ref["costs"])).max()), _abs(p, ref["pair_grads"]),
                _abs(da, ref["dam"]), _abs(dl_fixed, ref["dlm"]), _abs(dl, ref["dlm_total"]))

    return (five(costs, pg, dam, dlm_fixed, dlm), five(y["costs"], y["pair_grads"], y["dam"], y_fixed["dlm"], y["dlm"]),
            kernel)


@pytest.mark.parametrize("shape,blank", GRID_CASES, ids=GRID_IDS)
def test_costs_and_gradients_against_fp64(shape, blank):
    from warp_rnnt_amd import debug
    BARS = bars_of(shape)
    for k, scales in enumerate(SCALES):
        lam = lam_of(k, blanks_of(shape[3]).index(blank))
        got, yard, kernel = errors(shape, blank, scales, lam)
        print(f"{shape} blank {blank} scales {scales} lam {lam}: " +
              "  ".join(f"{name} {g:.3e} (yardstick {y:.3e}, bar {BARS[name]:.3e})" for name, g, y in zip(FIGURES, got, yard)) +
              f"  {kernel}")
        for name, g in zip(FIGURES, got):
            assert g <= BARS[name], (name, shape, blank, scales, lam)
        if shape in KERNEL_OF:      # the producer carries no ring preparation: the unfolded plan
            assert kernel == KERNEL_OF[shape] == debug.lattice_plan(*shape[:3], folded=False).kernel, (shape, kernel)


def test_gradients_are_exactly_zero_outside_the_window_and_not_inside():
    shape, blank = (2, 70, 35, 130), 65
    am, lm, labels, xn, yn = case(shape, blank)
    assert (xn < shape[1]).any() and (yn + 1 < shape[2]).any()
    for scales in ((0.25, 0.0), (0.25, 0.1)):
        _, pg, dam, dlm = fused_run(dev(am), dev(lm), dev(labels), dev(xn), dev(yn), blank, scales, 0.01, dev(_go(shape[0])))
        _, dlm_fixed, _ = fused_fixed_q(dev(am), dev(lm), dev(labels), dev(xn), dev(yn), blank, scales, 0.01,
                                        dev(_go(shape[0])))
        for n in range(shape[0]):
            assert (dam[n, xn[n]:] == 0).all() and (dlm_fixed[n, yn[n] + 1:] == 0).all(), n
            assert (pg[n, xn[n]:] == 0).all() and (pg[n, :, yn[n] + 1:] == 0).all(), n
            assert (dam[n, :xn[n]] != 0).all() and (dlm_fixed[n, :yn[n] + 1] != 0).all(), n
            if scales[1] == 0:          # (through q every row of lm moves the batch unigram)
                assert (dlm[n, yn[n] + 1:] == 0).all() and torch.equal(dlm, dlm_fixed), n
    # an utterance whose upstream gradient is zero gets exactly zero rows
    go = dev(np.array([0.0, 0.75], np.float32))
    _, _, dam, dlm = fused_run(dev(am), dev(lm), dev(labels), dev(xn), dev(yn), blank, (0.25, 0.0), 0.0, go)
    assert (dam[0] == 0).all() and (dlm[0] == 0).all() and (dam[1] != 0).any() and (dlm[1] != 0).any()


# ---- bit for bit ----

HALF = {"bf16": torch.bfloat16, "f16": torch.float16}
BIT_SHAPES = [(2, 21, 9, 63), (2, 21, 9, 64), (2, 21, 9, 65), (2, 70, 35, 130), (2, 33, 17, 1025)]
BIT_IDS = ["N%d-T%d-U%d-V%d" % s for s in BIT_SHAPES]


def _blank_of(shape):
    return (0, shape[3] // 2, shape[3] - 1)[shape[3] % 3]


def _args(shape, blank):
    am, lm, labels, xn, yn = case(shape, blank)
    return dev(am), dev(lm), dev(labels), dev(xn), dev(yn), dev(_go(shape[0]))


@pytest.mark.parametrize("dname", list(HALF))
@pytest.mark.parametrize("shape", BIT_SHAPES, ids=BIT_IDS)
def test_half_precision_inputs_give_the_bits_of_their_upcast(shape, dname):
    blank = _blank_of(shape)
    a, l, ty, txn, tyn, go = _args(shape, blank)
    ah, lh = a.to(HALF[dname]), l.to(HALF[dname])
    for scales in ((0.25, 0.0), (0.25, 0.1)):
        h = fused_run(ah, lh, ty, txn, tyn, blank, scales, 0.01, go)
        f = fused_run(ah.float(), lh.float(), ty, txn, tyn, blank, scales, 0.01, go)
        assert h[0].dtype == torch.float32 and h[2].dtype == h[3].dtype == HALF[dname] and f[2].dtype == torch.float32
        assert torch.isfinite(h[0]).all() and (h[2] != 0).any() and (h[3] != 0).any()
        assert torch.equal(h[0], f[0]) and torch.equal(h[1], f[1])
        assert torch.equal(h[2], f[2].to(HALF[dname]))            # the fp32 result rounded once
        if scales[1] == 0:      # (through q, autograd adds a second half-precision term to d lm: compared at ops level)
            assert torch.equal(h[3], f[3].to(HALF[dname]))
        dh = fused_fixed_q(ah, lh, ty, txn, tyn, blank, scales, 0.01, go)
        df = fused_fixed_q(ah.float(), lh.float(), ty, txn, tyn, blank, scales, 0.01, go)
        assert torch.equal(dh[0], df[0].to(HALF[dname])) and torch.equal(dh[1], df[1].to(HALF[dname]))
        assert (dh[2] is None and df[2] is None) or torch.equal(dh[2], df[2])


@pytest.mark.parametrize("shape", BIT_SHAPES, ids=BIT_IDS)
def test_bits_depend_on_the_utterance_alone(shape):
    """With am_only_scale = 0: an utterance alone, in its batch and in the permuted batch; costs without gradients."""
    blank = _blank_of(shape)
    a, l, ty, txn, tyn, go = _args(shape, blank)
    scales = (0.25, 0.0)
    costs, pg, dam, dlm = fused_run(a, l, ty, txn, tyn, blank, scales, 0.01, go)
    only = fused_run(a, l, ty, txn, tyn, blank, scales, 0.01, grad=False)
    assert torch.equal(costs, only[0]) and torch.equal(pg, only[1])
    perm = torch.arange(shape[0] - 1, -1, -1, device=DEV)
    p = fused_run(*(t[perm].contiguous() for t in (a, l, ty, txn, tyn)), blank, scales, 0.01, go[perm].contiguous())
    for got, want in zip(p, (costs, pg, dam, dlm)):
        assert torch.equal(got, want[perm])
    for n in range(shape[0]):
        one = [t[n:n + 1].contiguous() for t in (a, l, ty, txn, tyn)]
        c1, p1, da1, dl1 = fused_run(*one, blank, scales, 0.01, go[n:n + 1].contiguous())
        assert torch.equal(c1, costs[n:n + 1]) and torch.equal(p1[0], pg[n]), n
        assert torch.equal(da1[0], dam[n]) and torch.equal(dl1[0], dlm[n]), n
        assert (dam[n] != 0).any() and (dlm[n] != 0).any(), n


@pytest.mark.parametrize("scales", [(0.25, 0.0), (0.25, 0.1)])
def test_two_runs_give_the_same_bits_with_repeated_labels(scales):
    shape, blank = (2, 130, 67, 257), 128
    am, lm, labels, xn, yn = case(shape, blank)
    assert all(len(set(labels[n, :yn[n]].tolist())) < yn[n] for n in range(shape[0]))          # labels repeat
    args = _args(shape, blank)
    first = fused_run(*args[:5], blank, scales, 0.01, args[5])
    for _ in range(2):
        again = fused_run(*args[:5], blank, scales, 0.01, args[5])
        assert all(torch.equal(x, y) for x, y in zip(first, again))


@pytest.mark.parametrize("dname", ["f32", "bf16"])
def test_an_address_that_narrows_the_access_moves_no_bit(dname):
    """Rows of 64 elements are 16-byte rows at every type, so here it is the tensors' addresses alone that narrow the
    access: the same am and lm in tensors of their own, and in contiguous slices that start one element into larger
    buffers.  The element map does not depend on the access: everything is equal bit for bit."""
    from warp_rnnt_amd import ops
    from warp_rnnt_amd.simple import batch_log_unigram
    dtype = {"f32": torch.float32, "bf16": torch.bfloat16}[dname]
    shape, blank = (2, 21, 9, 64), 21
    a, l, ty, txn, tyn, go = _args(shape, blank)

    def shifted(x):
        off = torch.empty(x.numel() + 1, dtype=x.dtype, device=DEV)[1:].view(x.shape)
        off.copy_(x)
        assert off.is_contiguous() and x.data_ptr() % 16 == 0 and off.data_ptr() % 16 == x.element_size()
        return off

    own = (a.to(dtype), l.to(dtype))
    q = batch_log_unigram(own[1])

    def both(am, lm):
        costs, pg, zn = ops.simple_loss(am, lm, q, ty, txn, tyn, blank, 0.25, 0.1, 0.01)
        return (costs, pg, zn) + ops.simple_backward(am, lm, q, ty, txn, tyn, pg, zn, go, blank, 0.25, 0.1)

    want = both(*own)
    assert all(torch.isfinite(t.float()).all() for t in want) and (want[3] != 0).any() and (want[4] != 0).any()
    for got in (both(shifted(own[0]), own[1]), both(own[0], shifted(own[1])), both(shifted(own[0]), shifted(own[1]))):
        assert got[3].dtype == dtype and all(torch.equal(x, y) for x, y in zip(got, want))


# ---- behaviour ----

def test_reductions_and_the_module_are_the_function():
    from warp_rnnt_amd.simple import SimpleRNNTLoss, simple_rnnt_loss
    shape, blank = (2, 21, 9, 63), 31
    a, l, ty, txn, tyn, _ = _args(shape, blank)
    kw = dict(blank=blank, lm_only_scale=0.25, am_only_scale=0.1)
    none = simple_rnnt_loss(a, l, ty, txn, tyn, **kw)
    assert isinstance(none, torch.Tensor) and none.dtype == torch.float32 and none.shape == (shape[0],)
    assert torch.isfinite(none).all()
    assert torch.equal(simple_rnnt_loss(a, l, ty, txn, tyn, reduction=None, **kw), none)
    with_grad = simple_rnnt_loss(a, l, ty, txn, tyn, return_grad=True, **kw)
    assert isinstance(with_grad, tuple) and len(with_grad) == 2 and torch.equal(with_grad[0], none)
    for average in (False, True):
        base = none / txn.to(none) if average else none
        for reduction, want in (("none", base), ("sum", base.sum()), ("mean", base.mean())):
            got = simple_rnnt_loss(a, l, ty, txn, tyn, average_frames=average, reduction=reduction, **kw)
            assert torch.equal(got, want), (average, reduction)
            got, pg = simple_rnnt_loss(a, l, ty, txn, tyn, average_frames=average, reduction=reduction, return_grad=True, **kw)
            assert torch.equal(got, want) and torch.equal(pg, with_grad[1])          # the pairs are not scaled
    for reduction in ("none", "sum", "mean"):
        xa, xb = (a.clone().requires_grad_(True), l.clone().requires_grad_(True)), \
                 (a.clone().requires_grad_(True), l.clone().requires_grad_(True))
        m = SimpleRNNTLoss(blank=blank, lm_only_scale=0.25, am_only_scale=0.1, fastemit_lambda=0.01, reduction=reduction)
        u = m(*xa, ty, txn, tyn)
        v = simple_rnnt_loss(*xb, ty, txn, tyn, reduction=reduction, fastemit_lambda=0.01, **kw)
        assert torch.equal(u, v)
        u.sum().backward()
        v.sum().backward()
        assert torch.equal(xa[0].grad, xb[0].grad) and torch.equal(xa[1].grad, xb[1].grad) and (xa[0].grad != 0).any()
        assert torch.equal(m(a, l, ty, txn, tyn, return_grad=True)[1],
                           simple_rnnt_loss(a, l, ty, txn, tyn, fastemit_lambda=0.01, return_grad=True, **kw)[1])
    with pytest.raises(RuntimeError, match="status 5"):
        simple_rnnt_loss(a, l, ty, txn, tyn, blank=shape[3])
    with pytest.raises(RuntimeError, match="status 5"):
        simple_rnnt_loss(a, l, ty, txn, tyn, lm_only_scale=0.7, am_only_scale=0.4)


def test_scales_zero_are_the_first_pass_on_simple_pairs():
    """With both scales 0 the entry is warp_rnnt.rnnt_loss(simple_pairs(...), blank=-1): the same lattice kernels on pairs
    formed in another fp32 order, so the costs agree within the cost bar and the occupancies within the pair bar."""
    import warp_rnnt
    from warp_rnnt_amd.pruned import simple_pairs
    shape, blank = (2, 70, 35, 130), 0
    a, l, ty, txn, tyn, _ = _args(shape, blank)
    costs, pg, _, _ = fused_run(a, l, ty, txn, tyn, blank, grad=False)
    BARS = bars_of(shape)
    pairs = simple_pairs(a, l, ty, blank).contiguous().requires_grad_(True)
    want = warp_rnnt.rnnt_loss(pairs, ty, txn, tyn, blank=-1)
    (wpg,) = torch.autograd.grad(want.sum(), pairs)
    want = want.detach()
    cost, grad = float(((costs - want).abs() / want.abs()).max()), float((pg - wpg).abs().max())
    print(f"scales (0,0) against simple_pairs: cost rel {cost:.3e} (bar {2 * BARS['cost rel']:.3e}) "
          f"pair_grads abs {grad:.3e} (bar {2 * BARS['pair_grads abs']:.3e})")
    assert cost <= 2 * BARS["cost rel"] and grad <= 2 * BARS["pair_grads abs"]      # (both sides carry an fp32 error)


def test_forward_and_backward_replay_from_a_graph():
    from warp_rnnt_amd.simple import simple_rnnt_loss
    shape, blank = (2, 70, 35, 130), 65
    _, _, labels, xn, yn = case(shape, blank)
    ty, txn, tyn = dev(labels), dev(xn), dev(yn)
    batches = [tuple(dev(t) for t in case(shape, blank, seed=s)[:2]) for s in (1, 2, 3)]

    def step(a, l):
        loss, pg = simple_rnnt_loss(a, l, ty, txn, tyn, blank=blank, lm_only_scale=0.25, am_only_scale=0.1,
                                    fastemit_lambda=0.01, reduction="sum", return_grad=True)
        loss.backward()
        return loss, pg

    want = []
    for b in batches:
        a, l = b[0].clone().requires_grad_(True), b[1].clone().requires_grad_(True)
        loss, pg = step(a, l)
        want.append((loss.detach().clone(), pg.clone(), a.grad.clone(), l.grad.clone()))
    a, l = batches[0][0].clone().requires_grad_(True), batches[0][1].clone().requires_grad_(True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            a.grad = l.grad = None
            step(a, l)
    torch.cuda.current_stream().wait_stream(side)
    a.grad = l.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss, pg = step(a, l)
    for rep in range(6):
        k = rep % len(batches)
        with torch.no_grad():
            a.copy_(batches[k][0])
            l.copy_(batches[k][1])
        graph.replay()
        torch.cuda.synchronize()
        assert torch.isfinite(loss).all()
        assert torch.equal(loss, want[k][0]) and torch.equal(pg, want[k][1]), f"replay {rep}"
        assert torch.equal(a.grad, want[k][2]) and torch.equal(l.grad, want[k][3]), f"replay {rep}"


def test_the_recipe_end_to_end():
    """simple_rnnt_loss(return_grad=True) -> prune_ranges -> prune_joint_inputs -> a torch joiner -> the pruned loss.  The
    band drops paths, so the pruned cost is not below the full lattice's (minus the cost bar of tests/test_gpu_pruned.py);
    with S = U it is the full lattice.  (Not asserted: that the starts equal another implementation's -- near-ties of
    window sums may fall either way.)"""
    from warp_rnnt_amd.fused import rnnt_loss_from_logits
    from warp_rnnt_amd.pruned import prune_joint_inputs, prune_ranges, pruned_rnnt_loss_from_logits
    from warp_rnnt_amd.simple import simple_rnnt_loss
    cost_bar = max(4 * 2.141e-06, 4 * EPS)                  # tests/test_gpu_pruned.py: COST_BAR
    N, T, U, S, V, H = 2, 40, 12, 4, 17, 32
    gen = torch.Generator().manual_seed(12)
    f = (torch.randn(N, T, H, generator=gen) * 0.7).to(DEV)
    g = (torch.randn(N, U, H, generator=gen) * 0.7).to(DEV)
    am_w, lm_w = (torch.randn(H, V, generator=gen) / H ** 0.5).to(DEV), (torch.randn(H, V, generator=gen) / H ** 0.5).to(DEV)
    w = (torch.randn(H, V, generator=gen) / H ** 0.5).to(DEV)
    am_w.requires_grad_(True)
    lm_w.requires_grad_(True)
    labels = torch.randint(1, V, (N, U - 1), generator=gen, dtype=torch.int32).to(DEV)
    xn, yn = torch.tensor([T, T - 7], dtype=torch.int32, device=DEV), torch.tensor([U - 1, U - 4], dtype=torch.int32, device=DEV)

    def joiner(fp, gp):
        return torch.tanh(fp + gp) @ w

    simple, pair_grads = simple_rnnt_loss((f @ am_w).contiguous(), (g @ lm_w).contiguous(), labels, xn, yn,
                                          lm_only_scale=0.25, reduction="sum", return_grad=True)
    assert tuple(pair_grads.shape) == (N, T, U, 2) and not pair_grads.requires_grad and (pair_grads <= 0).all()
    full = rnnt_loss_from_logits(joiner(f[:, :, None, :], g[:, None, :, :]).contiguous(), labels, xn, yn)
    for s_range in (S, U):
        starts = prune_ranges(pair_grads, xn, yn, s_range)
        assert starts.dtype == torch.int32 and tuple(starts.shape) == (N, T) and starts.is_cuda
        fp, gp = prune_joint_inputs(f, g, starts, s_range)
        fp.requires_grad_(True)
        logits = joiner(fp, gp).contiguous()
        assert tuple(logits.shape) == (N, T, s_range, V)
        costs = pruned_rnnt_loss_from_logits(logits, labels, starts, xn, yn)
        costs.sum().backward()
        print(f"S = {s_range}: pruned {costs.tolist()} full lattice {full.tolist()} (cost bar {cost_bar:.3e})")
        assert torch.isfinite(costs).all() and torch.isfinite(fp.grad).all() and (fp.grad != 0).any()
        assert (costs >= full - cost_bar * full.abs()).all()
        if s_range == U:
            assert (starts == 0).all()
            assert ((costs - full).abs() <= cost_bar * full.abs()).all()
    # the first pass trains: its gradient reaches the two projections
    assert torch.isfinite(simple).all()
    simple.backward()
    assert torch.isfinite(am_w.grad).all() and (am_w.grad != 0).any() and torch.isfinite(lm_w.grad).all() and (lm_w.grad != 0).any()
