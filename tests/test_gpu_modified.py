"""k2's modified topology and delay penalty on the GPU, in both passes of the pruned recipe:
pruned_rnnt_loss_from_logits(..., rnnt_type=, delay_penalty=) and simple_rnnt_loss(..., rnnt_type=, delay_penalty=).

Against fp64 (tests/modified_reference.py: the modified recurrence written out frame by frame, true -inf outside the band --
not the sheared regular lattice the kernels run) over shapes with an ordinary utterance, T_n == U_n, no labels, one frame
and one label, T_n < U_n (no path), every row width of the pruned kernels, more than one column block with U > T + 1, the
full band and each of the three sweep kernels.  The bars are not taken from the code under test: they are four times the
largest error the REGULAR entries without a penalty show against their own fp64 references on the same generator, shapes
and lengths, measured once by tools/modified_loss_values.py -- profiles/modified_loss_values.txt holds every figure, the
modified loss's beside the yardstick's.  Then the aliasing trap (a padding frame's band covers the terminal cell's
address), what holds bit for bit, an independent kernel (the TDT loss with the one duration 1 is the same lattice), graph
capture and the three-step recipe end to end.

Every figure is printed before it is asserted (pytest -s)."""
import functools

import numpy as np
import pytest
import torch

import modified_reference as mr
import pruned_reference as pr
import simple_reference as sr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 2.0 ** -24
LAMS = (0.0, 0.01)

# (N, T, U, S, V) -> (xn, yn); None: ragged lengths of the generator with T_n >= U_n
VALUES = {
    # an ordinary utterance, T_n == U_n, no labels, one frame and one label, T_n < U_n (no path)
    (5, 12, 6, 3, 7): ((12, 5, 7, 1, 3), (5, 5, 0, 1, 5)),
    (2, 21, 9, 5, 2): None, (2, 21, 9, 5, 63): None, (2, 21, 9, 5, 65): None, (2, 21, 9, 5, 1030): None,
    (2, 11, 70, 5, 7): ((11, 8), (9, 30)),       # more than one column block, U > T + 1; the second: no path
    (2, 80, 70, 70, 7): ((80, 75), (69, 40)),    # the full band
}
VALUE_DPS = (0.0, 0.1)
# one shape per sweep kernel: debug.lattice_plan(N, T + 1, U, folded=False) names it
SWEEPS = {
    (2, 40, 130, 5, 8): ((40, 33), (30, 20)),
    (2, 60, 400, 8, 8): ((60, 50), (45, 33)),
    # (the labels' summed penalty, at most U_n dp (T_n - 1) / 2 = 1.2e3 here, stays below the cost without a penalty --
    #  0.85 per frame on the simple loss's inputs, 1.7e3 -- so that the relative cost error keeps its meaning)
    (2, 2048, 260, 5, 8): ((2048, 1500), (120, 90)),
}
KERNEL_OF = {(2, 40, 130, 5, 8): "lattice_wl", (2, 60, 400, 8, 8): "lattice_ws", (2, 2048, 260, 5, 8): "lattice_wd"}
SWEEP_DPS = (0.0, 0.01)          # (the summed penalties stay the size of the costs)


def topologies_of(shape, dp):
    """The topologies a case runs with the penalty dp.  The regular one takes a penalty on the shapes with T <= 21 only: it
    may emit every label in the first frames, where each gains up to dp (T_n - 1) / 2, so at T = 80, U_n = 69 and dp = 0.1 the
    gain reaches 270 against a cost of 230 and the cost is what two large sums leave of each other -- a relative cost error
    says nothing there.  The modified topology emits one label per frame at most: 38 at that shape."""
    return ("modified", "regular") if dp and shape[1] <= 21 else ("modified",)
SIMPLE_VS = (7, 65)
LM_ONLY = 0.25

# profiles/modified_loss_values.txt (tools/modified_loss_values.py on an MI355X): the regular entries without a penalty --
# pruned_rnnt_loss_from_logits and simple_rnnt_loss as they were before the topology existed -- against their fp64
# references (tests/pruned_reference.py, tests/simple_reference.py) over the cases below: largest |cost - fp64| / |fp64| and
# largest absolute gradient errors at the upstream gradients 0.5 + 0.25 n.  The bars are four times these.
YARDSTICK = {
    # group: (cost rel, gradient abs ...)            pruned: d/d logits; simple: pair_grads, d am, d lm
    "pruned values": (1.975e-07, 4.238e-05),
    "pruned sweeps": (1.043e-06, 5.505e-03),
    "simple values": (2.892e-07, 1.627e-04, 3.123e-04, 1.176e-03),
    "simple sweeps": (1.435e-06, 3.546e-03, 1.380e-03, 9.827e-01),
}


def bars(group):
    y = YARDSTICK[group]
    return (max(4 * y[0], 4 * EPS),) + tuple(4 * v for v in y[1:])


def blanks_of(V):
    return (0, V - 1) if V == 2 else (0, V // 2, V - 1)


def lengths_of(shape):
    return VALUES[shape] if shape in VALUES else SWEEPS[shape]


def dev(a, dtype=None):
    return torch.tensor(np.asarray(a), device=DEV, dtype=dtype)


def _go(N):
    return pr.upstream(N).astype(np.float32)


def modified_starts(rng, T, U, S, xn, yn):
    """(N,T) int32 starts of bands that hold a modified path where there is one: a random path u(t) (U_n of the T_n frames
    emit), start[t] = u(t) - a random offset below S, clamped to [0, max(U_n + 1 - S, 0)]; frames t >= T_n repeat
    max(U_n + 1 - S, 0) as prune_ranges does -- their bands cover column U_n."""
    out = np.zeros((len(xn), T), np.int32)
    for n in range(len(xn)):
        Tn, Un = int(xn[n]), int(yn[n])
        hi = max(min(Un + 1 - S, U - S), 0)
        emit = np.zeros(Tn, np.int64)
        emit[rng.permutation(Tn)[:min(Un, Tn)]] = 1
        u = np.concatenate([[0], np.cumsum(emit)[:-1]])
        out[n, :Tn] = np.clip(u - rng.randint(0, S, size=Tn), 0, hi)
        out[n, Tn:] = hi
    return out


@functools.lru_cache(maxsize=None)
def pruned_case(shape, blank, seed=0):
    """Host inputs (read-only): logits, labels, the modified case's (starts, xn, yn), the yardstick's (starts, xn, yn) --
    the same logits, labels and lengths with a band that holds a regular path (pruned_reference.make_band_case)."""
    N, T, U, S, V = shape
    lengths = lengths_of(shape)
    s = 7000 * V + 10 * T + S + blank + seed
    if lengths is None:
        rng = np.random.RandomState(s + 1)
        xn = np.array([T] + list(rng.randint(U, T + 1, size=N - 1)), np.int32)
        yn = np.array([U - 1] + list(rng.randint(U // 2, U, size=N - 1)), np.int32)
        lengths = (tuple(xn), tuple(yn))
    logits, labels, ystarts, yxn, yyn = pr.make_band_case(s, N, T, U, S, V, blank=blank, lengths=lengths)
    xn, yn = np.array(lengths[0], np.int32), np.array(lengths[1], np.int32)
    starts = np.zeros((N, T), np.int32) if S == U else modified_starts(np.random.RandomState(s + 2), T, U, S, xn, yn)
    out = (logits, labels, (starts, xn, yn), (ystarts, yxn, yyn))
    for a in (logits, labels, starts, xn, yn, ystarts, yxn, yyn):
        a.setflags(write=False)
    return out


def inputs_of(shape, blank, rnnt_type):
    """logits, labels and (starts, xn, yn): the modified topology on its own band, the regular one (with a penalty) on the
    yardstick's, which holds a regular path."""
    logits, labels, modified, regular = pruned_case(shape, blank)
    return logits, labels, modified if rnnt_type == "modified" else regular


@functools.lru_cache(maxsize=None)
def pruned_reference(shape, blank, lam, dp, rnnt_type):
    logits, labels, (starts, xn, yn) = inputs_of(shape, blank, rnnt_type)
    ref = mr.pruned64(logits, labels, starts, xn, yn, blank, lam, dp, rnnt_type)
    for a in ref.values():
        a.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def pruned_yardstick_reference(shape, blank, lam):
    logits, labels, _, (starts, xn, yn) = pruned_case(shape, blank)
    ref = pr.pruned_loss64(logits, labels, starts, xn, yn, blank, lam)
    for a in ref.values():
        a.setflags(write=False)
    return ref


def pruned_run(logits, labels, starts, xn, yn, blank, lam=0.0, go=None, grad=True, **kw):
    from warp_rnnt_amd.pruned import pruned_rnnt_loss_from_logits
    x = logits.detach().clone().requires_grad_(grad)
    costs = pruned_rnnt_loss_from_logits(x, labels, starts, xn, yn, blank=blank, fastemit_lambda=lam, **kw)
    if not grad:
        return costs, None
    g = torch.ones_like(costs) if go is None else go
    (costs * g).sum().backward()
    return costs.detach(), x.grad


def cost_error(costs, want):
    """Largest relative cost error over the utterances with a path; the others must be +inf on both sides."""
    costs = costs.double().cpu().numpy()
    inf = np.isinf(want)
    assert (np.isinf(costs) == inf).all() and (costs[inf] > 0).all(), (costs, want)
    assert np.isfinite(costs[~inf]).all()
    return float((np.abs(costs[~inf] - want[~inf]) / np.abs(want[~inf])).max())


def grad_error(got, want):
    assert torch.isfinite(got).all()
    return float(np.abs(got.double().cpu().numpy() - want).max())


def pruned_errors(shape, blank, lam, dp, rnnt_type="modified"):
    """(cost rel, d/d logits abs, the sweep kernel) of one case against fp64."""
    from warp_rnnt_amd import debug
    logits, labels, (starts, xn, yn) = inputs_of(shape, blank, rnnt_type)
    ref = pruned_reference(shape, blank, lam, dp, rnnt_type)
    costs, grad = pruned_run(dev(logits), dev(labels), dev(starts), dev(xn), dev(yn), blank, lam, dev(_go(shape[0])),
                             rnnt_type=rnnt_type, delay_penalty=dp)
    kernel = debug.last_lattice_kernel()
    return cost_error(costs, ref["costs"]), grad_error(grad, ref["dlogits"]), kernel


def pruned_yardstick_errors(shape, blank, lam):
    """The regular entry without the keywords on the yardstick's band: (cost rel, d/d logits abs)."""
    logits, labels, _, (starts, xn, yn) = pruned_case(shape, blank)
    ref = pruned_yardstick_reference(shape, blank, lam)
    costs, grad = pruned_run(dev(logits), dev(labels), dev(starts), dev(xn), dev(yn), blank, lam, dev(_go(shape[0])))
    return cost_error(costs, ref["costs"]), grad_error(grad, ref["dlogits"])


PRUNED_VALUE_CASES = [(shape, b) for shape in VALUES for b in blanks_of(shape[4])]
PRUNED_SWEEP_CASES = [(shape, b) for shape in SWEEPS for b in blanks_of(shape[4])]
IDS = lambda cases: ["N%d-T%d-U%d-S%d-V%d-b%d" % (*shape, b) for shape, b in cases]      # noqa: E731


@pytest.mark.parametrize("shape,blank", PRUNED_VALUE_CASES, ids=IDS(PRUNED_VALUE_CASES))
def test_pruned_costs_and_gradients_against_fp64(shape, blank):
    cost_bar, grad_bar = bars("pruned values")
    for lam in LAMS:
        for dp in VALUE_DPS:
            for rnnt_type in topologies_of(shape, dp):
                cost, grad, kernel = pruned_errors(shape, blank, lam, dp, rnnt_type)
                print(f"{shape} blank {blank} lam {lam} dp {dp} {rnnt_type}: cost rel {cost:.3e} (bar {cost_bar:.3e})  "
                      f"grad abs {grad:.3e} (bar {grad_bar:.3e})  {kernel}")
                assert cost <= cost_bar, (shape, blank, lam, dp, rnnt_type)
                assert grad <= grad_bar, (shape, blank, lam, dp, rnnt_type)
    want = pruned_reference(shape, blank, 0.0, 0.0, "modified")["costs"]
    xn, yn = pruned_case(shape, blank)[2][1:]
    assert (np.isinf(want) == (xn < yn)).all()            # exactly the utterances with T_n < U_n have no path


@pytest.mark.parametrize("shape,blank", PRUNED_SWEEP_CASES, ids=IDS(PRUNED_SWEEP_CASES))
def test_pruned_on_each_sweep_kernel(shape, blank):
    from warp_rnnt_amd import debug
    cost_bar, grad_bar = bars("pruned sweeps")
    N, T, U = shape[:3]
    for lam, dp in zip(LAMS, SWEEP_DPS):
        cost, grad, kernel = pruned_errors(shape, blank, lam, dp)
        print(f"{shape} blank {blank} lam {lam} dp {dp}: cost rel {cost:.3e} (bar {cost_bar:.3e})  "
              f"grad abs {grad:.3e} (bar {grad_bar:.3e})  {kernel}")
        assert cost <= cost_bar and grad <= grad_bar, (shape, blank, lam, dp)
        # the sheared lattice's plane has T + 1 rows; the producer carries no ring preparation: the unfolded plan
        assert kernel == KERNEL_OF[shape] == debug.lattice_plan(N, T + 1, U, folded=False).kernel, (shape, kernel)


# ---- the simple loss ----

@functools.lru_cache(maxsize=None)
def simple_case(shape, V):
    N, T, U = shape[:3]
    lengths = lengths_of(shape)
    if lengths is None:
        lengths = pruned_case(shape, 0)[2][1:]
    out = sr.make_case(300 * V + T + U, N, T, U, V, blank=V // 2, scale=1.0, lengths=lengths)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def simple_reference(shape, V, lam, dp, rnnt_type):
    am, lm, labels, xn, yn = simple_case(shape, V)
    if rnnt_type is None:                         # the yardstick's: tests/simple_reference.py as it stands
        ref = sr.simple_loss64(am, lm, labels, xn, yn, V // 2, LM_ONLY, 0.0, lam)
    else:
        ref = mr.simple64(am, lm, labels, xn, yn, V // 2, LM_ONLY, lam, dp, rnnt_type)
    return {k: ref[k] for k in ("costs", "pair_grads", "dam", "dlm")}


def simple_run(am, lm, labels, xn, yn, blank, lam=0.0, go=None, **kw):
    from warp_rnnt_amd.simple import simple_rnnt_loss
    a, l = am.detach().clone().requires_grad_(True), lm.detach().clone().requires_grad_(True)
    costs, pairs = simple_rnnt_loss(a, l, labels, xn, yn, blank=blank, lm_only_scale=LM_ONLY, fastemit_lambda=lam,
                                    return_grad=True, **kw)
    g = torch.ones_like(costs) if go is None else go
    (costs * g).sum().backward()
    return costs.detach(), pairs, a.grad, l.grad


def simple_errors(shape, V, lam, dp, rnnt_type="modified"):
    """(cost rel, pair_grads abs, d am abs, d lm abs) of one case against fp64; rnnt_type None: the yardstick -- the call
    without the keywords."""
    am, lm, labels, xn, yn = simple_case(shape, V)
    ref = simple_reference(shape, V, lam, dp, rnnt_type)
    kw = {} if rnnt_type is None else dict(rnnt_type=rnnt_type, delay_penalty=dp)
    costs, pairs, dam, dlm = simple_run(dev(am), dev(lm), dev(labels), dev(xn), dev(yn), V // 2, lam, dev(_go(shape[0])), **kw)
    assert tuple(pairs.shape) == (shape[0], shape[1], shape[2], 2) and not pairs.requires_grad
    return (cost_error(costs, ref["costs"]), grad_error(pairs, ref["pair_grads"]), grad_error(dam, ref["dam"]),
            grad_error(dlm, ref["dlm"]))


SIMPLE_VALUE_CASES = [(shape, V) for shape in list(VALUES)[:1] + list(VALUES)[-3:] for V in SIMPLE_VS]
SIMPLE_SWEEP_CASES = [(shape, 7) for shape in SWEEPS]
SIDS = lambda cases: ["N%d-T%d-U%d-V%d" % (*shape[:3], V) for shape, V in cases]      # noqa: E731


@pytest.mark.parametrize("shape,V", SIMPLE_VALUE_CASES, ids=SIDS(SIMPLE_VALUE_CASES))
def test_simple_costs_and_gradients_against_fp64(shape, V):
    b = bars("simple values")
    for lam in LAMS:
        for dp in VALUE_DPS:
            for rnnt_type in topologies_of(shape, dp):
                e = simple_errors(shape, V, lam, dp, rnnt_type)
                print(f"{shape[:3]} V {V} lam {lam} dp {dp} {rnnt_type}: cost rel {e[0]:.3e} (bar {b[0]:.3e})  pair_grads "
                      f"{e[1]:.3e} ({b[1]:.3e})  d am {e[2]:.3e} ({b[2]:.3e})  d lm {e[3]:.3e} ({b[3]:.3e})")
                assert all(x <= y for x, y in zip(e, b)), (shape, V, lam, dp, rnnt_type)


@pytest.mark.parametrize("shape,V", SIMPLE_SWEEP_CASES, ids=SIDS(SIMPLE_SWEEP_CASES))
def test_simple_on_each_sweep_kernel(shape, V):
    from warp_rnnt_amd import debug
    b = bars("simple sweeps")
    for lam, dp in zip(LAMS, SWEEP_DPS):
        e = simple_errors(shape, V, lam, dp)
        kernel = debug.last_lattice_kernel()
        print(f"{shape[:3]} V {V} lam {lam} dp {dp}: cost rel {e[0]:.3e} (bar {b[0]:.3e})  pair_grads {e[1]:.3e} "
              f"({b[1]:.3e})  d am {e[2]:.3e} ({b[2]:.3e})  d lm {e[3]:.3e} ({b[3]:.3e})  {kernel}")
        assert all(x <= y for x, y in zip(e, b)), (shape, V, lam, dp)
        assert kernel == KERNEL_OF[shape], (shape, kernel)


# ---- the aliasing trap ----

def test_padding_frames_whose_band_covers_the_terminal_cell():
    """A ragged batch with starts from prune_ranges: frames t >= T_n repeat U_n + 1 - S, so the band of frame T_n covers
    column U_n -- the address of the virtual terminal cell.  Those rows get exactly zero gradient, the cost is that of
    the utterance alone with T = T_n bit for bit, and garbage behind T_n (logits and starts) moves no bit."""
    from warp_rnnt_amd.pruned import prune_ranges
    N, T, U, S, V, blank = 3, 14, 7, 3, 9, 4
    am, lm, labels, xn, yn = sr.make_case(77, N, T, U, V, blank=blank, scale=1.0, lengths=((14, 9, 11), (6, 4, 6)))
    tl, txn, tyn = dev(labels), dev(xn), dev(yn)
    kw = dict(rnnt_type="modified", delay_penalty=0.1)
    _, pairs, _, _ = simple_run(dev(am), dev(lm), tl, txn, tyn, blank, 0.01, **kw)
    for n in range(N):
        assert (pairs[n, xn[n]:] == 0).all(), n               # (the terminal cell's pair (-1, 0) lies in row T_n of the plane)
        assert (pairs[n, :xn[n]] != 0).any(), n
    starts = prune_ranges(pairs, txn, tyn, S)
    host = starts.cpu().numpy()
    for n in range(1, N):
        assert host[n, xn[n]] <= yn[n] < host[n, xn[n]] + S   # the trap is set: (T_n, U_n) is a row of the logits
    logits = dev(np.random.RandomState(5).randn(N, T, S, V).astype(np.float32))
    go = dev(_go(N))
    costs, grad = pruned_run(logits, tl, starts, txn, tyn, blank, 0.01, go, **kw)
    print(f"costs {costs.tolist()}")
    assert torch.isfinite(costs).all()
    bad_logits, bad_starts = logits.clone(), starts.clone()
    garbage = torch.tensor([-5, U + 3, 2 ** 31 - 1, -2 ** 31, 0, U - 1, 3, -1], dtype=torch.int32, device=DEV)
    for n in range(N):
        Tn = int(xn[n])
        assert (grad[n, Tn:] == 0).all() and (grad[n, :Tn] != 0).any(), n
        one = [a[n:n + 1, :Tn].contiguous() for a in (logits, starts)]
        c1, g1 = pruned_run(one[0], tl[n:n + 1], one[1], txn[n:n + 1], tyn[n:n + 1], blank, 0.01, go[n:n + 1], **kw)
        assert torch.equal(c1, costs[n:n + 1]) and torch.equal(g1[0], grad[n, :Tn]), n
        bad_logits[n, Tn:] = float("nan")
        bad_starts[n, Tn:] = garbage[:T - Tn] if T - Tn else bad_starts[n, Tn:]
    c2, g2 = pruned_run(bad_logits, tl, bad_starts, txn, tyn, blank, 0.01, go, **kw)
    assert torch.equal(c2, costs) and torch.equal(g2, grad)
    # the simple loss: garbage behind T_n and U_n in am and lm moves no bit of the costs and the pairs
    bad_am, bad_lm = dev(am), dev(lm)
    for n in range(N):
        bad_am[n, xn[n]:] = 1e4
        bad_lm[n, yn[n] + 1:] = -1e4
    c3, p3, _, _ = simple_run(bad_am, bad_lm, tl, txn, tyn, blank, 0.01, **kw)
    c0, _, _, _ = simple_run(dev(am), dev(lm), tl, txn, tyn, blank, 0.01, **kw)
    assert torch.equal(c3, c0) and torch.equal(p3, pairs)


# ---- bit for bit ----

BIT_SHAPE, BIT_BLANK = (2, 21, 9, 5, 65), 32


def test_regular_without_a_penalty_is_the_call_without_the_keywords():
    from warp_rnnt_amd import ops
    logits, labels, _, (starts, xn, yn) = pruned_case(BIT_SHAPE, BIT_BLANK)
    x, tl, ts, txn, tyn = dev(logits), dev(labels), dev(starts), dev(xn), dev(yn)
    args = (x, tl, ts, txn, tyn, BIT_BLANK, 0.01, dev(_go(2)))
    a, b = pruned_run(*args), pruned_run(*args, rnnt_type="regular", delay_penalty=0.0)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and (a[1] != 0).any()
    am, lm, slabels, sxn, syn = simple_case(BIT_SHAPE, 65)
    args = (dev(am), dev(lm), dev(slabels), dev(sxn), dev(syn), 32, 0.01, dev(_go(2)))
    a, b = simple_run(*args), simple_run(*args, rnnt_type="regular", delay_penalty=0.0)
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and (a[2] != 0).any()
    # ... and the entries with a topology, asked for the regular one without a penalty, are the entries without
    c0, g0 = ops.pruned_loss(x, tl, ts, txn, tyn, BIT_BLANK, 0.01)
    c1, g1 = ops.pruned_loss_topology(x, tl, ts, txn, tyn, BIT_BLANK, 0.01, True, 0, 0.0)
    assert torch.equal(c0, c1) and torch.equal(g0, g1)
    go = dev(_go(2))
    assert torch.equal(ops.pruned_logits_backward(x, tl, ts, g0, go, BIT_BLANK),
                       ops.pruned_logits_backward_topology(x, tl, ts, txn, tyn, g1, go, BIT_BLANK, 0))


@pytest.mark.parametrize("dname", ["bf16", "f16"])
def test_half_precision_inputs_give_the_bits_of_their_upcast(dname):
    dtype = {"bf16": torch.bfloat16, "f16": torch.float16}[dname]
    kw = dict(rnnt_type="modified", delay_penalty=0.1)
    logits, labels, (starts, xn, yn), _ = pruned_case(BIT_SHAPE, BIT_BLANK)
    tl, ts, txn, tyn, go = dev(labels), dev(starts), dev(xn), dev(yn), dev(_go(2))
    xh = dev(logits).to(dtype)
    h, f = pruned_run(xh, tl, ts, txn, tyn, BIT_BLANK, 0.01, go, **kw), pruned_run(xh.float(), tl, ts, txn, tyn, BIT_BLANK, 0.01, go, **kw)
    assert h[1].dtype == dtype and torch.equal(h[0], f[0]) and torch.equal(h[1], f[1].to(dtype)) and (h[1] != 0).any()
    am, lm, labels, xn, yn = simple_case(BIT_SHAPE, 65)
    ah, lh = dev(am).to(dtype), dev(lm).to(dtype)
    h = simple_run(ah, lh, dev(labels), dev(xn), dev(yn), 32, 0.01, go, **kw)
    f = simple_run(ah.float(), lh.float(), dev(labels), dev(xn), dev(yn), 32, 0.01, go, **kw)
    assert torch.equal(h[0], f[0]) and torch.equal(h[1], f[1])
    assert torch.equal(h[2], f[2].to(dtype)) and torch.equal(h[3], f[3].to(dtype)) and (h[2] != 0).any()


def test_bits_depend_on_the_utterance_alone():
    kw = dict(rnnt_type="modified", delay_penalty=0.1)
    shape, blank = (5, 12, 6, 3, 7), 3
    logits, labels, (starts, xn, yn), _ = pruned_case(shape, blank)
    x, tl, ts, txn, tyn, go = dev(logits), dev(labels), dev(starts), dev(xn), dev(yn), dev(_go(5))
    costs, grad = pruned_run(x, tl, ts, txn, tyn, blank, 0.01, go, **kw)
    only, _ = pruned_run(x, tl, ts, txn, tyn, blank, 0.01, grad=False, **kw)
    assert torch.equal(only, costs)
    am, lm, slabels, _, _ = simple_case(shape, 7)
    ta, tlm, sl = dev(am), dev(lm), dev(slabels)
    whole = simple_run(ta, tlm, sl, txn, tyn, 3, 0.01, go, **kw)
    for n in range(shape[0]):
        one = [a[n:n + 1].contiguous() for a in (x, tl, ts, txn, tyn)]
        c1, g1 = pruned_run(*one, blank, 0.01, go[n:n + 1].contiguous(), **kw)
        assert torch.equal(c1, costs[n:n + 1]) and torch.equal(g1[0], grad[n]), n
        assert (grad[n] != 0).any() == bool(xn[n] >= yn[n]), n            # T_n < U_n: +inf and zero rows
        s1 = simple_run(*[a[n:n + 1].contiguous() for a in (ta, tlm, sl, txn, tyn)], 3, 0.01, go[n:n + 1].contiguous(), **kw)
        assert all(torch.equal(a[0], b[n]) for a, b in zip(s1, whole)), n
    assert torch.isinf(costs[4]) and torch.isinf(whole[0][4]) and (whole[1][4] == 0).all() and (whole[2][4] == 0).all()


# ---- an independent kernel ----

def test_full_band_against_the_tdt_loss_with_the_one_duration_1():
    """Token-and-duration with durations = (1,): blank and label both take one frame, the duration head is one column whose
    log-softmax is 0.  That is the modified lattice but for its end: a TDT label never lands on frame T_n, so the last
    frame's edge is the blank of cell (T_n - 1, U_n).  In exact arithmetic the TDT cost is the modified cost of the first
    T_n - 1 frames minus that blank's log-prob (fp64 here).  Costs within the sum of the two features' cost bars."""
    from test_gpu_tdt import COST_BAR as TDT_COST_BAR
    from warp_rnnt_amd.tdt import tdt_loss_from_logits
    shape, blank = (2, 80, 70, 70, 7), 3
    logits, labels, (starts, xn, yn), _ = pruned_case(shape, blank)
    x, tl, txn, tyn = dev(logits), dev(labels), dev(xn), dev(yn)
    costs, _ = pruned_run(x, tl, dev(starts), txn - 1, tyn, blank, grad=False, rnnt_type="modified")
    last = torch.stack([torch.log_softmax(x[n, xn[n] - 1, yn[n]].double(), -1)[blank] for n in range(shape[0])])
    costs = costs.double() - last
    tdt = tdt_loss_from_logits(torch.cat([x, torch.zeros_like(x[..., :1])], -1).contiguous(), tl, txn, tyn, durations=(1,),
                               sigma=0.0, blank=blank)
    bar = bars("pruned values")[0] + TDT_COST_BAR
    diff = ((costs - tdt.double()).abs() / tdt.double().abs()).max().item()
    print(f"modified {costs.tolist()} TDT(1,) {tdt.tolist()}: relative difference {diff:.3e} (bar {bar:.3e})")
    assert torch.isfinite(costs).all() and diff <= bar


# ---- behaviour ----

def test_forward_and_backward_replay_from_a_graph():
    from warp_rnnt_amd.pruned import pruned_rnnt_loss_from_logits
    from warp_rnnt_amd.simple import simple_rnnt_loss
    shape, blank = BIT_SHAPE, BIT_BLANK
    N, T, _, _, V = shape
    _, labels, (starts, xn, yn), _ = pruned_case(shape, blank)
    tl, ts, txn, tyn = dev(labels), dev(starts), dev(xn), dev(yn)
    batches = [dev(pruned_case(shape, blank, seed=s)[0]) for s in (1, 2, 3)]
    ams = [dev(np.random.RandomState(s).randn(N, T, V).astype(np.float32)) for s in (1, 2, 3)]
    lm = dev(simple_case(shape, V)[1])
    kw = dict(rnnt_type="modified", delay_penalty=0.1)

    def step(x, am):
        loss = pruned_rnnt_loss_from_logits(x, tl, ts, txn, tyn, reduction="sum", blank=blank, fastemit_lambda=0.01, **kw)
        first, pairs = simple_rnnt_loss(am, lm, tl, txn, tyn, blank=blank, lm_only_scale=LM_ONLY, reduction="sum",
                                        return_grad=True, **kw)
        (loss + 0.5 * first).backward()
        return loss, first, pairs

    want = []
    for b, a in zip(batches, ams):
        x, am = b.clone().requires_grad_(True), a.clone().requires_grad_(True)
        out = step(x, am)
        want.append(tuple(o.detach().clone() for o in out) + (x.grad.clone(), am.grad.clone()))
    x, am = batches[0].clone().requires_grad_(True), ams[0].clone().requires_grad_(True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            x.grad = am.grad = None
            step(x, am)
    torch.cuda.current_stream().wait_stream(side)
    x.grad = am.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step(x, am)
    for rep in (1, 2, 1):                         # replayed with new inputs, and again
        with torch.no_grad():
            x.copy_(batches[rep])
            am.copy_(ams[rep])
        graph.replay()
        torch.cuda.synchronize()
        got = tuple(out) + (x.grad, am.grad)
        assert torch.isfinite(out[0]).all() and (x.grad != 0).any() and (am.grad != 0).any()
        assert all(torch.equal(g, w) for g, w in zip(got, want[rep])), f"replay of batch {rep}"


def test_the_three_step_recipe_end_to_end():
    """simple_rnnt_loss(return_grad=True) -> prune_ranges -> prune_joint_inputs -> a torch joiner -> the pruned loss, the
    modified topology and the penalty in both passes.  The band drops paths: the pruned cost is not below the full band's
    (minus the cost bar); with s_range >= U it is the full band's."""
    from warp_rnnt_amd.pruned import prune_joint_inputs, prune_ranges, pruned_rnnt_loss_from_logits
    from warp_rnnt_amd.simple import simple_rnnt_loss
    N, T, U, S, V, H = 3, 40, 12, 5, 33, 32
    kw = dict(rnnt_type="modified", delay_penalty=0.01)
    gen = torch.Generator().manual_seed(12)
    f = (torch.randn(N, T, H, generator=gen) * 0.7).to(DEV)
    g = (torch.randn(N, U, H, generator=gen) * 0.7).to(DEV)
    am_w, lm_w, w = ((torch.randn(H, V, generator=gen) / H ** 0.5).to(DEV) for _ in range(3))
    labels = torch.randint(1, V, (N, U - 1), generator=gen, dtype=torch.int32).to(DEV)
    xn = torch.tensor([T, T - 7, 15], dtype=torch.int32, device=DEV)
    yn = torch.tensor([U - 1, U - 4, U - 1], dtype=torch.int32, device=DEV)
    cost_bar = bars("pruned values")[0]

    def joiner(fp, gp):
        return torch.tanh(fp + gp) @ w

    f.requires_grad_(True)
    simple, pair_grads = simple_rnnt_loss((f @ am_w).contiguous(), (g @ lm_w).contiguous(), labels, xn, yn,
                                          lm_only_scale=LM_ONLY, return_grad=True, **kw)
    assert tuple(pair_grads.shape) == (N, T, U, 2) and torch.isfinite(simple).all()
    zeros = torch.zeros((N, T), dtype=torch.int32, device=DEV)
    full = pruned_rnnt_loss_from_logits(joiner(f[:, :, None, :], g[:, None, :, :]).contiguous(), labels, zeros, xn, yn, **kw)
    for s_range in (S, U):
        starts = prune_ranges(pair_grads, xn, yn, s_range)            # (the view of the (N,T+1,U,2) pairs, as it is)
        assert starts.dtype == torch.int32 and tuple(starts.shape) == (N, T)
        fp, gp = prune_joint_inputs(f, g, starts, s_range)
        costs = pruned_rnnt_loss_from_logits(joiner(fp, gp).contiguous(), labels, starts, xn, yn, **kw)
        f.grad = None
        (0.5 * simple.sum() + costs.sum()).backward(retain_graph=True)
        print(f"S = {s_range}: pruned {costs.tolist()} full band {full.tolist()} (cost bar {cost_bar:.3e})")
        assert torch.isfinite(costs).all() and torch.isfinite(f.grad).all() and (f.grad != 0).any()
        assert (costs >= full - cost_bar * full.abs()).all()
        if s_range == U:
            assert (starts == 0).all() and ((costs - full).abs() <= cost_bar * full.abs()).all()
