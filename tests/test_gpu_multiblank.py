"""The multi-blank transducer loss on the GPU: warp_rnnt_amd.multiblank.multiblank_loss_from_logits, logits -> costs ->
d/d logits.

Against fp64 (tests/multiblank_reference.py, itself held to exhaustive path enumeration and central differences by
tests/test_host_multiblank.py) over a grid of shapes and big-blank sets: every lane-group size of the streaming kernels,
rows of 64 and 65 elements, two id layouts, sigma and FastEmit, a skew that wraps with jumps longer than the utterance, two
waves of columns, more than 64 diagonals with the longest jump, durations unsorted, no big blank at all, an utterance of one
frame and one without labels.  The bars are not taken from the code under test: they are four times the largest error that
the STANDARD fused loss, rnnt_loss_from_logits, shows on the same logits (the standard blank as its blank) over the same
grid against its own fp64 reference, measured once by tools/multiblank_loss_values.py --
profiles/multiblank_loss_values.txt holds every figure, this loss's beside the yardstick's.  The lattice depth and the fp32
arithmetic are the same; a cell sums up to 1+B <= 5 terms instead of 2: 4x is TDT's margin, for the same reason.  Then the
properties that hold bit for bit, masked logits, the value range, reductions and graph capture.

Every figure is printed before it is asserted (pytest -s)."""
import functools

import numpy as np
import pytest
import torch

import multiblank_reference as mr
from helpers import make_case
from oracle import transduce_np

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 2.0 ** -24

B3 = (2, 4, 8)
# (N, T, U, V, big-blank durations)
GRID = [(3, 12, 6, 3, (2,)),            # its batch holds a one-frame and a no-label utterance
        (2, 9, 5, 5, (2, 4)),           # a small vocabulary
        (3, 30, 12, 50, B3),            # the common big-blank set
        (2, 21, 9, 64, B3), (2, 21, 9, 65, B3),                 # the row edge at 64 and 65 elements
        (2, 15, 9, 256, (2, 3)), (2, 9, 5, 1024, B3), (2, 9, 5, 5000, B3),      # the three lane-group sizes
        (2, 3, 6, 7, B3),               # U > T: the skew wraps, the jumps are longer than the utterance
        (2, 11, 70, 7, (2,)),           # two waves of columns
        (2, 60, 9, 5, (8,)),            # more than 64 diagonals with the longest jump
        (2, 14, 5, 6, (4, 2)),          # durations unsorted
        (2, 14, 5, 6, ())]              # B = 1
LAYOUTS = ("nemo", "spread")
SIGMAS = (0.0, 0.05)
LAMS = (0.0, 0.01)

# profiles/multiblank_loss_values.txt (tools/multiblank_loss_values.py on an MI355X): rnnt_loss_from_logits on the same
# logits over GRID x LAYOUTS x LAMS -- largest |cost - fp64| / |fp64|, largest |d/d logits - fp64| at the upstream
# gradients of _go()
YARDSTICK_COST_REL = 2.399e-07   # at (2, 60, 9, 5), big blank (8,), NeMo's layout, lambda 0.01; this loss's largest: 1.747e-07 at (2, 9, 5, 5), (2, 4), spread
YARDSTICK_GRAD_ABS = 2.393e-05   # at (3, 30, 12, 50), (2, 4, 8), NeMo's layout, lambda 0.01; this loss's largest: 2.185e-05 at (2, 11, 70, 7), (2,), spread
COST_BAR = max(4 * YARDSTICK_COST_REL, 4 * EPS)      # relative to the fp64 cost
GRAD_BAR = 4 * YARDSTICK_GRAD_ABS                    # absolute

GRID_CASES = [(shape, layout) for shape in GRID for layout in LAYOUTS]
GRID_IDS = ["N%d-T%d-U%d-V%d-d%s-%s" % (*shape[:4], "".join(map(str, shape[4])) or "none", layout)
            for shape, layout in GRID_CASES]


def blanks_of(shape, layout):
    """(standard blank, big-blank ids): NeMo's layout -- the blank last, big blank i at V-2-i -- or a spread one -- the
    standard blank 0, the big blanks from V//2 up."""
    V, big = shape[3], shape[4]
    if layout == "nemo":
        return V - 1, tuple(V - 2 - i for i in range(len(big)))
    return 0, tuple(V // 2 + i for i in range(len(big)))


def _go(N):
    """The upstream gradient of utterance n: not 1, exact in fp32."""
    return np.array([0.5 + 0.25 * n for n in range(N)], np.float32)


def case(shape, layout, seed=0):
    """The inputs of a grid case (fp32 logits (N,T,U,V) on the host), ragged lengths; labels that collide with a blank
    id are remapped to a free token.  The first shape's batch holds an utterance of one frame and one without labels
    beside a full one."""
    N, T, U, V, big = shape
    blank, big_ids = blanks_of(shape, layout)
    logits, labels, xn, yn = make_case(1000 * V + 10 * T + blank + seed, N, T, U, V, ragged=True, blank=blank)
    free = next(v for v in range(V) if v != blank and v not in big_ids)
    labels[np.isin(labels, big_ids)] = free
    if shape == GRID[0]:
        xn[:], yn[:] = (T, 1, T // 2), (U - 1, U // 2, 0)
    return logits, labels, xn, yn


def sets_of(shape, layout):
    """(blank_ids, blank_durations) as the reference takes them: the standard blank first."""
    blank, big_ids = blanks_of(shape, layout)
    return (blank,) + big_ids, (1,) + tuple(shape[4])


@functools.lru_cache(maxsize=None)
def reference(shape, layout, sigma, lam):
    """fp64, computed once per case and shared (read-only): the costs and d/d z at the upstream _go()."""
    logits, labels, xn, yn = case(shape, layout)
    go = _go(shape[0]).astype(np.float64)
    costs, dz, _ = mr.multiblank_loss64(logits, labels, xn, yn, *sets_of(shape, layout), sigma, lam)
    out = (costs, dz * go[:, None, None, None])
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def standard_reference(shape, layout, lam):
    """fp64: the standard loss's costs and d/d z on the same logits, at the upstream _go()."""
    logits, labels, xn, yn = case(shape, layout)
    go = _go(shape[0]).astype(np.float64)
    lp = transduce_np.log_softmax(logits)
    costs, glp = transduce_np.transduce_batch(lp, labels, xn, yn, blank=blanks_of(shape, layout)[0], fastemit_lambda=lam,
                                              fast=True)
    dz = glp - np.exp(lp) * glp.sum(-1, keepdims=True)
    return costs, dz * go[:, None, None, None]


def dev(a, dtype=None):
    return torch.tensor(a, device=DEV, dtype=dtype)


def mb_run(logits, labels, xn, yn, shape, layout, sigma=0.0, lam=0.0, go=None, grad=True):
    """costs (N,) and d (sum_n go[n] cost[n]) / d logits for device tensors; grad=False: costs only, nothing requires
    grad."""
    from warp_rnnt_amd.multiblank import multiblank_loss_from_logits
    blank, big_ids = blanks_of(shape, layout)
    x = logits.detach().clone().requires_grad_(grad)
    costs = multiblank_loss_from_logits(x, labels, xn, yn, big_blank_durations=shape[4], sigma=sigma, blank=blank,
                                        big_blank_ids=big_ids, fastemit_lambda=lam)
    if not grad:
        return costs, None
    g = torch.ones_like(costs) if go is None else go
    (costs * g).sum().backward()
    return costs.detach(), x.grad


def errors(shape, layout, sigma, lam):
    """One grid case on the GPU: the cost error relative to fp64 and the largest d/d logits error."""
    logits, labels, xn, yn = case(shape, layout)
    c64, dz64 = reference(shape, layout, sigma, lam)
    costs, grad = mb_run(dev(logits), dev(labels), dev(xn), dev(yn), shape, layout, sigma, lam, dev(_go(shape[0])))
    costs = costs.double().cpu().numpy()
    assert np.isfinite(costs).all() and torch.isfinite(grad).all()
    return float((np.abs(costs - c64) / np.abs(c64)).max()), float(np.abs(grad.double().cpu().numpy() - dz64).max())


def standard_run(shape, layout, lam):
    """rnnt_loss_from_logits on the logits of the case, the standard blank as its blank: costs and d/d logits (numpy)."""
    from warp_rnnt_amd.fused import rnnt_loss_from_logits
    logits, labels, xn, yn = case(shape, layout)
    x = dev(logits).requires_grad_(True)
    costs = rnnt_loss_from_logits(x, dev(labels), dev(xn), dev(yn), blank=blanks_of(shape, layout)[0], fastemit_lambda=lam)
    (costs * dev(_go(shape[0]))).sum().backward()
    return costs.detach().double().cpu().numpy(), x.grad.double().cpu().numpy()


def yardstick_errors(shape, layout, lam):
    """The same two figures for rnnt_loss_from_logits on the case (tools/multiblank_loss_values.py)."""
    c64, dz64 = standard_reference(shape, layout, lam)
    costs, grad = standard_run(shape, layout, lam)
    return float((np.abs(costs - c64) / np.abs(c64)).max()), float(np.abs(grad - dz64).max())


@pytest.mark.parametrize("shape,layout", GRID_CASES, ids=GRID_IDS)
def test_costs_and_gradients_against_fp64(shape, layout):
    for sigma in SIGMAS:
        for lam in LAMS:
            cost, grad = errors(shape, layout, sigma, lam)
            print(f"{shape} {layout} sigma {sigma} lam {lam}: cost rel {cost:.3e} (bar {COST_BAR:.3e})  "
                  f"grad abs {grad:.3e} (bar {GRAD_BAR:.3e})")
            assert cost <= COST_BAR, (shape, layout, sigma, lam)
            assert grad <= GRAD_BAR, (shape, layout, sigma, lam)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_one_blank_is_the_standard_loss_plus_sigma_per_step(layout):
    """B = 1: costs minus sigma (T_n + U_n), and gradients, against rnnt_loss_from_logits itself under the same bars."""
    shape = GRID[-1]
    assert shape[4] == ()
    logits, labels, xn, yn = case(shape, layout)
    for sigma in SIGMAS:
        for lam in LAMS:
            want_costs, want_grad = standard_run(shape, layout, lam)
            costs, grad = mb_run(dev(logits), dev(labels), dev(xn), dev(yn), shape, layout, sigma, lam, dev(_go(shape[0])))
            costs = costs.double().cpu().numpy() - sigma * (xn + yn).astype(np.float64)
            cost = float((np.abs(costs - want_costs) / np.abs(want_costs)).max())
            err = float(np.abs(grad.double().cpu().numpy() - want_grad).max())
            print(f"{shape} {layout} sigma {sigma} lam {lam}: cost rel {cost:.3e} (bar {COST_BAR:.3e})  "
                  f"grad abs {err:.3e} (bar {GRAD_BAR:.3e})")
            assert cost <= COST_BAR and err <= GRAD_BAR, (sigma, lam)


def test_the_default_ids_are_nemos_convention():
    """big_blank_ids=None is blank - 1 - i: the bits of the same ids spelt out."""
    from warp_rnnt_amd.multiblank import multiblank_loss_from_logits
    shape = (3, 30, 12, 50, B3)
    logits, labels, xn, yn = case(shape, "nemo")
    x, tl, txn, tyn = dev(logits), dev(labels), dev(xn), dev(yn)
    costs, _ = mb_run(x, tl, txn, tyn, shape, "nemo", 0.05, grad=False)
    assert torch.equal(multiblank_loss_from_logits(x, tl, txn, tyn, sigma=0.05, blank=shape[3] - 1), costs)


# ---- bit for bit ----

HALF = {"bf16": torch.bfloat16, "f16": torch.float16}
# the grid's shapes (every lane-group size, rows of 64 and 65 elements, two waves of columns, a skew that wraps, the longest
# jump) and rows whose pitch narrows the access: 12 elements are 16-byte rows in fp32 and 8-byte rows in half precision, 10
# are 8-byte rows in fp32 and 4-byte rows in half precision, 257 and 513 rows of single elements past a group's edge
BIT_SHAPES = [s for s in GRID if s[3] >= 5] + [(2, 7, 4, 12, B3), (2, 7, 4, 10, B3), (2, 7, 4, 257, B3), (2, 7, 4, 513, B3)]
BIT_IDS = ["N%d-T%d-U%d-V%d-d%s" % (*s[:4], "".join(map(str, s[4])) or "none") for s in BIT_SHAPES]


def _layout_of(shape):
    return LAYOUTS[shape[3] % 2]


@pytest.mark.parametrize("dname", list(HALF))
@pytest.mark.parametrize("shape", BIT_SHAPES, ids=BIT_IDS)
def test_half_precision_logits_give_the_bits_of_their_upcast(shape, dname):
    layout = _layout_of(shape)
    logits, labels, xn, yn = case(shape, layout)
    xh = dev(logits).to(HALF[dname])
    args = (dev(labels), dev(xn), dev(yn), shape, layout, 0.05, 0.01, dev(_go(shape[0])))
    costs_h, grad_h = mb_run(xh, *args)
    costs_f, grad_f = mb_run(xh.float(), *args)
    assert costs_h.dtype == torch.float32 and grad_h.dtype == HALF[dname] and grad_f.dtype == torch.float32
    assert torch.equal(costs_h, costs_f)
    assert torch.equal(grad_h, grad_f.to(HALF[dname]))


@pytest.mark.parametrize("shape", BIT_SHAPES, ids=BIT_IDS)
def test_bits_depend_on_the_utterance_alone(shape):
    """An utterance alone and inside its batch; a second call; nothing outside the window; costs without gradients."""
    layout = _layout_of(shape)
    N = shape[0]
    logits, labels, xn, yn = case(shape, layout)
    x, tl, txn, tyn, go = dev(logits), dev(labels), dev(xn), dev(yn), dev(_go(N))
    costs, grad = mb_run(x, tl, txn, tyn, shape, layout, 0.05, 0.01, go)
    again = mb_run(x, tl, txn, tyn, shape, layout, 0.05, 0.01, go)
    assert torch.equal(costs, again[0]) and torch.equal(grad, again[1])
    only, _ = mb_run(x, tl, txn, tyn, shape, layout, 0.05, 0.01, grad=False)
    assert torch.equal(costs, only)
    for n in range(N):
        c1, g1 = mb_run(x[n:n + 1].clone(), tl[n:n + 1].clone(), txn[n:n + 1].clone(), tyn[n:n + 1].clone(), shape,
                        layout, 0.05, 0.01, go[n:n + 1].clone())
        assert torch.equal(c1, costs[n:n + 1]), n
        assert torch.equal(g1[0, :xn[n], :yn[n] + 1], grad[n, :xn[n], :yn[n] + 1]), n
        assert (grad[n, xn[n]:] == 0).all() and (grad[n, :, yn[n] + 1:] == 0).all(), n
        assert (grad[n, :xn[n], :yn[n] + 1] != 0).any(), n


@pytest.mark.parametrize("dname", ["f32", "bf16"])
def test_an_address_that_narrows_the_access_moves_no_bit(dname):
    """Rows of 64 elements are 16-byte rows at every type, so here it is the tensor's address alone that narrows the
    access: the same logits in a tensor of their own, and in a contiguous view that starts one element into a larger
    buffer.  The element map does not depend on the access: costs and d/d logits are equal bit for bit."""
    from warp_rnnt_amd import ops
    dtype = {"f32": torch.float32, "bf16": torch.bfloat16}[dname]
    shape, layout = (2, 5, 3, 64, B3), "spread"
    logits, labels, xn, yn = case(shape, layout)
    ids, durations = sets_of(shape, layout)
    own = dev(logits).to(dtype)
    off = torch.empty(own.numel() + 1, dtype=dtype, device=DEV)[1:].view(own.shape)
    off.copy_(own)
    assert off.is_contiguous() and own.data_ptr() % 16 == 0 and off.data_ptr() % 16 == own.element_size()
    tl, txn, tyn, go = dev(labels), dev(xn), dev(yn), dev(_go(shape[0]))

    def both(x):
        costs, planes = ops.multiblank_loss(x, tl, txn, tyn, ids, durations, 0.05, 0.01)
        return costs, ops.multiblank_logits_backward(x, tl, planes, go, ids)

    (costs, dz), (costs_off, dz_off) = both(own), both(off)
    assert torch.isfinite(costs).all() and torch.isfinite(dz.float()).all() and (dz != 0).any()
    assert dz_off.dtype == dtype and torch.equal(costs, costs_off) and torch.equal(dz, dz_off)


def test_an_utterance_with_lengths_out_of_range_is_nan_and_zero():
    shape, layout = (4, 9, 5, 6, (2, 4)), "nemo"
    logits, labels, xn, yn = case(shape, layout)
    xn[:], yn[:] = (9, 10, 7, 0), (4, 2, 5, 1)           # fine, too many frames, too many labels, no frame
    go = dev(_go(4))
    costs, grad = mb_run(dev(logits), dev(labels), dev(xn), dev(yn), shape, layout, 0.0, 0.0, go)
    only, _ = mb_run(dev(logits), dev(labels), dev(xn), dev(yn), shape, layout, grad=False)
    assert torch.isfinite(costs[0]) and torch.isnan(costs[1:]).all() and torch.isnan(only[1:]).all()
    assert torch.equal(costs[:1], only[:1])
    assert (grad[1:] == 0).all() and (grad[0] != 0).any() and torch.isfinite(grad).all()
    c1, g1 = mb_run(dev(logits[:1]), dev(labels[:1]), dev(xn[:1]), dev(yn[:1]), shape, layout, 0.0, 0.0, go[:1].clone())
    assert torch.equal(c1, costs[:1]) and torch.equal(g1[0], grad[0])


# ---- masked logits, value range ----

@pytest.mark.parametrize("shape", [(3, 30, 12, 50, B3), (2, 9, 5, 1024, B3), (2, 9, 5, 5000, B3), (2, 14, 5, 12, (4, 2))],
                         ids=["V50", "V1024", "V5000", "d42"])
def test_masked_logits_get_exactly_zero_gradients(shape):
    """-inf at a token that is neither a blank nor a label, and at the last big blank: finite costs, exactly zero
    gradients there, and the rest inside the bars around the fp64 result for the same logits."""
    layout = "nemo"
    logits, labels, xn, yn = case(shape, layout)
    ids, durations = sets_of(shape, layout)
    token = next(v for v in range(shape[3]) if v not in ids and v not in set(labels.ravel().tolist()))
    column = ids[-1]
    logits = logits.copy()
    logits[..., token] = -np.inf
    logits[..., column] = -np.inf
    go = _go(shape[0])
    costs, grad = mb_run(dev(logits), dev(labels), dev(xn), dev(yn), shape, layout, 0.05, 0.01, dev(go))
    assert torch.isfinite(costs).all() and torch.isfinite(grad).all()
    assert (grad[..., token] == 0).all() and (grad[..., column] == 0).all()
    c64, dz64, _ = mr.multiblank_loss64(logits, labels, xn, yn, ids, durations, 0.05, 0.01)
    dz64 = dz64 * go.astype(np.float64)[:, None, None, None]
    cost = float((np.abs(costs.double().cpu().numpy() - c64) / np.abs(c64)).max())
    err = float(np.abs(grad.double().cpu().numpy() - dz64).max())
    print(f"{shape} masked token {token} and big blank {column}: cost rel {cost:.3e} (bar {COST_BAR:.3e}) "
          f"grad abs {err:.3e} (bar {GRAD_BAR:.3e})")
    assert cost <= COST_BAR and err <= GRAD_BAR


@pytest.mark.parametrize("shape", [(3, 30, 12, 50, B3), (2, 9, 5, 5000, B3), (2, 60, 9, 5, (8,))],
                         ids=["V50", "V5000", "d8"])
def test_logits_scaled_by_30_stay_finite(shape):
    layout = "spread"
    logits, labels, xn, yn = case(shape, layout)
    for dtype in (torch.float32, torch.bfloat16):
        costs, grad = mb_run(dev(logits * 30.0).to(dtype), dev(labels), dev(xn), dev(yn), shape, layout, 0.05, 0.01,
                             dev(_go(shape[0])))
        print(f"{shape} x 30 {dtype}: costs {costs.tolist()}")
        assert torch.isfinite(costs).all() and (costs > 0).all() and torch.isfinite(grad).all()


# ---- reductions, module, graph capture ----

def test_reductions_and_the_module_are_the_function():
    from warp_rnnt_amd.multiblank import MultiblankLoss, multiblank_loss_from_logits
    shape, layout = (2, 9, 5, 5, (2, 4)), "nemo"
    blank, big_ids = blanks_of(shape, layout)
    kw = dict(big_blank_durations=shape[4], blank=blank, big_blank_ids=big_ids)
    logits, labels, xn, yn = case(shape, layout)
    x, tl, txn, tyn = dev(logits), dev(labels), dev(xn), dev(yn)
    none = multiblank_loss_from_logits(x, tl, txn, tyn, **kw)
    assert none.dtype == torch.float32 and none.shape == (shape[0],)
    assert torch.equal(multiblank_loss_from_logits(x, tl, txn, tyn, reduction=None, **kw), none)
    assert torch.equal(multiblank_loss_from_logits(x, tl, txn, tyn, big_blank_durations=[2, 4], blank=blank), none)
    for average in (False, True):
        base = none / txn.to(none) if average else none
        for reduction, want in (("none", base), ("sum", base.sum()), ("mean", base.mean())):
            got = multiblank_loss_from_logits(x, tl, txn, tyn, average_frames=average, reduction=reduction, **kw)
            assert torch.equal(got, want), (average, reduction)
    for reduction in ("none", "sum", "mean"):
        xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
        a = MultiblankLoss(sigma=0.05, fastemit_lambda=0.01, reduction=reduction, **kw)(xa, tl, txn, tyn)
        b = multiblank_loss_from_logits(xb, tl, txn, tyn, sigma=0.05, fastemit_lambda=0.01, reduction=reduction, **kw)
        assert torch.equal(a, b)
        a.sum().backward()
        b.sum().backward()
        assert torch.equal(xa.grad, xb.grad)
    with pytest.raises(RuntimeError, match="status 5"):
        multiblank_loss_from_logits(x, tl, txn, tyn, big_blank_durations=(2, 4), blank=shape[3])
    with pytest.raises(RuntimeError, match="status 5"):
        multiblank_loss_from_logits(x, tl, txn, tyn, big_blank_durations=(2, 9), blank=blank)
    with pytest.raises(RuntimeError, match="status 5"):
        multiblank_loss_from_logits(x, tl, txn, tyn, big_blank_durations=(2, 4), blank=blank, big_blank_ids=(0, 0))
    with pytest.raises(RuntimeError, match="status 5"):
        multiblank_loss_from_logits(x, tl, txn, tyn, sigma=-1.0, **kw)


def test_forward_and_backward_replay_from_a_graph():
    from warp_rnnt_amd.multiblank import multiblank_loss_from_logits
    shape, layout = (3, 30, 12, 50, B3), "spread"
    blank, big_ids = blanks_of(shape, layout)
    _, labels, xn, yn = case(shape, layout)
    tl, txn, tyn = dev(labels), dev(xn), dev(yn)
    batches = [dev(case(shape, layout, seed=s)[0]) for s in (1, 2, 3)]

    def step(x):
        loss = multiblank_loss_from_logits(x, tl, txn, tyn, big_blank_durations=B3, sigma=0.05, blank=blank,
                                           big_blank_ids=big_ids, fastemit_lambda=0.01, reduction="sum")
        loss.backward()
        return loss

    want = []
    for b in batches:
        x = b.clone().requires_grad_(True)
        want.append((step(x).detach().clone(), x.grad.clone()))
    x = batches[0].clone().requires_grad_(True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            x.grad = None
            step(x)
    torch.cuda.current_stream().wait_stream(side)
    x.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss = step(x)
    for rep in range(6):
        k = rep % len(batches)
        with torch.no_grad():
            x.copy_(batches[k])
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(loss, want[k][0]), f"replay {rep}"
        assert torch.equal(x.grad, want[k][1]), f"replay {rep}"
