"""The factorised-blank (HAT) loss on the GPU: warp_rnnt_amd.hat.hat_loss_from_logits, logits -> costs -> d/d logits.

Against fp64 (tests/hat_reference.py) over a grid of shapes that reaches every form of the two kernels -- 16, 32 and 64
lanes per row with their edges, the wave-per-row form, both access paths -- every blank position, FastEmit, a skew that
wraps, more than one column block, an utterance of one frame and one without labels.  The bars are not taken from the
code under test: they are four times the largest error that the STANDARD fused loss, rnnt_loss_from_logits, shows on the
same grid (its costs on the identity's shifted logits z' rounded to fp32, its d/d logits on z against the fp64 standard
gradient), measured once by tools/hat_loss_values.py -- profiles/hat_loss_values.txt holds every figure, HAT's beside the
yardstick's.  HAT adds two softplus evaluations and one addition per cell to the same lattice; 4x leaves room for that
and nothing more.  Then the properties that hold bit for bit, the value range, reductions, graph capture, the last column.

Every figure is printed before it is asserted (pytest -s)."""
import functools

import numpy as np
import pytest
import torch

import hat_reference as hr
from helpers import make_case
from oracle import transduce_np

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 2.0 ** -24

GRID = [(3, 12, 6, 2), (2, 9, 5, 3), (3, 30, 12, 50), (2, 21, 9, 63), (2, 21, 9, 64), (2, 21, 9, 65), (2, 15, 9, 255),
        (2, 15, 9, 256), (2, 11, 7, 258), (2, 9, 5, 1024), (2, 9, 5, 1025), (2, 6, 4, 1030), (2, 9, 5, 5000),
        (2, 3, 6, 7),           # U > T: the skew wraps
        (2, 11, 70, 7)]         # more than one column block
LAMS = (0.0, 0.01)

# profiles/hat_loss_values.txt (tools/hat_loss_values.py on an MI355X), the standard fused loss over GRID x blanks x LAMS:
# largest |cost - fp64| / |fp64| on the shifted logits, largest |d/d logits - fp64| at the upstream gradients of _go()
YARDSTICK_COST_REL = 3.298e-07   # at (2, 11, 70, 7), blank 3; HAT's largest: 2.244e-07
YARDSTICK_GRAD_ABS = 2.795e-05   # at (2, 11, 70, 7), blank 3, lambda 0.01; HAT's largest: 3.293e-05
COST_BAR = max(4 * YARDSTICK_COST_REL, 4 * EPS)      # relative to the fp64 cost
GRAD_BAR = 4 * YARDSTICK_GRAD_ABS                    # absolute


def blanks_of(V):
    return (0, V - 1) if V == 2 else (0, V // 2, V - 1)


GRID_CASES = [(shape, b) for shape in GRID for b in blanks_of(shape[3])]
GRID_IDS = ["N%d-T%d-U%d-V%d-b%d" % (*shape, b) for shape, b in GRID_CASES]


def _go(N):
    """The upstream gradient of utterance n: not 1, exact in fp32."""
    return np.array([0.5 + 0.25 * n for n in range(N)], np.float32)


def case(shape, blank, seed=0):
    """The inputs of a grid case (fp32 logits on the host).  The first shape's batch holds an utterance of one frame and
    one without labels beside a full one."""
    N, T, U, V = shape
    logits, labels, xn, yn = make_case(1000 * V + 10 * T + blank + seed, N, T, U, V, ragged=True, blank=blank)
    if shape == GRID[0]:
        xn[:], yn[:] = (T, 1, T // 2), (U - 1, U // 2, 0)
    return logits, labels, xn, yn


@functools.lru_cache(maxsize=None)
def reference(shape, blank, lam):
    """fp64, computed once per case and shared (read-only): HAT's costs and d/d z at the upstream _go(), and the standard
    loss's on the same logits."""
    logits, labels, xn, yn = case(shape, blank)
    go = _go(shape[0]).astype(np.float64)
    costs, dz = hr.hat_loss64(logits, labels, xn, yn, blank, lam)
    lp = transduce_np.log_softmax(logits)
    std_costs, glp = transduce_np.transduce_batch(lp, labels, xn, yn, blank=blank, fastemit_lambda=lam, fast=True)
    std_dz = glp - np.exp(lp) * glp.sum(-1, keepdims=True)
    out = (costs, dz * go[:, None, None, None], std_costs, std_dz * go[:, None, None, None])
    for a in out:
        a.setflags(write=False)
    return out


def dev(a, dtype=None):
    return torch.tensor(a, device=DEV, dtype=dtype)


def run(fn, logits, labels, xn, yn, blank, lam=0.0, go=None, grad=True, **kw):
    """costs (N,) and d (sum_n go[n] cost[n]) / d logits of ``fn`` for device tensors; grad=False: costs only, nothing
    requires grad."""
    x = logits.detach().clone().requires_grad_(grad)
    costs = fn(x, labels, xn, yn, blank=blank, fastemit_lambda=lam, **kw)
    if not grad:
        return costs, None
    g = torch.ones_like(costs) if go is None else go
    (costs * g).sum().backward()
    return costs.detach(), x.grad


def hat_run(logits, labels, xn, yn, blank, lam=0.0, go=None, grad=True):
    from warp_rnnt_amd.hat import hat_loss_from_logits
    return run(hat_loss_from_logits, logits, labels, xn, yn, blank, lam, go, grad)


def errors(shape, blank, lam):
    """One grid case on the GPU: (HAT cost error relative to fp64, HAT gradient error, the yardstick's two, the largest
    relative distance between HAT's costs and the standard loss's on the shifted logits)."""
    from warp_rnnt_amd.fused import rnnt_loss_from_logits
    logits, labels, xn, yn = case(shape, blank)
    c64, dz64, s64, sdz64 = reference(shape, blank, lam)
    tl, txn, tyn, go = dev(labels), dev(xn), dev(yn), dev(_go(shape[0]))
    costs, grad = hat_run(dev(logits), tl, txn, tyn, blank, lam, go)
    shifted = hr.shifted_logits64(logits, blank).astype(np.float32)
    ycosts, _ = run(rnnt_loss_from_logits, dev(shifted), tl, txn, tyn, blank, lam, go)
    _, ygrad = run(rnnt_loss_from_logits, dev(logits), tl, txn, tyn, blank, lam, go)
    costs, ycosts = costs.double().cpu().numpy(), ycosts.double().cpu().numpy()
    assert np.isfinite(costs).all() and torch.isfinite(grad).all()
    return (float((np.abs(costs - c64) / np.abs(c64)).max()), float(np.abs(grad.double().cpu().numpy() - dz64).max()),
            float((np.abs(ycosts - c64) / np.abs(c64)).max()), float(np.abs(ygrad.double().cpu().numpy() - sdz64).max()),
            float((np.abs(costs - ycosts) / np.abs(c64)).max()))


@pytest.mark.parametrize("shape,blank", GRID_CASES, ids=GRID_IDS)
def test_costs_and_gradients_against_fp64(shape, blank):
    for lam in LAMS:
        cost, grad, ycost, ygrad, cross = errors(shape, blank, lam)
        print(f"{shape} blank {blank} lam {lam}: cost rel {cost:.3e} (yardstick {ycost:.3e}, bar {COST_BAR:.3e})  "
              f"grad abs {grad:.3e} (yardstick {ygrad:.3e}, bar {GRAD_BAR:.3e})  HAT vs standard on z' {cross:.3e}")
        assert cost <= COST_BAR, (shape, blank, lam)
        assert grad <= GRAD_BAR, (shape, blank, lam)
        # the identity, against code that exists: both sit inside their bars around the same fp64 costs
        assert cross <= COST_BAR + max(YARDSTICK_COST_REL, EPS), (shape, blank, lam)


# ---- bit for bit ----

HALF = {"bf16": torch.bfloat16, "f16": torch.float16}
# every access width at both element sizes (the widest of 16, 8, 4, 2 bytes that divides the row pitch): V = 64, 256, 1024
# and 5000 are 16-byte rows in fp32 and in half precision, V = 52 and 1028 in fp32 only (8 bytes in half precision), V = 50,
# 258 and 1030 are 8-byte rows in fp32 and 4-byte rows in half precision, V = 65 and 1025 are rows of single elements
BIT_SHAPES = [(3, 30, 12, 50), (2, 9, 5, 52), (2, 21, 9, 64), (2, 21, 9, 65), (2, 15, 9, 256), (2, 11, 7, 258),
              (2, 9, 5, 1024), (2, 9, 5, 1025), (2, 5, 3, 1028), (2, 6, 4, 1030), (2, 9, 5, 5000)]
BIT_IDS = ["N%d-T%d-U%d-V%d" % s for s in BIT_SHAPES]


def _blank_of(shape):
    return (0, shape[3] // 2, shape[3] - 1)[shape[3] % 3]


@pytest.mark.parametrize("dname", list(HALF))
@pytest.mark.parametrize("shape", BIT_SHAPES, ids=BIT_IDS)
def test_half_precision_logits_give_the_bits_of_their_upcast(shape, dname):
    blank = _blank_of(shape)
    logits, labels, xn, yn = case(shape, blank)
    go = dev(_go(shape[0]))
    xh = dev(logits).to(HALF[dname])
    args = (dev(labels), dev(xn), dev(yn), blank, 0.01, go)
    costs_h, grad_h = hat_run(xh, *args)
    costs_f, grad_f = hat_run(xh.float(), *args)
    assert costs_h.dtype == torch.float32 and grad_h.dtype == HALF[dname] and grad_f.dtype == torch.float32
    assert torch.equal(costs_h, costs_f)
    assert torch.equal(grad_h, grad_f.to(HALF[dname]))


@pytest.mark.parametrize("shape", BIT_SHAPES, ids=BIT_IDS)
def test_bits_depend_on_the_utterance_alone(shape):
    """An utterance alone and inside its batch; a second call; nothing outside the window; costs without gradients."""
    blank = _blank_of(shape)
    N, T, U, V = shape
    logits, labels, xn, yn = case(shape, blank)
    x, tl, txn, tyn, go = dev(logits), dev(labels), dev(xn), dev(yn), dev(_go(N))
    costs, grad = hat_run(x, tl, txn, tyn, blank, 0.01, go)
    again = hat_run(x, tl, txn, tyn, blank, 0.01, go)
    assert torch.equal(costs, again[0]) and torch.equal(grad, again[1])
    only, _ = hat_run(x, tl, txn, tyn, blank, 0.01, grad=False)
    assert torch.equal(costs, only)
    for n in range(N):
        c1, g1 = hat_run(x[n:n + 1].contiguous(), tl[n:n + 1].contiguous(), txn[n:n + 1].contiguous(),
                         tyn[n:n + 1].contiguous(), blank, 0.01, go[n:n + 1].contiguous())
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
    shape, blank = (2, 5, 3, 64), 21
    logits, labels, xn, yn = case(shape, blank)
    own = dev(logits).to(dtype)
    off = torch.empty(own.numel() + 1, dtype=dtype, device=DEV)[1:].view(shape)
    off.copy_(own)
    assert off.is_contiguous() and own.data_ptr() % 16 == 0 and off.data_ptr() % 16 == own.element_size()
    tl, txn, tyn, go = dev(labels), dev(xn), dev(yn), dev(_go(shape[0]))

    def both(x):
        costs, pairs = ops.hat_loss(x, tl, txn, tyn, blank, 0.01)
        return costs, ops.hat_logits_backward(x, tl, pairs, go, blank)

    (costs, dz), (costs_off, dz_off) = both(own), both(off)
    assert torch.isfinite(costs).all() and torch.isfinite(dz.float()).all() and (dz != 0).any()
    assert dz_off.dtype == dtype and torch.equal(costs, costs_off) and torch.equal(dz, dz_off)


def _masked_case(shape, blank, masked):
    """Logits with the non-blank columns ``masked`` at -inf and labels that avoid them; the same problem with those
    columns removed (V smaller, blank and labels remapped)."""
    N, T, U, V = shape
    kept = [v for v in range(V) if v not in set(masked)]
    small_blank = kept.index(blank)
    small_logits, small_labels, xn, yn = make_case(77 + V, N, T, U, len(kept), ragged=True, blank=small_blank)
    logits = np.full(shape, -np.inf, np.float32)
    logits[..., kept] = small_logits
    labels = np.asarray(kept, np.int32)[small_labels]
    return logits, labels, xn, yn, kept, small_logits, small_labels, small_blank


@pytest.mark.parametrize("which", [0, 1, 2], ids=["blank0", "blank-mid", "blank-last"])
@pytest.mark.parametrize("shape,n_masked", [((3, 30, 12, 50), 6), ((2, 15, 9, 256), 10), ((2, 9, 5, 5000), 11)],
                         ids=["V50", "V256", "V5000"])
def test_masked_trailing_columns_are_columns_that_are_not_there(shape, n_masked, which):
    """-inf at the last non-blank columns: exactly zero gradients there, and the bits -- costs and the other gradients --
    of the call with those columns removed.  Bit-equality needs every kept non-blank column to keep its index: a row's sum
    is taken in the order of its columns, in fp32, and no fixed order of fp32 additions is invariant under moving its
    terms -- so the masked columns are the trailing ones (the blank may move: it is not part of the sum), and V stays in
    its form (16 lanes, 64 lanes, a wave per row)."""
    V = shape[3]
    blank = blanks_of(V)[which]
    masked = [v for v in range(V - 1, -1, -1) if v != blank][:n_masked]
    logits, labels, xn, yn, kept, small_logits, small_labels, small_blank = _masked_case(shape, blank, masked)
    go, txn, tyn = dev(_go(shape[0])), dev(xn), dev(yn)
    costs, grad = hat_run(dev(logits), dev(labels), txn, tyn, blank, 0.01, go)
    small_costs, small_grad = hat_run(dev(small_logits), dev(small_labels), txn, tyn, small_blank, 0.01, go)
    assert torch.isfinite(costs).all()
    assert (grad[..., masked] == 0).all()
    assert torch.equal(costs, small_costs)
    assert torch.equal(grad[..., kept], small_grad)


@pytest.mark.parametrize("shape", [(3, 30, 12, 50), (2, 9, 5, 1025), (2, 9, 5, 5000)], ids=["V50", "V1025", "V5000"])
def test_masked_columns_anywhere_against_fp64(shape):
    """-inf at every third non-blank column: exactly zero gradients there, costs and gradients inside the bars."""
    V = shape[3]
    blank = V // 2
    masked = [v for v in range(V) if v != blank][1::3]
    logits, labels, xn, yn, *_ = _masked_case(shape, blank, masked)
    go = _go(shape[0])
    costs, grad = hat_run(dev(logits), dev(labels), dev(xn), dev(yn), blank, 0.0, dev(go))
    c64, dz64 = hr.hat_loss64(logits, labels, xn, yn, blank, 0.0)
    dz64 = dz64 * go.astype(np.float64)[:, None, None, None]
    assert (grad[..., masked] == 0).all() and (dz64[..., masked] == 0).all()
    cost = float((np.abs(costs.double().cpu().numpy() - c64) / np.abs(c64)).max())
    err = float(np.abs(grad.double().cpu().numpy() - dz64).max())
    print(f"{shape} masked {len(masked)} columns: cost rel {cost:.3e} (bar {COST_BAR:.3e}) grad abs {err:.3e} (bar {GRAD_BAR:.3e})")
    assert cost <= COST_BAR and err <= GRAD_BAR


# ---- value range ----

@pytest.mark.parametrize("shape", [(3, 30, 12, 50), (2, 21, 9, 64), (2, 9, 5, 5000)], ids=["V50", "V64", "V5000"])
def test_a_shift_of_the_non_blank_logits_moves_no_bit(shape):
    """Logits on a grid of 1/64, so that +-60000 is added without rounding in fp32: z_v - m is then the same float, and
    with it every cost and gradient bit."""
    V = shape[3]
    blank = V // 2
    logits, labels, xn, yn = case(shape, blank)
    logits = (np.round(logits * 64) / 64).astype(np.float32)
    keep = np.arange(V) != blank
    args = (dev(labels), dev(xn), dev(yn), blank, 0.01, dev(_go(shape[0])))
    costs, grad = hat_run(dev(logits), *args)
    for shift in (60000.0, -60000.0):
        moved = logits.copy()
        moved[..., keep] += np.float32(shift)
        assert ((moved[..., keep].astype(np.float64) - shift) == logits[..., keep]).all()      # exact
        c, g = hat_run(dev(moved), *args)
        assert torch.equal(c, costs), shift
        assert torch.equal(g, grad), shift


@pytest.mark.parametrize("zb", [80.0, -80.0])
def test_a_saturated_blank_logit_stays_finite_and_inside_the_bars(zb):
    shape, blank = (2, 9, 5, 3), 1
    logits, labels, xn, yn = case(shape, blank)
    logits = logits.copy()
    logits[..., blank] = zb
    go = _go(shape[0])
    costs, grad = hat_run(dev(logits), dev(labels), dev(xn), dev(yn), blank, 0.0, dev(go))
    assert torch.isfinite(costs).all() and torch.isfinite(grad).all()
    c64, dz64 = hr.hat_loss64(logits, labels, xn, yn, blank, 0.0)
    dz64 = dz64 * go.astype(np.float64)[:, None, None, None]
    cost = float((np.abs(costs.double().cpu().numpy() - c64) / np.abs(c64)).max())
    err = float(np.abs(grad.double().cpu().numpy() - dz64).max())
    print(f"z_b = {zb}: costs {costs.tolist()} cost rel {cost:.3e} (bar {COST_BAR:.3e}) grad abs {err:.3e} (bar {GRAD_BAR:.3e})")
    assert cost <= COST_BAR and err <= GRAD_BAR


# ---- reductions, module, graph capture, last column ----

def test_reductions_and_the_module_are_the_function():
    from warp_rnnt_amd.hat import HATLoss, hat_loss_from_logits
    shape, blank = (2, 9, 5, 3), 2
    logits, labels, xn, yn = case(shape, blank)
    x, tl, txn, tyn = dev(logits), dev(labels), dev(xn), dev(yn)
    none = hat_loss_from_logits(x, tl, txn, tyn, blank=blank)
    assert none.dtype == torch.float32 and none.shape == (shape[0],)
    assert torch.equal(hat_loss_from_logits(x, tl, txn, tyn, reduction=None, blank=blank), none)
    for average in (False, True):
        base = none / txn.to(none) if average else none
        for reduction, want in (("none", base), ("sum", base.sum()), ("mean", base.mean())):
            got = hat_loss_from_logits(x, tl, txn, tyn, average_frames=average, reduction=reduction, blank=blank)
            assert torch.equal(got, want), (average, reduction)
    for reduction in ("none", "sum", "mean"):
        xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
        a = HATLoss(blank=blank, fastemit_lambda=0.01, reduction=reduction)(xa, tl, txn, tyn)
        b = hat_loss_from_logits(xb, tl, txn, tyn, reduction=reduction, blank=blank, fastemit_lambda=0.01)
        assert torch.equal(a, b)
        a.sum().backward()
        b.sum().backward()
        assert torch.equal(xa.grad, xb.grad)
    with pytest.raises(RuntimeError, match="status 5"):
        hat_loss_from_logits(x, tl, txn, tyn, blank=shape[3])
    with pytest.raises(RuntimeError, match="status 5"):
        hat_loss_from_logits(x[..., :1].contiguous(), tl, txn, tyn, blank=0)


def test_forward_and_backward_replay_from_a_graph():
    from warp_rnnt_amd.hat import hat_loss_from_logits
    shape, blank = (3, 30, 12, 50), 25
    _, labels, xn, yn = case(shape, blank)
    tl, txn, tyn = dev(labels), dev(xn), dev(yn)
    batches = [dev(case(shape, blank, seed=s)[0]) for s in (1, 2, 3)]

    def step(x):
        loss = hat_loss_from_logits(x, tl, txn, tyn, reduction="sum", blank=blank, fastemit_lambda=0.01)
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


@pytest.mark.parametrize("blank", [0, 4])
def test_a_lattice_of_one_column_is_a_sum_of_blanks(blank):
    """U = 1, no labels at all: cost = -sum_t lpB, and nothing but z_b gets a gradient."""
    N, T, U, V = 2, 7, 1, 5
    logits, labels, xn, yn = make_case(9, N, T, U, V, ragged=True, blank=blank)
    costs, grad = hat_run(dev(logits), dev(labels), dev(xn), dev(yn), blank)
    lpB = hr.hat_log_probs64(logits, blank)[..., 0, blank]
    want = np.array([-lpB[n, :xn[n]].sum() for n in range(N)])
    rel = float((np.abs(costs.double().cpu().numpy() - want) / np.abs(want)).max())
    print(f"U = 1 blank {blank}: cost rel {rel:.3e} (bar {COST_BAR:.3e})")
    assert rel <= COST_BAR
    keep = [v for v in range(V) if v != blank]
    assert (grad[..., keep] == 0).all()
    sig = 1.0 / (1.0 + np.exp(-logits[..., 0, blank].astype(np.float64)))
    for n in range(N):
        np.testing.assert_allclose(grad[n, :xn[n], 0, blank].double().cpu().numpy(), -(1.0 - sig[n, :xn[n]]),
                                   rtol=0, atol=max(GRAD_BAR, 4 * EPS))
