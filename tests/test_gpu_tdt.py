"""The token-and-duration (TDT) loss on the GPU: warp_rnnt_amd.tdt.tdt_loss_from_logits, logits -> costs -> d/d logits.

Against fp64 (tests/tdt_reference.py, itself held to exhaustive path enumeration and central differences by
tests/test_host_tdt.py) over a grid of shapes and duration sets: every lane-group size of the streaming kernels with its
edges, rows of 64 and 65 elements, every blank position, sigma and FastEmit, a skew that wraps with durations longer than
the utterance, two column blocks, more than 64 diagonals with the longest jump, durations unsorted and without 0, an
utterance of one frame and one without labels.  The bars are not taken from the code under test: they are four times the
largest error that the STANDARD fused loss, rnnt_loss_from_logits, shows on the token slice z[..., :V] of the same grid
against its own fp64 reference, measured once by tools/tdt_loss_values.py -- profiles/tdt_loss_values.txt holds every
figure, TDT's beside the yardstick's.  The lattice depth and the fp32 arithmetic are the same; TDT's cell sums up to 2D-1
terms instead of 2, each with one more addition and a second softmax: 4x leaves room for that and nothing more.  Then the
properties that hold bit for bit, masked logits, the value range, reductions and graph capture.

Every figure is printed before it is asserted (pytest -s)."""
import functools

import numpy as np
import pytest
import torch

import tdt_reference as tr
from helpers import make_case
from oracle import transduce_np

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 2.0 ** -24

D5 = (0, 1, 2, 3, 4)
# (N, T, U, V, durations)
GRID = [(3, 12, 6, 2, (0, 1)), (2, 9, 5, 3, D5), (3, 30, 12, 50, D5),
        (2, 21, 9, 59, D5), (2, 21, 9, 60, D5),                 # V + D = 64 and 65
        (2, 15, 9, 252, (0, 1, 2, 3)), (2, 9, 5, 1020, D5), (2, 9, 5, 5000, D5),
        (2, 3, 6, 7, D5),               # U > T: the skew wraps, durations longer than the utterance
        (2, 11, 70, 7, (0, 1, 2)),      # two column blocks
        (2, 60, 9, 5, (0, 1, 8)),       # more than 64 diagonals, the longest jump
        (2, 14, 5, 6, (2, 0, 1)),       # unsorted
        (2, 14, 5, 6, (1, 2))]          # no zero
SIGMAS = (0.0, 0.05)
LAMS = (0.0, 0.01)

# profiles/tdt_loss_values.txt (tools/tdt_loss_values.py on an MI355X): rnnt_loss_from_logits on z[..., :V] over
# GRID x blanks x LAMS -- largest |cost - fp64| / |fp64|, largest |d/d logits - fp64| at the upstream gradients of _go()
YARDSTICK_COST_REL = 2.569e-07   # at (2, 21, 9, 60), blank 59; TDT's largest: 3.880e-07 at (2, 11, 70, 7), blank 6, sigma 0.05
YARDSTICK_GRAD_ABS = 2.795e-05   # at (2, 11, 70, 7), blank 3, lambda 0.01; TDT's largest: 6.675e-05 at blank 6, sigma 0.05
COST_BAR = max(4 * YARDSTICK_COST_REL, 4 * EPS)      # relative to the fp64 cost
GRAD_BAR = 4 * YARDSTICK_GRAD_ABS                    # absolute


def blanks_of(V):
    return (0, V - 1) if V == 2 else (0, V // 2, V - 1)


GRID_CASES = [(shape, b) for shape in GRID for b in blanks_of(shape[3])]
GRID_IDS = ["N%d-T%d-U%d-V%d-d%s-b%d" % (*shape[:4], "".join(map(str, shape[4])), b) for shape, b in GRID_CASES]


def _go(N):
    """The upstream gradient of utterance n: not 1, exact in fp32."""
    return np.array([0.5 + 0.25 * n for n in range(N)], np.float32)


def case(shape, blank, seed=0):
    """The inputs of a grid case (fp32 logits (N,T,U,V+D) on the host), ragged lengths.  The first shape's batch holds an
    utterance of one frame and one without labels beside a full one."""
    N, T, U, V, durations = shape
    D = len(durations)
    tokens, labels, xn, yn = make_case(1000 * V + 10 * T + blank + seed, N, T, U, V, ragged=True, blank=blank)
    extra = np.random.RandomState(7 * V + T + D + seed).randn(N, T, U, D).astype(np.float32)
    logits = np.ascontiguousarray(np.concatenate([tokens, extra], axis=-1))
    if shape == GRID[0]:
        xn[:], yn[:] = (T, 1, T // 2), (U - 1, U // 2, 0)
    return logits, labels, xn, yn


@functools.lru_cache(maxsize=None)
def reference(shape, blank, sigma, lam):
    """fp64, computed once per case and shared (read-only): TDT's costs and d/d z at the upstream _go()."""
    logits, labels, xn, yn = case(shape, blank)
    go = _go(shape[0]).astype(np.float64)
    costs, dz, _ = tr.tdt_loss64(logits, labels, xn, yn, shape[4], blank, sigma, lam)
    out = (costs, dz * go[:, None, None, None])
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def standard_reference(shape, blank, lam):
    """fp64: the standard loss's costs and d/d z on the token slice, at the upstream _go()."""
    logits, labels, xn, yn = case(shape, blank)
    go = _go(shape[0]).astype(np.float64)
    lp = transduce_np.log_softmax(logits[..., :shape[3]])
    costs, glp = transduce_np.transduce_batch(lp, labels, xn, yn, blank=blank, fastemit_lambda=lam, fast=True)
    dz = glp - np.exp(lp) * glp.sum(-1, keepdims=True)
    return costs, dz * go[:, None, None, None]


def dev(a, dtype=None):
    return torch.tensor(a, device=DEV, dtype=dtype)


def tdt_run(logits, labels, xn, yn, durations, blank, sigma=0.0, lam=0.0, go=None, grad=True):
    """costs (N,) and d (sum_n go[n] cost[n]) / d logits for device tensors; grad=False: costs only, nothing requires
    grad."""
    from warp_rnnt_amd.tdt import tdt_loss_from_logits
    x = logits.detach().clone().requires_grad_(grad)
    costs = tdt_loss_from_logits(x, labels, xn, yn, durations=durations, sigma=sigma, blank=blank, fastemit_lambda=lam)
    if not grad:
        return costs, None
    g = torch.ones_like(costs) if go is None else go
    (costs * g).sum().backward()
    return costs.detach(), x.grad


def errors(shape, blank, sigma, lam):
    """One grid case on the GPU: TDT's cost error relative to fp64 and its largest d/d logits error."""
    logits, labels, xn, yn = case(shape, blank)
    c64, dz64 = reference(shape, blank, sigma, lam)
    costs, grad = tdt_run(dev(logits), dev(labels), dev(xn), dev(yn), shape[4], blank, sigma, lam, dev(_go(shape[0])))
    costs = costs.double().cpu().numpy()
    assert np.isfinite(costs).all() and torch.isfinite(grad).all()
    return float((np.abs(costs - c64) / np.abs(c64)).max()), float(np.abs(grad.double().cpu().numpy() - dz64).max())


def yardstick_errors(shape, blank, lam):
    """The same two figures for rnnt_loss_from_logits on the token slice of the case (tools/tdt_loss_values.py)."""
    from warp_rnnt_amd.fused import rnnt_loss_from_logits
    logits, labels, xn, yn = case(shape, blank)
    c64, dz64 = standard_reference(shape, blank, lam)
    x = dev(np.ascontiguousarray(logits[..., :shape[3]])).requires_grad_(True)
    costs = rnnt_loss_from_logits(x, dev(labels), dev(xn), dev(yn), blank=blank, fastemit_lambda=lam)
    (costs * dev(_go(shape[0]))).sum().backward()
    costs = costs.detach().double().cpu().numpy()
    return float((np.abs(costs - c64) / np.abs(c64)).max()), float(np.abs(x.grad.double().cpu().numpy() - dz64).max())


@pytest.mark.parametrize("shape,blank", GRID_CASES, ids=GRID_IDS)
def test_costs_and_gradients_against_fp64(shape, blank):
    for sigma in SIGMAS:
        for lam in LAMS:
            cost, grad = errors(shape, blank, sigma, lam)
            print(f"{shape} blank {blank} sigma {sigma} lam {lam}: cost rel {cost:.3e} (bar {COST_BAR:.3e})  "
                  f"grad abs {grad:.3e} (bar {GRAD_BAR:.3e})")
            assert cost <= COST_BAR, (shape, blank, sigma, lam)
            assert grad <= GRAD_BAR, (shape, blank, sigma, lam)


# ---- bit for bit ----

HALF = {"bf16": torch.bfloat16, "f16": torch.float16}
D4 = (0, 1, 2, 3)
# every lane-group size with its edges (rows of up to 256 elements: 16 lanes, up to 512: 32, longer: 64) and every access
# width at both element sizes (the widest of 16, 8, 4, 2 bytes that divides the row pitch V + D): rows of 64, 256, 512 and
# 5008 elements are 16-byte rows at every type; rows of 12 elements are 16-byte rows in fp32 and 8-byte rows in half
# precision; rows of 10 are 8-byte rows in fp32 and 4-byte rows in half precision; rows of 55, 65, 257, 513, 1025 and 5005
# are rows of single elements; then two column blocks, a skew that wraps and the longest jump for the sweeps
BIT_SHAPES = [(3, 30, 12, 50, D5), (2, 21, 9, 59, D5), (2, 21, 9, 60, D5), (2, 15, 9, 252, D4), (2, 9, 5, 253, D4),
              (2, 7, 4, 508, D4), (2, 7, 4, 509, D4), (2, 9, 5, 1020, D5), (2, 5, 3, 5000, D5), (2, 5, 3, 4999, tuple(range(9))),
              (2, 3, 6, 7, D5), (2, 11, 70, 7, (0, 1, 2)), (2, 60, 9, 5, (0, 1, 8)), (2, 14, 5, 6, (2, 0, 1))]
BIT_IDS = ["N%d-T%d-U%d-V%d-d%s" % (*s[:4], "".join(map(str, s[4]))) for s in BIT_SHAPES]


def _blank_of(shape):
    return (0, shape[3] // 2, shape[3] - 1)[shape[3] % 3]


@pytest.mark.parametrize("dname", list(HALF))
@pytest.mark.parametrize("shape", BIT_SHAPES, ids=BIT_IDS)
def test_half_precision_logits_give_the_bits_of_their_upcast(shape, dname):
    blank = _blank_of(shape)
    logits, labels, xn, yn = case(shape, blank)
    xh = dev(logits).to(HALF[dname])
    args = (dev(labels), dev(xn), dev(yn), shape[4], blank, 0.05, 0.01, dev(_go(shape[0])))
    costs_h, grad_h = tdt_run(xh, *args)
    costs_f, grad_f = tdt_run(xh.float(), *args)
    assert costs_h.dtype == torch.float32 and grad_h.dtype == HALF[dname] and grad_f.dtype == torch.float32
    assert torch.equal(costs_h, costs_f)
    assert torch.equal(grad_h, grad_f.to(HALF[dname]))


@pytest.mark.parametrize("shape", BIT_SHAPES, ids=BIT_IDS)
def test_bits_depend_on_the_utterance_alone(shape):
    """An utterance alone and inside its batch; a second call; nothing outside the window; costs without gradients."""
    blank = _blank_of(shape)
    N = shape[0]
    logits, labels, xn, yn = case(shape, blank)
    x, tl, txn, tyn, go = dev(logits), dev(labels), dev(xn), dev(yn), dev(_go(N))
    costs, grad = tdt_run(x, tl, txn, tyn, shape[4], blank, 0.05, 0.01, go)
    again = tdt_run(x, tl, txn, tyn, shape[4], blank, 0.05, 0.01, go)
    assert torch.equal(costs, again[0]) and torch.equal(grad, again[1])
    only, _ = tdt_run(x, tl, txn, tyn, shape[4], blank, 0.05, 0.01, grad=False)
    assert torch.equal(costs, only)
    for n in range(N):
        c1, g1 = tdt_run(x[n:n + 1].clone(), tl[n:n + 1].clone(), txn[n:n + 1].clone(), tyn[n:n + 1].clone(), shape[4],
                         blank, 0.05, 0.01, go[n:n + 1].clone())
        assert torch.equal(c1, costs[n:n + 1]), n
        assert torch.equal(g1[0, :xn[n], :yn[n] + 1], grad[n, :xn[n], :yn[n] + 1]), n
        assert (grad[n, xn[n]:] == 0).all() and (grad[n, :, yn[n] + 1:] == 0).all(), n
        assert (grad[n, :xn[n], :yn[n] + 1] != 0).any(), n


@pytest.mark.parametrize("dname", ["f32", "bf16"])
def test_an_address_that_narrows_the_access_moves_no_bit(dname):
    """Rows of 59 + 5 = 64 elements are 16-byte rows at every type, so here it is the tensor's address alone that narrows
    the access: the same logits in a tensor of their own, and in a contiguous view that starts one element into a larger
    buffer.  The element map does not depend on the access: costs and d/d logits are equal bit for bit."""
    from warp_rnnt_amd import ops
    dtype = {"f32": torch.float32, "bf16": torch.bfloat16}[dname]
    shape, blank = (2, 5, 3, 59, D5), 29
    logits, labels, xn, yn = case(shape, blank)
    own = dev(logits).to(dtype)
    off = torch.empty(own.numel() + 1, dtype=dtype, device=DEV)[1:].view(own.shape)
    off.copy_(own)
    assert off.is_contiguous() and own.data_ptr() % 16 == 0 and off.data_ptr() % 16 == own.element_size()
    tl, txn, tyn, go = dev(labels), dev(xn), dev(yn), dev(_go(shape[0]))

    def both(x):
        costs, planes = ops.tdt_loss(x, tl, txn, tyn, D5, blank, 0.05, 0.01)
        return costs, ops.tdt_logits_backward(x, tl, planes, go, len(D5), blank)

    (costs, dz), (costs_off, dz_off) = both(own), both(off)
    assert torch.isfinite(costs).all() and torch.isfinite(dz.float()).all() and (dz != 0).any()
    assert dz_off.dtype == dtype and torch.equal(costs, costs_off) and torch.equal(dz, dz_off)


def test_an_utterance_with_lengths_out_of_range_is_nan_and_zero():
    shape, blank = (4, 9, 5, 6, D5), 5
    logits, labels, xn, yn = case(shape, blank)
    xn[:], yn[:] = (9, 10, 7, 0), (4, 2, 5, 1)           # fine, too many frames, too many labels, no frame
    go = dev(_go(4))
    costs, grad = tdt_run(dev(logits), dev(labels), dev(xn), dev(yn), shape[4], blank, 0.0, 0.0, go)
    only, _ = tdt_run(dev(logits), dev(labels), dev(xn), dev(yn), shape[4], blank, grad=False)
    assert torch.isfinite(costs[0]) and torch.isnan(costs[1:]).all() and torch.isnan(only[1:]).all()
    assert torch.equal(costs[:1], only[:1])
    assert (grad[1:] == 0).all() and (grad[0] != 0).any() and torch.isfinite(grad).all()
    c1, g1 = tdt_run(dev(logits[:1]), dev(labels[:1]), dev(xn[:1]), dev(yn[:1]), shape[4], blank, 0.0, 0.0, go[:1].clone())
    assert torch.equal(c1, costs[:1]) and torch.equal(g1[0], grad[0])


# ---- masked logits, value range ----

@pytest.mark.parametrize("shape", [(3, 30, 12, 50, D5), (2, 9, 5, 1020, D5), (2, 5, 3, 5000, D5), (2, 14, 5, 12, (2, 0, 1))],
                         ids=["V50", "V1020", "V5000", "d201"])
def test_masked_logits_get_exactly_zero_gradients(shape):
    """-inf at a token that is neither the blank nor a label, and at the last duration other than 1 (never the 0 of
    (0..4): an utterance with as many labels as frames needs it): finite costs, exactly zero gradients there, and the rest
    inside the bars around the fp64 result for the same logits."""
    V, durations = shape[3], shape[4]
    blank = V - 1
    logits, labels, xn, yn = case(shape, blank)
    token = next(v for v in range(V) if v != blank and v not in set(labels.ravel().tolist()))
    column = V + [i for i, d in enumerate(durations) if d != 1][-1]
    logits = logits.copy()
    logits[..., token] = -np.inf
    logits[..., column] = -np.inf
    go = _go(shape[0])
    costs, grad = tdt_run(dev(logits), dev(labels), dev(xn), dev(yn), durations, blank, 0.05, 0.01, dev(go))
    assert torch.isfinite(costs).all() and torch.isfinite(grad).all()
    assert (grad[..., token] == 0).all() and (grad[..., column] == 0).all()
    c64, dz64, _ = tr.tdt_loss64(logits, labels, xn, yn, durations, blank, 0.05, 0.01)
    dz64 = dz64 * go.astype(np.float64)[:, None, None, None]
    cost = float((np.abs(costs.double().cpu().numpy() - c64) / np.abs(c64)).max())
    err = float(np.abs(grad.double().cpu().numpy() - dz64).max())
    print(f"{shape} masked token {token} and column {column}: cost rel {cost:.3e} (bar {COST_BAR:.3e}) "
          f"grad abs {err:.3e} (bar {GRAD_BAR:.3e})")
    assert cost <= COST_BAR and err <= GRAD_BAR


@pytest.mark.parametrize("shape", [(3, 30, 12, 50, D5), (2, 9, 5, 5000, D5), (2, 60, 9, 5, (0, 1, 8))],
                         ids=["V50", "V5000", "d018"])
def test_logits_scaled_by_30_stay_finite(shape):
    blank = shape[3] // 2
    logits, labels, xn, yn = case(shape, blank)
    for dtype in (torch.float32, torch.bfloat16):
        costs, grad = tdt_run(dev(logits * 30.0).to(dtype), dev(labels), dev(xn), dev(yn), shape[4], blank, 0.05, 0.01,
                              dev(_go(shape[0])))
        print(f"{shape} x 30 {dtype}: costs {costs.tolist()}")
        assert torch.isfinite(costs).all() and (costs > 0).all() and torch.isfinite(grad).all()


# ---- reductions, module, graph capture ----

def test_reductions_and_the_module_are_the_function():
    from warp_rnnt_amd.tdt import TDTLoss, tdt_loss_from_logits
    shape, blank = (2, 9, 5, 3, D5), 2
    logits, labels, xn, yn = case(shape, blank)
    x, tl, txn, tyn = dev(logits), dev(labels), dev(xn), dev(yn)
    none = tdt_loss_from_logits(x, tl, txn, tyn, blank=blank)
    assert none.dtype == torch.float32 and none.shape == (shape[0],)
    assert torch.equal(tdt_loss_from_logits(x, tl, txn, tyn, reduction=None, blank=blank), none)
    assert torch.equal(tdt_loss_from_logits(x, tl, txn, tyn, durations=list(D5), blank=blank), none)
    for average in (False, True):
        base = none / txn.to(none) if average else none
        for reduction, want in (("none", base), ("sum", base.sum()), ("mean", base.mean())):
            got = tdt_loss_from_logits(x, tl, txn, tyn, average_frames=average, reduction=reduction, blank=blank)
            assert torch.equal(got, want), (average, reduction)
    for reduction in ("none", "sum", "mean"):
        xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
        a = TDTLoss(sigma=0.05, blank=blank, fastemit_lambda=0.01, reduction=reduction)(xa, tl, txn, tyn)
        b = tdt_loss_from_logits(xb, tl, txn, tyn, sigma=0.05, blank=blank, fastemit_lambda=0.01, reduction=reduction)
        assert torch.equal(a, b)
        a.sum().backward()
        b.sum().backward()
        assert torch.equal(xa.grad, xb.grad)
    with pytest.raises(RuntimeError, match="status 5"):
        tdt_loss_from_logits(x, tl, txn, tyn, blank=shape[3])
    with pytest.raises(RuntimeError, match="status 5"):
        tdt_loss_from_logits(x, tl, txn, tyn, durations=(0, 2, 3, 4, 5), blank=blank)
    with pytest.raises(RuntimeError, match="status 5"):
        tdt_loss_from_logits(x, tl, txn, tyn, sigma=-1.0, blank=blank)


def test_forward_and_backward_replay_from_a_graph():
    from warp_rnnt_amd.tdt import tdt_loss_from_logits
    shape, blank = (3, 30, 12, 50, D5), 25
    _, labels, xn, yn = case(shape, blank)
    tl, txn, tyn = dev(labels), dev(xn), dev(yn)
    batches = [dev(case(shape, blank, seed=s)[0]) for s in (1, 2, 3)]

    def step(x):
        loss = tdt_loss_from_logits(x, tl, txn, tyn, sigma=0.05, blank=blank, fastemit_lambda=0.01, reduction="sum")
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
