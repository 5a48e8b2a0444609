"""The pruned transducer loss on the GPU: warp_rnnt_amd.pruned.pruned_rnnt_loss_from_logits, logits (N,T,S,V) -> costs ->
d/d logits.

Against fp64 (tests/pruned_reference.py: the band recursion with true -inf outside the band) over a grid of shapes that
reaches 16, 32 and 64 lanes per row with their edges, rows beyond 1024 elements, every access width, three blank
positions, FastEmit, a skew that wraps, more than one column block, the full band, an utterance of one frame and one
without labels, and each of the three sweep kernels.  The bars are not taken from the code under test: they are four times
the largest error that the STANDARD fused loss, rnnt_loss_from_logits, shows on dense (N,T,U,V) logits of the same
generator, shapes and lengths, measured once by tools/pruned_loss_values.py -- profiles/pruned_loss_values.txt holds every
figure, the pruned loss's beside the yardstick's.  The pruned loss sums over the same lattice in another order (the floor's
cells add nothing); 4x is the margin the HAT and TDT tests give such a feature.  Then what holds bit for bit, the band
without a path, reductions, graph capture and the three-step recipe end to end.

Every figure is printed before it is asserted (pytest -s)."""
import functools

import numpy as np
import pytest
import torch

import pruned_reference as pr
from oracle import transduce_np

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 2.0 ** -24

# (N, T, U, S, V)
GRID = [(3, 12, 6, 2, 2),        # an utterance of one frame and one without labels
        (2, 9, 5, 3, 3), (3, 30, 12, 4, 50), (2, 21, 9, 5, 63), (2, 21, 9, 5, 64), (2, 21, 9, 5, 65), (2, 15, 9, 3, 255),
        (2, 15, 9, 3, 256), (2, 11, 7, 2, 258), (2, 9, 5, 5, 1024), (2, 9, 5, 2, 1025), (2, 6, 4, 4, 1030),
        (2, 9, 5, 3, 5000),
        (2, 3, 6, 3, 7),         # U > T: the skew wraps
        (2, 11, 70, 5, 7),       # more than one column block
        (2, 11, 70, 70, 7),      # the full band
        # one shape per sweep kernel, chosen with the pure planner of lattice_plan.h (KERNEL_OF below)
        (2, 40, 130, 5, 8), (2, 60, 400, 8, 8), (2, 2048, 260, 5, 8)]
KERNEL_OF = {(2, 40, 130, 5, 8): "lattice_wl", (2, 60, 400, 8, 8): "lattice_ws", (2, 2048, 260, 5, 8): "lattice_wd"}
LAMS = (0.0, 0.01)

# profiles/pruned_loss_values.txt (tools/pruned_loss_values.py on an MI355X), the standard fused loss on dense logits over
# GRID x blanks x LAMS: largest |cost - fp64| / |fp64|, largest |d/d logits - fp64| at the upstream gradients 0.5 + 0.25 n
YARDSTICK_COST_REL = 2.141e-06   # at (2, 2048, 260, 5, 8), blank 4; the pruned loss's largest: 1.370e-06, there too
YARDSTICK_GRAD_ABS = 4.532e-03   # at (2, 2048, 260, 5, 8), blank 4; the pruned loss's largest: 4.089e-03, at blank 7
#                                  (costs of 3e3 to 4.4e3 there: one ulp of a lattice value is 2.4e-4 to 4.9e-4)
COST_BAR = max(4 * YARDSTICK_COST_REL, 4 * EPS)      # relative to the fp64 cost
GRAD_BAR = 4 * YARDSTICK_GRAD_ABS                    # absolute


def blanks_of(V):
    return (0, V - 1) if V == 2 else (0, V // 2, V - 1)


GRID_CASES = [(shape, b) for shape in GRID for b in blanks_of(shape[4])]
GRID_IDS = ["N%d-T%d-U%d-S%d-V%d-b%d" % (*shape, b) for shape, b in GRID_CASES]


def _go(N):
    return pr.upstream(N).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _case(shape, blank, seed):
    N, T, U, S, V = shape
    lengths = ((T, 1, T // 2), (U - 1, 1, 0)) if shape == GRID[0] else None
    out = pr.make_band_case(1000 * V + 10 * T + S + blank + seed, N, T, U, S, V, blank=blank, lengths=lengths)
    for a in out:
        a.setflags(write=False)
    return out


def case(shape, blank, seed=0):
    """The inputs of a grid case on the host (read-only): logits (N,T,S,V) fp32, labels, starts, xn, yn."""
    return _case(tuple(shape), blank, seed)


@functools.lru_cache(maxsize=None)
def reference(shape, blank, lam):
    """fp64, computed once per case and shared (read-only): the pruned costs and d/d logits at the upstream _go(), and the
    standard loss's on the dense logits of dense_of()."""
    logits, labels, starts, xn, yn = case(shape, blank)
    ref = pr.pruned_loss64(logits, labels, starts, xn, yn, blank, lam)
    go = pr.upstream(shape[0])
    lp = transduce_np.log_softmax(dense_of(shape, blank))
    std_costs, glp = transduce_np.transduce_batch(lp, labels, xn, yn, blank=blank, fastemit_lambda=lam, fast=True)
    std_dz = (glp - np.exp(lp) * glp.sum(-1, keepdims=True)) * go[:, None, None, None]
    out = (ref["costs"], ref["dlogits"], std_costs, std_dz)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def dense_of(shape, blank):
    """The yardstick's input: dense (N,T,U,V) logits of the same generator (N(0,1)), the band's rows in their cells."""
    logits, _, starts, _, _ = case(shape, blank)
    dense = pr.dense_from_band(logits, starts, shape[2], fill_seed=shape[4] + blank)
    dense.setflags(write=False)
    return dense


def dev(a, dtype=None):
    return torch.tensor(np.asarray(a), device=DEV, dtype=dtype)


def pruned_run(logits, labels, ranges, xn, yn, blank, lam=0.0, go=None, grad=True):
    """costs (N,) and d (sum_n go[n] cost[n]) / d logits for device tensors; grad=False: costs only."""
    from warp_rnnt_amd.pruned import pruned_rnnt_loss_from_logits
    x = logits.detach().clone().requires_grad_(grad)
    costs = pruned_rnnt_loss_from_logits(x, labels, ranges, xn, yn, blank=blank, fastemit_lambda=lam)
    if not grad:
        return costs, None
    g = torch.ones_like(costs) if go is None else go
    (costs * g).sum().backward()          # (a cost of +inf: its upstream gradient is g[n] all the same)
    return costs.detach(), x.grad


def errors(shape, blank, lam):
    """One grid case on the GPU: (pruned cost error relative to fp64, pruned gradient error, the yardstick's two, the sweep
    kernel the pruned call ran)."""
    from warp_rnnt_amd import debug
    from warp_rnnt_amd.fused import rnnt_loss_from_logits
    logits, labels, starts, xn, yn = case(shape, blank)
    c64, dz64, s64, sdz64 = reference(shape, blank, lam)
    tl, ts, txn, tyn, go = dev(labels), dev(starts), dev(xn), dev(yn), dev(_go(shape[0]))
    costs, grad = pruned_run(dev(logits), tl, ts, txn, tyn, blank, lam, go)
    kernel = debug.last_lattice_kernel()
    x = dev(dense_of(shape, blank)).requires_grad_(True)
    ycosts = rnnt_loss_from_logits(x, tl, txn, tyn, blank=blank, fastemit_lambda=lam)
    (ycosts * go).sum().backward()
    costs, ycosts = costs.double().cpu().numpy(), ycosts.detach().double().cpu().numpy()
    assert np.isfinite(costs).all() and torch.isfinite(grad).all()
    return (float((np.abs(costs - c64) / np.abs(c64)).max()), float(np.abs(grad.double().cpu().numpy() - dz64).max()),
            float((np.abs(ycosts - s64) / np.abs(s64)).max()), float(np.abs(x.grad.double().cpu().numpy() - sdz64).max()),
            kernel)


@pytest.mark.parametrize("shape,blank", GRID_CASES, ids=GRID_IDS)
def test_costs_and_gradients_against_fp64(shape, blank):
    from warp_rnnt_amd import debug
    for lam in LAMS:
        cost, grad, ycost, ygrad, kernel = errors(shape, blank, lam)
        print(f"{shape} blank {blank} lam {lam}: cost rel {cost:.3e} (yardstick {ycost:.3e}, bar {COST_BAR:.3e})  "
              f"grad abs {grad:.3e} (yardstick {ygrad:.3e}, bar {GRAD_BAR:.3e})  {kernel}")
        assert cost <= COST_BAR, (shape, blank, lam)
        assert grad <= GRAD_BAR, (shape, blank, lam)
        if shape in KERNEL_OF:      # the producer carries no ring preparation: the unfolded plan
            assert kernel == KERNEL_OF[shape] == debug.lattice_plan(*shape[:3], folded=False).kernel, (shape, kernel)


def test_gradient_is_exactly_zero_outside_the_window_and_not_inside():
    shape, blank = (3, 30, 12, 4, 50), 25
    logits, labels, starts, xn, yn = case(shape, blank)
    _, grad = pruned_run(dev(logits), dev(labels), dev(starts), dev(xn), dev(yn), blank, 0.01, dev(_go(shape[0])))
    N, T, U, S, V = shape
    u = starts[:, :, None].astype(np.int64) + np.arange(S)
    t = np.arange(T)[None, :, None]
    dead = torch.tensor((t >= xn[:, None, None]) | (u > yn[:, None, None]), device=DEV)
    assert dead.any() and (~dead).any()
    assert (grad[dead] == 0).all()
    for n in range(N):
        assert (grad[n][~dead[n]] != 0).any(), n


# ---- bit for bit ----

HALF = {"bf16": torch.bfloat16, "f16": torch.float16}
# every access width at both element sizes: V = 64, 256, 1024 and 5000 are 16-byte rows in fp32 and in half precision, V = 50,
# 258 and 1030 are 8-byte rows in fp32 and 4-byte rows in half precision, V = 63, 65, 255 and 1025 are rows of single elements
BIT_SHAPES = [(3, 30, 12, 4, 50), (2, 21, 9, 5, 63), (2, 21, 9, 5, 64), (2, 21, 9, 5, 65), (2, 15, 9, 3, 256),
              (2, 11, 7, 2, 258), (2, 9, 5, 5, 1024), (2, 9, 5, 2, 1025), (2, 6, 4, 4, 1030), (2, 9, 5, 3, 5000)]
BIT_IDS = ["N%d-T%d-U%d-S%d-V%d" % s for s in BIT_SHAPES]


def _blank_of(shape):
    return (0, shape[4] // 2, shape[4] - 1)[shape[4] % 3]


def _args(shape, blank):
    logits, labels, starts, xn, yn = case(shape, blank)
    return dev(logits), dev(labels), dev(starts), dev(xn), dev(yn), dev(_go(shape[0]))


@pytest.mark.parametrize("dname", list(HALF))
@pytest.mark.parametrize("shape", BIT_SHAPES, ids=BIT_IDS)
def test_half_precision_logits_give_the_bits_of_their_upcast(shape, dname):
    blank = _blank_of(shape)
    x, tl, ts, txn, tyn, go = _args(shape, blank)
    xh = x.to(HALF[dname])
    costs_h, grad_h = pruned_run(xh, tl, ts, txn, tyn, blank, 0.01, go)
    costs_f, grad_f = pruned_run(xh.float(), tl, ts, txn, tyn, blank, 0.01, go)
    assert costs_h.dtype == torch.float32 and grad_h.dtype == HALF[dname] and grad_f.dtype == torch.float32
    assert torch.isfinite(costs_h).all() and (grad_h != 0).any()
    assert torch.equal(costs_h, costs_f)
    assert torch.equal(grad_h, grad_f.to(HALF[dname]))       # the fp32 result rounded once


@pytest.mark.parametrize("shape", BIT_SHAPES, ids=BIT_IDS)
def test_bits_depend_on_the_utterance_alone(shape):
    """An utterance alone and inside its batch; a second call; costs without gradients."""
    blank = _blank_of(shape)
    x, tl, ts, txn, tyn, go = _args(shape, blank)
    costs, grad = pruned_run(x, tl, ts, txn, tyn, blank, 0.01, go)
    again = pruned_run(x, tl, ts, txn, tyn, blank, 0.01, go)
    assert torch.equal(costs, again[0]) and torch.equal(grad, again[1])
    only, _ = pruned_run(x, tl, ts, txn, tyn, blank, 0.01, grad=False)
    assert torch.equal(costs, only)
    for n in range(shape[0]):
        one = [a[n:n + 1].contiguous() for a in (x, tl, ts, txn, tyn)]
        c1, g1 = pruned_run(*one, blank, 0.01, go[n:n + 1].contiguous())
        assert torch.equal(c1, costs[n:n + 1]), n
        assert torch.equal(g1[0], grad[n]), n
        assert (grad[n] != 0).any(), n


def test_both_forms_of_the_ranges_give_the_same_bits():
    shape, blank = (3, 30, 12, 4, 50), 0
    x, tl, ts, txn, tyn, go = _args(shape, blank)
    k2 = ts.long()[..., None] + torch.arange(shape[3], device=DEV)
    assert k2.dtype == torch.int64 and tuple(k2.shape) == shape[:2] + (shape[3],)
    a = pruned_run(x, tl, ts, txn, tyn, blank, 0.01, go)
    b = pruned_run(x, tl, k2, txn, tyn, blank, 0.01, go)
    c = pruned_run(x, tl, k2[:, :, :1].expand(-1, -1, shape[3]), txn, tyn, blank, 0.01, go)     # only [..., 0] is used
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])


def test_garbage_starts_behind_the_last_frame_move_no_bit():
    shape, blank = (3, 30, 12, 4, 50), 49
    logits, labels, starts, xn, yn = case(shape, blank)
    assert (xn < shape[1]).any()
    x, tl, ts, txn, tyn, go = _args(shape, blank)
    costs, grad = pruned_run(x, tl, ts, txn, tyn, blank, 0.01, go)
    garbage = np.array([-5, shape[2] + 3, 2 ** 31 - 1, -2 ** 31, 0, shape[2] - 1, 3, -1], np.int64)
    bad = starts.copy()
    for n in range(shape[0]):
        k = shape[1] - int(xn[n])
        bad[n, xn[n]:] = np.resize(garbage, k).astype(np.int32)
    c2, g2 = pruned_run(x, tl, dev(bad), txn, tyn, blank, 0.01, go)
    assert torch.equal(costs, c2)
    for n in range(shape[0]):
        assert torch.equal(grad[n, :xn[n]], g2[n, :xn[n]]), n
        assert (g2[n, xn[n]:] == 0).all(), n


@pytest.mark.parametrize("dname", ["f32", "bf16"])
def test_an_address_that_narrows_the_access_moves_no_bit(dname):
    """Rows of 64 elements are 16-byte rows at every type, so here it is the tensor's address alone that narrows the
    access: the same logits in a tensor of their own, and in a contiguous slice that starts one element into a larger
    buffer.  The element map does not depend on the access: costs and d/d logits are equal bit for bit."""
    from warp_rnnt_amd import ops
    dtype = {"f32": torch.float32, "bf16": torch.bfloat16}[dname]
    shape, blank = (2, 21, 9, 5, 64), 21
    x, tl, ts, txn, tyn, go = _args(shape, blank)
    own = x.to(dtype)
    off = torch.empty(own.numel() + 1, dtype=dtype, device=DEV)[1:].view(own.shape)
    off.copy_(own)
    assert off.is_contiguous() and own.data_ptr() % 16 == 0 and off.data_ptr() % 16 == own.element_size()

    def both(z):
        costs, pairs = ops.pruned_loss(z, tl, ts, txn, tyn, blank, 0.01)
        return costs, ops.pruned_logits_backward(z, tl, ts, pairs, go, blank)

    (costs, dz), (costs_off, dz_off) = both(own), both(off)
    assert torch.isfinite(costs).all() and torch.isfinite(dz.float()).all() and (dz != 0).any()
    assert dz_off.dtype == dtype and torch.equal(costs, costs_off) and torch.equal(dz, dz_off)


@pytest.mark.parametrize("V", [7, 64, 1030])
def test_rows_mapped_outside_the_grid_are_not_part_of_the_call(V):
    """start = -1 on the first frame and start = U - S + 1 on the last ones: row s = 0 of the first and row s = S - 1 of
    the last map to u = -1 and u = U.  They get exactly zero gradient rows, and whatever they hold -- NaN here -- moves no
    bit of anything else."""
    N, T, U, S, blank = 2, 9, 5, 3, 1
    logits, labels, _, xn, yn = pr.make_band_case(V, N, T, U, S, V, blank=blank, ragged=False)
    starts = np.tile(np.array([-1, 0, 0, 1, 1, 1, 2, 3, 3], np.int32), (N, 1))
    starts[1] = [0, 0, 0, 1, 1, 1, 2, 2, 2]
    outside = np.zeros((N, T, S), bool)
    outside[0, 0, 0] = outside[0, 7, S - 1] = outside[0, 8, S - 1] = True
    ref = pr.pruned_loss64(logits, labels, starts, xn, yn, blank, 0.01)
    assert np.isfinite(ref["costs"]).all() and (ref["dlogits"][outside] == 0).all()
    tl, ts, txn, tyn, go = dev(labels), dev(starts), dev(xn), dev(yn), dev(_go(N))
    costs, grad = pruned_run(dev(logits), tl, ts, txn, tyn, blank, 0.01, go)
    cost = float((np.abs(costs.double().cpu().numpy() - ref["costs"]) / np.abs(ref["costs"])).max())
    err = float(np.abs(grad.double().cpu().numpy() - ref["dlogits"]).max())
    print(f"V {V}: rows outside the grid: cost rel {cost:.3e} (bar {COST_BAR:.3e}) grad abs {err:.3e} (bar {GRAD_BAR:.3e})")
    assert cost <= COST_BAR and err <= GRAD_BAR
    mask = torch.tensor(outside, device=DEV)
    assert (grad[mask] == 0).all() and (grad[~mask] != 0).any(dim=-1).all()
    other = logits.copy()
    other[outside] = np.nan
    c2, g2 = pruned_run(dev(other), tl, ts, txn, tyn, blank, 0.01, go)
    assert torch.equal(costs, c2) and torch.equal(grad, g2)


# ---- behaviour ----

def test_a_band_without_a_path_gives_inf_and_zero_rows_and_leaves_the_others_alone():
    shape, blank = (3, 30, 12, 4, 50), 25
    logits, labels, starts, xn, yn = case(shape, blank)
    x, tl, ts, txn, tyn, go = _args(shape, blank)
    costs, grad = pruned_run(x, tl, ts, txn, tyn, blank, 0.01, go)
    for which, new in (("(0,0) outside", 1), ("the last cell outside", 0)):
        bad = starts.copy()
        if new:
            bad[1, 0] = 1                      # the first band begins behind (0,0)
        else:
            bad[1, :] = 0                      # the band never reaches column U_n: S = 4 < U_n + 1
            assert yn[1] + 1 > shape[3]
        c2, g2 = pruned_run(x, tl, dev(bad), txn, tyn, blank, 0.01, go)
        print(f"{which}: costs {c2.tolist()}")
        assert torch.isinf(c2[1]) and c2[1] > 0, which
        assert (g2[1] == 0).all(), which
        for n in (0, 2):
            assert torch.equal(c2[n], costs[n]) and torch.equal(g2[n], grad[n]), (which, n)
        only, _ = pruned_run(x, tl, dev(bad), txn, tyn, blank, 0.01, grad=False)
        assert torch.equal(only, c2)
    # the C entry's own answer, which the front end turns into +inf: at least 1e29
    from warp_rnnt_amd import ops
    raw, _ = ops.pruned_loss(x, tl, dev(bad), txn, tyn, blank, 0.0, with_grads=False)
    print(f"the C entry's cost of a band without a path: {raw[1].item():.3e}")
    assert raw[1].item() >= 1e29 and torch.equal(raw[[0, 2]], pruned_run(x, tl, ts, txn, tyn, blank, grad=False)[0][[0, 2]])


def test_reductions_and_the_module_are_the_function():
    from warp_rnnt_amd.pruned import PrunedRNNTLoss, pruned_rnnt_loss_from_logits
    shape, blank = (2, 9, 5, 3, 3), 2
    x, tl, ts, txn, tyn, _ = _args(shape, blank)
    none = pruned_rnnt_loss_from_logits(x, tl, ts, txn, tyn, blank=blank)
    assert none.dtype == torch.float32 and none.shape == (shape[0],) and torch.isfinite(none).all()
    assert torch.equal(pruned_rnnt_loss_from_logits(x, tl, ts, txn, tyn, reduction=None, blank=blank), none)
    for average in (False, True):
        base = none / txn.to(none) if average else none
        for reduction, want in (("none", base), ("sum", base.sum()), ("mean", base.mean())):
            got = pruned_rnnt_loss_from_logits(x, tl, ts, txn, tyn, average_frames=average, reduction=reduction, blank=blank)
            assert torch.equal(got, want), (average, reduction)
    for reduction in ("none", "sum", "mean"):
        xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
        a = PrunedRNNTLoss(blank=blank, fastemit_lambda=0.01, reduction=reduction)(xa, tl, ts, txn, tyn)
        b = pruned_rnnt_loss_from_logits(xb, tl, ts, txn, tyn, reduction=reduction, blank=blank, fastemit_lambda=0.01)
        assert torch.equal(a, b)
        a.sum().backward()
        b.sum().backward()
        assert torch.equal(xa.grad, xb.grad) and (xa.grad != 0).any()
    with pytest.raises(RuntimeError, match="status 5"):
        pruned_rnnt_loss_from_logits(x, tl, ts, txn, tyn, blank=shape[4])
    with pytest.raises(RuntimeError, match="status 5"):         # S > U
        pruned_rnnt_loss_from_logits(x, tl[:, :1].contiguous(), ts, txn, tyn.clamp(max=1), blank=blank)


def test_forward_and_backward_replay_from_a_graph():
    from warp_rnnt_amd.pruned import pruned_rnnt_loss_from_logits
    shape, blank = (3, 30, 12, 4, 50), 25
    _, labels, starts, xn, yn = case(shape, blank)
    tl, ts, txn, tyn = dev(labels), dev(starts), dev(xn), dev(yn)
    batches = [dev(case(shape, blank, seed=s)[0]) for s in (1, 2, 3)]

    def step(x):
        loss = pruned_rnnt_loss_from_logits(x, tl, ts, txn, tyn, reduction="sum", blank=blank, fastemit_lambda=0.01)
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
        assert torch.isfinite(loss).all()
        assert torch.equal(loss, want[k][0]), f"replay {rep}"
        assert torch.equal(x.grad, want[k][1]), f"replay {rep}"


def test_the_three_step_recipe_end_to_end():
    """simple_pairs -> rnnt_loss(blank=-1) -> prune_ranges -> prune_joint_inputs -> a torch joiner -> the pruned loss.
    The band drops paths, so the pruned cost is not below the full lattice's (minus the cost bar); with S = U it is the
    full lattice."""
    import warp_rnnt
    from warp_rnnt_amd.fused import rnnt_loss_from_logits
    from warp_rnnt_amd.pruned import prune_joint_inputs, prune_ranges, pruned_rnnt_loss_from_logits, simple_pairs
    N, T, U, S, V, H = 2, 40, 12, 4, 17, 32
    gen = torch.Generator().manual_seed(12)
    f = (torch.randn(N, T, H, generator=gen) * 0.7).to(DEV)
    g = (torch.randn(N, U, H, generator=gen) * 0.7).to(DEV)
    am_w, lm_w = (torch.randn(H, V, generator=gen) / H ** 0.5).to(DEV), (torch.randn(H, V, generator=gen) / H ** 0.5).to(DEV)
    w = (torch.randn(H, V, generator=gen) / H ** 0.5).to(DEV)
    labels = torch.randint(1, V, (N, U - 1), generator=gen, dtype=torch.int32).to(DEV)
    xn, yn = torch.tensor([T, T - 7], dtype=torch.int32, device=DEV), torch.tensor([U - 1, U - 4], dtype=torch.int32, device=DEV)

    def joiner(fp, gp):
        return torch.tanh(fp + gp) @ w

    pairs = simple_pairs(f @ am_w, g @ lm_w, labels).requires_grad_(True)
    simple = warp_rnnt.rnnt_loss(pairs.contiguous(), labels, xn, yn, blank=-1, reduction="sum")
    (pair_grads,) = torch.autograd.grad(simple, pairs)
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
        print(f"S = {s_range}: pruned {costs.tolist()} full lattice {full.tolist()} (cost bar {COST_BAR:.3e})")
        assert torch.isfinite(costs).all() and torch.isfinite(fp.grad).all() and (fp.grad != 0).any()
        assert (costs >= full - COST_BAR * full.abs()).all()
        if s_range == U:
            assert (starts == 0).all()
            assert ((costs - full).abs() <= COST_BAR * full.abs()).all()
