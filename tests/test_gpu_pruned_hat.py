"""The factorised-blank (HAT) loss on the pruned band on the GPU: pruned_rnnt_loss_from_logits(..., use_hat_loss=True),
csrc/pruned_hat.hip, against fp64 (tests/pruned_hat_reference.py) and bit for bit against the dense HAT loss.  The bars are
not taken from the code under test: four times the largest error the SOFTMAX pruned loss -- the same call without the
keyword -- shows against its own fp64 reference on the same cases (tools/pruned_hat_values.py measured both:
profiles/pruned_hat_loss_values.txt).  Every figure is printed before it is asserted (pytest -s)."""
import functools

import numpy as np
import pytest
import torch

import modified_reference as mr
import pruned_hat_reference as phr
import pruned_reference as pr
from test_gpu_modified import cost_error, dev, grad_error, modified_starts, pruned_run

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -24
HALF = {"bf16": torch.bfloat16, "f16": torch.float16}
# (N, T, U, S, V); the first: an utterance of one frame and one without labels
SHAPES = [(3, 12, 6, 2, 2), (2, 9, 5, 1, 3), (3, 30, 12, 4, 50), (2, 21, 9, 5, 129), (2, 15, 9, 3, 257), (2, 9, 5, 3, 1024),
          (2, 9, 5, 3, 1025)]
AXES = [(lam, dp, rnnt_type) for lam in (0.0, 0.01) for dp in (0.0, 0.1) for rnnt_type in ("regular", "modified")]
CASES = [(s, b) for s in SHAPES for b in ((0, 1) if s[4] == 2 else (0, s[4] // 2, s[4] - 1))]
IDS = ["N%d-T%d-U%d-S%d-V%d-b%d" % (*s, b) for s, b in CASES]

# profiles/pruned_hat_loss_values.txt, over CASES x AXES: largest |cost - fp64| / |fp64| and |d/d logits - fp64|
YARDSTICK_COST_REL = 5.820e-07   # (the softmax pruned loss) at (3, 12, 6, 2, 2), blank 1, lambda 0.01, dp 0.1, modified
YARDSTICK_GRAD_ABS = 2.250e-05   # at (3, 30, 12, 4, 50), blank 25, lambda 0.01, dp 0.0, regular
HAT_COST_REL = 2.766e-07         # (use_hat_loss=True) at (3, 30, 12, 4, 50), blank 25, lambda 0.01, dp 0.1, regular
HAT_GRAD_ABS = 9.609e-06         # at (3, 30, 12, 4, 50), blank 25, lambda 0.01, dp 0.1, regular
COST_BAR = max(4 * YARDSTICK_COST_REL, 4 * EPS)      # relative to the fp64 cost
GRAD_BAR = 4 * YARDSTICK_GRAD_ABS                    # absolute


@functools.lru_cache(maxsize=None)
def case(shape, blank, seed=0):
    """Host inputs: logits, labels, {topology: (starts, xn, yn)} -- ragged lengths with T_n >= U_n; the regular band by
    make_band_case (it shortens the labels until its band can climb them), the modified one by modified_starts."""
    N, T, U, S, V = shape
    s = 9000 * V + 10 * T + S + blank + seed
    rng = np.random.RandomState(s + 1)
    xn = np.array([T] + list(rng.randint(U, T + 1, size=N - 1)), np.int32)
    yn = np.array([U - 1] + list(rng.randint(U // 2, U, size=N - 1)), np.int32)
    if shape == SHAPES[0]:
        xn[1:], yn[1:] = (1, T // 2), (1, 0)
    logits, labels, rstarts, rxn, ryn = pr.make_band_case(s, N, T, U, S, V, blank=blank, lengths=(xn, yn))
    mstarts = np.zeros((N, T), np.int32) if S == U else modified_starts(np.random.RandomState(s + 2), T, U, S, xn, yn)
    return logits, labels, {"regular": (rstarts, rxn, ryn), "modified": (mstarts, xn, yn)}


def tensors(shape, blank, rnnt_type, seed=0):
    logits, labels, bands = case(shape, blank, seed)
    return [dev(a) for a in (logits, labels) + bands[rnnt_type]] + [dev(pr.upstream(shape[0]).astype(np.float32))]


def run(x, tl, ts, txn, tyn, go, blank, lam=0.01, dp=0.1, rnnt_type="regular", hat=True, grad=True):
    return pruned_run(x, tl, ts, txn, tyn, blank, lam, go, grad, rnnt_type=rnnt_type, delay_penalty=dp, use_hat_loss=hat)


def errors(shape, blank, lam, dp, rnnt_type, hat):
    """(cost rel, d/d logits abs) of one case against fp64; hat=False: the yardstick."""
    logits, labels, bands = case(shape, blank)
    ref = (phr.pruned_hat64 if hat else mr.pruned64)(logits, labels, *bands[rnnt_type], blank, lam, dp, rnnt_type)
    costs, grad = run(*tensors(shape, blank, rnnt_type), blank, lam, dp, rnnt_type, hat)
    return cost_error(costs, ref["costs"]), grad_error(grad, ref["dlogits"])


@pytest.mark.parametrize("shape,blank", CASES, ids=IDS)
def test_costs_and_gradients_against_fp64(shape, blank):
    for lam, dp, rnnt_type in AXES:
        cost, grad = errors(shape, blank, lam, dp, rnnt_type, True)
        print(f"{shape} blank {blank} lam {lam} dp {dp} {rnnt_type}: cost rel {cost:.3e} (bar {COST_BAR:.3e})  "
              f"grad abs {grad:.3e} (bar {GRAD_BAR:.3e})")
        assert cost <= COST_BAR and grad <= GRAD_BAR, (shape, blank, lam, dp, rnnt_type)


@pytest.mark.parametrize("V", [50, 129, 1025])
def test_the_full_band_is_the_dense_hat_loss_bit_for_bit(V):
    from warp_rnnt_amd.hat import hat_loss_from_logits
    shape, blank = (3, 11, 6, 6, V), V // 3
    x, tl, _, txn, tyn, go = tensors(shape, blank, "modified")            # (S == U: zero starts; ragged lengths)
    costs, grad = run(x, tl, torch.zeros(shape[:2], dtype=torch.int32, device=x.device), txn, tyn, go, blank, dp=0.0)
    xd = x.clone().requires_grad_(True)
    dense = hat_loss_from_logits(xd, tl, txn, tyn, blank=blank, fastemit_lambda=0.01)
    (dense * go).sum().backward()
    assert (txn < shape[1]).any() and torch.isfinite(costs).all() and (grad != 0).any()
    assert torch.equal(costs, dense.detach()) and torch.equal(grad, xd.grad)


@pytest.mark.parametrize("rnnt_type", ["regular", "modified"])
@pytest.mark.parametrize("dname", list(HALF))
@pytest.mark.parametrize("V", [50, 65, 256, 1025])
def test_half_precision_gives_the_bits_of_its_upcast_and_bits_depend_on_the_utterance_alone(V, dname, rnnt_type):
    shape, blank = (2, 15, 9, 3, V), V // 2
    x, tl, ts, txn, tyn, go = tensors(shape, blank, rnnt_type)
    xh = x.to(HALF[dname])
    (ch, gh), (cf, gf) = run(xh, tl, ts, txn, tyn, go, blank, rnnt_type=rnnt_type), run(xh.float(), tl, ts, txn, tyn, go, blank,
                                                                                      rnnt_type=rnnt_type)
    assert gh.dtype == HALF[dname] and torch.isfinite(ch).all() and (gh != 0).any()
    assert torch.equal(ch, cf) and torch.equal(gh, gf.to(HALF[dname]))          # the fp32 result rounded once
    assert torch.equal(run(xh, tl, ts, txn, tyn, go, blank, rnnt_type=rnnt_type, grad=False)[0], ch)
    for n in range(shape[0]):
        c1, g1 = run(*[a[n:n + 1].contiguous() for a in (xh, tl, ts, txn, tyn, go)], blank, rnnt_type=rnnt_type)
        assert torch.equal(c1, ch[n:n + 1]) and torch.equal(g1[0], gh[n]), n


@pytest.mark.parametrize("V", [7, 257, 1030])
def test_dead_rows_regular(V):
    """Rows that starts put outside [0,U) hold NaN: exactly zero gradient rows, the others inside the bars.  A band without
    a path: +inf, zero rows, the neighbours' bits untouched."""
    N, T, U, S, blank = 3, 9, 5, 3, 1
    logits, labels, _, xn, yn = pr.make_band_case(V, N, T, U, S, V, blank=blank, ragged=False)
    starts = np.tile(np.array([0, 0, 0, 1, 1, 1, 2, 2, 2], np.int32), (N, 1))
    starts[0] = [-1, 0, 0, 1, 1, 1, 2, 3, 3]
    outside = np.zeros((N, T, S), bool)
    outside[0, 0, 0] = outside[0, 7, S - 1] = outside[0, 8, S - 1] = True
    ref = phr.pruned_hat64(logits, labels, starts, xn, yn, blank, 0.01)
    logits = logits.copy()
    logits[outside] = np.nan
    args = [dev(a) for a in (labels, starts, xn, yn, pr.upstream(N).astype(np.float32))]
    costs, grad = run(dev(logits), *args, blank, dp=0.0)
    cost, err = cost_error(costs, ref["costs"]), grad_error(grad, ref["dlogits"])
    print(f"V {V}: rows outside the grid: cost rel {cost:.3e} (bar {COST_BAR:.3e}) grad abs {err:.3e} (bar {GRAD_BAR:.3e})")
    mask = torch.tensor(outside, device=grad.device)
    assert cost <= COST_BAR and err <= GRAD_BAR and (grad[mask] == 0).all() and (grad[~mask] != 0).any(dim=-1).all()
    args[1] = args[1].clone()
    args[1][1, 0] = 1                                     # utterance 1: the first band begins behind (0,0)
    c2, g2 = run(dev(logits), *args, blank, dp=0.0)
    assert torch.isinf(c2[1]) and c2[1] > 0 and (g2[1] == 0).all()
    assert torch.equal(c2[[0, 2]], costs[[0, 2]]) and torch.equal(g2[[0, 2]], grad[[0, 2]])


def test_dead_rows_modified():
    """Padding frames repeat U_n + 1 - S: the band of frame T_n covers column U_n, the terminal cell's address -- NaN there
    moves no bit and gets zero rows.  T_n < U_n: +inf and zero rows."""
    N, T, U, S, V, blank = 3, 12, 6, 3, 9, 4
    lengths = (np.array([12, 7, 3], np.int32), np.array([5, 3, 5], np.int32))
    logits, labels, _, _, _ = pr.make_band_case(3, N, T, U, S, V, blank=blank, lengths=lengths)
    starts = modified_starts(np.random.RandomState(4), T, U, S, *lengths)
    assert starts[1, 7] <= 3 < starts[1, 7] + S           # the trap is set: (T_n, U_n) is a row of the logits
    bad = logits.copy()
    bad[1, 7:] = bad[2, 3:] = np.nan
    args = [dev(a) for a in (labels, starts) + lengths + (pr.upstream(N).astype(np.float32),)]
    (costs, grad), (c2, g2) = run(dev(logits), *args, blank, rnnt_type="modified"), run(dev(bad), *args, blank, rnnt_type="modified")
    ref = phr.pruned_hat64(logits, labels, starts, *lengths, blank, 0.01, 0.1, "modified")
    assert cost_error(costs, ref["costs"]) <= COST_BAR and grad_error(grad, ref["dlogits"]) <= GRAD_BAR
    assert torch.equal(costs, c2) and torch.equal(grad, g2) and torch.isinf(costs[2]) and torch.isfinite(costs[:2]).all()
    assert (grad[1, 7:] == 0).all() and (grad[2] == 0).all() and (grad[1, :7] != 0).any()


@pytest.mark.parametrize("zb", [-90.0, 90.0])
def test_a_saturated_blank_logit_and_a_shift_of_the_others(zb):
    shape, blank = (2, 9, 5, 3, 50), 7
    logits, labels, bands = case(shape, blank)
    logits = np.round(logits * 64) / 64                   # (a grid on which the shift below is exact)
    logits[..., blank] = zb
    ref = phr.pruned_hat64(logits, labels, *bands["regular"], blank, 0.01, 0.1)
    args = tensors(shape, blank, "regular")[1:]
    costs, grad = run(dev(logits), *args, blank)
    cost, err = cost_error(costs, ref["costs"]), grad_error(grad, ref["dlogits"])
    print(f"z_b {zb}: cost rel {cost:.3e} (bar {COST_BAR:.3e}) grad abs {err:.3e} (bar {GRAD_BAR:.3e})")
    assert torch.isfinite(costs).all() and cost <= COST_BAR and err <= GRAD_BAR
    shifted = logits + 16.0
    shifted[..., blank] = zb
    assert ((shifted - 16.0 == logits) | (np.arange(shape[4]) == blank)).all()
    c2, g2 = run(dev(shifted.astype(np.float32)), *args, blank)
    assert torch.equal(c2, costs) and torch.equal(g2, grad)


def test_forward_and_backward_replay_from_a_graph():
    from warp_rnnt_amd.pruned import pruned_rnnt_loss_from_logits
    shape, blank = (2, 21, 9, 5, 129), 64
    _, tl, ts, txn, tyn, _ = tensors(shape, blank, "modified")
    batches = [tensors(shape, blank, "modified", seed)[0] for seed in (1, 2, 3)]

    def step(x):
        loss = pruned_rnnt_loss_from_logits(x, tl, ts, txn, tyn, reduction="sum", blank=blank, fastemit_lambda=0.01,
                                            rnnt_type="modified", delay_penalty=0.1, use_hat_loss=True)
        loss.backward()
        return loss

    want = []
    for x in (b.clone().requires_grad_(True) for b in batches):
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
    for rep in (1, 2, 1, 0):                              # replayed with new inputs, and again
        with torch.no_grad():
            x.copy_(batches[rep])
        graph.replay()
        torch.cuda.synchronize()
        assert torch.isfinite(loss).all() and (x.grad != 0).any()
        assert torch.equal(loss, want[rep][0]) and torch.equal(x.grad, want[rep][1]), f"replay of batch {rep}"


@pytest.mark.parametrize("rnnt_type,dp,entry", [("regular", 0.0, "pruned_loss"), ("modified", 0.1, "pruned_loss_topology")])
def test_without_the_keyword_it_is_the_call_of_today_and_the_module_is_the_function(monkeypatch, rnnt_type, dp, entry):
    from warp_rnnt_amd import ops
    from warp_rnnt_amd.pruned import PrunedRNNTLoss
    shape, blank, calls = (2, 15, 9, 3, 65), 32, []
    for name in ("pruned_loss", "pruned_loss_topology", "pruned_hat_loss"):
        monkeypatch.setattr(ops, name, lambda *a, _f=getattr(ops, name), _n=name, **k: (calls.append(_n), _f(*a, **k))[1])
    x, tl, ts, txn, tyn, go = tensors(shape, blank, rnnt_type)
    a = pruned_run(x, tl, ts, txn, tyn, blank, 0.01, go, rnnt_type=rnnt_type, delay_penalty=dp)
    b = run(x, tl, ts, txn, tyn, go, blank, 0.01, dp, rnnt_type, hat=False)
    h = run(x, tl, ts, txn, tyn, go, blank, 0.01, dp, rnnt_type, hat=True)
    assert calls == [entry, entry, "pruned_hat_loss"]
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and not torch.equal(a[0], h[0])
    xm = x.clone().requires_grad_(True)
    module = PrunedRNNTLoss(blank, 0.01, "none", rnnt_type, dp, use_hat_loss=True)(xm, tl, ts, txn, tyn)
    (module * go).sum().backward()
    assert torch.equal(module.detach(), h[0]) and torch.equal(xm.grad, h[1])
