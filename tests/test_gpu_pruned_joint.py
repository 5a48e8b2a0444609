"""The joint network fused into the pruned loss: pruned_rnnt_loss_from_joint (csrc/pruned_joint.hip).

Costs and the four gradients against the fp64 reference of tests/pruned_joint_reference.py at the smallest shapes at which
the kernels can go wrong.  The yardstick is the library's own unfused chain -- prune_joint_inputs, a torch joint (under
autocast for half inputs), pruned_rnnt_loss_from_logits -- against the same reference on the same grid: both round the same
quantities and differ in summation order, so the bars are four times the chain's largest figure per quantity and dtype
(tools/pruned_joint_values.py measures, profiles/pruned_joint_values.txt holds every figure)."""
import functools

import numpy as np
import pytest
import torch

from pruned_joint_reference import nrel, pruned_joint_reference
from pruned_reference import make_band_case, upstream

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EDGE = (4, 9, 6, 5, 17, 64, "tanh", 5)
CASES = [  # N, T, U (lattice columns: labels are (N,U-1)), S, V, H, activation, blank
    (3, 6, 4, 1, 2, 32, "tanh", 0),          # S = 1, the minimum V
    (2, 6, 4, 4, 16, 32, "relu", 3),         # S = U: the band is the lattice; V ends a 16-row block
    (2, 13, 9, 5, 17, 64, "tanh", 0),        # 12 frames per tile: the second tile holds one; V = 17
    EDGE,                                    # a tile larger than the utterance; the edge utterances (make)
    (2, 5, 7, 5, 33, 96, "relu", 32),        # V = 33: the half chunk, the W^T pitch; the blank in a block of its own
    (2, 6, 5, 3, 1025, 320, "tanh", 0),      # V = 1025, blank first; H not a multiple of the dW column tile
    (2, 6, 5, 3, 1025, 320, "tanh", 1024),   # ... blank last
    (2, 4, 4, 3, 37, 1024, "relu", 1),       # H = 1024: 16 rows per chunk in fp32, 32 in half precision
    (2, 5, 40, 36, 9, 544, "tanh", 2),       # S above a chunk's rows (16 in fp32, 32 in half): a frame in three / two chunks
    (2, 70, 63, 5, 7, 32, "relu", 0),        # 700 rows: several row chunks per dW split, many tiles
]
HALF_CASES = CASES[:6] + CASES[7:9]        # ... and the reduced tile of H > 512
LAMS = (0.0, 0.01)
QUANTITIES = ("cost", "df", "dg", "dW", "db")
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
# The unfused chain's largest error against fp64 over the dtype's cases x LAMS, measured on an MI355X
# (profiles/pruned_joint_values.txt): cost relative to the fp64 cost, gradients normwise; each with the case it was reached at.
YARDSTICK = {
    "fp32": {
        "cost": 1.101e-07,   # at N2_T13_U9_S5_V17_H64_tanh_b0, lambda 0.00; the fused entry's largest: 9.335e-08
        "df": 1.367e-05,   # at N2_T70_U63_S5_V7_H32_relu_b0, lambda 0.00; the fused entry's largest: 1.531e-05
        "dg": 1.373e-05,   # at N2_T70_U63_S5_V7_H32_relu_b0, lambda 0.00; the fused entry's largest: 1.565e-05
        "dW": 5.769e-06,   # at N2_T5_U40_S36_V9_H544_tanh_b2, lambda 0.01; the fused entry's largest: 5.936e-06
        "db": 5.603e-06,   # at N2_T5_U40_S36_V9_H544_tanh_b2, lambda 0.00; the fused entry's largest: 3.621e-06
    },
    "bf16": {
        "cost": 1.172e-03,   # at N3_T6_U4_S1_V2_H32_tanh_b0, lambda 0.00; the fused entry's largest: 1.577e-07
        "df": 4.026e-03,   # at N2_T5_U40_S36_V9_H544_tanh_b2, lambda 0.01; the fused entry's largest: 2.311e-03
        "dg": 4.145e-03,   # at N2_T13_U9_S5_V17_H64_tanh_b0, lambda 0.01; the fused entry's largest: 2.467e-03
        "dW": 3.102e-03,   # at N2_T5_U40_S36_V9_H544_tanh_b2, lambda 0.01; the fused entry's largest: 2.046e-04
        "db": 2.666e-03,   # at N2_T13_U9_S5_V17_H64_tanh_b0, lambda 0.01; the fused entry's largest: 5.790e-06
    },
    "fp16": {
        "cost": 1.485e-04,   # at N3_T6_U4_S1_V2_H32_tanh_b0, lambda 0.00; the fused entry's largest: 2.331e-07
        "df": 5.699e-04,   # at N2_T5_U40_S36_V9_H544_tanh_b2, lambda 0.01; the fused entry's largest: 2.962e-04
        "dg": 4.742e-04,   # at N2_T5_U40_S36_V9_H544_tanh_b2, lambda 0.00; the fused entry's largest: 2.790e-04
        "dW": 4.335e-04,   # at N2_T5_U40_S36_V9_H544_tanh_b2, lambda 0.00; the fused entry's largest: 7.347e-05
        "db": 4.453e-04,   # at N2_T5_U40_S36_V9_H544_tanh_b2, lambda 0.00; the fused entry's largest: 9.400e-06
    },
}


def bars(name):
    return {q: 4 * YARDSTICK[name][q] for q in QUANTITIES}


def case_id(c):
    return f"N{c[0]}_T{c[1]}_U{c[2]}_S{c[3]}_V{c[4]}_H{c[5]}_{c[6]}_b{c[7]}"


def make(case, dtype=torch.float32, dyadic=False):
    """f (N,T,H), g (N,U,H) in ``dtype``, fp32 weight (V,H) and bias (V,), labels (N,U-1) never blank, starts (N,T) of a
    band that holds a path, ragged lengths.  EDGE's batch: utterance 0 has non-monotone starts and rows mapped below 0 and
    beyond U; 1 has one frame, 2 no labels, 3 a band without a path (cell (0,0) is outside it).  dyadic: small dyadic
    values whose logits are exact in fp32 in any summation order (tests/joint_values.py has the argument; relu, H <= 128)."""
    N, T, U, S, V, H, act, blank = case
    lengths = ([T, 1, T - 2, T], [U - 1, 0, 0, U - 2]) if case == EDGE else None
    _, labels, starts, xn, yn = make_band_case(1000 * V + 10 * H + T, N, T, U, S, V, blank, lengths=lengths)
    if case == EDGE:
        starts[0, 0], starts[0, 3], starts[0, 4] = -1, starts[0, 4], starts[0, 3] - 1
        starts[0, T - 1] = U - 2
        starts[3, 0] = 2
    gen = torch.Generator().manual_seed(1000 * V + 10 * H + T)
    if dyadic:
        assert act == "relu" and H <= 128
        ints = lambda lo, hi, shape: torch.randint(lo, hi + 1, shape, generator=gen).to(torch.float32)  # noqa: E731
        f, g = ints(-8, 8, (N, T, H)) / 4, ints(-8, 8, (N, U, H)) / 4
        w, b = ints(-8, 8, (V, H)) / 16, ints(-16, 16, (V,)) / 8
    else:
        f, g = torch.randn(N, T, H, generator=gen) * 0.5, torch.randn(N, U, H, generator=gen) * 0.5
        w, b = torch.randn(V, H, generator=gen) / H ** 0.5, torch.randn(V, generator=gen) * 0.1
    return (f.to(dtype), g.to(dtype), w, b, torch.from_numpy(labels), torch.from_numpy(starts), torch.from_numpy(xn),
            torch.from_numpy(yn))


@functools.lru_cache(maxsize=None)
def reference(case, lam=0.0, dtype=torch.float32, go=None):
    """The fp64 reference of the case, computed once and shared.  Half inputs: it sees the rounded f and g."""
    f, g, w, b, labels, starts, xn, yn = make(case, dtype)
    return pruned_joint_reference(f, g, w, b, labels, starts, case[3], xn, yn, case[6], case[7], lam,
                                  None if go is None else np.array(go))


def run(loss_of, case, inputs, go=None):
    f, g, w, b, labels, starts, xn, yn = inputs
    leaves = [x.detach().to(DEV).requires_grad_(True) for x in (f, g, w, b)]
    out = loss_of(leaves, labels.to(DEV), starts.to(DEV), xn.to(DEV), yn.to(DEV))
    up = torch.from_numpy(upstream(case[0])).float() if go is None else go
    finite = torch.isfinite(out)                      # (an infinite cost's weight would make the sum's gradient NaN-free anyway)
    (torch.where(finite, out, torch.zeros_like(out)) * up.to(DEV)).sum().backward()
    return (out.detach(),) + tuple(x.grad for x in leaves)


def fused(case, inputs, lam=0.0, go=None):
    from warp_rnnt_amd.pruned import pruned_rnnt_loss_from_joint
    return run(lambda p, labels, starts, xn, yn: pruned_rnnt_loss_from_joint(
        *p, labels, starts, xn, yn, activation=case[6], blank=case[7], fastemit_lambda=lam, s_range=case[3]), case, inputs, go)


def chain(case, inputs, lam=0.0, autocast_dtype=None):
    """The unfused path: prune_joint_inputs -> the joint in torch (under autocast for half inputs) -> the logits entry."""
    from warp_rnnt_amd.pruned import prune_joint_inputs, pruned_rnnt_loss_from_logits
    act = torch.tanh if case[6] == "tanh" else torch.relu

    def loss_of(p, labels, starts, xn, yn):
        fp, gp = prune_joint_inputs(p[0], p[1], starts, case[3])
        with torch.autocast("cuda", dtype=autocast_dtype or torch.bfloat16, enabled=autocast_dtype is not None):
            z = torch.nn.functional.linear(act(fp + gp), p[2], p[3])
        return pruned_rnnt_loss_from_logits(z.contiguous(), labels, starts, xn, yn, blank=case[7], fastemit_lambda=lam)

    return run(loss_of, case, inputs)


def errors(result, ref):
    """The five figures of a result against the reference's; the infinite costs must be the reference's."""
    got, want = result[0].double().cpu(), ref[0]
    assert torch.equal(torch.isinf(got), torch.isinf(want)), (got, want)
    ok = torch.isfinite(want)
    out = {"cost": float(((got[ok] - want[ok]).abs() / want[ok].abs()).max())}
    for q, x, r in zip(QUANTITIES[1:], result[1:], ref[1:]):
        assert torch.isfinite(x).all(), q
        out[q] = nrel(x, r)
    return out


# ---- 1. against fp64, the chain as the yardstick ----

@pytest.mark.parametrize("name,case", [("fp32", c) for c in CASES] + [(d, c) for d in ("bf16", "fp16") for c in HALF_CASES],
                         ids=lambda x: x if isinstance(x, str) else case_id(x))
def test_against_fp64_within_four_times_the_chain(name, case):
    dtype = DTYPES[name]
    inputs = make(case, dtype)
    worst = dict.fromkeys(QUANTITIES, 0.0)
    for lam in LAMS:
        got = fused(case, inputs, lam)
        e = errors(got, reference(case, lam, dtype))
        print(case_id(case), name, f"lambda {lam}:", " ".join(f"{q} {e[q]:.3e}" for q in QUANTITIES))
        worst = {q: max(worst[q], e[q]) for q in QUANTITIES}
        assert got[1].dtype == dtype and got[2].dtype == dtype and got[3].dtype == torch.float32
        if case == EDGE:                      # the band without a path: +inf, exactly zero gradient rows
            assert torch.isinf(got[0][3]) and got[0][3] > 0
            assert torch.count_nonzero(got[1][3]) == 0 and torch.count_nonzero(got[2][3]) == 0
    for q in QUANTITIES:
        assert worst[q] <= bars(name)[q], (q, worst[q], bars(name)[q])


# ---- 2. exactness on dyadic inputs ----

@pytest.mark.parametrize("case", [CASES[1], (2, 13, 9, 5, 17, 64, "relu", 0)], ids=case_id)
def test_dyadic_rows_carry_the_chains_bits(case):
    """Every logit is exact in fp32 in any summation order.  (a) The row maximum the producer stores is the chain's logits'
    maximum, bit for bit, in every live row.  (b) With biases 2048 apart every exponential but the maximum's is exactly 0,
    so every sum the log-softmax forms is exact too: the pairs, and with them the costs and the gradient pairs of the whole
    lattice, are the chain's bit for bit."""
    from warp_rnnt_amd import ops
    from warp_rnnt_amd.pruned import prune_joint_inputs
    N, T, U, S, V, H, act, blank = case
    f, g, w, b, labels, starts, xn, yn = (x.to(DEV) for x in make(case, dyadic=True))
    fp, gp = prune_joint_inputs(f, g, starts, S)
    u = starts[..., None] + torch.arange(S, device=DEV)
    live = (torch.arange(T, device=DEV)[None, :, None] < xn[:, None, None]) & (u >= 0) & (u <= yn[:, None, None])
    for bias in (b, -2048.0 * ((torch.arange(V, device=DEV) + V - blank) % V).float()):
        z = torch.nn.functional.linear(torch.relu(fp + gp), w, bias).contiguous()
        costs, stats, grads = ops.pruned_joint_loss(f, g, w, bias, labels, starts, S, xn, yn, act, blank, 0.0, True)
        assert torch.equal(stats[..., 0][live], z.max(-1).values[live])
    c_costs, c_grads = ops.pruned_loss(z, labels, starts, xn, yn, blank, 0.0, True)
    assert torch.equal(stats[..., 1][live], torch.zeros_like(stats[..., 1][live]))
    assert torch.equal(costs, c_costs) and torch.equal(grads, c_grads)


# ---- 3. bit contracts ----

@pytest.mark.parametrize("name", ["fp32", "bf16"])
def test_bits_run_to_run_and_batch_independence(name):
    case = EDGE
    inputs = make(case, DTYPES[name])
    ones = torch.ones(case[0])
    a, a2 = fused(case, inputs, 0.01, ones), fused(case, inputs, 0.01, ones)
    for x, y in zip(a, a2):
        assert torch.equal(x, y)
    without = fused(case, tuple(x[:3] if x.shape[0] == 4 else x for x in inputs), 0.01, ones[:3])   # no utterance 3
    for k in range(3):
        assert torch.equal(without[k], a[k][:3]), k
    f, g, w, b, labels, starts, xn, yn = inputs
    for n in range(3):
        tn, un = int(xn[n]), int(yn[n]) + 1
        alone = fused(case, (f[n:n + 1], g[n:n + 1], w, b, labels[n:n + 1], starts[n:n + 1], xn[n:n + 1], yn[n:n + 1]),
                      0.01, torch.ones(1))
        assert torch.equal(alone[0][0], a[0][n])
        assert torch.equal(alone[1][0], a[1][n]) and torch.equal(alone[2][0], a[2][n])
        assert torch.count_nonzero(a[1][n, tn:]) == 0 and torch.count_nonzero(a[2][n, un:]) == 0


def test_graph_replays_with_fresh_inputs():
    from warp_rnnt_amd.pruned import pruned_rnnt_loss_from_joint
    case = CASES[2]
    f, g, w, b, labels, starts, xn, yn = make(case)
    fd, gd, wd, bd = (x.to(DEV).requires_grad_(True) for x in (f, g, w, b))
    rest = [x.to(DEV) for x in (labels, starts, xn, yn)]
    kw = dict(activation=case[6], blank=case[7], fastemit_lambda=0.01, s_range=case[3])

    def step():
        for p in (fd, gd, wd, bd):
            p.grad = None
        pruned_rnnt_loss_from_joint(fd, gd, wd, bd, *rest, **kw).sum().backward()
        return [p.grad.clone() for p in (fd, gd, wd, bd)]

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()                                          # warm-up on the side stream
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    for p in (fd, gd, wd, bd):
        p.grad = None
    with torch.cuda.graph(graph):
        pruned_rnnt_loss_from_joint(fd, gd, wd, bd, *rest, **kw).sum().backward()
    static = [p.grad for p in (fd, gd, wd, bd)]         # (what the replays write; step() below rebinds .grad)
    for scale in (1.0, 0.5, 2.0):                       # fresh inputs in place, several replays against eager
        with torch.no_grad():
            fd.copy_(f.to(DEV) * scale)
        graph.replay()
        torch.cuda.synchronize()
        replayed = [x.clone() for x in static]
        for x, y in zip(replayed, step()):
            assert torch.equal(x, y), scale


# ---- 4. the module, the reductions, the refusals ----

@pytest.mark.parametrize("reduction", ["none", "sum", "mean"])
def test_module_and_reductions_are_the_function(reduction):
    from warp_rnnt_amd.pruned import PrunedJointLoss, pruned_rnnt_loss_from_joint
    case = CASES[2]
    N, T, U, S, V, H, act, blank = case
    f, g, w, b, labels, starts, xn, yn = (x.to(DEV) for x in make(case))
    module = PrunedJointLoss(H, V, activation=act, blank=blank, fastemit_lambda=0.01, reduction=reduction).to(DEV)
    with torch.no_grad():
        module.weight.copy_(w)
        module.bias.copy_(b)
    ranges = starts[..., None] + torch.arange(S, device=DEV)                     # k2's (N,T,S) form
    plain = pruned_rnnt_loss_from_joint(f, g, w, b, labels, starts, xn, yn, act, blank, 0.01, s_range=S)
    want = plain if reduction == "none" else (plain.sum() if reduction == "sum" else plain.mean())
    out = module(f, g, labels, ranges, xn, yn)
    torch.testing.assert_close(out, want, rtol=1e-6, atol=0)
    averaged = pruned_rnnt_loss_from_joint(f, g, w, b, labels, ranges, xn, yn, act, blank, 0.01, True, "none")
    torch.testing.assert_close(averaged, plain / xn, rtol=1e-6, atol=0)
    out.sum().backward()
    assert torch.isfinite(module.weight.grad).all() and torch.isfinite(module.bias.grad).all()


def test_refusals_come_before_any_launch():
    from warp_rnnt_amd import _lib
    from warp_rnnt_amd.pruned import pruned_rnnt_loss_from_joint
    f, g, w, b, labels, starts, xn, yn = (x.to(DEV) for x in make(CASES[2]))
    with pytest.raises(ValueError, match="regular"):
        pruned_rnnt_loss_from_joint(f, g, w, b, labels, starts, xn, yn, s_range=5, rnnt_type="modified")
    with pytest.raises(RuntimeError, match="status 5"):
        pruned_rnnt_loss_from_joint(f[..., :48], g[..., :48], w[:, :48], b, labels, starts, xn, yn, s_range=5)
    L = _lib.load()
    N, T, U, S, V, H = CASES[2][:6]
    ws = torch.empty(L.rnnt_amd_pruned_joint_workspace_size(0, N, T, U, S, H, V), dtype=torch.uint8, device=DEV)
    costs = torch.full((N,), 7.0, device=DEV)
    odd = torch.zeros(f.numel() + 1, device=DEV)[1:]                             # 4 bytes off a 16-byte boundary
    status = L.rnnt_amd_pruned_joint_loss(None, ws.data_ptr(), 0, 0, odd.data_ptr(), g.data_ptr(), w.data_ptr(),
                                          b.data_ptr(), labels.data_ptr(), starts.data_ptr(), xn.data_ptr(), yn.data_ptr(),
                                          costs.data_ptr(), None, None, N, T, U, S, H, V, 0, 0.0)
    torch.cuda.synchronize()
    assert status == 5 and bool((costs == 7.0).all())


# ---- 5. the memory contract ----

def test_memory_stays_under_the_headers_formula_and_the_logits():
    from warp_rnnt_amd import _lib
    from warp_rnnt_amd.pruned import pruned_rnnt_loss_from_joint
    N, T, U, S, V, H = 4, 300, 60, 5, 1025, 256
    torch.manual_seed(0)
    f = (torch.randn(N, T, H, device=DEV) * 0.5).to(torch.bfloat16).requires_grad_(True)
    g = (torch.randn(N, U, H, device=DEV) * 0.5).to(torch.bfloat16).requires_grad_(True)
    w = (torch.randn(V, H, device=DEV) / H ** 0.5).requires_grad_(True)           # an fp32 master weight
    b = torch.zeros(V, device=DEV, requires_grad=True)
    labels = torch.randint(1, V, (N, U - 1), dtype=torch.int32, device=DEV)
    xn = torch.full((N,), T, dtype=torch.int32, device=DEV)
    yn = torch.full((N,), U - 1, dtype=torch.int32, device=DEV)
    starts = (torch.arange(T, device=DEV) * (U - S) // (T - 1)).to(torch.int32).repeat(N, 1).contiguous()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    c = pruned_rnnt_loss_from_joint(f, g, w, b, labels, starts, xn, yn, s_range=S)
    c.sum().backward()
    torch.cuda.synchronize()
    returned = sum(x.grad.numel() * x.grad.element_size() for x in (f, g, w, b))
    extra = torch.cuda.max_memory_allocated() - before - returned
    # the header's count with its two Python terms: the bf16 copy of the master weight, 64 KiB for the (N,) vectors and
    # the allocator's granules
    bound = (_lib.load().rnnt_amd_pruned_joint_workspace_size(1, N, T, U, S, H, V) + 8 * N * T * S + 8 * N * T * U +
             2 * V * H + (64 << 10))
    logits_bytes = N * T * S * V * 2
    print(f"peak extra {extra} B; the header's count {bound} B; the bf16 logits {logits_bytes} B")
    assert torch.isfinite(c).all()
    assert extra < bound < logits_bytes, (extra, bound, logits_bytes)
