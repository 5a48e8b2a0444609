"""The joint network fused into the TDT loss: tdt_loss_from_joint (csrc/tdt_joint.hip).

Costs and gradients to f, g, weight and bias against the fp64 reference of tests/tdt_joint_reference.py, at the smallest
shapes at which the kernels can go wrong -- where the duration rows sit among the 16-row blocks of W and the four lane
groups, the half-precision 32-row chunk, one wave per workgroup, the skew's wrap, several cell groups per split.  The
yardstick of the fp32 errors is the library's own unfused chain -- a torch fp32 joint, then tdt_loss_from_logits -- against
the same reference on the same grid: both round the same quantities in fp32 and differ in summation order only (MFMA K
order, online against two-pass softmax), so the bars are four times the chain's largest figure per quantity, the margin
tests/test_gpu_tdt.py gives TDT against its yardstick (tools/tdt_joint_values.py measures, profiles/tdt_joint_values.txt
holds every figure)."""
import functools

import pytest
import torch

from tdt_joint_reference import nrel, tdt_joint_reference

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
D5 = (0, 1, 2, 3, 4)
CASES = [  # N, T, U (labels: the lattice has U + 1 columns), V, durations, H, activation, blank
    (4, 7, 4, 2, (0, 1), 32, "tanh", 0),              # minimum V and D; T, U+1 not multiples of 4; the edge utterances
    (2, 6, 3, 11, D5, 64, "relu", 10),                # V+D = 16: durations end one 16-row block; NeMo's blank
    (2, 6, 3, 14, D5, 64, "tanh", 7),                 # durations straddle blocks 0/1 and lane groups 3/0
    (2, 6, 3, 16, D5, 32, "relu", 0),                 # durations start a block
    (2, 5, 3, 12, tuple(range(9)), 64, "tanh", 11),   # D = 9 over three lane groups of two blocks
    (2, 6, 3, 27, D5, 96, "tanh", 13),                # V+D = 32: the half-precision 32-row chunk, the W^T pitch
    (2, 6, 3, 28, D5, 96, "tanh", 13),                # V+D = 33
    (2, 5, 3, 1025, D5, 320, "tanh", 1024),           # Parakeet's head; H not a multiple of the 256-column dW tile
    (2, 4, 3, 37, (0, 1, 8), 1024, "relu", 1),        # H = 1024: one wave per workgroup in fp32; the longest jump
    (2, 3, 6, 7, (2, 0, 1), 32, "tanh", 3),           # U > T (the skew wraps), unsorted durations
    (2, 70, 63, 7, (1, 2), 32, "relu", 0),            # 8960 cells: several cell groups per split; no duration 0
]
HALF_CASES = CASES[:8]
SIGMAS, LAMS = (0.0, 0.05), (0.0, 0.01)
QUANTITIES = ("cost", "df", "dg", "dW", "db")
# The unfused chain's largest error against fp64 over CASES x SIGMAS x LAMS, measured on an MI355X
# (profiles/tdt_joint_values.txt): cost relative to the fp64 cost, gradients normwise.  Each with the case it was reached at.
YARDSTICK = {
    "cost": 1.600e-07,   # at (2, 70, 63, 7, (1, 2), 32, relu), sigma 0.05, lambda 0;    the fused entry's largest: 1.775e-07
    "df": 9.386e-06,     # at (2, 70, 63, 7, (1, 2), 32, relu), sigma 0.05, lambda 0.01; the fused entry's largest: 1.108e-05
    "dg": 8.380e-06,     # at (2, 70, 63, 7, (1, 2), 32, relu), sigma 0.05, lambda 0.01; the fused entry's largest: 1.047e-05
    "dW": 5.362e-06,     # at (2, 70, 63, 7, (1, 2), 32, relu), sigma 0.05, lambda 0.01; the fused entry's largest: 7.668e-06
    "db": 4.818e-06,     # at (2, 70, 63, 7, (1, 2), 32, relu), sigma 0, lambda 0.01;    the fused entry's largest: 6.698e-06
}
BARS = {q: 4 * YARDSTICK[q] for q in QUANTITIES}


def case_id(c):
    return f"N{c[0]}_T{c[1]}_U{c[2]}_V{c[3]}_D{len(c[4])}_H{c[5]}_{c[6]}"


def make(case, dtype=torch.float32, dyadic=False):
    """f (N,T,H), g (N,U+1,H) in ``dtype``, fp32 weight (V+D,H) and bias (V+D,), labels (N,U) int32 (never the blank),
    ragged lengths.  The first case's batch also holds an utterance of one frame, one without labels and one whose
    lengths are out of range.  dyadic: small dyadic values whose logits, and the logits plus a bias of a few thousand, are
    exact in fp32 in any summation order (tests/joint_values.py has the argument; relu, H <= 128)."""
    N, T, U, V, durations, H, act, blank = case
    D = len(durations)
    gen = torch.Generator().manual_seed(1000 * V + 10 * H + T)
    if dyadic:
        assert act == "relu" and H <= 128
        ints = lambda lo, hi, shape: torch.randint(lo, hi + 1, shape, generator=gen).to(torch.float32)  # noqa: E731
        f, g = ints(-8, 8, (N, T, H)) / 4, ints(-8, 8, (N, U + 1, H)) / 4
        w, b = ints(-8, 8, (V + D, H)) / 16, ints(-16, 16, (V + D,)) / 8
    else:
        f = torch.randn(N, T, H, generator=gen) * 0.5
        g = torch.randn(N, U + 1, H, generator=gen) * 0.5
        w = torch.randn(V + D, H, generator=gen) / H ** 0.5
        b = torch.randn(V + D, generator=gen) * 0.1
    labels = ((blank + 1 + torch.randint(0, V - 1, (N, U), generator=gen)) % V).to(torch.int32)
    xn = torch.tensor(([T, max(1, T - 1)] + [T] * (N - 2))[:N], dtype=torch.int32)
    yn = torch.tensor(([U, U - 1] + [U] * (N - 2))[:N], dtype=torch.int32)
    if N == 4:
        xn[1], yn[1] = 1, 0                  # one frame
        xn[2], yn[2] = T - 2, 0              # no labels
        xn[3], yn[3] = T + 2, 2              # out of range: NaN cost, zero gradient rows
    return f.to(dtype), g.to(dtype), w, b, labels, xn, yn


def upstream(N):
    return 0.5 + 0.25 * torch.arange(N, dtype=torch.float32)


@functools.lru_cache(maxsize=None)
def reference(case, sigma=0.0, lam=0.0, dtype=torch.float32, dropout=0.0, seed=None, dyadic=False, weights=None):
    """The fp64 reference of the case, computed once and shared: (costs, df, dg, dW, db).  Half inputs: the reference sees
    the rounded f and g and the fp32 master weights."""
    f, g, w, b, labels, xn, yn = make(case, dtype, dyadic)
    up = upstream(case[0]) if weights is None else torch.tensor(weights)
    return tdt_joint_reference(f, g, w, b, labels, xn, yn, case[4], case[6], case[7], sigma, lam, weights=up,
                               dropout=dropout, seed=seed)


def fused(case, inputs, sigma=0.0, lam=0.0, weights=None, **kw):
    from warp_rnnt_amd.tdt import tdt_loss_from_joint
    f, g, w, b, labels, xn, yn = inputs
    leaves = [x.detach().to(DEV).requires_grad_(True) if x is not None else None for x in (f, g, w, b)]
    out = tdt_loss_from_joint(*leaves, labels.to(DEV), xn.to(DEV), yn.to(DEV), durations=case[4], sigma=sigma,
                              blank=case[7], activation=case[6], fastemit_lambda=lam, **kw)
    up = upstream(case[0]) if weights is None else weights
    # (a NaN cost does not reach the gradients: d/d out of the sum is the weight)
    (out * up.to(DEV)).sum().backward() if out.dim() else out.backward()
    return (out.detach(),) + tuple(x.grad if x is not None else None for x in leaves)


def chain(case, inputs, sigma=0.0, lam=0.0, autocast_dtype=None):
    """The unfused path: the joint in torch (under autocast for half inputs) -> tdt_loss_from_logits."""
    from warp_rnnt_amd.tdt import tdt_loss_from_logits
    f, g, w, b, labels, xn, yn = inputs
    act = torch.tanh if case[6] == "tanh" else torch.relu
    leaves = [x.detach().to(DEV).requires_grad_(True) for x in (f, g, w, b)]
    with torch.autocast("cuda", dtype=autocast_dtype or torch.bfloat16, enabled=autocast_dtype is not None):
        z = torch.nn.functional.linear(act(leaves[0][:, :, None] + leaves[1][:, None]), leaves[2], leaves[3])
    out = tdt_loss_from_logits(z, labels.to(DEV), xn.to(DEV), yn.to(DEV), durations=case[4], sigma=sigma, blank=case[7],
                               fastemit_lambda=lam)
    (out * upstream(case[0]).to(DEV)).sum().backward()
    return (out.detach(),) + tuple(x.grad for x in leaves)


def cost_error(got, ref):
    """Largest error of a cost relative to its fp64 value; the NaNs (lengths out of range) must be the reference's."""
    got, ref = got.double().cpu(), ref.double()
    assert torch.equal(torch.isnan(got), torch.isnan(ref)), (got, ref)
    ok = ~torch.isnan(ref)
    return float(((got[ok] - ref[ok]).abs() / ref[ok].abs()).max())


def errors(result, ref):
    """The five figures of a result (costs, df, dg, dW, db) against the reference's."""
    out = {"cost": cost_error(result[0], ref[0])}
    for q, got, want in zip(QUANTITIES[1:], result[1:], ref[1:]):
        out[q] = nrel(got, want)
    return out


# ---- 1. fp32 against fp64, the chain as the yardstick ----

@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_fp32_against_fp64_within_four_times_the_chain(case):
    inputs = make(case)
    worst = dict.fromkeys(QUANTITIES, 0.0)
    for sigma in SIGMAS:
        for lam in LAMS:
            ref = reference(case, sigma, lam)
            got = fused(case, inputs, sigma, lam)
            e = errors(got, ref)
            print(case_id(case), f"sigma {sigma} lambda {lam}:", " ".join(f"{q} {e[q]:.3e}" for q in QUANTITIES))
            worst = {q: max(worst[q], e[q]) for q in QUANTITIES}
            if case[0] == 4:             # the utterance whose lengths are out of range: zero rows, finite elsewhere
                assert torch.isnan(got[0][3]) and torch.isfinite(got[0][:3]).all()
                assert torch.count_nonzero(got[1][3]) == 0 and torch.count_nonzero(got[2][3]) == 0
            for x in got[1:]:
                assert torch.isfinite(x).all()
    for q in QUANTITIES:
        assert worst[q] <= BARS[q], (q, worst[q], BARS[q])


# ---- 2. bf16 and fp16 against the autocast chain ----

@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("case", HALF_CASES, ids=case_id)
def test_half_error_within_twice_autocast_chain(case, dtype):
    inputs = make(case, dtype)
    ref = reference(case, 0.05, 0.01, dtype)
    ours = fused(case, inputs, 0.05, 0.01)               # fp32 master weights, half activations
    assert ours[1].dtype == dtype and ours[2].dtype == dtype
    assert ours[3].dtype == torch.float32 and ours[4].dtype == torch.float32
    theirs = chain(case, inputs, 0.05, 0.01, autocast_dtype=dtype)
    e_ours, e_chain = errors(ours, ref), errors(theirs, ref)
    for q, floor in zip(QUANTITIES, (1e-3, 2e-3, 2e-3, 2e-3, 2e-3)):
        print(case_id(case), dtype, q, f"fused {e_ours[q]:.3e} chain {e_chain[q]:.3e}")
    for q, floor in zip(QUANTITIES, (1e-3, 2e-3, 2e-3, 2e-3, 2e-3)):
        assert e_ours[q] <= 2 * e_chain[q] + floor, (q, e_ours[q], e_chain[q])
    # weights in the activations' dtype: their gradients come back in it
    half = (inputs[0], inputs[1], inputs[2].to(dtype), inputs[3].to(dtype)) + inputs[4:]
    again = fused(case, half, 0.05, 0.01)
    assert again[3].dtype == dtype and again[4].dtype == dtype


# ---- 3. bit contracts ----

BIT_CASES = [CASES[2], CASES[5]]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", BIT_CASES, ids=case_id)
def test_bits_run_to_run_batch_independence_padding_and_no_grad(case, dtype):
    from warp_rnnt_amd.tdt import tdt_loss_from_joint
    N = case[0]
    inputs = make(case, dtype)
    f, g, w, b, labels, xn, yn = inputs
    ones = torch.ones(N)
    a = fused(case, inputs, 0.05, 0.01, weights=ones)
    a2 = fused(case, inputs, 0.05, 0.01, weights=ones)
    for x, y in zip(a, a2):
        assert torch.equal(x, y)
    for n in range(N):
        tn, un = int(xn[n]), int(yn[n])
        alone = fused(case, (f[n:n + 1, :tn].contiguous(), g[n:n + 1, :un + 1].contiguous(), w, b,
                             labels[n:n + 1, :un].contiguous(), xn[n:n + 1], yn[n:n + 1]), 0.05, 0.01,
                      weights=torch.ones(1))
        assert torch.equal(alone[0][0], a[0][n])
        assert torch.equal(alone[1][0], a[1][n, :tn])
        assert torch.equal(alone[2][0], a[2][n, :un + 1])
        assert torch.count_nonzero(a[1][n, tn:]) == 0
        assert torch.count_nonzero(a[2][n, un + 1:]) == 0
    dev = [x.to(DEV) for x in inputs]
    kw = dict(durations=case[4], sigma=0.05, blank=case[7], activation=case[6], fastemit_lambda=0.01)
    with torch.no_grad():
        assert torch.equal(tdt_loss_from_joint(*dev, **kw), a[0])                 # costs without gradients
    assert torch.equal(tdt_loss_from_joint(*dev, **kw), a[0])                     # nothing requires grad
    for extra in (dict(dropout=0.0), dict(dropout=0.3, training=False)):
        again = fused(case, inputs, 0.05, 0.01, weights=ones, **extra)
        for x, y in zip(a, again):
            assert torch.equal(x, y)
    # only f requires grad, no bias: the others are not computed
    fd = f.to(DEV).requires_grad_(True)
    tdt_loss_from_joint(fd, dev[1], dev[2], None, *dev[4:], **kw).sum().backward()
    assert fd.grad is not None and torch.isfinite(fd.grad).all()
    # only the weight, only the bias: the bits they have when everything is asked for (split 0 of d weight is written into
    # the result itself, and not at all when only d bias is wanted)
    for k in (2, 3):
        leaf = dev[k].clone().requires_grad_(True)
        args = dev[:k] + [leaf] + dev[k + 1:]
        tdt_loss_from_joint(*args, **kw).sum().backward()
        assert torch.equal(leaf.grad, a[1 + k]), k


def test_single_split_weight_gradient_against_fp64():
    """One utterance of 15 cells: a single cell group, so joint_w_splits is 1, there is no partial, and d weight is what
    the weight kernel wrote into the result."""
    case = (1, 5, 2, 14, D5, 64, "tanh", 7)
    inputs = make(case)
    ref = reference(case, 0.05, 0.01)
    e = errors(fused(case, inputs, 0.05, 0.01), ref)
    print("single split:", " ".join(f"{q} {e[q]:.3e}" for q in QUANTITIES))
    for q in QUANTITIES:
        assert e[q] <= BARS[q], (q, e[q], BARS[q])


def test_graph_capture_replays_eager_bits():
    from warp_rnnt_amd.tdt import tdt_loss_from_joint
    case = BIT_CASES[0]
    f, g, w, b, labels, xn, yn = make(case)
    fd, gd, wd, bd = (x.to(DEV).requires_grad_(True) for x in (f, g, w, b))
    lab, txn, tyn = labels.to(DEV), xn.to(DEV), yn.to(DEV)
    kw = dict(durations=case[4], sigma=0.05, blank=case[7], activation=case[6], fastemit_lambda=0.01)

    def step():
        for p in (fd, gd, wd, bd):
            p.grad = None
        tdt_loss_from_joint(fd, gd, wd, bd, lab, txn, tyn, **kw).sum().backward()
        return [p.grad.clone() for p in (fd, gd, wd, bd)]

    eager = step()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()                                          # warm-up on the side stream
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    for p in (fd, gd, wd, bd):
        p.grad = None
    with torch.cuda.graph(graph):
        loss = tdt_loss_from_joint(fd, gd, wd, bd, lab, txn, tyn, **kw).sum()
        loss.backward()
    graph.replay()
    torch.cuda.synchronize()
    for p, e in zip((fd, gd, wd, bd), eager):
        assert torch.equal(p.grad, e)


# ---- 4. the normaliser is two floats ----

def test_shifted_biases_leave_costs_and_gradients_alone():
    """+1000 on every token bias and +3000 on every duration bias: the two log-softmaxes do not move, so the reference is
    the unshifted one.  The inputs are dyadic, so that z + 3000 is exact in fp32 and what is tested is the max / sum / log
    arithmetic, not the rounding of a logit at magnitude 3000 that any fp32 joint pays.  A normaliser folded into one
    float (m + ls) rounds at ulp(3000) = 2.4e-4 and misses the bars by orders of magnitude."""
    case = CASES[3]
    V = case[3]
    f, g, w, b, labels, xn, yn = make(case, dyadic=True)
    ref = reference(case, 0.05, 0.01, dyadic=True)
    plain = errors(fused(case, (f, g, w, b, labels, xn, yn), 0.05, 0.01), ref)
    shifted_b = b.clone()
    shifted_b[:V] += 1000.0
    shifted_b[V:] += 3000.0
    shifted = errors(fused(case, (f, g, w, shifted_b, labels, xn, yn), 0.05, 0.01), ref)
    for q in QUANTITIES:
        print(f"{q}: plain {plain[q]:.3e} shifted {shifted[q]:.3e} bar {BARS[q]:.3e}")
    for q in QUANTITIES:
        assert plain[q] <= BARS[q] and shifted[q] <= BARS[q], (q, plain[q], shifted[q], BARS[q])


# ---- 5. masked entries ----

def test_masked_token_and_duration():
    case = CASES[2]
    N, T, U, V, durations, H, act, blank = case
    f, g, w, b, labels, xn, yn = make(case)
    tok, dur = 3, durations.index(3)                        # not the blank (7), not duration 1
    labels = torch.where(labels == tok, torch.full_like(labels, tok + 1), labels)
    b = b.clone()
    b[tok] = float("-inf")
    b[V + dur] = float("-inf")
    ref = tdt_joint_reference(f, g, w, b, labels, xn, yn, durations, act, blank, 0.05, 0.01, want_grads=False)
    got = fused(case, (f, g, w, b, labels, xn, yn), 0.05, 0.01)
    for x in got:
        assert torch.isfinite(x).all()
    assert got[4][tok] == 0 and got[4][V + dur] == 0
    assert torch.count_nonzero(got[3][tok]) == 0 and torch.count_nonzero(got[3][V + dur]) == 0
    e = cost_error(got[0], ref[0])
    print(f"masked: cost {e:.3e} bar {BARS['cost']:.3e}")
    assert e <= BARS["cost"]


# ---- 6. dropout ----

@pytest.mark.parametrize("case", [CASES[2], CASES[7]], ids=case_id)
def test_dropout_against_the_host_mask(case):
    from warp_rnnt_amd.tdt import tdt_loss_from_joint
    p, seed = 0.3, 20230417
    inputs = make(case)
    ref = reference(case, 0.05, 0.01, dropout=p, seed=seed)
    word = torch.tensor([seed], dtype=torch.int64, device=DEV)
    got = fused(case, inputs, 0.05, 0.01, dropout=p, dropout_seed=word)
    e = errors(got, ref)
    print(case_id(case), "dropout:", " ".join(f"{q} {e[q]:.3e}" for q in QUANTITIES))
    for q in QUANTITIES:
        assert e[q] <= BARS[q], (q, e[q], BARS[q])
    again = fused(case, inputs, 0.05, 0.01, dropout=p, dropout_seed=word)
    for x, y in zip(got, again):
        assert torch.equal(x, y)
    other = fused(case, inputs, 0.05, 0.01, dropout=p, dropout_seed=word + 1)
    assert not torch.equal(other[0], got[0])
    dev = [x.to(DEV) for x in inputs]
    kw = dict(durations=case[4], sigma=0.05, blank=case[7], activation=case[6], fastemit_lambda=0.01, dropout=p)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        tdt_loss_from_joint(*dev, dropout_seed=word, **kw)          # warm-up on the side stream
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        with pytest.raises(RuntimeError, match="explicit dropout_seed"):
            tdt_loss_from_joint(*dev, **kw)                          # refused before any launch
        costs = tdt_loss_from_joint(*dev, dropout_seed=word, **kw)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(costs, got[0])


# ---- 7. reductions and the module ----

@pytest.mark.parametrize("reduction,average_frames", [("none", True), ("sum", False), ("mean", False), ("mean", True)])
def test_module_reductions_train_and_eval(reduction, average_frames):
    from warp_rnnt_amd.tdt import TDTJointLoss
    case = CASES[1]
    N, T, U, V, durations, H, act, blank = case
    f, g, w, b, labels, xn, yn = make(case)
    scale = (1.0 / xn.double()) if average_frames else torch.ones(N, dtype=torch.float64)
    weights = tuple((scale / N if reduction == "mean" else scale).tolist())
    module = TDTJointLoss(H, V, durations, sigma=0.05, blank=blank, activation=act, dropout=0.3, fastemit_lambda=0.01,
                          average_frames=average_frames, reduction=reduction).to(DEV)
    with torch.no_grad():
        module.weight.copy_(w)
        module.bias.copy_(b)
    seed = torch.tensor([77], dtype=torch.int64, device=DEV)
    for training, p in ((False, 0.0), (True, 0.3)):
        module.train(training)
        ref = reference(case, 0.05, 0.01, dropout=p, seed=77 if p else None, weights=weights)
        fd, gd = f.to(DEV).requires_grad_(True), g.to(DEV).requires_grad_(True)
        module.zero_grad()
        out = module(fd, gd, labels.to(DEV), xn.to(DEV), yn.to(DEV), dropout_seed=seed)
        (out.sum() if out.dim() else out).backward()
        want = ref[0] * scale
        want = want if reduction == "none" else (want.sum() if reduction == "sum" else want.mean())
        torch.testing.assert_close(out.detach().double().cpu(), want, rtol=1e-5, atol=1e-6)
        for q, got, r in zip(QUANTITIES[1:], (fd.grad, gd.grad, module.weight.grad, module.bias.grad), ref[1:]):
            assert nrel(got, r) <= BARS[q], (training, q, nrel(got, r))


# ---- 8. memory ----

def test_fused_memory_bf16():
    """Peak extra memory of forward plus backward beyond the returned gradients: below the workspace plus 92 B per cell plus
    1 MiB, and below a quarter of one (N,T,U+1,V+D) bf16 logits tensor.  Measured on an MI355X: peak extra 18128360 B,
    workspace 15011584 B, a quarter of the bf16 logits 21012000 B (DESIGN.md 3.16 says where the bytes are)."""
    from warp_rnnt_amd import _lib
    from warp_rnnt_amd.tdt import tdt_loss_from_joint
    N, T, U, V, H, D = 4, 200, 50, 1025, 640, 5
    torch.manual_seed(0)
    f = (torch.randn(N, T, H, device=DEV) * 0.5).to(torch.bfloat16).requires_grad_(True)
    g = (torch.randn(N, U + 1, H, device=DEV) * 0.5).to(torch.bfloat16).requires_grad_(True)
    lin = torch.nn.Linear(H, V + D).to(DEV)
    labels = torch.randint(0, V - 1, (N, U), dtype=torch.int32, device=DEV)
    xn = torch.full((N,), T, dtype=torch.int32, device=DEV)
    yn = torch.full((N,), U, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        c = tdt_loss_from_joint(f, g, lin.weight, lin.bias, labels, xn, yn, durations=D5, blank=V - 1)
    c.sum().backward()
    torch.cuda.synchronize()
    returned = sum(x.numel() * x.element_size() for x in (f.grad, g.grad, lin.weight.grad, lin.bias.grad))
    extra = torch.cuda.max_memory_allocated() - before - returned
    cells = N * T * (U + 1)
    ws = _lib.load().rnnt_amd_tdt_joint_workspace_size(N, T, U + 1, H, V, D)
    logits_bytes = cells * (V + D) * 2
    print(f"peak extra {extra} B; workspace {ws} B; per cell {4 * (2 + D) + 16 + 48} B x {cells}; "
          f"a quarter of the bf16 logits {logits_bytes // 4} B")
    assert torch.isfinite(c).all()
    assert extra < ws + (4 * (2 + D) + 16 + 48) * cells + (1 << 20), (extra, ws)
    assert extra < logits_bytes // 4, (extra, logits_bytes // 4)
