"""Dropout inside the fused joint on the GPU: rnnt_loss_from_joint(..., dropout=p) and JointLoss.

One reference holds the three kernels (which map cells to lanes in three different ways) to one mask: the float64 autograd
joint of tests/test_gpu_joint.py with act(f+g) multiplied by the NumPy mask of tests/joint_dropout_mask.py and
float64(scale).  Shapes are the smallest that cross every tile edge: H of one, three and four waves per workgroup, V no
multiple of 16, ragged lengths (dead cells inside the 4x4 tiles, t and u past one tile), several utterances."""
import functools

import pytest
import torch

from oracle.transduce_np import transduce_batch
from joint_dropout_mask import keep_mask, scale as scale_of
from test_gpu_joint import act_of, make, nrel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

CASES = [  # seed, N, T, U (labels), V, H, act, blank
    (1, 3, 7, 4, 23, 32, "tanh", 0),
    (2, 2, 9, 5, 50, 320, "relu", 3),
    (4, 2, 4, 3, 37, 1024, "relu", 1),
]
CASE_IDS = [f"V{c[4]}_H{c[5]}_{c[6]}" for c in CASES]
LAM = 0.01
MASK_SEED = {0.2: 1234, 0.5: -7}            # one of them negative: the key is the int64's bits as a uint64


def mask_of(seed, p, f, g):
    """The keep mask (N,T,U+1,H) as a float64 tensor and float64(scale)."""
    N, T, H = f.shape
    return torch.from_numpy(keep_mask(seed, p, N, T, g.shape[1], H)).double(), scale_of(p)


def reference(f, g, w, b, labels, xn, yn, act, blank, lam, weights, keep, scale):
    """test_gpu_joint.reference with the mask: float64 on the CPU, gradients of sum_n weights[n] * cost[n]."""
    f, g, w, b = (x.detach().double().cpu().requires_grad_(True) for x in (f, g, w, b))
    h = act_of(act)(f[:, :, None] + g[:, None]) * keep * scale
    lp = torch.log_softmax(torch.nn.functional.linear(h, w, b), -1)
    costs, dlp = transduce_batch(lp.detach().numpy(), labels.numpy(), xn.numpy(), yn.numpy(), blank, lam)
    (lp * torch.from_numpy(dlp) * weights.double()[:, None, None, None]).sum().backward()
    return torch.from_numpy(costs), f.grad, g.grad, w.grad, b.grad


@functools.lru_cache(maxsize=None)
def case_reference(case, p, dtype):
    """Inputs and the fp64 reference (unit weights) of a case: computed once, shared, never modified."""
    seed, N, T, U, V, H, act, blank = case
    ins = make(seed, N, T, U, V, H, dtype=dtype, blank=blank)
    keep, scale = mask_of(MASK_SEED[p], p, ins[0], ins[1])
    return ins, reference(*ins, act, blank, LAM, torch.ones(N), keep, scale)


def seed_tensor(seed):
    return torch.tensor([seed], dtype=torch.int64, device=DEV)


def fused(f, g, w, b, labels, xn, yn, act="tanh", blank=0, lam=0.0, reduction="none", upstream=None, **drop):
    """costs and the four gradients of rnnt_loss_from_joint; drop: dropout / training / dropout_seed (an int: a fresh
    tensor holding it)."""
    from warp_rnnt_amd.joint import rnnt_loss_from_joint
    if isinstance(drop.get("dropout_seed"), int):
        drop["dropout_seed"] = seed_tensor(drop["dropout_seed"])
    f, g, w, b = (x.detach().to(DEV).requires_grad_(True) for x in (f, g, w, b))
    out = rnnt_loss_from_joint(f, g, w, b, labels.to(DEV), xn.to(DEV), yn.to(DEV), activation=act, reduction=reduction,
                               blank=blank, fastemit_lambda=lam, **drop)
    (out * (upstream.to(DEV) if upstream is not None else 1.0)).sum().backward()
    return out.detach(), f.grad, g.grad, w.grad, b.grad


def assert_fp32_close(got, ref):
    torch.testing.assert_close(got[0].double().cpu(), ref[0], rtol=1e-5, atol=1e-5)
    for x, r, name in zip(got[1:], ref[1:], ("f", "g", "weight", "bias")):
        assert nrel(x, r) < 1e-4, (name, nrel(x, r))


# ---- 1. fp32 against fp64 ----

@pytest.mark.parametrize("p", [0.2, 0.5])
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_joint_dropout_fp32_against_fp64(case, p):
    act, blank = case[6], case[7]
    ins, ref = case_reference(case, p, torch.float32)
    got = fused(*ins, act, blank, LAM, dropout=p, dropout_seed=MASK_SEED[p])
    assert_fp32_close(got, ref)


def test_joint_dropout_fp32_upstream_weights_and_mean():
    case, p = CASES[1], 0.2
    seed, N, T, U, V, H, act, blank = case
    ins, _ = case_reference(case, p, torch.float32)
    keep, scale = mask_of(MASK_SEED[p], p, ins[0], ins[1])
    up = torch.linspace(0.5, 2.0, N)
    ref = reference(*ins, act, blank, LAM, up, keep, scale)
    got = fused(*ins, act, blank, LAM, upstream=up, dropout=p, dropout_seed=MASK_SEED[p])
    assert_fp32_close(got, ref)
    # reduction="mean" under an upstream factor: weights factor / N
    ref = reference(*ins, act, blank, LAM, torch.full((N,), 1.7 / N), keep, scale)
    got = fused(*ins, act, blank, LAM, reduction="mean", upstream=torch.tensor(1.7), dropout=p,
                dropout_seed=MASK_SEED[p])
    torch.testing.assert_close(got[0].double().cpu(), ref[0].mean(), rtol=1e-5, atol=1e-5)
    for x, r, name in zip(got[1:], ref[1:], ("f", "g", "weight", "bias")):
        assert nrel(x, r) < 1e-4, (name, nrel(x, r))


# ---- 2. bf16 and fp16: no further from fp64 than twice the autocast chain with the same mask ----

def chain(f, g, w, b, labels, xn, yn, act, blank, lam, autocast_dtype, keep, scale):
    """The unfused path: the torch joint under autocast with the mask tensor applied -> rnnt_loss_from_logits."""
    from warp_rnnt_amd.fused import rnnt_loss_from_logits
    f, g, w, b = (x.detach().to(DEV).requires_grad_(True) for x in (f, g, w, b))
    m = (keep * scale).to(DEV, f.dtype)
    with torch.autocast("cuda", dtype=autocast_dtype):
        z = torch.nn.functional.linear(act_of(act)(f[:, :, None] + g[:, None]) * m, w, b)
    c = rnnt_loss_from_logits(z, labels.to(DEV), xn.to(DEV), yn.to(DEV), blank=blank, fastemit_lambda=lam)
    c.sum().backward()
    return c.detach(), f.grad, g.grad, w.grad, b.grad


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_joint_dropout_half_error_within_twice_autocast_chain(case, dtype):
    p = 0.2
    act, blank = case[6], case[7]
    ins, ref = case_reference(case, p, dtype)
    keep, scale = mask_of(MASK_SEED[p], p, ins[0], ins[1])
    ours = fused(*ins, act, blank, LAM, dropout=p, dropout_seed=MASK_SEED[p])
    assert ours[1].dtype == dtype and ours[2].dtype == dtype and ours[3].dtype == torch.float32
    theirs = chain(*ins, act, blank, LAM, dtype, keep, scale)
    for i, (r, floor) in enumerate(zip(ref, (1e-3, 2e-3, 2e-3, 2e-3, 2e-3))):
        e_ours, e_chain = nrel(ours[i], r), nrel(theirs[i], r)
        print(f"{case[4:7]} {dtype} output {i}: ours {e_ours:.3e} chain {e_chain:.3e}")
        assert e_ours <= 2 * e_chain + floor, (i, e_ours, e_chain)


# ---- 3. no dropout is the call without the new arguments ----

@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_joint_without_dropout_is_todays_bits(dtype):
    from warp_rnnt_amd.joint import JointLoss
    seed, N, T, U, V, H, act, blank = CASES[0]
    ins = make(seed, N, T, U, V, H, dtype=dtype, blank=blank)
    plain = fused(*ins, act, blank, LAM)
    for kw in (dict(dropout=0.3, training=False), dict(dropout=0.0), dict(dropout=0.0, dropout_seed=5),
               dict(dropout=0.3, training=False, dropout_seed=5)):
        got = fused(*ins, act, blank, LAM, **kw)
        for x, y in zip(got, plain):
            assert torch.equal(x, y), kw
    f, g, w, b, labels, xn, yn = ins
    module = JointLoss(H, V, activation=act, dropout=0.3, blank=blank, fastemit_lambda=LAM, reduction="none").to(DEV)
    with torch.no_grad():
        module.weight.copy_(w)
        module.bias.copy_(b)
    module.eval()
    fd, gd = (x.to(DEV).requires_grad_(True) for x in (f, g))
    out = module(fd, gd, labels.to(DEV), xn.to(DEV), yn.to(DEV))
    out.sum().backward()
    for x, y in zip((out.detach(), fd.grad, gd.grad, module.weight.grad, module.bias.grad), plain):
        assert torch.equal(x, y)
    # and in training mode it is the function with dropout on
    module.train()
    fd.grad = gd.grad = module.weight.grad = module.bias.grad = None
    out = module(fd, gd, labels.to(DEV), xn.to(DEV), yn.to(DEV), dropout_seed=seed_tensor(77))
    out.sum().backward()
    want = fused(*ins, act, blank, LAM, dropout=0.3, dropout_seed=77)
    for x, y in zip((out.detach(), fd.grad, gd.grad, module.weight.grad, module.bias.grad), want):
        assert torch.equal(x, y)
    assert not torch.equal(want[0], plain[0])


# ---- 4. the mask is carried, not inferred from a staged zero ----

def test_joint_dropout_kept_zero_activation_has_derivative_scale():
    """f = g = 0 under tanh: every staged value is an exact zero, kept or not; a kept one has derivative scale."""
    N, T, U, V, H, p, seed = 2, 6, 3, 19, 64, 0.5, 4321
    f, g, w, b, labels, xn, yn = make(7, N, T, U, V, H)
    f, g = torch.zeros_like(f), torch.zeros_like(g)
    keep, scale = mask_of(seed, p, f, g)
    ref = reference(f, g, w, b, labels, xn, yn, "tanh", 0, LAM, torch.ones(N), keep, scale)
    got = fused(f, g, w, b, labels, xn, yn, "tanh", 0, LAM, dropout=p, dropout_seed=seed)
    assert float(ref[1].norm()) > 0 and float(ref[2].norm()) > 0
    assert torch.count_nonzero(got[1]) > 0 and torch.count_nonzero(got[2]) > 0
    assert_fp32_close(got, ref)
    # a dropped column of an utterance's f row gets exactly nothing: the row's mask over all its cells
    dropped_everywhere = ~keep[0, 0, :int(yn[0]) + 1].bool().any(0)
    assert dropped_everywhere.any() and torch.count_nonzero(got[1][0, 0].cpu()[dropped_everywhere]) == 0


# ---- 5. determinism and layout ----

@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_joint_dropout_bits_seed_and_padding(dtype):
    N, T, U, V, H, p = 3, 9, 5, 37, 96, 0.2
    f, g, w, b, labels, xn, yn = make(21, N, T, U, V, H, dtype=dtype)
    xn[1], yn[1] = 5, 2
    a = fused(f, g, w, b, labels, xn, yn, "tanh", 0, LAM, dropout=p, dropout_seed=11)
    a2 = fused(f, g, w, b, labels, xn, yn, "tanh", 0, LAM, dropout=p, dropout_seed=11)
    for x, y in zip(a, a2):
        assert torch.equal(x, y)
    other = fused(f, g, w, b, labels, xn, yn, "tanh", 0, LAM, dropout=p, dropout_seed=12)
    assert not torch.equal(other[0], a[0])
    # the batch padded to (T + 3, U + 2), f and g as views into larger buffers (H kept): the counter holds n, t, u, not
    # a cell index over the padded shape.  dW / db are exempt (their split count is a function of the shape)
    fbuf = torch.randn(N, T + 3 + 2, H).to(dtype)
    gbuf = torch.randn(N, U + 1 + 2 + 1, H).to(dtype)
    fbuf[:, 1:T + 1], gbuf[:, 1:U + 2] = f, g
    fp, gp = fbuf[:, 1:T + 4], gbuf[:, 1:U + 4]
    assert not fp.is_contiguous() and fp.shape == (N, T + 3, H) and gp.shape == (N, U + 3, H)
    lp = torch.cat([labels, torch.ones(N, 2, dtype=torch.int32)], 1)
    c = fused(fp, gp, w, b, lp, xn, yn, "tanh", 0, LAM, dropout=p, dropout_seed=11)
    assert torch.equal(c[0], a[0])
    assert torch.equal(c[1][:, :T], a[1]) and torch.equal(c[2][:, :U + 1], a[2])
    for n in range(N):
        assert torch.count_nonzero(c[1][n, int(xn[n]):]) == 0 and torch.count_nonzero(c[2][n, int(yn[n]) + 1:]) == 0
    for i in (3, 4):
        assert nrel(c[i], a[i]) < (1e-5 if dtype == torch.float32 else 1e-2)


# ---- 6. a drawn seed ----

def test_joint_dropout_drawn_seed_follows_torch_manual_seed():
    seed, N, T, U, V, H, act, blank = CASES[0]
    ins = make(seed, N, T, U, V, H, blank=blank)
    torch.manual_seed(123)
    a = fused(*ins, act, blank, LAM, dropout=0.5)
    b = fused(*ins, act, blank, LAM, dropout=0.5)          # no reseeding: another draw
    torch.manual_seed(123)
    a2 = fused(*ins, act, blank, LAM, dropout=0.5)
    for x, y in zip(a, a2):
        assert torch.equal(x, y)
    assert not torch.equal(a[0], b[0])


# ---- 7. graph capture ----

def test_joint_dropout_graph_capture_replays_eager_bits_of_the_seed_it_finds():
    from warp_rnnt_amd.joint import rnnt_loss_from_joint
    N, T, U, V, H, p = 3, 10, 5, 40, 64, 0.2
    f, g, w, b, labels, xn, yn = make(41, N, T, U, V, H)
    fd, gd, wd, bd = (x.to(DEV).requires_grad_(True) for x in (f, g, w, b))
    lab, txn, tyn = labels.to(DEV), xn.to(DEV), yn.to(DEV)
    seed = seed_tensor(1001)

    def loss_of(s):
        return rnnt_loss_from_joint(fd, gd, wd, bd, lab, txn, tyn, blank=1, fastemit_lambda=0.01, dropout=p,
                                    dropout_seed=s)

    def step(s):
        for q in (fd, gd, wd, bd):
            q.grad = None
        c = loss_of(s)
        c.sum().backward()
        return [c.detach().clone()] + [q.grad.clone() for q in (fd, gd, wd, bd)]

    eager = step(seed_tensor(1001))
    eager_other = step(seed_tensor(-5))
    assert not torch.equal(eager[0], eager_other[0])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step(seed)                                      # warm-up on the side stream
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    for q in (fd, gd, wd, bd):
        q.grad = None
    with torch.cuda.graph(graph):
        with pytest.raises(RuntimeError, match="explicit dropout_seed"):
            rnnt_loss_from_joint(fd, gd, wd, bd, lab, txn, tyn, blank=1, dropout=p)     # refused before any launch
        costs = loss_of(seed)
        costs.sum().backward()
    graph.replay()
    torch.cuda.synchronize()
    for got, e in zip([costs] + [q.grad for q in (fd, gd, wd, bd)], eager):
        assert torch.equal(got, e)
    seed.copy_(seed_tensor(-5))                         # what a training loop does between replays
    graph.replay()
    torch.cuda.synchronize()
    for got, e in zip([costs] + [q.grad for q in (fd, gd, wd, bd)], eager_other):
        assert torch.equal(got, e)
