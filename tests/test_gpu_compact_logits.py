"""The fused logits -> loss path on the compact (ragged packed) layout: rnnt_loss_from_logits(compact=True).

Costs and d/d logits against the oracle and against the materialised chain (log-softmax + rnnt_loss(compact=True)), the
bit contracts of the fused path (half = fp32 on the upcast, position in the batch, bounded = unbounded, every lattice
kernel, = the dense fused path), graph capture, edge cases and the memory it does not use."""
import numpy as np
import pytest
import torch

import oracle
from helpers import make_case, np_log_softmax32
from test_gpu_half import CASES

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def T(a):
    return torch.tensor(np.ascontiguousarray(a), device=DEV)


def pack(x, labels, xn, yn):
    V = x.shape[-1]
    xs = np.concatenate([x[n, :xn[n], :yn[n] + 1].reshape(-1, V) for n in range(x.shape[0])])
    ys = np.concatenate([labels[n, :yn[n]] for n in range(x.shape[0])] + [np.zeros((0,), np.int32)]).astype(np.int32)
    return np.ascontiguousarray(xs), ys


def fused(xs, ys, xn, yn, up=None, blank=0, lam=0.01, **kw):
    from warp_rnnt_amd.fused import rnnt_loss_from_logits
    z = xs.detach().clone().requires_grad_(True)
    c = rnnt_loss_from_logits(z, ys, xn, yn, blank=blank, fastemit_lambda=lam, compact=True, **kw)
    c.backward(up if c.dim() else None)
    return c.detach(), z.grad


def chain(xs, ys, xn, yn, up, blank=0, lam=0.01, lazy_lib=False):
    """(b) the library's log-softmax (eager) or (a) torch's, then rnnt_loss(compact=True)."""
    import warp_rnnt
    from warp_rnnt_amd import functional
    z = xs.detach().clone().requires_grad_(True)
    lp = functional.log_softmax(z, lazy=False) if lazy_lib else torch.log_softmax(z.float(), -1)
    c = warp_rnnt.rnnt_loss(lp, ys, xn, yn, blank=blank, fastemit_lambda=lam, compact=True)
    c.backward(up)
    return c.detach(), z.grad


def case(seed, N, Tm, Um, V, blank):
    logits, labels, xn, yn = make_case(seed, N, Tm, Um, V, ragged=True, blank=blank)
    xs, ys = pack(logits, labels, xn, yn)
    return logits, labels, xn, yn, xs, ys


@pytest.mark.parametrize("N,Tm,Um,V", CASES)
def test_compact_fused_against_oracle_and_chain(N, Tm, Um, V):
    blank = 0 if V % 2 else V - 1
    logits, labels, xn, yn, xs, ys = case(11 + V, N, Tm, Um, V, blank)
    up = np.random.RandomState(V).rand(N).astype(np.float32) + 0.5
    c, g = fused(T(xs), T(ys), T(xn), T(yn), T(up), blank)
    lp = np_log_softmax32(logits)
    ref = oracle.rnnt_loss_f32(lp, labels, xn, yn, blank=blank, fastemit_lambda=0.01)
    np.testing.assert_allclose(c.cpu().numpy(), ref["costs"], rtol=1e-5)
    # oracle d/d log-probs, scaled, through an fp64 log-softmax backward
    gl = ref["grads"].astype(np.float64) * up[:, None, None, None]
    p = np.exp(lp.astype(np.float64))
    dz = gl - p * gl.sum(-1, keepdims=True)
    want, _ = pack(dz, labels, xn, yn)
    np.testing.assert_allclose(g.cpu().numpy(), want, atol=1e-4)
    # the materialised compact chain
    cc, gc = chain(T(xs), T(ys), T(xn), T(yn), T(up), blank)
    np.testing.assert_allclose(c.cpu().numpy(), cc.cpu().numpy(), rtol=2e-6)
    np.testing.assert_allclose(g.cpu().numpy(), gc.cpu().numpy(), rtol=1e-4, atol=2e-6)
    # half logits: costs of the fp32 upcast, d/d logits = the fp32 ones rounded once
    for dt in (torch.bfloat16, torch.float16):
        xh = (T(xs) * 2).to(dt)
        c32, g32 = fused(xh.float(), T(ys), T(xn), T(yn), T(up), blank)
        ch, gh = fused(xh, T(ys), T(xn), T(yn), T(up), blank)
        assert ch.dtype == torch.float32 and gh.dtype == dt
        assert torch.equal(ch, c32) and torch.equal(gh, g32.to(dt))


@pytest.mark.parametrize("V", [50, 7, 128, 1030])
def test_compact_fused_bits_alone_bounded_kernels_and_dense(V):
    from warp_rnnt_amd import debug
    from warp_rnnt_amd.fused import rnnt_loss_from_logits
    N, Tm, Um, blank = 5, 37, 19, 3
    logits, labels, xn, yn, xs, ys = case(3 + V, N, Tm, Um, V, blank)
    up = T(np.linspace(0.5, 1.5, N).astype(np.float32))
    c, g = fused(T(xs), T(ys), T(xn), T(yn), up, blank)
    # bounded = unbounded
    cb, gb = fused(T(xs), T(ys), T(xn), T(yn), up, blank, max_frames=Tm + 3, max_labels=Um)
    assert torch.equal(cb, c) and torch.equal(gb, g)
    # every lattice kernel
    for k in ("ws", "wd", "wl"):
        with debug.lattice_kernel(k):
            ck, gk = fused(T(xs), T(ys), T(xn), T(yn), up, blank)
        assert torch.equal(ck, c) and torch.equal(gk, g), k
    # each utterance alone = inside the batch, at every position
    rows = np.concatenate([[0], np.cumsum(xn * (yn + 1))])
    labs = np.concatenate([[0], np.cumsum(yn)])
    for n in range(N):
        cn, gn = fused(T(xs[rows[n]:rows[n + 1]]), T(ys[labs[n]:labs[n + 1]]), T(xn[n:n + 1]), T(yn[n:n + 1]),
                       up[n:n + 1], blank)
        assert torch.equal(cn, c[n:n + 1]) and torch.equal(gn, g[rows[n]:rows[n + 1]]), n
    # the dense fused path on the same utterances padded: the same costs (the same log-softmax kernel at these V)
    cd = rnnt_loss_from_logits(T(logits), T(labels), T(xn), T(yn), blank=blank, fastemit_lambda=0.01)
    assert torch.equal(cd, c)


def test_compact_fused_graph_capture_and_refused_replay():
    from warp_rnnt_amd.fused import rnnt_loss_from_logits
    N, Tm, Um, V, blank = 4, 30, 12, 50, 1
    _, _, xn, yn, xs, ys = case(5, N, Tm, Um, V, blank)
    sx, sys_, sxn, syn = T(xs), T(ys), T(xn), T(yn)
    z = sx.clone().requires_grad_(True)
    up = torch.ones(N, device=DEV)
    want_c, want_g = fused(sx, sys_, sxn, syn, up, blank, max_frames=Tm, max_labels=Um - 1)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):             # warm-up outside the capture
        for _ in range(2):
            z.grad = None
            rnnt_loss_from_logits(z, sys_, sxn, syn, blank=blank, fastemit_lambda=0.01, compact=True, max_frames=Tm,
                                  max_labels=Um - 1).sum().backward()
    torch.cuda.current_stream().wait_stream(s)
    z.grad = None
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cost = rnnt_loss_from_logits(z, sys_, sxn, syn, blank=blank, fastemit_lambda=0.01, compact=True,
                                     max_frames=Tm, max_labels=Um - 1)
        cost.sum().backward()
    # replay on new data of the same shape
    rng = np.random.RandomState(6)
    xs2 = rng.randn(*xs.shape).astype(np.float32)
    ys2 = rng.randint(2, V, size=ys.shape).astype(np.int32)
    z.data.copy_(T(xs2)); sys_.copy_(T(ys2))
    g.replay()
    torch.cuda.synchronize()
    c2, g2 = fused(T(xs2), T(ys2), T(xn), T(yn), up, blank)
    assert torch.equal(cost, c2) and torch.equal(z.grad, g2)
    z.data.copy_(sx); sys_.copy_(T(ys)); sxn.copy_(T(xn)); syn.copy_(T(yn))
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(cost, want_c) and torch.equal(z.grad, want_g)
    # a batch that does not fit its bounds: NaN costs, all-zero d/d logits
    bad = xn.copy()
    bad[0] = Tm + 5
    sxn.copy_(T(bad))
    g.replay()
    torch.cuda.synchronize()
    assert torch.isnan(cost).all() and (z.grad == 0).all()


def test_compact_fused_edge_cases():
    N, Tm, Um, V = 4, 21, 7, 6
    logits, labels, xn, yn = make_case(5, N, Tm, Um, V, ragged=True)
    # an utterance with xn = 0 owns no rows: NaN cost, the others untouched
    keep = [0, 2, 3]
    xs, ys = pack(logits[keep], labels[keep], xn[keep], yn[keep])
    xn_bad = xn.copy()
    xn_bad[1] = 0
    yb = np.concatenate([labels[n, :yn[n]] for n in range(N)]).astype(np.int32)
    up = torch.ones(N, device=DEV)
    c, g = fused(T(xs), T(yb), T(xn_bad), T(yn), up)
    ck, gk = fused(T(xs), T(ys), T(xn[keep]), T(yn[keep]), up[:3])
    assert torch.isnan(c[1]) and torch.equal(c[keep], ck) and torch.equal(g, gk)
    # a logits view one element off alignment
    _, _, xn3, yn3, xs3, ys3 = case(8, 3, 17, 9, 64, 0)
    base = torch.empty(xs3.size + 1, device=DEV)
    view = base[1:].view(xs3.shape)
    view.copy_(T(xs3))
    from warp_rnnt_amd.fused import rnnt_loss_from_logits as f
    c_al = f(T(xs3), T(ys3), T(xn3), T(yn3), compact=True)
    c_un = f(view, T(ys3), T(xn3), T(yn3), compact=True)
    np.testing.assert_allclose(c_un.cpu().numpy(), c_al.cpu().numpy(), rtol=1e-6)
    # reduction / average_frames: the reference's arithmetic
    for red in ("sum", "mean"):
        for af in (False, True):
            got = f(T(xs3), T(ys3), T(xn3), T(yn3), compact=True, reduction=red, average_frames=af)
            cc = c_al / T(xn3).to(c_al) if af else c_al
            want = cc.sum() if red == "sum" else cc.mean()
            assert torch.equal(got, want)


def test_compact_fused_memory_bf16():
    from warp_rnnt_amd import _lib
    from warp_rnnt_amd.fused import rnnt_loss_from_logits
    N, Tm, Um, V = 8, 120, 40, 512
    _, _, xn, yn, xs, ys = case(9, N, Tm, Um, V, 0)
    STU = xs.shape[0]
    z = T(xs).to(torch.bfloat16).requires_grad_(True)
    tys, txn, tyn = T(ys), T(xn), T(yn)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    c = rnnt_loss_from_logits(z, tys, txn, tyn, compact=True)
    c.sum().backward()
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - before - z.grad.numel() * z.grad.element_size()
    ws = _lib.load().rnnt_amd_workspace_size_compact(N, STU, int(xn.max()), int(yn.max()) + 1)
    assert extra < ws + 64 * STU + (1 << 20), (extra, ws, STU)
    assert extra < STU * V * 4            # far less than one fp32 (STU,V) tensor


def test_compact_fused_c4_bf16():
    N, Tm, Um, V = 16, 1500, 301, 50
    rng = np.random.RandomState(4)
    xn = rng.randint(Tm // 2, Tm + 1, size=N).astype(np.int32)
    yn = rng.randint((Um - 1) // 2, Um, size=N).astype(np.int32)
    xn[0], yn[0] = Tm, Um - 1
    STU = int((xn * (yn + 1)).sum())
    g = torch.Generator(device=DEV).manual_seed(4)
    xs = torch.randn((STU, V), device=DEV, generator=g).to(torch.bfloat16)
    ys = T(rng.randint(1, V, size=int(yn.sum())).astype(np.int32))
    up = torch.ones(N, device=DEV)
    ch, gh = fused(xs, ys, T(xn), T(yn), up, 0, 0.0)
    c32, g32 = fused(xs.float(), ys, T(xn), T(yn), up, 0, 0.0)
    assert torch.equal(ch, c32) and torch.equal(gh, g32.to(torch.bfloat16))
    del gh, g32
    # the oracle's costs on the fp32 log-probs of the upcast, utterance by utterance
    lp = torch.log_softmax(xs.float(), -1).cpu().numpy()
    ysn = ys.cpu().numpy()
    rows = np.concatenate([[0], np.cumsum(xn * (yn + 1))])
    labs = np.concatenate([[0], np.cumsum(yn)])
    for n in range(N):
        lpn = lp[rows[n]:rows[n + 1]].reshape(1, xn[n], yn[n] + 1, V)
        ref = oracle.rnnt_loss_f32(lpn, ysn[labs[n]:labs[n + 1]].reshape(1, -1), xn[n:n + 1], yn[n:n + 1])
        np.testing.assert_allclose(ch[n].item(), ref["costs"][0], rtol=1e-5)
