"""ctc_loss_from_logits (csrc/ctc.hip) against torch's ctc_loss on the CPU in float64 (tests/ctc_reference.py).

Every batch is ragged and holds four utterances: one without labels, one of the full width with adjacent and non-adjacent
repeats, one that is exactly feasible (T_n == L_n + its adjacent repeats) and one that is one frame short of that (no
path; at L == 1 no utterance with a frame can be, and the fourth is an ordinary one).  T is three frames more than the
longest needs.

The yardstick is the same reference in float32: its error against float64 at the very case is what a correct fp32
implementation with another summation order looks like, and the bar is four times that (floored at four fp32 ulp).  The
margin: costs and gradients carry the rounding of alpha and beta, values of magnitude ~T log V that go through one
log-sum-exp per state and frame; two correct orders of those T steps differ like two random walks of the same step, whose
maxima over a tensor lie within a small factor of each other (tools/ctc_loss_values.py measures both,
profiles/ctc_loss_values.txt holds the rows: the kernels' largest error is 1.31 times its yardstick).  An error is
max |x - ref| / max |ref| over the finite entries.  bf16 / fp16: the reference runs on the rounded logits, its gradient is
rounded to the dtype, and every element may be off by one ulp of the dtype at its magnitude plus the fp32 bar."""
import ctypes
import functools

import pytest
import torch

from ctc_reference import ctc_reference      # (tests/ is on the path: conftest.py's rootdir insert and pytest's own)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
EPS = {"fp32": 2.0 ** -23, "bf16": 2.0 ** -7, "fp16": 2.0 ** -10}
SHAPES = [(1, 2), (5, 5), (63, 37), (64, 500), (65, 1025), (130, 37)]        # (L, V): one wave, its edge, three waves
GRAD_COSTS = torch.tensor([0.5, -1.25, 2.0, 0.75])


@functools.lru_cache(maxsize=None)
def make(L, V, last_blank, name):
    """logits (4,T,V) in the dtype, labels (4,L), frames_lengths, labels_lengths, blank; on the CPU."""
    blank = V - 1 if last_blank else 0
    gen = torch.Generator().manual_seed(1000 * L + V)
    labels = torch.randint(0, V - 1, (4, L), generator=gen) + (0 if last_blank else 1)
    if L >= 4:
        labels[:, 1], labels[:, 3] = labels[:, 0], labels[:, 0]                 # a a b a: adjacent and non-adjacent
        labels[:, 2] = (labels[:, 0] - (0 if last_blank else 1) + 1) % (V - 1) + (0 if last_blank else 1)
    yn = torch.tensor([0, L, max(L - 1, 1), L])
    repeats = torch.tensor([int((labels[n, 1:yn[n]] == labels[n, :yn[n] - 1]).sum()) if yn[n] > 1 else 0 for n in range(4)])
    need = yn + repeats
    T = int(need.max()) + 3
    xn = torch.stack([torch.tensor(max(T // 2, 1)), torch.tensor(T), need[2], (need[3] - 1).clamp(min=1)])
    logits = (2.0 * torch.randn(4, T, V, generator=gen)).to(DTYPES[name])
    return logits, labels.int(), xn.int(), yn.int(), blank


@functools.lru_cache(maxsize=None)
def reference(L, V, last_blank, name):
    """(costs, gradient) in float64, and the errors of the float32 yardstick against them."""
    logits, labels, xn, yn, blank = make(L, V, last_blank, name)
    ref = ctc_reference(logits, labels, xn, yn, blank, grad_output=GRAD_COSTS)
    yard = ctc_reference(logits, labels, xn, yn, blank, grad_output=GRAD_COSTS, dtype=torch.float32)
    return ref, errors(yard, ref)


def errors(result, ref):
    out = []
    for x, r in zip(result, ref):
        x, r, finite = x.double().cpu(), r.double(), torch.isfinite(r)
        assert torch.equal(torch.isinf(x), ~finite) and not torch.isnan(x).any()      # no path: exactly +inf, never NaN
        out.append(float((x[finite] - r[finite]).abs().max() / r[finite].abs().max()))
    return tuple(out)


def kernel(L, V, last_blank, name, rows=slice(None)):
    from warp_rnnt_amd.ctc import ctc_loss_from_logits
    logits, labels, xn, yn, blank = make(L, V, last_blank, name)
    z = logits[rows].contiguous().to(DEV).requires_grad_(True)
    costs = ctc_loss_from_logits(z, labels[rows].contiguous().to(DEV), xn[rows].to(DEV), yn[rows].to(DEV),
                                 blank=blank - V if last_blank else blank, reduction="none")
    costs.backward(GRAD_COSTS[rows].to(DEV))
    return costs.detach(), z.grad


def poisoned(L, V, last_blank, name):
    """The two C entries on a workspace and outputs full of NaN."""
    from warp_rnnt_amd import _lib, ops
    lib = _lib.load()
    logits, labels, xn, yn, blank = (x.to(DEV) if isinstance(x, torch.Tensor) else x for x in make(L, V, last_blank, name))
    N, T, _ = logits.shape
    ws = torch.full((lib.rnnt_amd_ctc_workspace_size(N, T, L, V) // 4,), float("nan"), device=DEV)
    costs, grad = torch.full((N,), float("nan"), device=DEV), torch.full_like(logits, float("nan"))
    stream, go = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), GRAD_COSTS.to(DEV)
    head = (stream, ws.data_ptr(), ops.LOGITS_DTYPES[logits.dtype], logits.data_ptr(), labels.data_ptr(), xn.data_ptr(),
            yn.data_ptr())
    assert lib.rnnt_amd_ctc_loss_logits(*head, costs.data_ptr(), N, T, L, V, blank) == 0
    assert lib.rnnt_amd_ctc_logits_backward(*head, go.data_ptr(), grad.data_ptr(), N, T, L, V, blank) == 0
    return costs, grad


@pytest.mark.parametrize("name", list(DTYPES))
@pytest.mark.parametrize("last_blank", [False, True])
@pytest.mark.parametrize("L,V", SHAPES)
def test_against_fp64(L, V, last_blank, name):
    logits, labels, xn, yn, blank = make(L, V, last_blank, name)
    (ref_costs, ref_grad), yard = reference(L, V, last_blank, name)
    costs, grad = kernel(L, V, last_blank, name)
    assert costs.dtype == torch.float32 and grad.dtype == DTYPES[name] and grad.shape == logits.shape
    assert bool(torch.isinf(ref_costs[3])) == (L > 1) and torch.isfinite(ref_costs[:3]).all()
    bars = tuple(4 * max(y, EPS["fp32"]) for y in yard)
    e = errors((costs, grad), (ref_costs, ref_grad.to(DTYPES[name])))
    print(L, V, blank, name, "costs %.3e grad %.3e" % e, "yardstick %.3e %.3e" % yard)
    assert e[0] <= bars[0], (e, bars)
    exponent = torch.frexp(ref_grad.abs())[1] - 1
    ulp = 0.0 if name == "fp32" else torch.clamp(torch.ldexp(torch.tensor(EPS[name]).double(), exponent), min=2.0 ** -24)
    off = (grad.double().cpu() - ref_grad.to(DTYPES[name]).double()).abs()
    assert (off <= ulp + bars[1] * ref_grad.abs().max()).all(), float(off.max())
    # rows behind the frames, and the utterance without a path: written, as zeros
    dead = torch.arange(logits.shape[1])[None, :] >= xn[:, None]
    dead[3] |= L > 1
    assert torch.count_nonzero(grad.cpu()[dead]) == 0
    # stale reads and unwritten rows would show on poisoned buffers; a second run gives the same bits
    for again in (poisoned(L, V, last_blank, name), kernel(L, V, last_blank, name)):
        assert torch.equal(again[0], costs) and torch.equal(again[1], grad)


@pytest.mark.parametrize("L,V,name", [(5, 5, "fp32"), (65, 1025, "bf16"), (130, 37, "fp16")])
def test_an_utterance_has_the_same_bits_in_another_batch(L, V, name):
    costs, grad = kernel(L, V, False, name)
    for rows in ([1], [3, 1, 0], [2, 2, 1, 1, 0]):
        c, g = kernel(L, V, False, name, rows=rows)
        assert torch.equal(c, costs[rows]) and torch.equal(g, grad[rows])


@pytest.mark.parametrize("L,V,name", [(5, 5, "bf16"), (130, 37, "fp32")])
def test_graph_replay_gives_the_eager_bits(L, V, name):
    from warp_rnnt_amd.ctc import CTCLoss
    eager = kernel(L, V, True, name)
    logits, labels, xn, yn, blank = (x.to(DEV) if isinstance(x, torch.Tensor) else x for x in make(L, V, True, name))
    logits.requires_grad_(True)
    go, loss = GRAD_COSTS.to(DEV), CTCLoss(blank=blank, reduction="none")

    def step():
        costs = loss(logits, labels, xn, yn)
        return (costs,) + torch.autograd.grad(costs, logits, go)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                          # (warm-up outside the capture)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    for _ in range(3):                                  # several replays, each against the eager result
        for x in out:
            x.detach().zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a.detach(), b) for a, b in zip(out, eager))
