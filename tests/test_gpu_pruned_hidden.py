"""The pruned joiner's hidden activations: pruned_joint_hidden (csrc/pruned_hidden.hip) against fp64 on the CPU.

h, df and dg at the smallest shapes at which each kernel can go wrong.  The yardstick is the torch chain on the same GPU
inputs -- prune_joint_inputs, add, activation, autograd, all in the inputs' dtype -- against the same reference over the
same grid: a bar is four times the chain's largest error per dtype and quantity, floored at one ulp of the dtype at the
reference's magnitude (tools/pruned_hidden_values.py measures both, profiles/pruned_hidden_values.txt holds the rows).
An error is max |x - ref| / max |ref| over the tensor."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
ULP = {"fp32": 2.0 ** -23, "bf16": 2.0 ** -7, "fp16": 2.0 ** -10}
CASES = {  # name: (N, T, U, S, H)
    "base": (3, 7, 5, 2, 8),            # ragged frames_lengths; one 16-byte chunk per row in bf16
    "wide": (2, 5, 4, 3, 520),          # H not a power of two; more chunks than one wave holds
    "tiny": (1, 1, 1, 1, 8),            # T = 1, no labels
    "S=U": (2, 6, 4, 4, 40),            # every column in every frame
    "clamp": (2, 6, 4, 3, 8),           # starts from -2 up to U: both clamps hit
    "jump": (2, 9, 12, 2, 8),           # starts jump by more than S: columns no row maps to
    "run": (1, 300, 4, 2, 8),           # one start held for hundreds of frames: a long [lo,hi)
    "non-monotone": (2, 8, 6, 2, 8),    # utterance 0's starts decrease (the scan path), utterance 1 on the range path
    "no lengths": (3, 7, 5, 2, 8),      # frames_lengths=None: every frame live
}
# The torch chain's largest error against fp64 over CASES x both activations on an MI355X, per dtype: (h, df, dg)
# (profiles/pruned_hidden_values.txt, the rows "chain"; the kernels' own largest stand beside them there).
YARDSTICK = {
    "fp32": (8.794e-08, 1.524e-07, 1.684e-07),   # the kernels' largest: 8.794e-08 1.739e-07 5.939e-07 (dg: "run", a serial sum
    "bf16": (3.336e-03, 1.200e-02, 1.571e-02),   # the kernels' largest: 3.241e-03 3.180e-03 3.221e-03    of 290 fp32 terms)
    "fp16": (4.210e-04, 1.302e-03, 1.989e-03),   # the kernels' largest: 4.087e-04 4.477e-04 4.665e-04
}


def bars(name):
    return tuple(max(4 * y, ULP[name]) for y in YARDSTICK[name])


@functools.lru_cache(maxsize=None)
def make(case, name):
    """f, g in the dtype, dh fp32 (cast by the caller), starts (N,T) int32, frames_lengths or None; all on the CPU."""
    N, T, U, S, H = CASES[case]
    gen = torch.Generator().manual_seed(100 * T + H + len(case))
    f, g = (torch.randn(N, x, H, generator=gen).to(DTYPES[name]) for x in (T, U))
    dh = torch.randn(N, T, S, H, generator=gen)
    ramp = (torch.arange(T)[None, :] * max(U - S, 0) // max(T - 1, 1)).repeat(N, 1)
    if case == "clamp":
        ramp = torch.linspace(-2, U, T).round().long()[None, :].repeat(N, 1)
    elif case == "jump":
        ramp = (torch.arange(T)[None, :] // 3 * 4).repeat(N, 1)              # 0 0 0 4 4 4 8 8 8: half the columns unmapped
    elif case == "run":
        ramp = torch.cat([torch.zeros(10), torch.ones(T - 20), torch.full((10,), 2.0)]).long()[None, :]
    elif case == "non-monotone":
        ramp[0] = torch.tensor([0, 2, 1, 3, 3, 2, 4, 4])
    xn = None if case in ("no lengths", "tiny") else torch.tensor([T, max(T - 3, 1), max(T // 2, 1)][:N], dtype=torch.int32)
    return f, g, dh, ramp.to(torch.int32), xn


@functools.lru_cache(maxsize=None)
def reference(case, name, act):
    """The definition in fp64 with its autograd; for the half types act' starts from the rounded h, as the kernel's does."""
    f, g, dh, starts, xn = make(case, name)
    N, T, U, S, H = CASES[case]
    f64, g64 = f.double().requires_grad_(True), g.double().requires_grad_(True)
    idx = (starts.long()[..., None] + torch.arange(S)).clamp(0, U - 1)                               # (N,T,S)
    live = (torch.arange(T)[None, :] < (xn.long()[:, None] if xn is not None else T)).expand(N, T)[..., None, None]
    pre = f64[:, :, None, :] + g64[torch.arange(N)[:, None, None], idx]
    h = torch.where(live, torch.tanh(pre) if act == "tanh" else torch.relu(pre), 0.0)
    y = h.detach().to(DTYPES[name]).double()
    p = dh.to(DTYPES[name]).double() * live * ((1 - y * y) if act == "tanh" else (y > 0).double())
    df, dg = torch.autograd.grad(pre, (f64, g64), p)
    mapped = torch.zeros(N, U, dtype=torch.long).scatter_add_(1, idx.reshape(N, -1), live.expand(N, T, S, 1).reshape(N, -1).long())
    return h.detach(), df, dg, live.reshape(N, T), mapped > 0


def kernel(case, name, act, need=(True, True), three_dim_ranges=False):
    from warp_rnnt_amd.pruned import pruned_joint_hidden
    f, g, dh, starts, xn = (x if x is None else x.to(DEV) for x in make(case, name))
    S = CASES[case][3]
    f.requires_grad_(need[0]), g.requires_grad_(need[1])
    if three_dim_ranges:
        h = pruned_joint_hidden(f, g, starts[..., None] + torch.arange(S, device=DEV), xn, activation=act)
    else:
        h = pruned_joint_hidden(f, g, starts, xn, s_range=S, activation=act)
    h.backward(dh.to(h.dtype))
    return h.detach(), f.grad, g.grad


def chain(case, name, act):
    from warp_rnnt_amd.pruned import prune_joint_inputs
    f, g, dh, starts, xn = (x if x is None else x.to(DEV) for x in make(case, name))
    f.requires_grad_(True), g.requires_grad_(True)
    fp, gp = prune_joint_inputs(f, g, starts, CASES[case][3])
    h = (torch.tanh if act == "tanh" else torch.relu)(fp + gp)
    if xn is not None:
        h = h * (torch.arange(h.shape[1], device=DEV)[None, :] < xn[:, None])[..., None, None]
    h.backward(dh.to(h.dtype))
    return h.detach(), f.grad, g.grad


def errors(result, ref):
    return tuple(float((x.double().cpu() - r).abs().max() / r.abs().max().clamp(min=1e-30)) for x, r in zip(result, ref[:3]))


@pytest.mark.parametrize("act", ["tanh", "relu"])
@pytest.mark.parametrize("name", list(DTYPES))
@pytest.mark.parametrize("case", list(CASES))
def test_against_fp64_and_bit_for_bit_with_itself(case, name, act):
    ref = reference(case, name, act)
    h, df, dg = kernel(case, name, act)
    assert h.dtype == df.dtype == dg.dtype == DTYPES[name] and h.is_contiguous()
    assert h.shape == ref[0].shape and df.shape == ref[1].shape and dg.shape == ref[2].shape
    e = errors((h, df, dg), ref)
    print(case, name, act, "h %.3e df %.3e dg %.3e" % e, "bars %.3e %.3e %.3e" % bars(name))
    assert all(x <= b for x, b in zip(e, bars(name))), (e, bars(name))
    live, mapped = ref[3].to(DEV), ref[4].to(DEV)
    assert torch.count_nonzero(h[~live]) == 0 and torch.count_nonzero(df[~live]) == 0
    assert torch.count_nonzero(dg[~mapped]) == 0
    # one gradient alone, a second run, ranges as (N,T,S): the same bits
    assert torch.equal(kernel(case, name, act, need=(True, False))[1], df)
    assert torch.equal(kernel(case, name, act, need=(False, True))[2], dg)
    for again in (kernel(case, name, act), kernel(case, name, act, three_dim_ranges=True)):
        assert all(torch.equal(a, b) for a, b in zip(again, (h, df, dg)))


@pytest.mark.parametrize("case,name", [("base", "bf16"), ("non-monotone", "fp32")])
def test_graph_replay_gives_the_eager_bits(case, name):
    from warp_rnnt_amd.pruned import pruned_joint_hidden
    eager = kernel(case, name, "tanh")
    f, g, dh, starts, xn = (x.to(DEV) for x in make(case, name))
    f.requires_grad_(True), g.requires_grad_(True)
    dh = dh.to(f.dtype)

    def step():
        h = pruned_joint_hidden(f, g, starts, xn, s_range=CASES[case][3])
        return (h,) + torch.autograd.grad(h, (f, g), dh)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                          # (warm-up outside the capture)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    for x in out:
        x.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(out, eager))
