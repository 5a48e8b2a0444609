#!/usr/bin/env python
"""The blank plane piece by piece: blank_plane_probe.py [N T U V]  (default: c4 of bench.py)

Times, alone and interleaved round by round, on the in-tree library:
  lsm            rnnt_amd_log_softmax                               lsm+plane     rnnt_amd_log_softmax_plane
  gather         rnnt_amd_debug_gather_only                         gather+plane  rnnt_amd_debug_gather_only_blank_plane
  loss           rnnt_amd_loss (dense log-probs, diagonal pairs)    loss+plane    rnnt_amd_loss_blank_plane
  pair           lsm, then loss -- the materialised step            pair+plane    lsm+plane, then loss+plane
and checks that the plane is the column and that costs and gradient pairs are the same bits both ways."""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from warp_rnnt_amd import _lib  # noqa: E402

N, T, U, V = (int(v) for v in sys.argv[1:5]) if len(sys.argv) > 4 else (16, 1500, 300, 50)
L = _lib.load()
dev = torch.device("cuda:0")
g = torch.Generator(device=dev).manual_seed(1)
xs = torch.randn((N, T, U, V), device=dev, generator=g)
ys = torch.randint(1, V, (N, U - 1), dtype=torch.int32, device=dev, generator=g)
xn = torch.full((N,), T, dtype=torch.int32, device=dev)
yn = torch.full((N,), U - 1, dtype=torch.int32, device=dev)
rows = N * T * U
lp, plane = torch.empty_like(xs), torch.empty((rows,), device=dev)
costs, grads = torch.empty((N,), device=dev), torch.empty((N, T, U, 2), device=dev)
ws = torch.empty((L.rnnt_amd_workspace_size(N, T, U),), dtype=torch.uint8, device=dev)
s = torch.cuda.current_stream().cuda_stream
p = lambda t: t.data_ptr()  # noqa: E731


def lsm():
    return L.rnnt_amd_log_softmax(s, p(xs), p(lp), rows, V)


def lsm_plane():
    return L.rnnt_amd_log_softmax_plane(s, p(xs), p(lp), p(plane), rows, V, 0)


def gather():
    return L.rnnt_amd_debug_gather_only(s, p(ws), p(lp), p(ys), N, T, U, V, 0)


def gather_plane():
    return L.rnnt_amd_debug_gather_only_blank_plane(s, p(ws), p(lp), p(plane), p(ys), N, T, U, V, 0)


def loss():
    return L.rnnt_amd_loss(s, p(ws), 0, p(lp), p(ys), p(xn), p(yn), p(costs), p(grads), 1, N, T, U, V, 0, 0.0)


def loss_plane():
    return L.rnnt_amd_loss_blank_plane(s, p(ws), p(lp), p(plane), p(ys), p(xn), p(yn), p(costs), p(grads), 1, N, T, U, V,
                                       0, 0.0)


def pair():
    return lsm() or loss()


def pair_plane():
    return lsm_plane() or loss_plane()


assert lsm_plane() == 0 and loss_plane() == 0
c1, g1 = costs.clone(), grads.clone()
assert torch.equal(plane, lp[..., 0].reshape(-1)), "plane != column 0"
assert lsm() == 0 and loss() == 0
assert torch.equal(c1, costs) and torch.equal(g1, grads), "costs / gradient pairs differ with the plane"
forms = [("lsm", lsm), ("lsm+plane", lsm_plane), ("gather", gather), ("gather+plane", gather_plane), ("loss", loss),
         ("loss+plane", loss_plane), ("pair", pair), ("pair+plane", pair_plane)]
REPS, ROUNDS = 5, 12
ts = {name: [] for name, _ in forms}
for r in range(ROUNDS + 2):
    for name, fn in forms:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(REPS):
            st = fn()
        e1.record()
        torch.cuda.synchronize()
        assert st == 0, (name, st)
        if r >= 2:
            ts[name].append(e0.elapsed_time(e1) / REPS * 1e3)
print(f"N={N} T={T} U={U} V={V}: us per call, median / min / max over {ROUNDS} interleaved rounds of {REPS}; bits equal")
for name, _ in forms:
    v = ts[name]
    print(f"  {name:13s} {statistics.median(v):8.1f} {min(v):8.1f} {max(v):8.1f}")
