#!/usr/bin/env python
"""ms per fused training step -- rnnt_loss_from_logits(...).sum().backward(): logits -> costs -> d/d logits -- with the
gradient clamp off and on, and against another checkout of the library (the commit before the clamp), interleaved.

    python tools/clamp_rate.py [--rounds R] [--other DIR]

Configurations: `other` (DIR's packages, called without the keyword; only with --other), `off` (this tree, no keyword)
and `clamp=1.0` (this tree).  Every (round, configuration) is a process of its own, the configurations alternating inside
a round and their order reversed every other round, so that a drift of the box falls on all of them; `off` against `other` is the same instantiation of the same
kernels and has to sit inside the spread between the rounds of one configuration.  Shapes: c4 (N=16, T=1500, U=300,
V=50) in fp32 and bf16, c3 (N=32, T=150, U=20, V=5000) in fp32.  Per line: HIP events around 20 steps, median of 7, after
30 warm-up steps."""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = (("c4", 16, 1500, 300, 50, "float32"), ("c4", 16, 1500, 300, 50, "bfloat16"), ("c3", 32, 150, 20, 5000, "float32"))


def child(root, clamp):
    sys.path.insert(0, root)
    import torch
    from warp_rnnt_amd.fused import rnnt_loss_from_logits
    dev = torch.device("cuda:0")
    kw = {} if clamp is None else {"clamp": clamp}
    for name, N, T, U, V, dtype in SHAPES:
        g = torch.Generator(device=dev).manual_seed(V)
        x = torch.randn((N, T, U, V), device=dev, generator=g).to(getattr(torch, dtype)).requires_grad_(True)
        ys = torch.randint(1, V, (N, U - 1), dtype=torch.int32, device=dev, generator=g)
        xn = torch.full((N,), T, dtype=torch.int32, device=dev)
        yn = torch.full((N,), U - 1, dtype=torch.int32, device=dev)

        def step():
            x.grad = None
            loss = rnnt_loss_from_logits(x, ys, xn, yn, reduction="sum", **kw)
            loss.backward()
            return loss

        for _ in range(30):
            step()
        ts = []
        for _ in range(7):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(20):
                loss = step()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) / 20)
        print(f"{name} N={N} T={T} U={U} V={V:5d} {dtype:8s} {statistics.median(ts):8.4f} ms per step  (min {min(ts):.4f}, "
              f"max {max(ts):.4f})  loss {float(loss.detach()):.3f}  |d/d logits| sum {float(x.grad.double().abs().sum()):.4f}",
              flush=True)
        del x


if __name__ == "__main__":
    p = argparse.ArgumentParser()
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--other", default=None, help="another checkout of the repository to time against")
    p.add_argument("--child", nargs=2, metavar=("ROOT", "CLAMP"), help=argparse.SUPPRESS)
    a = p.parse_args()
    if a.child:
        child(a.child[0], None if a.child[1] == "none" else float(a.child[1]))
    else:
        configs = [("off", ROOT, "none"), ("clamp=1.0", ROOT, "1.0")]
        if a.other:
            configs.insert(0, ("other", os.path.abspath(a.other), "none"))
        for r in range(a.rounds):
            for label, root, clamp in (configs if r % 2 == 0 else configs[::-1]):      # (order reversed every other round)
                print(f"== round {r + 1} {label}", flush=True)
                subprocess.run([sys.executable, os.path.abspath(__file__), "--child", root, clamp], check=True, timeout=300)
