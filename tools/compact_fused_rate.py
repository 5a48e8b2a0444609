#!/usr/bin/env python
"""Rate of the compact (ragged packed) layout from logits: three routes, fp32 and bf16 logits.

    python tools/compact_fused_rate.py --shape c4 --dtype bf16      (one case per process: run each under its own timeout)
    python tools/compact_fused_rate.py --shape c4 --dtype bf16 --route c --steps 20     (one route, no table: for a profiler)

Routes: (a) torch.log_softmax + rnnt_loss(compact=True); (b) functional.log_softmax(lazy=False) + rnnt_loss(compact=True);
(c) rnnt_loss_from_logits(compact=True), the fused path.  Per route: ms of the forward (logits -> costs, no gradient) and of
the training step to d/d logits, HIP events around 10 back-to-back calls, median of 5, after 10 warm-up calls; the routes
alternate --repeats times in one process (median and range).  Ragged batches, lengths at 50-100 % of the maxima."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"c4": (16, 1500, 300, 50), "v1024": (32, 500, 100, 1024), "v5000": (32, 150, 40, 5000)}


def timed(torch, fn, warmup=10, reps=10, rounds=5):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / reps)
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=sorted(SHAPES), default="c4")
    ap.add_argument("--dtype", choices=("f32", "bf16"), default="f32")
    ap.add_argument("--route", choices=("a", "b", "c"), default=None)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    import numpy as np
    import torch
    import warp_rnnt
    from warp_rnnt_amd import functional
    from warp_rnnt_amd.fused import rnnt_loss_from_logits

    N, Tm, Um, V = SHAPES[args.shape]
    rng = np.random.RandomState(0)
    xn = rng.randint(Tm // 2, Tm + 1, size=N).astype(np.int32)
    yn = rng.randint(Um // 2, Um + 1, size=N).astype(np.int32)
    xn[0], yn[0] = Tm, Um
    STU = int((xn * (yn + 1)).sum())
    dt = torch.float32 if args.dtype == "f32" else torch.bfloat16
    dev = "cuda:0"
    x = torch.randn((STU, V), device=dev).to(dt)
    ys = torch.tensor(rng.randint(1, V, size=int(yn.sum())).astype(np.int32), device=dev)
    txn, tyn = torch.tensor(xn, device=dev), torch.tensor(yn, device=dev)

    def loss(route, z):
        if route == "c":
            return rnnt_loss_from_logits(z, ys, txn, tyn, compact=True)
        lp = torch.log_softmax(z.float(), -1) if route == "a" else functional.log_softmax(z, lazy=False)
        return warp_rnnt.rnnt_loss(lp, ys, txn, tyn, compact=True)

    def fwd(route):
        with torch.no_grad():
            loss(route, x)

    def step(route):
        z = x.detach().requires_grad_(True)
        loss(route, z).sum().backward()

    if args.route:
        for _ in range(args.steps):
            step(args.route)
        torch.cuda.synchronize()
        return
    res = {r: {"fwd": [], "step": []} for r in "abc"}
    for _ in range(args.repeats):
        for r in "abc":
            res[r]["fwd"].append(timed(torch, lambda: fwd(r)))
            res[r]["step"].append(timed(torch, lambda: step(r)))
    print(f"{args.shape} N={N} T<={Tm} U<={Um} V={V} STU={STU} {args.dtype} ({args.repeats} alternations, ms: median [min-max])")
    for r, name in (("a", "torch.log_softmax + compact"), ("b", "library log_softmax + compact"), ("c", "fused compact")):
        f, s = res[r]["fwd"], res[r]["step"]
        print(f"  ({r}) {name:32s} fwd {statistics.median(f):8.3f} [{min(f):.3f}-{max(f):.3f}]"
              f"  step {statistics.median(s):8.3f} [{min(s):.3f}-{max(s):.3f}]")


if __name__ == "__main__":
    main()
