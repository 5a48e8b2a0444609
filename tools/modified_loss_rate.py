#!/usr/bin/env python
"""One training step of the pruned and the simple loss in the two topologies, side by side.

    python tools/modified_loss_rate.py [--out profiles/modified_loss_rate.txt]

Shape: N=16, T=1500, U=300, S=5, V=500 and 1025, bf16, full lengths (T_n = T, U_n = U - 1), random feasible bands.  Per case,
ms per step (forward + backward) of
  regular    the call without the keywords
  modified   rnnt_type="modified", delay_penalty=0.01
HIP events around 10 back-to-back steps, median of 5 rounds after 20 warm-up steps; the two interleaved --repeats times in
one process (median and range).  The expectation this file checks: the modified step sweeps one plane row more but T + 1
diagonals instead of T + U, and adds one small launch (the simple loss: a floor fill and a clear as well) -- it should
cost no more than the regular step beside it."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

N, T, U, S = 16, 1500, 300, 5
DP = 0.01


def timed(torch, fn, warmup=20, reps=10, rounds=5):
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "modified_loss_rate.txt"))
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    import numpy as np
    import torch
    from warp_rnnt_amd import _build
    from warp_rnnt_amd.pruned import pruned_rnnt_loss_from_logits
    from warp_rnnt_amd.simple import simple_rnnt_loss
    _build.ensure_built()
    dev = torch.device("cuda:0")
    props = torch.cuda.get_device_properties(0)
    lines = [f"# {props.name or 'device 0'} ({getattr(props, 'gcnArchName', '?')}); N={N} T={T} U={U} S={S} bf16; ms per training "
             f"step, median of {a.repeats} interleaved repeats (each: median of 5 x 10 steps after 20 warm-up steps) "
             f"[min - max]; modified: rnnt_type=\"modified\", delay_penalty={DP}"]
    print(lines[0], flush=True)
    # a band that holds a path in both topologies: it climbs one label every fifth frame, S = 5 wide
    starts = torch.tensor(np.clip(np.arange(T) // 5 - 2, 0, U - S), dtype=torch.int32, device=dev).repeat(N, 1).contiguous()
    xn = torch.full((N,), T, dtype=torch.int32, device=dev)
    yn = torch.full((N,), U - 1, dtype=torch.int32, device=dev)
    kw = dict(rnnt_type="modified", delay_penalty=DP)
    for V in (500, 1025):
        g = torch.Generator(device=dev).manual_seed(V)
        ys = torch.randint(1, V, (N, U - 1), dtype=torch.int32, device=dev, generator=g)
        x = torch.randn((N, T, S, V), device=dev, generator=g).bfloat16().requires_grad_(True)
        am = (torch.randn((N, T, V), device=dev, generator=g) * 2).bfloat16().requires_grad_(True)
        lm = (torch.randn((N, U, V), device=dev, generator=g) * 2).bfloat16().requires_grad_(True)

        def pruned(**k):
            x.grad = None
            pruned_rnnt_loss_from_logits(x, ys, starts, xn, yn, **k).sum().backward()

        def simple(**k):
            am.grad = lm.grad = None
            simple_rnnt_loss(am, lm, ys, xn, yn, lm_only_scale=0.25, **k).sum().backward()

        for name, step in (("pruned", pruned), ("simple", simple)):
            for k in ({}, kw):
                step(**k)
            torch.cuda.synchronize()
            tr, tm = [], []
            for _ in range(a.repeats):
                tr.append(timed(torch, step))
                tm.append(timed(torch, lambda: step(**kw)))
            r, m = statistics.median(tr), statistics.median(tm)
            lines.append(f"{name} V={V:5d}: regular {r:7.4f} ms [{min(tr):.4f} - {max(tr):.4f}]   modified {m:7.4f} ms "
                         f"[{min(tm):.4f} - {max(tm):.4f}]   modified / regular {m / r:5.3f}x")
            print(lines[-1], flush=True)
        del x, am, lm
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
