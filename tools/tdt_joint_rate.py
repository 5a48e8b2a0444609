#!/usr/bin/env python
"""One TDT training step -- joint network plus loss, forward and backward -- two ways: time per step and peak extra HBM.

  chain : act(f[:, :, None] + g[:, None]) -> Linear(H, V+D) in torch (autocast for bf16) -> tdt_loss_from_logits
  fused : tdt_loss_from_joint(f, g, weight, bias, ...)

    python tools/tdt_joint_rate.py [--steps 5] [--warmup 2] [--shapes T,U ...] [--out profiles/tdt_joint_rate.txt]

Shapes: N = 16, H = 640, V = 1025, durations (0,1,2,3,4); (T,U) = (200,60) and (1500,300), in fp32 and bf16.  Every step
is timed on its own with events after the warm-up steps; the figure is the median, with the spread beside it.  Peak extra
memory is what the step allocates beyond its inputs and parameters (the returned gradients included).  A way that does
not fit is reported as such.  --ways fused --steps 1 --warmup 1 is the run to put under a kernel trace."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

D5 = (0, 1, 2, 3, 4)


def batch(N, T, U, V, H, dtype, dev):
    gen = torch.Generator().manual_seed(0)
    f = (torch.randn(N, T, H, generator=gen) * 0.5).to(dev).to(dtype).requires_grad_(True)
    g = (torch.randn(N, U + 1, H, generator=gen) * 0.5).to(dev).to(dtype).requires_grad_(True)
    labels = torch.randint(0, V - 1, (N, U), generator=gen, dtype=torch.int32).to(dev)
    xn = torch.randint(T // 2, T + 1, (N,), generator=gen, dtype=torch.int32)
    yn = torch.randint(U // 2, U + 1, (N,), generator=gen, dtype=torch.int32)
    xn[0], yn[0] = T, U
    return f, g, labels, xn.to(dev), yn.to(dev)


def step_fn(way, lin, f, g, labels, xn, yn, V, half):
    from warp_rnnt_amd.tdt import tdt_loss_from_joint, tdt_loss_from_logits

    def step():
        lin.zero_grad(set_to_none=True)
        f.grad = g.grad = None
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=half):
            if way == "chain":
                z = lin(torch.tanh(f[:, :, None] + g[:, None]))
                loss = tdt_loss_from_logits(z, labels, xn, yn, durations=D5, blank=V - 1)
            else:
                loss = tdt_loss_from_joint(f, g, lin.weight, lin.bias, labels, xn, yn, durations=D5, blank=V - 1)
        loss.sum().backward()
    return step


def measure(step, steps, warmup):
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    times = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        step()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return times, (torch.cuda.max_memory_allocated() - base) / 1e9


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--steps", type=int, default=5)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--N", type=int, default=16)
    p.add_argument("--H", type=int, default=640)
    p.add_argument("--V", type=int, default=1025)
    p.add_argument("--shapes", nargs="*", default=["200,60", "1500,300"])
    p.add_argument("--dtypes", default="fp32,bf16")
    p.add_argument("--ways", default="chain,fused")
    p.add_argument("--out", default=None)
    args = p.parse_args()
    dev = torch.device("cuda:0")
    lines = []
    for T, U in (tuple(int(v) for v in s.split(",")) for s in args.shapes):
        for dtype in args.dtypes.split(","):
            half = dtype == "bf16"
            for way in args.ways.split(","):
                rec = {"N": args.N, "T": T, "U": U, "V": args.V, "D": len(D5), "H": args.H, "dtype": dtype, "way": way}
                try:
                    torch.manual_seed(0)
                    # (the fused way takes what an autocast encoder / predictor hands over; the chain casts inside)
                    f, g, labels, xn, yn = batch(args.N, T, U, args.V, args.H,
                                                 torch.bfloat16 if half and way == "fused" else torch.float32, dev)
                    lin = torch.nn.Linear(args.H, args.V + len(D5)).to(dev)
                    times, gb = measure(step_fn(way, lin, f, g, labels, xn, yn, args.V, half), args.steps, args.warmup)
                    rec.update(ms_per_step=round(statistics.median(times), 3), ms_min=round(min(times), 3),
                               ms_max=round(max(times), 3), steps=args.steps, peak_extra_GB=round(gb, 4))
                except torch.cuda.OutOfMemoryError:
                    rec["does_not_fit"] = True
                lines.append(json.dumps(rec))
                print(lines[-1], flush=True)
                f = g = lin = None
                torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as out:
            out.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
