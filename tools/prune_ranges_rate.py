#!/usr/bin/env python
"""The band selection of the pruned recipe in HIP beside the torch chain, and beside a device copy of the bytes it reads.

    python tools/prune_ranges_rate.py [--out profiles/prune_ranges_rate.txt]
    python tools/prune_ranges_rate.py --steps 50          (calls of prune_ranges_hip and the copy only: what a kernel trace wraps)

Shapes: N=16, S=5 at T=1500, U=300 (the headline shape) with full and with ragged lengths, and at T=3000, U=600, full.
pair_grads is what simple_rnnt_loss(return_grad=True) hands back for random am / lm (V=500, bf16): real occupancies,
concentrated around the alignment.  Per case, microseconds per call:
  chain    warp_rnnt_amd.pruned.prune_ranges      (about fifteen torch operations over (N,T,U) temporaries)
  hip      warp_rnnt_amd.pruned.prune_ranges_hip  (two launches: the window kernel over the pairs, the scans over (N,T))
  scans    prune_ranges_hip on the first 3 columns with S=2: the same two launches and the same scans with a window kernel
           that reads 24 bytes per frame -- what of `hip` is not the pass over the pairs
  copy     torch's device copy of the (N,T,U,2) pairs into a second buffer: reads the same bytes and writes them back, the
           yardstick of the window kernel, which only reads them
HIP events around 20 back-to-back calls, median of 5 rounds after 20 warm-up calls; the three interleaved --repeats times
(median and range).  Also: how many starts differ between the two (near-ties of real-valued sums may fall either way),
and the loss side of a training step -- simple_rnnt_loss + ranges + pruned_rnnt_loss_from_logits, forward and backward,
V=500 bf16 -- with either band selection."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, S, V = 16, 5, 500


def timed(torch, fn, warmup=20, reps=20, rounds=5):
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
        ts.append(e0.elapsed_time(e1) / reps * 1e3)
    return statistics.median(ts)


def spread(ts):
    return f"{statistics.median(ts):8.1f} us [{min(ts):.1f} - {max(ts):.1f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prune_ranges_rate.txt"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=0,
                    help="run this many calls of prune_ranges_hip per case and exit (what a kernel trace wraps)")
    a = ap.parse_args()
    import torch
    from warp_rnnt_amd import _build
    from warp_rnnt_amd.pruned import prune_joint_inputs, prune_ranges, prune_ranges_hip, pruned_rnnt_loss_from_logits
    from warp_rnnt_amd.simple import simple_rnnt_loss
    _build.ensure_built()
    dev = torch.device("cuda:0")
    props = torch.cuda.get_device_properties(0)
    lines = [f"# {props.name or 'device 0'} ({getattr(props, 'gcnArchName', '?')}); N={N} S={S}; us per call, median of "
             f"{a.repeats} interleaved repeats (each: median of 5 x 20 calls after 20 warm-up calls) [min - max]"]
    print(lines[0], flush=True)
    for T, U, ragged in ((1500, 300, False), (1500, 300, True), (3000, 600, False)):
        g = torch.Generator(device=dev).manual_seed(T + U + ragged)
        am = torch.randn((N, T, V), device=dev, generator=g).bfloat16().requires_grad_(True)
        lm = torch.randn((N, U, V), device=dev, generator=g).bfloat16().requires_grad_(True)
        ys = torch.randint(1, V, (N, U - 1), dtype=torch.int32, device=dev, generator=g)
        xn = torch.full((N,), T, dtype=torch.int32, device=dev)
        yn = torch.full((N,), U - 1, dtype=torch.int32, device=dev)
        if ragged:
            xn = (xn.float() * torch.linspace(1.0, 0.5, N, device=dev)).to(torch.int32)
            yn = (yn.float() * torch.linspace(1.0, 0.5, N, device=dev)).to(torch.int32)
        _, pairs = simple_rnnt_loss(am, lm, ys, xn, yn, lm_only_scale=0.25, return_grad=True)
        pairs = pairs.contiguous()
        other = torch.empty_like(pairs)
        if a.steps:
            for _ in range(a.steps):
                prune_ranges_hip(pairs, xn, yn, S)
                other.copy_(pairs)
            torch.cuda.synchronize()
            print(f"T={T} U={U} {'ragged' if ragged else 'full'}: {a.steps} calls done", flush=True)
            continue
        starts = prune_ranges_hip(pairs, xn, yn, S)
        differ = int((starts != prune_ranges(pairs, xn, yn, S)).sum())
        narrow, yn2 = pairs[:, :, :3].contiguous(), yn.clamp(max=2)
        tc, th, tp, ts = [], [], [], []
        for _ in range(a.repeats):
            tc.append(timed(torch, lambda: prune_ranges(pairs, xn, yn, S)))
            th.append(timed(torch, lambda: prune_ranges_hip(pairs, xn, yn, S)))
            tp.append(timed(torch, lambda: other.copy_(pairs)))
            ts.append(timed(torch, lambda: prune_ranges_hip(narrow, xn, yn2, 2)))
        mb = pairs.numel() * 4 / 1e6
        c, h, p = statistics.median(tc), statistics.median(th), statistics.median(tp)
        lines.append(f"T={T} U={U} {'ragged' if ragged else 'full  '}: pairs {mb:6.1f} MB   chain {spread(tc)}   hip {spread(th)}   "
                     f"copy {spread(tp)}   scans {spread(ts)}   chain / hip {c / h:6.1f}x   hip reads at {mb / h * 1e3:6.0f} GB/s, the copy moves "
                     f"{2 * mb / p * 1e3:6.0f} GB/s (read + write)   starts that differ from the chain's: {differ} of {N * T}")
        print(lines[-1], flush=True)
        if (T, U, ragged) != (1500, 300, False):
            continue
        # the loss side of a training step at the headline shape: simple + ranges + pruned, forward and backward
        f = torch.randn((N, T, 1, V), device=dev, generator=g).bfloat16()
        gg = torch.randn((N, U, V), device=dev, generator=g).bfloat16()

        def step(ranges):
            am.grad = lm.grad = None
            simple, pg = simple_rnnt_loss(am, lm, ys, xn, yn, lm_only_scale=0.25, return_grad=True)
            st = ranges(pg, xn, yn, S)
            x = (f + prune_joint_inputs(f[:, :, 0], gg, st, S)[1]).requires_grad_(True)       # stands in for the joiner's output
            (0.5 * simple.sum() + pruned_rnnt_loss_from_logits(x, ys, st, xn, yn).sum()).backward()

        sc, sh = [], []
        for _ in range(a.repeats):
            sc.append(timed(torch, lambda: step(prune_ranges), reps=10))
            sh.append(timed(torch, lambda: step(prune_ranges_hip), reps=10))
        lines.append(f"T={T} U={U} full  : the loss side of a step (simple_rnnt_loss + ranges + band gather + "
                     f"pruned_rnnt_loss_from_logits, forward and backward, V={V} bf16): with the chain {spread(sc)}   with "
                     f"prune_ranges_hip {spread(sh)}")
        print(lines[-1], flush=True)
    if not a.steps:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
