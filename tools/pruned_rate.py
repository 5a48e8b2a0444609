#!/usr/bin/env python
"""One training step of the pruned transducer loss beside the unfused chain on the same inputs.

    python tools/pruned_rate.py [--out profiles/pruned_loss_rate.txt]
    python tools/pruned_rate.py --steps 20 --v 500 --dtype bf16          (steps of the pruned loss only: what a kernel trace wraps)

Shape: N=16, T=1500, U=300, S=5, V=500 and 1025, logits (N,T,S,V) in bf16 and fp32, full lengths, the band a straight ramp
from column 0 to column U-S.  Per case, ms per step (forward + backward to d/d logits):
  pruned   warp_rnnt_amd.pruned.pruned_rnnt_loss_from_logits(...).sum().backward()
  chain    torch.log_softmax (fp32), gather of the blank and the label, scatter into (N,T,U,2) pairs over the floor -1e30,
           warp_rnnt.rnnt_loss(pairs, ..., blank=-1).sum().backward() -- index tensors built once, outside the timing
HIP events around 10 back-to-back steps, median of 5 rounds after 20 warm-up steps; the two interleaved --repeats times
(median and range).  Peak memory beyond the inputs: torch's max_memory_allocated over one step minus what was allocated
before it, with no gradient of an earlier step alive (so d/d logits, the size of the logits, is part of it)."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, T, U, S = 16, 1500, 300, 5
FLOOR = -1e30


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


def peak_beyond_inputs(torch, fn, x):
    fn()
    torch.cuda.synchronize()
    x.grad = None                 # (the step's own result counts: d/d logits is part of the peak)
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pruned_loss_rate.txt"))
    ap.add_argument("--v", type=int, action="append")
    ap.add_argument("--dtype", choices=("bf16", "f32"), action="append")
    ap.add_argument("--steps", type=int, default=0, help="run this many steps of the pruned loss of one case and exit")
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    import torch
    import warp_rnnt
    from warp_rnnt_amd import _build
    from warp_rnnt_amd.pruned import pruned_rnnt_loss_from_logits
    _build.ensure_built()
    dev = torch.device("cuda:0")
    props = torch.cuda.get_device_properties(0)
    lines = [f"# {props.name or 'device 0'} ({getattr(props, 'gcnArchName', '?')}); N={N} T={T} U={U} S={S}; ms per training step, "
             f"median of {a.repeats} interleaved repeats (each: median of 5 x 10 steps after 20 warm-up steps) [min - max]; "
             f"peak memory beyond the inputs, MB"]
    print(lines[0], flush=True)
    tdt = {"f32": torch.float32, "bf16": torch.bfloat16}
    for V in a.v or [500, 1025]:
        g = torch.Generator(device=dev).manual_seed(V)
        x32 = torch.randn((N, T, S, V), device=dev, generator=g)
        ys = torch.randint(1, V, (N, U - 1), dtype=torch.int32, device=dev, generator=g)
        xn = torch.full((N,), T, dtype=torch.int32, device=dev)
        yn = torch.full((N,), U - 1, dtype=torch.int32, device=dev)
        starts = (torch.arange(T, device=dev) * (U - S) // (T - 1)).to(torch.int32)[None, :].expand(N, T).contiguous()
        # the chain's index tensors: the lattice column of every row, its label (the blank in the last column)
        u = starts.long()[..., None] + torch.arange(S, device=dev)                                  # (N,T,S) in [0,U)
        lab = torch.cat([ys.long(), torch.zeros((N, 1), dtype=torch.long, device=dev)], 1).gather(1, u.reshape(N, -1))
        lab = lab.reshape(N, T, S, 1)
        for dn in a.dtype or ["bf16", "f32"]:
            x = x32.to(tdt[dn]).requires_grad_(True)

            def pruned():
                x.grad = None
                pruned_rnnt_loss_from_logits(x, ys, starts, xn, yn).sum().backward()

            def chain():
                x.grad = None
                lp = torch.log_softmax(x, -1, dtype=torch.float32)
                band = torch.cat([lp[..., 0:1], lp.gather(-1, lab)], -1)                            # (N,T,S,2)
                pairs = torch.full((N, T, U, 2), FLOOR, device=dev).scatter(2, u[..., None].expand(N, T, S, 2), band)
                warp_rnnt.rnnt_loss(pairs, ys, xn, yn, blank=-1).sum().backward()

            if a.steps:
                for _ in range(a.steps):
                    pruned()
                torch.cuda.synchronize()
                print(f"V={V} {dn}: {a.steps} steps done", flush=True)
                continue
            pruned()
            gp = x.grad.clone()
            chain()
            close = float((x.grad.float() - gp.float()).abs().max())
            tp, tc = [], []
            for _ in range(a.repeats):
                tp.append(timed(torch, pruned))
                tc.append(timed(torch, chain))
            mp, mc = peak_beyond_inputs(torch, pruned, x), peak_beyond_inputs(torch, chain, x)
            p, c = statistics.median(tp), statistics.median(tc)
            lines.append(f"V={V:5d} {dn:>4}: logits {x.numel() * x.element_size() / 1e6:7.1f} MB  pruned {p:7.4f} ms "
                         f"[{min(tp):.4f} - {max(tp):.4f}] peak {mp / 1e6:7.1f} MB   chain {c:7.4f} ms "
                         f"[{min(tc):.4f} - {max(tc):.4f}] peak {mc / 1e6:7.1f} MB   chain / pruned {c / p:5.2f}x   "
                         f"max |d/d logits difference| {close:.2e}")
            print(lines[-1], flush=True)
            del x
        del x32
        torch.cuda.empty_cache()
    if not a.steps:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
