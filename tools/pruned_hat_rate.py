#!/usr/bin/env python
"""One training step of the factorised-blank (HAT) loss on the pruned band beside the softmax pruned step and the unfused
torch HAT chain on the same inputs -- the protocol of tools/pruned_rate.py, whose helpers it uses.

    python tools/pruned_hat_rate.py [--out profiles/pruned_hat_loss_rate.txt]
    python tools/pruned_hat_rate.py --steps 20 --v 500 --dtype bf16      (steps of the HAT loss only: what a kernel trace wraps)

Shape: N=16, T=1500, U=300, S=5, V=500 and 1025, logits (N,T,S,V) in bf16 and fp32, full lengths, the band a straight ramp.
Per case, ms per step (forward + backward to d/d logits), the three interleaved --repeats times:
  hat      pruned_rnnt_loss_from_logits(..., use_hat_loss=True).sum().backward()
  softmax  pruned_rnnt_loss_from_logits(...).sum().backward()
  chain    warp_rnnt_amd.hat.hat_log_probs (fp32), gather of the blank and the label, scatter into (N,T,U,2) pairs over the
           floor -1e30, warp_rnnt.rnnt_loss(pairs, ..., blank=-1).sum().backward() -- index tensors built outside the timing
and the peak memory of one step beyond the inputs."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]
from pruned_rate import FLOOR, N, S, T, U, peak_beyond_inputs, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pruned_hat_loss_rate.txt"))
    ap.add_argument("--v", type=int, action="append")
    ap.add_argument("--dtype", choices=("bf16", "f32"), action="append")
    ap.add_argument("--steps", type=int, default=0, help="run this many steps of the HAT loss of one case and exit")
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    import torch
    import warp_rnnt
    from warp_rnnt_amd import _build
    from warp_rnnt_amd.hat import hat_log_probs
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
        u = starts.long()[..., None] + torch.arange(S, device=dev)                                  # (N,T,S) in [0,U)
        lab = torch.cat([ys.long(), torch.zeros((N, 1), dtype=torch.long, device=dev)], 1).gather(1, u.reshape(N, -1))
        lab = lab.reshape(N, T, S, 1)
        for dn in a.dtype or ["bf16", "f32"]:
            x = x32.to(tdt[dn]).requires_grad_(True)

            def hat():
                x.grad = None
                pruned_rnnt_loss_from_logits(x, ys, starts, xn, yn, use_hat_loss=True).sum().backward()

            def softmax():
                x.grad = None
                pruned_rnnt_loss_from_logits(x, ys, starts, xn, yn).sum().backward()

            def chain():
                x.grad = None
                lp = hat_log_probs(x.float(), 0)
                band = torch.cat([lp[..., 0:1], lp.gather(-1, lab)], -1)                            # (N,T,S,2)
                pairs = torch.full((N, T, U, 2), FLOOR, device=dev).scatter(2, u[..., None].expand(N, T, S, 2), band)
                warp_rnnt.rnnt_loss(pairs, ys, xn, yn, blank=-1).sum().backward()

            if a.steps:
                for _ in range(a.steps):
                    hat()
                torch.cuda.synchronize()
                print(f"V={V} {dn}: {a.steps} steps done", flush=True)
                continue
            hat()
            gh = x.grad.clone()
            chain()
            close = float((x.grad.float() - gh.float()).abs().max())
            steps = (hat, softmax, chain)
            ts = [[] for _ in steps]
            for _ in range(a.repeats):
                for t, fn in zip(ts, steps):
                    t.append(timed(torch, fn))
            peaks = [peak_beyond_inputs(torch, fn, x) / 1e6 for fn in steps]
            med = [statistics.median(t) for t in ts]
            lines.append(f"V={V:5d} {dn:>4}: logits {x.numel() * x.element_size() / 1e6:7.1f} MB  " + "   ".join(
                f"{fn.__name__} {m:7.4f} ms [{min(t):.4f} - {max(t):.4f}] peak {p:7.1f} MB"
                for fn, m, t, p in zip(steps, med, ts, peaks)) +
                f"   hat / softmax {med[0] / med[1]:5.3f}   chain / hat {med[2] / med[0]:5.2f}x   "
                f"max |d/d logits difference hat - chain| {close:.2e}")
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
