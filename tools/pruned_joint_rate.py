#!/usr/bin/env python
"""One training step of pruned_rnnt_loss_from_joint beside the unfused chain on the same inputs.

    python tools/pruned_joint_rate.py [--out profiles/pruned_joint_rate.txt]
    python tools/pruned_joint_rate.py --steps 20 --v 1025 --dtype bf16     (steps of the fused entry only: what a kernel trace wraps)

Shape: N=16, T=1500, U=300, S=5, H=512, V=500, 1025 and 5000, f / g in bf16 and fp32 with an fp32 master weight, tanh, full
lengths, the band a straight ramp from column 0 to column U-S.  Per case, ms per step (forward + backward to f, g, weight
and bias):
  fused    warp_rnnt_amd.pruned.pruned_rnnt_loss_from_joint(...).sum().backward()
  chain    prune_joint_inputs -> F.linear(tanh(fp + gp), weight, bias) (under autocast for bf16) ->
           pruned_rnnt_loss_from_logits(...).sum().backward()
The protocol is tools/pruned_rate.py's: HIP events around 10 back-to-back steps, median of 5 rounds after 20 warm-up steps;
the two interleaved --repeats times (median and range).  Peak memory beyond the inputs: torch's max_memory_allocated over
one step minus what was allocated before it, with no gradient of an earlier step alive (the returned gradients are part of
it, for both)."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]

from pruned_rate import timed  # noqa: E402

N, T, U, S, H = 16, 1500, 300, 5, 512


def peak_beyond_inputs(torch, fn, leaves):
    fn()
    torch.cuda.synchronize()
    for x in leaves:
        x.grad = None
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pruned_joint_rate.txt"))
    ap.add_argument("--v", type=int, action="append")
    ap.add_argument("--dtype", choices=("bf16", "f32"), action="append")
    ap.add_argument("--steps", type=int, default=0, help="run this many steps of the fused entry of one case and exit")
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    import torch
    from warp_rnnt_amd import _build
    from warp_rnnt_amd.pruned import prune_joint_inputs, pruned_rnnt_loss_from_joint, pruned_rnnt_loss_from_logits
    _build.ensure_built()
    dev = torch.device("cuda:0")
    props = torch.cuda.get_device_properties(0)
    lines = [f"# {props.name or 'device 0'} ({getattr(props, 'gcnArchName', '?')}); N={N} T={T} U={U} S={S} H={H} tanh; ms per "
             f"training step, median of {a.repeats} interleaved repeats (each: median of 5 x 10 steps after 20 warm-up steps) "
             f"[min - max]; peak memory beyond the inputs, MB"]
    print(lines[0], flush=True)
    tdt = {"f32": torch.float32, "bf16": torch.bfloat16}
    for V in a.v or [500, 1025, 5000]:
        gen = torch.Generator(device=dev).manual_seed(V)
        ys = torch.randint(1, V, (N, U - 1), dtype=torch.int32, device=dev, generator=gen)
        xn = torch.full((N,), T, dtype=torch.int32, device=dev)
        yn = torch.full((N,), U - 1, dtype=torch.int32, device=dev)
        starts = (torch.arange(T, device=dev) * (U - S) // (T - 1)).to(torch.int32)[None, :].expand(N, T).contiguous()
        w = (torch.randn((V, H), device=dev, generator=gen) / H ** 0.5).requires_grad_(True)
        b = (torch.randn((V,), device=dev, generator=gen) * 0.1).requires_grad_(True)
        for dn in a.dtype or ["bf16", "f32"]:
            f = (torch.randn((N, T, H), device=dev, generator=gen) * 0.5).to(tdt[dn]).requires_grad_(True)
            g = (torch.randn((N, U, H), device=dev, generator=gen) * 0.5).to(tdt[dn]).requires_grad_(True)
            leaves = (f, g, w, b)

            def fused():
                for x in leaves:
                    x.grad = None
                pruned_rnnt_loss_from_joint(f, g, w, b, ys, starts, xn, yn, s_range=S).sum().backward()

            def chain():
                for x in leaves:
                    x.grad = None
                fp, gp = prune_joint_inputs(f, g, starts, S)
                with torch.autocast("cuda", dtype=torch.bfloat16, enabled=dn == "bf16"):
                    z = torch.nn.functional.linear(torch.tanh(fp + gp), w, b)
                pruned_rnnt_loss_from_logits(z, ys, starts, xn, yn).sum().backward()

            if a.steps:
                for _ in range(a.steps):
                    fused()
                torch.cuda.synchronize()
                print(f"V={V} {dn}: {a.steps} steps done", flush=True)
                continue
            fused()
            gf = [x.grad.float().clone() for x in leaves]
            chain()
            close = max(float((x.grad.float() - y).norm() / y.norm()) for x, y in zip(leaves, gf))
            tf, tc = [], []
            for _ in range(a.repeats):
                tf.append(timed(torch, fused))
                tc.append(timed(torch, chain))
            mf, mc = peak_beyond_inputs(torch, fused, leaves), peak_beyond_inputs(torch, chain, leaves)
            p, c = statistics.median(tf), statistics.median(tc)
            logits = N * T * S * V * f.element_size()
            lines.append(f"V={V:5d} {dn:>4}: logits {logits / 1e6:7.1f} MB  fused {p:8.4f} ms [{min(tf):.4f} - {max(tf):.4f}] "
                         f"peak {mf / 1e6:7.1f} MB   chain {c:8.4f} ms [{min(tc):.4f} - {max(tc):.4f}] peak {mc / 1e6:7.1f} MB   "
                         f"chain / fused {c / p:5.2f}x   largest normwise gradient difference {close:.2e}")
            print(lines[-1], flush=True)
            del f, g
        torch.cuda.empty_cache()
    if not a.steps:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
