#!/usr/bin/env python
"""One training step of the fused simple transducer loss beside the unfused chain on the same inputs.

    python tools/simple_rate.py [--out profiles/simple_loss_rate.txt]
    python tools/simple_rate.py --steps 20 --v 500 --dtype bf16          (steps of the fused loss only: what a kernel trace wraps)

Shape: N=16, T=1500, U=300, V=500 and 1025, am (N,T,V) and lm (N,U,V) in bf16 and fp32, full lengths, lm_only_scale = 0.25,
am_only_scale = 0.  Per case, ms per step (forward + backward to d/d am and d/d lm):
  fused    warp_rnnt_amd.simple.simple_rnnt_loss(...).sum().backward()
  chain    tests/simple_reference.py's pairs32 on the fp32 upcast (two exp, a bmm, log, gathers, a stack),
           warp_rnnt.rnnt_loss(pairs, ..., blank=-1).sum().backward() -- autograd back through all of it
HIP events around 10 back-to-back steps, median of 5 rounds after 20 warm-up steps; the two interleaved --repeats times
(median and range).  Peak memory beyond the inputs: torch's max_memory_allocated over one step minus what was allocated
before it, with no gradient of an earlier step alive (so d/d am and d/d lm are part of it).  The fused step's three
T x U x V products are 6 N T U V flop: the last column is that over the step's time, against the 157.3 TF of the f32 MFMA."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

N, T, U = 16, 1500, 300
SCALES = (0.25, 0.0)
F32_MFMA_TF = 157.3


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


def peak_beyond_inputs(torch, fn, leaves):
    fn()
    torch.cuda.synchronize()
    for x in leaves:
        x.grad = None             # (the step's own results count: d/d am and d/d lm are part of the peak)
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "simple_loss_rate.txt"))
    ap.add_argument("--v", type=int, action="append")
    ap.add_argument("--dtype", choices=("bf16", "f32"), action="append")
    ap.add_argument("--steps", type=int, default=0, help="run this many steps of the fused loss of one case and exit")
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    import torch
    import warp_rnnt
    import simple_reference as sr
    from warp_rnnt_amd import _build
    from warp_rnnt_amd.simple import simple_rnnt_loss
    _build.ensure_built()
    dev = torch.device("cuda:0")
    props = torch.cuda.get_device_properties(0)
    lines = [f"# {props.name or 'device 0'} ({getattr(props, 'gcnArchName', '?')}); N={N} T={T} U={U} scales {SCALES}; ms per "
             f"training step, median of {a.repeats} interleaved repeats (each: median of 5 x 10 steps after 20 warm-up steps) "
             f"[min - max]; peak memory beyond the inputs, MB; the fused step's 6 N T U V flop over its time"]
    print(lines[0], flush=True)
    tdt = {"f32": torch.float32, "bf16": torch.bfloat16}
    for V in a.v or [500, 1025]:
        g = torch.Generator(device=dev).manual_seed(V)
        am32 = torch.randn((N, T, V), device=dev, generator=g) * 2
        lm32 = torch.randn((N, U, V), device=dev, generator=g) * 2
        ys = torch.randint(1, V, (N, U - 1), dtype=torch.int32, device=dev, generator=g)
        xn = torch.full((N,), T, dtype=torch.int32, device=dev)
        yn = torch.full((N,), U - 1, dtype=torch.int32, device=dev)
        for dn in a.dtype or ["bf16", "f32"]:
            am = am32.to(tdt[dn]).requires_grad_(True)
            lm = lm32.to(tdt[dn]).requires_grad_(True)

            def fused():
                am.grad = lm.grad = None
                simple_rnnt_loss(am, lm, ys, xn, yn, lm_only_scale=SCALES[0], am_only_scale=SCALES[1]).sum().backward()

            def chain():
                am.grad = lm.grad = None
                pairs = sr.pairs32(am.float(), lm.float(), ys, 0, SCALES[0], SCALES[1]).contiguous()
                warp_rnnt.rnnt_loss(pairs, ys, xn, yn, blank=-1).sum().backward()

            if a.steps:
                for _ in range(a.steps):
                    fused()
                torch.cuda.synchronize()
                print(f"V={V} {dn}: {a.steps} steps done", flush=True)
                continue
            fused()
            ga, gl = am.grad.clone(), lm.grad.clone()
            chain()
            close = max(float((am.grad.float() - ga.float()).abs().max()), float((lm.grad.float() - gl.float()).abs().max()))
            tf, tc = [], []
            for _ in range(a.repeats):
                tf.append(timed(torch, fused))
                tc.append(timed(torch, chain))
            mf, mc = peak_beyond_inputs(torch, fused, (am, lm)), peak_beyond_inputs(torch, chain, (am, lm))
            f, c = statistics.median(tf), statistics.median(tc)
            tflops = 6.0 * N * T * U * V / (f * 1e-3) / 1e12
            lines.append(f"V={V:5d} {dn:>4}: inputs {(am.numel() + lm.numel()) * am.element_size() / 1e6:6.1f} MB  fused {f:7.4f} ms "
                         f"[{min(tf):.4f} - {max(tf):.4f}] peak {mf / 1e6:7.1f} MB   chain {c:7.4f} ms "
                         f"[{min(tc):.4f} - {max(tc):.4f}] peak {mc / 1e6:7.1f} MB   chain / fused {c / f:5.2f}x   "
                         f"max |gradient difference| {close:.2e}   fused GEMMs {tflops:5.1f} TF = "
                         f"{100 * tflops / F32_MFMA_TF:4.1f} % of the f32 MFMA rate")
            print(lines[-1], flush=True)
            del am, lm
        del am32, lm32
        torch.cuda.empty_cache()
    if not a.steps:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
