#!/usr/bin/env python
"""ctc_loss_from_logits beside the torch chain it replaces, forward + backward, on the same logits.

    python tools/ctc_loss_rate.py [--out profiles/ctc_loss_rate.txt] [--trace]

Shapes: N=16, T=1500 with (L=300, V=500), (L=300, V=1025) and a BPE-like (L=80, V=500); ragged lengths (frames from T down
to 0.7 T, labels from L down to 0.7 L), every utterance feasible; logits in bf16 and fp32.  Per shape and dtype, ms per step
of forward + backward (reduction "sum", d/d logits out):
  hip     warp_rnnt_amd.ctc.ctc_loss_from_logits(logits, labels, xn, yn, reduction="sum") and autograd.grad
  chain   F.ctc_loss(torch.log_softmax(logits.float(), -1).transpose(0, 1), labels, xn, yn, reduction="sum") and autograd.grad
  copy    logits.clone(): the bandwidth yardstick (it reads and writes the logits once)
HIP events around 10 back-to-back steps, median of 5 rounds after 20 warm-up steps; the three interleaved --repeats times
(median and range: the range is the spread a difference has to exceed).  Peak memory beyond the inputs: torch's
max_memory_allocated over one step minus what was allocated before it (d/d logits is part of it).  --trace runs a few
steps of the first shape in bf16 and nothing else: the run to put under `rocprofv3 --kernel-trace --stats`."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

N, T = 16, 1500
SHAPES = ((300, 500), (300, 1025), (80, 500))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ctc_loss_rate.txt"))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--trace", action="store_true")
    a = ap.parse_args()
    import torch
    import torch.nn.functional as F
    from pruned_rate import timed
    from warp_rnnt_amd import _build
    from warp_rnnt_amd.ctc import ctc_loss_from_logits
    _build.ensure_built()
    dev = torch.device("cuda:0")
    props = torch.cuda.get_device_properties(0)
    lines = [f"# {props.name or 'device 0'} ({getattr(props, 'gcnArchName', '?')}); N={N} T={T}, ragged; ms per step of forward "
             f"+ backward, median of {a.repeats} interleaved repeats (each: median of 5 x 10 steps after 20 warm-up steps) "
             f"[min - max]; peak memory beyond the inputs, MB"]
    print(lines[0], flush=True)
    gen = torch.Generator(device=dev).manual_seed(T)
    for L, V in SHAPES:
        xn = torch.linspace(T, 0.7 * T, N).to(torch.int32).to(dev)
        yn = torch.linspace(L, 0.7 * L, N).to(torch.int32).to(dev)
        labels = torch.randint(1, V, (N, L), device=dev, generator=gen, dtype=torch.int32)
        for dn, dtype in (("bf16", torch.bfloat16), ("f32", torch.float32)):
            x = torch.randn((N, T, V), device=dev, generator=gen).to(dtype).requires_grad_(True)
            out = {}

            def hip():
                out["hip"] = torch.autograd.grad(ctc_loss_from_logits(x, labels, xn, yn, reduction="sum"), x)[0]

            def chain():
                lp = torch.log_softmax(x.float(), -1).transpose(0, 1)
                out["chain"] = torch.autograd.grad(F.ctc_loss(lp, labels, xn, yn, reduction="sum"), x)[0]

            def peak(fn):
                out.clear()
                torch.cuda.synchronize()
                torch.cuda.empty_cache()
                base = torch.cuda.memory_allocated()
                torch.cuda.reset_peak_memory_stats()
                fn()
                torch.cuda.synchronize()
                return torch.cuda.max_memory_allocated() - base

            if a.trace:
                for _ in range(5):
                    hip()
                torch.cuda.synchronize()
                return
            hip(), chain()
            close = float((out["hip"].float() - out["chain"].float()).abs().max())
            th, tc, tm = [], [], []
            for _ in range(a.repeats):
                th.append(timed(torch, hip))
                tc.append(timed(torch, chain))
                tm.append(timed(torch, lambda: x.detach().clone()))
            mh, mc = peak(hip), peak(chain)
            p, c, m = statistics.median(th), statistics.median(tc), statistics.median(tm)
            lines.append(f"L={L:<3} V={V:<4} {dn:>4}: logits {x.numel() * x.element_size() / 1e6:6.1f} MB  "
                         f"hip {p:7.4f} ms [{min(th):.4f} - {max(th):.4f}] peak {mh / 1e6:7.1f} MB   "
                         f"chain {c:7.4f} ms [{min(tc):.4f} - {max(tc):.4f}] peak {mc / 1e6:7.1f} MB   "
                         f"copy {m:7.4f} ms [{min(tm):.4f} - {max(tm):.4f}]   chain / hip {c / p:5.2f}x   "
                         f"max |d/d logits difference| {close:.2e}")
            print(lines[-1], flush=True)
            del x
            out.clear()
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fo:
        fo.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
