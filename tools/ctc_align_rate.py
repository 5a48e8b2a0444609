#!/usr/bin/env python
"""ctc_align beside the no-grad ctc_loss_from_logits call on the same logits: the barrier-free max-plus sweep against the
loss's alpha sweep, whose kernels are the yardstick.

    python tools/ctc_align_rate.py [--out profiles/ctc_align_rate.txt] [--trace]

Shapes: N=16, T=1500, V=500 in bf16 with L=300 and a BPE-like L=80; ragged lengths (frames from T down to 0.7 T, labels from
L down to 0.7 L), every utterance feasible.  Per shape, ms per call:
  align   warp_rnnt_amd.ctc.ctc_align(logits, labels, xn, yn): k_ctc_emit, then sweep and walk back in one launch
  loss    warp_rnnt_amd.ctc.ctc_loss_from_logits(logits, labels, xn, yn, reduction="none") under no_grad: k_ctc_emit, then
          the alpha sweep
  copy    logits.clone(): the bandwidth yardstick
HIP events around 10 back-to-back calls, median of 5 rounds after 20 warm-up calls; the three interleaved --repeats times
(median and range: the range is the spread a difference has to exceed).  The split between the kernels is not in these
figures: --trace runs a few calls of both at every shape and nothing else, the run to put under
`rocprofv3 --kernel-trace --stats` (the sweep and the walk back share k_ctc_align's launch: the trace gives their sum)."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

N, T, V = 16, 1500, 500
LS = (300, 80)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ctc_align_rate.txt"))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--trace", action="store_true")
    a = ap.parse_args()
    import torch
    from pruned_rate import timed
    from warp_rnnt_amd import _build
    from warp_rnnt_amd.ctc import ctc_align, ctc_loss_from_logits
    _build.ensure_built()
    dev = torch.device("cuda:0")
    props = torch.cuda.get_device_properties(0)
    lines = [f"# {props.name or 'device 0'} ({getattr(props, 'gcnArchName', '?')}); N={N} T={T} V={V} bf16, ragged; ms per call, "
             f"median of {a.repeats} interleaved repeats (each: median of 5 x 10 calls after 20 warm-up calls) [min - max]"]
    print(lines[0], flush=True)
    gen = torch.Generator(device=dev).manual_seed(T)
    for L in LS:
        xn = torch.linspace(T, 0.7 * T, N).to(torch.int32).to(dev)
        yn = torch.linspace(L, 0.7 * L, N).to(torch.int32).to(dev)
        labels = torch.randint(1, V, (N, L), device=dev, generator=gen, dtype=torch.int32)
        x = torch.randn((N, T, V), device=dev, generator=gen).to(torch.bfloat16)
        out = {}

        def align():
            out["align"] = ctc_align(x, labels, xn, yn)

        def loss():
            with torch.no_grad():
                out["loss"] = ctc_loss_from_logits(x, labels, xn, yn, reduction="none")

        if a.trace:
            for _ in range(5):
                align(), loss()
            torch.cuda.synchronize()
            continue
        align(), loss()
        gap = float((out["align"][0] + out["loss"]).max())       # best path <= all paths: never above rounding
        ta, tl, tm = [], [], []
        for _ in range(a.repeats):
            ta.append(timed(torch, align))
            tl.append(timed(torch, loss))
            tm.append(timed(torch, lambda: x.clone()))
        p, c, m = statistics.median(ta), statistics.median(tl), statistics.median(tm)
        lines.append(f"L={L:<3}: align {p:7.4f} ms [{min(ta):.4f} - {max(ta):.4f}]   loss (no grad) {c:7.4f} ms "
                     f"[{min(tl):.4f} - {max(tl):.4f}]   copy {m:7.4f} ms [{min(tm):.4f} - {max(tm):.4f}]   "
                     f"align / loss {p / c:5.2f}   max(score + cost) {gap:.2e}")
        print(lines[-1], flush=True)
    if a.trace:
        return
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fo:
        fo.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
