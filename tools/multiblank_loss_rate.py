#!/usr/bin/env python
"""ms per call of the multi-blank loss beside the TDT loss and the standard fused loss on logits of the same bytes, in one
process, alternating.

    python tools/multiblank_loss_rate.py [--rounds R] [--out profiles/multiblank_loss_rate.txt]
    python tools/multiblank_loss_rate.py --only c4  (ten calls of every leg at that shape in fp32, nothing timed -- the
                                                     command of a kernel trace)

Shapes: c4 (N=16, T=1500, U=300, V=50+3) and c3 (N=32, T=150, U=20, V=5000+3), in fp32 and bf16.  Legs: the multi-blank
training step (multiblank_loss_from_logits(...).sum().backward()) with big blanks (2, 4, 8) and its no-grad call, the TDT
training step with D = 5 durations (0..4) on the same tensor (V+3 = (V-2)+5 columns: the same bytes), the standard training
step of rnnt_loss_from_logits on it.  Per shape every leg is warmed up, then the legs are timed with device events in turn,
R rounds (order reversed every other round), every window at least half a second."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from warp_rnnt_amd.fused import rnnt_loss_from_logits  # noqa: E402
from warp_rnnt_amd.multiblank import multiblank_loss_from_logits  # noqa: E402
from warp_rnnt_amd.tdt import tdt_loss_from_logits  # noqa: E402

BIG_BLANKS = (2, 4, 8)
TDT_DURATIONS = (0, 1, 2, 3, 4)
SHAPES = (("c4", 16, 1500, 300, 50, "float32"), ("c4", 16, 1500, 300, 50, "bfloat16"),
          ("c3", 32, 150, 20, 5000, "float32"), ("c3", 32, 150, 20, 5000, "bfloat16"))
WINDOW_MS = 500.0


def make(N, T, U, V, dtype, dev):
    """Logits of V + 3 columns; labels in [1, V-2): no blank of any leg (0: TDT's and the standard loss's; the last four
    columns: the multi-blank set, NeMo's layout)."""
    g = torch.Generator(device=dev).manual_seed(V)
    x = torch.randn((N, T, U, V + len(BIG_BLANKS)), device=dev, generator=g).to(getattr(torch, dtype)).requires_grad_(True)
    ys = torch.randint(1, V - 2, (N, U - 1), dtype=torch.int32, device=dev, generator=g)
    xn = torch.full((N,), T, dtype=torch.int32, device=dev)
    yn = torch.full((N,), U - 1, dtype=torch.int32, device=dev)
    return x, ys, xn, yn


def legs(x, ys, xn, yn):
    def train(fn, **kw):
        def step():
            x.grad = None
            fn(x, ys, xn, yn, reduction="sum", **kw).backward()
        return step

    def infer(fn, **kw):
        def step():
            with torch.no_grad():
                fn(x, ys, xn, yn, reduction="sum", **kw)
        return step

    mb = dict(big_blank_durations=BIG_BLANKS, blank=x.size(3) - 1)
    return (("multiblank-step", train(multiblank_loss_from_logits, **mb)),
            ("multiblank-nograd", infer(multiblank_loss_from_logits, **mb)),
            ("tdt-step", train(tdt_loss_from_logits, durations=TDT_DURATIONS)),
            ("standard-step", train(rnnt_loss_from_logits)))


def timed(step, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        step()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


if __name__ == "__main__":
    p = argparse.ArgumentParser()
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "multiblank_loss_rate.txt"))
    p.add_argument("--only", default=None, help="a shape's name, e.g. c4: ten calls of every leg in fp32, nothing timed")
    a = p.parse_args()
    dev = torch.device("cuda:0")
    lines = []
    for name, N, T, U, V, dtype in SHAPES:
        if a.only and (a.only != name or dtype != "float32"):
            continue
        x, ys, xn, yn = make(N, T, U, V, dtype, dev)
        steps = legs(x, ys, xn, yn)
        if a.only:
            for _, step in steps:
                for _ in range(10):
                    step()
            torch.cuda.synchronize()
            continue
        count = {}
        for leg, step in steps:                       # warm up, and size the window: at least WINDOW_MS
            timed(step, 5)
            count[leg] = max(5, int(WINDOW_MS / (timed(step, 5) / 5)) + 1)
        for r in range(a.rounds):
            for leg, step in (steps if r % 2 == 0 else steps[::-1]):
                ms = timed(step, count[leg])
                lines.append(f"{name} N={N} T={T} U={U} V={V:5d}+{len(BIG_BLANKS)} {dtype:8s} round {r + 1} {leg:17s} "
                             f"{ms / count[leg]:8.4f} ms per call  ({count[leg]} calls in {ms:.0f} ms)")
                print(lines[-1], flush=True)
        del x
    if lines:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
