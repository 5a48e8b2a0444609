#!/usr/bin/env python
"""ms per call of tdt_align beside the no-grad TDT loss, in one process, alternating: under torch.no_grad(),
tdt_loss_from_logits(...) and tdt_align(...) on the same tensors -- logits -> costs and
logits -> (scores, emit_frames, emit_durations).  Both pay the same producer (tdt.hip's plane kernel); behind it the loss
runs its alpha sweep (log-sum-exp per cell), the alignment one max-plus sweep (add / compare per edge, a decision byte per
cell) and the trace.

    python tools/tdt_align_rate.py [--rounds R] [--out profiles/tdt_align_rate.txt]
    python tools/tdt_align_rate.py --only both-c4   (LEG-SHAPE, LEG = loss | align | both: ten calls in fp32, nothing
                                                     timed -- the command of a kernel trace)

Shapes: c4 (N=16, T=1500, U=300, V=50+5) in fp32 and bf16, c3 (N=32, T=150, U=20, V=5000+5) in fp32; durations
(0,1,2,3,4).  Per shape both legs are warmed up, then timed with device events in turn, R rounds (order reversed every
other round), every window at least half a second."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from warp_rnnt_amd.tdt import tdt_align, tdt_loss_from_logits  # noqa: E402

DURATIONS = (0, 1, 2, 3, 4)
SHAPES = (("c4", 16, 1500, 300, 50, "float32"), ("c4", 16, 1500, 300, 50, "bfloat16"), ("c3", 32, 150, 20, 5000, "float32"))
LEGS = (("loss", lambda x, ys, xn, yn: tdt_loss_from_logits(x, ys, xn, yn, durations=DURATIONS)),
        ("align", lambda x, ys, xn, yn: tdt_align(x, ys, xn, yn, durations=DURATIONS)))
WINDOW_MS = 500.0


def make(N, T, U, V, dtype, dev):
    g = torch.Generator(device=dev).manual_seed(V)
    x = torch.randn((N, T, U, V + len(DURATIONS)), device=dev, generator=g).to(getattr(torch, dtype))
    ys = torch.randint(1, V, (N, U - 1), dtype=torch.int32, device=dev, generator=g)
    xn = torch.full((N,), T, dtype=torch.int32, device=dev)
    yn = torch.full((N,), U - 1, dtype=torch.int32, device=dev)
    return x, ys, xn, yn


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
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "tdt_align_rate.txt"))
    p.add_argument("--only", default=None, help="LEG-SHAPE, e.g. both-c4: ten calls in fp32, nothing timed")
    a = p.parse_args()
    dev = torch.device("cuda:0")
    lines = []
    with torch.no_grad():
        for name, N, T, U, V, dtype in SHAPES:
            if a.only and (a.only.split("-")[1] != name or dtype != "float32"):
                continue
            x, ys, xn, yn = make(N, T, U, V, dtype, dev)
            steps = {leg: (lambda fn=fn: fn(x, ys, xn, yn)) for leg, fn in LEGS}
            if a.only:
                for leg, _ in LEGS:
                    if a.only.split("-")[0] in (leg, "both"):
                        for _ in range(10):
                            steps[leg]()
                torch.cuda.synchronize()
                continue
            count = {}
            for leg, _ in LEGS:                       # warm up, and size the window: at least WINDOW_MS
                timed(steps[leg], 10)
                count[leg] = max(10, int(WINDOW_MS / (timed(steps[leg], 10) / 10)) + 1)
            for r in range(a.rounds):
                for leg, _ in (LEGS if r % 2 == 0 else LEGS[::-1]):
                    ms = timed(steps[leg], count[leg])
                    lines.append(f"{name} N={N} T={T} U={U} V={V:5d}+{len(DURATIONS)} {dtype:8s} round {r + 1} {leg:8s} "
                                 f"{ms / count[leg]:8.4f} ms per call  ({count[leg]} calls in {ms:.0f} ms)")
                    print(lines[-1], flush=True)
            del x
    if lines:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
