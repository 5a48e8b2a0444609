#!/usr/bin/env python
"""ms per call of pruned_rnnt_align beside the no-grad pruned loss, in one process, alternating: under torch.no_grad(),
pruned_rnnt_loss_from_logits(...) and pruned_rnnt_align(...) on the same tensors -- band logits -> costs and band logits ->
(scores, emit_frames).  Both pay a producer with the same row arithmetic; behind it the loss fills the (N,T,U) floor and
runs its sweeps over T + U - 1 diagonals, the alignment runs T frame steps of one wave per utterance and walks back.

    python tools/pruned_align_rate.py [--rounds R] [--out profiles/pruned_align_rate.txt]
    python tools/pruned_align_rate.py --only both-500   (LEG-V, LEG = loss | align | both: ten calls in fp32, nothing
                                                         timed -- the command of a kernel trace)

Shapes: N=16, T=1500, U=300, S=5, V in {500, 1025}, bf16 and fp32, full lengths, the band a straight ramp.  Per shape both
legs are warmed up, then timed with device events in turn, R rounds (order reversed every other round), every window at
least half a second.  The workspace bytes of the call stand beside the dense align's."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import warp_rnnt_amd  # noqa: E402
from warp_rnnt_amd.pruned import pruned_rnnt_align, pruned_rnnt_loss_from_logits  # noqa: E402

N, T, U, S = 16, 1500, 300, 5
SHAPES = tuple((V, dtype) for V in (500, 1025) for dtype in ("bfloat16", "float32"))
LEGS = (("loss", pruned_rnnt_loss_from_logits), ("align", pruned_rnnt_align))
WINDOW_MS = 500.0


def make(V, dtype, dev):
    g = torch.Generator(device=dev).manual_seed(V)
    x = torch.randn((N, T, S, V), device=dev, generator=g).to(getattr(torch, dtype))
    ys = torch.randint(1, V, (N, U - 1), dtype=torch.int32, device=dev, generator=g)
    xn = torch.full((N,), T, dtype=torch.int32, device=dev)
    yn = torch.full((N,), U - 1, dtype=torch.int32, device=dev)
    ramp = (torch.arange(T, device=dev) * (U - S)) // (T - 1)          # 0 .. U - S: steps of 0 and 1
    return x, ys, ramp.to(torch.int32).expand(N, T).contiguous(), xn, yn


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
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "pruned_align_rate.txt"))
    p.add_argument("--only", default=None, help="LEG-V, e.g. both-500: ten calls in fp32, nothing timed")
    a = p.parse_args()
    dev = torch.device("cuda:0")
    L = warp_rnnt_amd.load()
    lines = [f"workspace bytes at N={N} T={T} U={U} S={S}: pruned align {L.rnnt_amd_pruned_align_workspace_size(N, T, S, 0)}, "
             f"dense align {L.rnnt_amd_align_workspace_size(N, T, U)}"]
    with torch.no_grad():
        for V, dtype in SHAPES:
            if a.only and (a.only.split("-")[1] != str(V) or dtype != "float32"):
                continue
            args = make(V, dtype, dev)
            steps = {leg: (lambda fn=fn: fn(*args)) for leg, fn in LEGS}
            if a.only:
                for leg, _ in LEGS:
                    if a.only.split("-")[0] in (leg, "both"):
                        for _ in range(10):
                            steps[leg]()
                torch.cuda.synchronize()
                continue
            assert torch.isfinite(steps["align"]()[0]).all() and torch.isfinite(steps["loss"]()).all()
            count = {}
            for leg, _ in LEGS:                       # warm up, and size the window: at least WINDOW_MS
                timed(steps[leg], 10)
                count[leg] = max(10, int(WINDOW_MS / (timed(steps[leg], 10) / 10)) + 1)
            for r in range(a.rounds):
                for leg, _ in (LEGS if r % 2 == 0 else LEGS[::-1]):
                    ms = timed(steps[leg], count[leg])
                    lines.append(f"N={N} T={T} U={U} S={S} V={V:5d} {dtype:8s} round {r + 1} {leg:6s} "
                                 f"{ms / count[leg]:8.4f} ms per call  ({count[leg]} calls in {ms:.0f} ms)")
                    print(lines[-1], flush=True)
            del args, steps
    if not a.only:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
