"""One training step of a joint network plus the loss, three ways, at the GRID shapes of examples/joint_benchmark.py
(H=512) in fp32 and under bf16 autocast: time per step and peak HBM.

  gather : JointNetwork (log-softmax) -> rnnt_loss(gather=True)
  logits : JointNetwork (logits)      -> rnnt_loss_from_logits
  joint  : rnnt_loss_from_joint(f, g, weight, bias, ...)

--dropout P puts Dropout(P) between the activation and the projection of the `joint` way (inside its kernels, the seed
tensor refreshed in place every step as a training loop would); the other two ways have no such
stage and are not run then.

python tools/joint_fused_rate.py [--steps 10] [--warmup 3] [--shapes T,U,V ...] [--dropout P]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))

from joint_benchmark import GRID, JointNetwork, make_batch  # noqa: E402


def step_fn(way, joint, f, g, ys, xn, yn, dtype, dropout=0.0):
    from warp_rnnt import rnnt_loss
    from warp_rnnt_amd.fused import rnnt_loss_from_logits
    from warp_rnnt_amd.joint import rnnt_loss_from_joint

    seed = torch.zeros(1, dtype=torch.int64, device=f.device)

    def step():
        if dropout > 0:
            seed.add_(1)
        joint.zero_grad(set_to_none=True)
        f.grad = g.grad = None
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=dtype == "bf16"):
            if way == "gather":
                joint.normalise = True
                loss = rnnt_loss(joint(f, g).float(), ys, xn, yn, gather=True)
            elif way == "logits":
                joint.normalise = False
                loss = rnnt_loss_from_logits(joint(f, g), ys, xn, yn)
            else:
                loss = rnnt_loss_from_joint(f, g, joint.proj.weight, joint.proj.bias, ys, xn, yn, dropout=dropout,
                                            dropout_seed=seed if dropout > 0 else None)
        loss.sum().backward()
    return step


def measure(step, steps, warmup):
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        step()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps, (torch.cuda.max_memory_allocated() - base) / 1e9


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--steps", type=int, default=10)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--N", type=int, default=16)
    p.add_argument("--H", type=int, default=512)
    p.add_argument("--shapes", nargs="*")
    p.add_argument("--ways", default="gather,logits,joint")
    p.add_argument("--dropout", type=float, default=0.0)
    args = p.parse_args()
    if args.dropout > 0:
        args.ways = "joint"
    grid = GRID if not args.shapes else [tuple(int(v) for v in s.split(",")) for s in args.shapes]
    dev = torch.device("cuda:0")
    for (T, U, V) in grid:
        for dtype in ("fp32", "bf16"):
            for way in args.ways.split(","):
                torch.manual_seed(0)
                f, g, ys, xn, yn = make_batch(args.N, T, U, V, args.H, False, dev)
                f.requires_grad_(True)
                g.requires_grad_(True)
                if dtype == "bf16" and way == "joint":   # what an autocast encoder / predictor hands over
                    f = f.detach().to(torch.bfloat16).requires_grad_(True)
                    g = g.detach().to(torch.bfloat16).requires_grad_(True)
                joint = JointNetwork(args.H, V).to(dev)
                try:
                    ms, gb = measure(step_fn(way, joint, f, g, ys, xn, yn, dtype, args.dropout), args.steps,
                                     args.warmup)
                    rec = {"T": T, "U": U, "V": V, "N": args.N, "H": args.H, "dtype": dtype, "way": way,
                           "dropout": args.dropout, "ms_per_step": round(ms, 3), "peak_extra_GB": round(gb, 3)}
                except torch.cuda.OutOfMemoryError:
                    rec = {"T": T, "U": U, "V": V, "N": args.N, "H": args.H, "dtype": dtype, "way": way, "oom": True}
                print(json.dumps(rec), flush=True)
                del f, g, joint
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
