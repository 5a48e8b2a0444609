#!/usr/bin/env python
"""Rate of the fused logits path for fp32, bf16 and fp16 logits at the BASELINE shapes (the shipped build).

    python tools/half_rate.py                    (every shape, every dtype)
    python tools/half_rate.py --shape c4 --dtype bf16 --steps 20     (one case, no table: what a profiler run wraps)

Per shape and dtype: ms per call of the forward (logits -> costs + diagonal-major gradient pairs: ops.loss with
IN_LOGITS_DENSE) and of the training step to d/d logits (that forward + ops.logits_backward), HIP events around 10
back-to-back calls, median of 5, after 20 warm-up calls; the dtypes interleaved --repeats times (median and range).
TB/s on the algorithmic bytes of the dtype (forward 2V+8 B/cell for half, 4V+8 for fp32; backward 4V+8 for half, 8V+8
for fp32; the step: their sum).  The bits of the half-precision
costs are those of the fp32 path on the upcast logits (tests/test_gpu_half.py); the table prints whether they match here."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (N, T, U, V) of BASELINE.md's configurations (c1's shape, one GPU)
SHAPES = {"c1": (1, 150, 40, 28), "c2": (16, 150, 40, 28), "c3": (32, 150, 20, 5000), "c4": (16, 1500, 300, 50)}
DTYPES = ("f32", "bf16", "f16")


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=sorted(SHAPES), action="append")
    ap.add_argument("--dtype", choices=DTYPES, action="append")
    ap.add_argument("--steps", type=int, default=0, help="run this many training steps of one case and exit (profiling)")
    ap.add_argument("--repeats", type=int, default=5, help="interleaved repeats of the dtypes per shape")
    a = ap.parse_args()
    import torch
    from warp_rnnt_amd import _build, ops
    _build.ensure_built()
    tdt = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
    dev = torch.device("cuda:0")
    props = torch.cuda.get_device_properties(0)
    print(f"# {props.name or 'device 0'} ({getattr(props, 'gcnArchName', '?')}); ms per call, median of {a.repeats} interleaved repeats "
          f"(each: median of 5 x 10 calls) [min - max]; TB/s on algorithmic bytes; ratio to f32 when f32 ran", flush=True)
    for name in a.shape or sorted(SHAPES):
        N, T, U, V = SHAPES[name]
        cells = N * T * U
        g = torch.Generator(device=dev).manual_seed(V)
        x32 = torch.randn((N, T, U, V), device=dev, generator=g)
        ys = torch.randint(1, V, (N, U - 1), dtype=torch.int32, device=dev, generator=g)
        xn = torch.full((N,), T, dtype=torch.int32, device=dev)
        yn = torch.full((N,), U - 1, dtype=torch.int32, device=dev)
        go = torch.ones((N,), device=dev)
        dts = a.dtype or list(DTYPES)
        xs = {dn: (x32.to(tdt[dn]) if dn != "f32" else x32) for dn in dts}

        def fwd(x):
            return ops.loss(x, ys, xn, yn, ops.IN_LOGITS_DENSE, ops.GRADS_GATHERED_DIAGONAL, 0, 0.0)

        def step(x):
            costs, pairs = fwd(x)
            return costs, ops.logits_backward(x, ys, pairs, go, 0)

        if a.steps:
            for dn in dts:
                for _ in range(a.steps):
                    step(xs[dn])
                torch.cuda.synchronize()
                print(f"{name} {dn}: {a.steps} steps done", flush=True)
            continue
        same = {}
        for dn in dts:
            c_up, _ = fwd(xs[dn].float() if dn != "f32" else x32)
            same[dn] = bool(torch.equal(fwd(xs[dn])[0], c_up))
        tf, ts = {dn: [] for dn in dts}, {dn: [] for dn in dts}
        for _ in range(a.repeats):          # the dtypes interleaved: drifts of the clock hit all of them alike
            for dn in dts:
                tf[dn].append(timed(torch, lambda: fwd(xs[dn])))
                ts[dn].append(timed(torch, lambda: step(xs[dn])))
        for dn in dts:
            eb = 4 if dn == "f32" else 2
            bf, bb = (eb * V + 8) * cells, (2 * eb * V + 8) * cells
            t_f, t_s = statistics.median(tf[dn]), statistics.median(ts[dn])
            rf = f", {t_f / statistics.median(tf['f32']):4.2f}x f32" if "f32" in dts else ""
            rs = f", {t_s / statistics.median(ts['f32']):4.2f}x f32" if "f32" in dts else ""
            print(f"{name} N={N:3d} T={T:4d} U={U:3d} V={V:5d} {dn:>4}:  forward {t_f:7.4f} ms "
                  f"[{min(tf[dn]):.4f} - {max(tf[dn]):.4f}] ({bf / t_f / 1e9:5.2f} TB/s{rf})  step {t_s:7.4f} ms "
                  f"[{min(ts[dn]):.4f} - {max(ts[dn]):.4f}] ({(bf + bb) / t_s / 1e9:5.2f} TB/s{rs})"
                  f"  costs == fp32 of upcast: {same[dn]}", flush=True)
        del xs, x32
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
