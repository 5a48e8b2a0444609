#!/usr/bin/env python
"""A/B of two builds of the library on the fused log-softmax kernel families (csrc/lsm.h), op by op, the way
tools/ab_kernels.py does it: one process per build and round, interleaved, us per call (HIP events around 10 calls, median of
5, after a warm-up load).

    python tools/lsm_ab.py parent=/path/lib.so new=/path/lib.so [--rounds 3]

The first build named is the yardstick: an op counts as unchanged when the other build's median over the rounds lies inside
the first build's own minimum ... maximum.  Ops: the c4 tensor (N=16, T=1500, U=300, V=50) dense and as ragged packed rows,
forward, backward and clamped backward; one V per family (LDS tiles 600, rows in registers 128, a row per workgroup 5000,
generic 1030), the row-per-workgroup kernels also on packed rows, fp32 and bf16."""
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def child():
    import numpy as np
    import torch
    from warp_rnnt_amd import ops
    dev = torch.device("cuda:0")

    def timed(fn):
        for _ in range(10):
            fn()
        ts = []
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(10):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) / 10)
        return statistics.median(ts)

    spin = torch.empty(64 << 20, device=dev)
    for _ in range(600):
        spin.mul_(1.0)
    torch.cuda.synchronize()
    del spin
    g = torch.Generator(device=dev).manual_seed(3)
    res = {}

    def dense(tag, N, T, U, V, dtype=torch.float32, clamp=True):
        x = torch.randn((N, T, U, V), device=dev, generator=g).to(dtype)
        ys = torch.randint(1, V, (N, U - 1), dtype=torch.int32, device=dev, generator=g)
        xn = torch.full((N,), T, dtype=torch.int32, device=dev)
        yn = torch.full((N,), U - 1, dtype=torch.int32, device=dev)
        res[tag + " fused forward"] = timed(lambda: ops.loss(x, ys, xn, yn, ops.IN_LOGITS_DENSE, ops.GRADS_GATHERED_DIAGONAL))
        _, grads = ops.loss(x, ys, xn, yn, ops.IN_LOGITS_DENSE, ops.GRADS_GATHERED_DIAGONAL)
        go = torch.ones((N,), device=dev)
        out = torch.empty_like(x)
        res[tag + " fused backward"] = timed(lambda: ops.logits_backward(x, ys, grads, go, 0, out=out))
        if clamp:
            res[tag + " fused backward clamp=1"] = timed(lambda: ops.logits_backward(x, ys, grads, go, 0, out=out, clamp=1.0))

    def compact(tag, N, T, U, V, dtype=torch.float32):
        rng = np.random.RandomState(0)
        xn = rng.randint(T // 2, T + 1, size=N).astype(np.int32)
        yn = rng.randint(U // 2, U, size=N).astype(np.int32)
        xn[0], yn[0] = T, U - 1
        x = torch.randn((int((xn * (yn + 1)).sum()), V), device=dev, generator=g).to(dtype)
        ys = torch.tensor(rng.randint(1, V, size=int(yn.sum())).astype(np.int32), device=dev)
        txn, tyn = torch.tensor(xn, device=dev), torch.tensor(yn, device=dev)
        res[tag + " compact fused forward"] = timed(lambda: ops.loss_compact_logits(x, ys, txn, tyn, max_frames=T, max_labels=U - 1))
        _, grads, offs, loffs = ops.loss_compact_logits(x, ys, txn, tyn)
        go = torch.ones((N,), device=dev)
        out = torch.empty_like(x)
        res[tag + " compact fused backward"] = timed(lambda: ops.compact_logits_backward(x, ys, txn, tyn, offs, loffs, grads, go, out=out))
        res[tag + " compact fused backward clamp=1"] = timed(
            lambda: ops.compact_logits_backward(x, ys, txn, tyn, offs, loffs, grads, go, out=out, clamp=1.0))

    def norm(V, rows):
        x = torch.randn((rows, V), device=dev, generator=g)
        out = torch.empty_like(x)
        res["log_softmax V=%d" % V] = timed(lambda: ops.log_softmax(x, out=out))

    dense("c4 V=50", 16, 1500, 300, 50)
    dense("c4 V=50 bf16", 16, 1500, 300, 50, torch.bfloat16, clamp=False)
    compact("c4 V=50", 16, 1500, 300, 50)
    norm(50, 16 * 1500 * 300)                 # (the register kernel, which no change to the families touches: a sanity line)
    norm(600, 600000)
    norm(5000, 96000)
    norm(1030, 300000)
    dense("V=128", 32, 500, 100, 128, clamp=False)
    dense("V=600", 32, 500, 100, 600, clamp=False)
    dense("V=5000", 32, 150, 20, 5000)
    compact("V=5000", 32, 150, 40, 5000)
    compact("V=4096 bf16", 32, 150, 40, 4096, torch.bfloat16)
    for k, v in res.items():
        print(f"{k}\t{v * 1e3:.1f}", flush=True)


def main():
    args = sys.argv[1:]
    rounds = 3
    if "--rounds" in args:
        i = args.index("--rounds"); rounds = int(args[i + 1]); del args[i:i + 2]
    libs = [a.split("=", 1) for a in args]
    table = {}
    for r in range(rounds):
        for name, path in libs:
            env = dict(os.environ, WARP_RNNT_AMD_LIB=os.path.abspath(path), WARP_RNNT_AMD_NO_NATIVE_BINDING="1")
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, capture_output=True,
                                 text=True, timeout=240)
            if out.returncode != 0:
                print(out.stderr[-2000:])
                sys.exit(1)                      # (nothing more is started behind a process that failed)
            for line in out.stdout.splitlines():
                if "\t" in line:
                    k, v = line.split("\t")
                    table.setdefault(k, {}).setdefault(name, []).append(float(v))
            print("round %d %s done" % (r, name), file=sys.stderr, flush=True)
    (base, _), (other, _) = libs
    print(f"{'op (us per call; every round, then the median)':44s}{base:>26s}{other:>26s}   {other} median in {base}'s range")
    for k, row in table.items():
        a, b = row[base], row[other]
        verdict = "yes" if min(a) <= statistics.median(b) <= max(a) else "NO"
        print(f"{k:44s}" + "".join(f"{' '.join('%.0f' % v for v in row[n]):>18s} {statistics.median(row[n]):7.1f}" for n in (base, other))
              + "   " + verdict)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child()
    else:
        main()
