#!/usr/bin/env python
"""pruned_joint_hidden beside the torch chain it replaces, forward + backward, on the same inputs.

    python tools/pruned_hidden_rate.py [--out profiles/pruned_hidden_rate.txt]

Shape: N=16, T=1500, U=300, S=5, H=512, full lengths, the band a straight ramp from column 0 to column U-S, f and g in bf16
and fp32.  Per dtype, ms per call of forward + backward (dh given, df and dg out):
  hip     warp_rnnt_amd.pruned.pruned_joint_hidden(f, g, starts, xn, s_range=S) and autograd.grad
  chain   fp, gp = prune_joint_inputs(f, g, starts, S); tanh(fp + gp) and autograd.grad
HIP events around 10 back-to-back calls, median of 5 rounds after 20 warm-up calls; the two interleaved --repeats times
(median and range: the range is the spread a difference has to exceed).  Peak memory beyond the inputs: torch's
max_memory_allocated over one call minus what was allocated before it (h, df and dg are part of it).
Then each half of the HIP pair alone against a device-to-device copy that moves the bytes it has to move (a copy of B / 2
bytes reads and writes B in all): the forward writes h and reads f and g once, the backward reads dh and h and writes df
and dg."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

N, T, U, S, H = 16, 1500, 300, 5, 512


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pruned_hidden_rate.txt"))
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    import torch
    from pruned_rate import timed
    from warp_rnnt_amd import _build, ops
    from warp_rnnt_amd.pruned import prune_joint_inputs, pruned_joint_hidden
    _build.ensure_built()
    dev = torch.device("cuda:0")
    props = torch.cuda.get_device_properties(0)
    lines = [f"# {props.name or 'device 0'} ({getattr(props, 'gcnArchName', '?')}); N={N} T={T} U={U} S={S} H={H} tanh; ms per "
             f"call, median of {a.repeats} interleaved repeats (each: median of 5 x 10 calls after 20 warm-up calls) "
             f"[min - max]; peak memory beyond the inputs, MB"]
    print(lines[0], flush=True)
    gen = torch.Generator(device=dev).manual_seed(H)
    xn = torch.full((N,), T, dtype=torch.int32, device=dev)
    starts = (torch.arange(T, device=dev) * (U - S) // (T - 1)).to(torch.int32)[None, :].expand(N, T).contiguous()
    for dn, dtype in (("bf16", torch.bfloat16), ("f32", torch.float32)):
        f = torch.randn((N, T, H), device=dev, generator=gen).to(dtype).requires_grad_(True)
        g = torch.randn((N, U, H), device=dev, generator=gen).to(dtype).requires_grad_(True)
        dh = torch.randn((N, T, S, H), device=dev, generator=gen).to(dtype)
        out = {}

        def hip():
            h = pruned_joint_hidden(f, g, starts, xn, s_range=S)
            out["hip"] = (h,) + torch.autograd.grad(h, (f, g), dh)

        def chain():
            fp, gp = prune_joint_inputs(f, g, starts, S)
            h = torch.tanh(fp + gp)
            out["chain"] = (h,) + torch.autograd.grad(h, (f, g), dh)

        def peak(fn):
            out.clear()
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            fn()
            torch.cuda.synchronize()
            return torch.cuda.max_memory_allocated() - base

        hip(), chain()
        close = [float((x.detach().float() - y.detach().float()).abs().max()) for x, y in zip(out["hip"], out["chain"])]
        th, tc = [], []
        for _ in range(a.repeats):
            th.append(timed(torch, hip))
            tc.append(timed(torch, chain))
        mh, mc = peak(hip), peak(chain)
        hb = N * T * S * H * f.element_size()
        p, c = statistics.median(th), statistics.median(tc)
        lines.append(f"{dn:>4}: h {hb / 1e6:6.1f} MB  hip {p:7.4f} ms [{min(th):.4f} - {max(th):.4f}] peak {mh / 1e6:7.1f} MB   "
                     f"chain {c:7.4f} ms [{min(tc):.4f} - {max(tc):.4f}] peak {mc / 1e6:7.1f} MB   chain / hip {c / p:5.2f}x   "
                     f"max |difference| h {close[0]:.2e} df {close[1]:.2e} dg {close[2]:.2e}")
        print(lines[-1], flush=True)
        # each half alone against a copy of its bytes
        out.clear()
        fd, gd = f.detach(), g.detach()
        h = ops.pruned_hidden(fd, gd, starts, xn, S)
        small = (N * T * H + N * U * H) * f.element_size()
        for what, fn, moved in (("forward", lambda: ops.pruned_hidden(fd, gd, starts, xn, S), hb + small),
                                ("backward", lambda: ops.pruned_hidden_backward(dh, h, starts, xn, U), 2 * hb + small),
                                ("backward, df only", lambda: ops.pruned_hidden_backward(dh, h, starts, xn, U, need_g=False),
                                 2 * hb + N * T * H * f.element_size()),
                                ("backward, dg only", lambda: ops.pruned_hidden_backward(dh, h, starts, xn, U, need_f=False),
                                 2 * hb + N * U * H * f.element_size())):
            if what == "backward":
                moved_by_kernels = 4 * hb + small       # (dh and h are read once for df and once for dg)
            src = torch.empty((moved // 2,), dtype=torch.uint8, device=dev)
            dst = torch.empty_like(src)
            tk, tm = [], []
            for _ in range(a.repeats):
                tk.append(timed(torch, fn))
                tm.append(timed(torch, lambda: dst.copy_(src)))
            k, m = statistics.median(tk), statistics.median(tm)
            lines.append(f"{dn:>4}: {what:<18} {k:7.4f} ms [{min(tk):.4f} - {max(tk):.4f}]   copy moving its {moved / 1e6:6.1f} MB "
                         f"{m:7.4f} ms [{min(tm):.4f} - {max(tm):.4f}]   kernel / copy {k / m:5.2f}x" +
                         (f"   (the two kernels read {moved_by_kernels / 1e6:.1f} MB)" if what == "backward" else ""))
            print(lines[-1], flush=True)
            del src, dst
        del f, g, dh, h, fd, gd
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fo:
        fo.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
