#!/usr/bin/env python
"""Error / bound of the lattice sweeps and the gradient kernel over the value range of their log-prob pairs: per profile,
shape and ragged setting of tests/test_gpu_lattice_values.py, the worst and the rms ratio (worst/rms) of alphas, betas and
gradients and the worst of the cost, against the fp64 reference under the derived bound of tests/lattice_values.py -- for
the C oracle and, when a GPU is present, for every kernel that serves the shape (the reference-named C entry, then the
native entry under each pin; a pin that runs a kernel already listed for the case is not repeated).  A figure above 1 is
outside the bound.  `x oracle` is the largest of the three rms figures over the oracle's (an oracle figure below 0.005
counted as 0.005).

    python tools/lattice_value_range.py [> profiles/lattice_value_range.txt]

Another build of the library: WARP_RNNT_AMD_LIB=<path>."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch

import lattice_values as lv

FLOOR = 0.005        # an oracle rms below this counts as this: the test's slack of 0.01 over its factor of 2


def row(case, who, r, o=None):
    cells = "".join(f"{r[k][0]:>8.3f}/{r[k][1]:<7.4f}" for k in ("alphas", "betas") if k in r)
    cells += f"{r['costs'][0]:>8.3f}" + f"{r['grads'][0]:>8.3f}/{r['grads'][1]:<7.4f}"
    factor = ""
    if o is not None:
        factor = f"{max(r[k][1] / max(o[k][1], FLOOR) for k in ('alphas', 'betas', 'grads')):>10.2f}"
    print(f"  {case:<34}{who:<32}{cells}{factor}")


def main():
    gpu = torch.cuda.is_available()
    if gpu:
        import test_gpu_lattice_values as tg
        from warp_rnnt_amd import _lib, debug
        print(f"# {os.path.relpath(_lib.lib_path(), ROOT)} on {torch.cuda.get_device_name(0)}, FastEmit {lv.LAMBDA}, seed {lv.SEED}")
    else:
        print("# no GPU: the C oracle only -- NOT measured on a GPU")
    print(f"# {'case':<34}{'who':<32}{'alphas':>16}{'betas':>16}{'cost':>8}{'gradients':>16}{'x oracle':>10}")
    worst, factor = (0.0, None), (0.0, None)
    for name in lv.PROFILES:
        for shape in lv.SHAPES:
            for ragged in (False, True):
                c = lv.case(name, shape, ragged)
                o = c["oracle_ratios"]
                case = f"{name} {'x'.join(map(str, shape))} {'ragged' if ragged else 'full'}"
                row(case, "C oracle", o)
                if not gpu:
                    continue
                legs = [("C entry", tg.c_entry(c["pairs"], c["xn"], c["yn"]))]
                xs, txn, tyn = tg._t(c["pairs"]), tg._t(c["xn"]), tg._t(c["yn"])
                for pin in tg.PINS:
                    with debug.lattice_kernel(pin):
                        legs.append((f"pin {pin}", tg.native(xs, txn, tyn)))
                seen = set()
                for who, got in legs:
                    if got["kernel"] in seen:
                        continue
                    seen.add(got["kernel"])
                    try:
                        r = tg.ratios_of(c, got, who)
                    except AssertionError as e:
                        print(f"  {case:<34}{who + ': ' + got['kernel']:<32}FAIL: {e}")
                        continue
                    row(case, who + ": " + got["kernel"], r, o)
                    w = max(v[0] for v in r.values())
                    f = max(r[k][1] / max(o[k][1], FLOOR) for k in ("alphas", "betas", "grads"))
                    if w > worst[0]:
                        worst = (w, f"{case}, {who}: {got['kernel']}")
                    if f > factor[0]:
                        factor = (f, f"{case}, {who}: {got['kernel']}")
    if gpu:
        print(f"# largest worst ratio on the GPU: {worst[0]:.3f} ({worst[1]})")
        print(f"# largest rms over the oracle's rms: {factor[0]:.2f} ({factor[1]})")


if __name__ == "__main__":
    main()
