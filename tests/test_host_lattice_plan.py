"""Which lattice kernel the library plans for a call (csrc/lattice_plan.h through rnnt_amd_debug_lattice_plan: host only,
no launch).  The kernels give the same bits, so a wrong threshold is a silent loss of speed that no other test sees.

The table was derived by hand from the source of the commit before the planner existed (takes_ring_kernel, launch_lattice,
launch_lattice_wd, wd_block_diagonals and wl_max_blocks of csrc/lattice.hip and csrc/lattice_wd.hip), not from the code
under test.  Unless a row says otherwise: 256 compute units, the diagonal-major loader, flags and rings present, pin auto."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOB_VARIABLES = ("RNNT_DEBUG_LATTICE_KERNEL", "RNNT_WD_K16_FROM_T", "RNNT_WL_MAX_BLOCKS", "RNNT_NO_PREP_FOLD")

WD, WL, WS, SINGLE = "lattice_wd", "lattice_wl", "lattice_ws", "lattice (single role)"
BOTH = (True, False)          # folded or not: the row holds for either
NONE, OFFS32 = dict(flags=False, rings=False), dict(flags=False, rings=False, offs32=True)

# (N, T, U), folded, other facts, expected kernel, rings (wd only), block diagonals (wd only), clause
TABLE = [
    ((16, 150, 40), BOTH, {}, WD, False, 8, "lone"),
    ((16, 500, 64), BOTH, {}, WD, False, 16, "lone-k16"),
    ((256, 500, 40), BOTH, {}, WD, False, 8, "lone-k16-cus"),
    ((2, 1500, 17), BOTH, {}, WD, False, 16, "lone-k16"),
    ((16, 1500, 300), BOTH, {}, WD, True, 16, "from_t"),
    ((16, 350, 300), True, {}, WD, True, 8, "from_t-folded"),
    ((16, 350, 300), False, {}, WL, None, None, "from_t-unfolded"),
    ((32, 1000, 128), True, {}, WD, True, 8, "from_t-folded"),
    ((32, 1000, 128), False, {}, WL, None, None, "from_t-unfolded"),
    ((32, 899, 128), True, {}, WL, None, None, "from_t"),
    ((64, 1000, 200), BOTH, {}, WL, None, None, "from_t2"),
    ((64, 1500, 256), BOTH, {}, WD, True, 16, "from_t2"),
    ((64, 1399, 256), BOTH, {}, WL, None, None, "from_t2"),
    ((128, 1500, 300), BOTH, {}, WS, None, None, "wl-batch"),
    ((128, 300, 128), BOTH, {}, WL, None, None, "wl-two"),
    ((97, 500, 129), BOTH, {}, WS, None, None, "N=96"),
    ((96, 500, 129), BOTH, {}, WL, None, None, "N=96"),
    ((4, 200, 400), BOTH, {}, WD, True, 8, "six-up"),
    ((4, 100, 400), BOTH, {}, WS, None, None, "six-up"),
    ((2, 60, 700), BOTH, {}, WD, True, 8, "nA>8"),
    ((2, 60, 700), BOTH, NONE, SINGLE, None, None, "no-rings"),
    ((2, 60, 700), BOTH, dict(pin="ws"), SINGLE, None, None, "pin-ws"),
    ((16, 1500, 300), BOTH, NONE, WL, None, None, "no-rings"),
    ((16, 1500, 300), BOTH, OFFS32, WL, None, None, "offs32"),
    ((16, 1500, 300), BOTH, dict(offs32=True), WL, None, None, "offs32-with-rings"),
    ((16, 150, 40), BOTH, OFFS32, WD, False, 8, "lone-offs32"),
    ((16, 150, 40), BOTH, dict(pin="ws"), WS, None, None, "pin-ws"),
    ((16, 1500, 200), BOTH, dict(pin="wd", **NONE), WS, None, None, "pin-wd"),
    ((128, 500, 300), BOTH, dict(pin="wl"), WL, None, None, "pin-wl"),
    ((4, 500, 330), BOTH, dict(pin="wl"), WS, None, None, "pin-wl"),
    ((16, 1500, 300), BOTH, dict(cus=64), WL, None, None, "cus"),
    ((16, 1500, 300), BOTH, dict(loader="rowmajor"), SINGLE, None, None, "loader"),
    ((16, 1500, 300), BOTH, dict(loader="dense"), SINGLE, None, None, "loader"),
    # one step on either side of each from_t, folded (a CU for every workgroup: 2N * column blocks <= 256)
    ((32, 900, 128), True, {}, WD, True, 8, "from_t"),
    ((16, 639, 192), True, {}, WL, None, None, "from_t"),
    ((16, 640, 192), True, {}, WD, True, 8, "from_t"),
    ((16, 399, 256), True, {}, WL, None, None, "from_t"),
    ((16, 400, 256), True, {}, WD, True, 8, "from_t"),
    ((16, 319, 320), True, {}, WL, None, None, "from_t"),
    ((16, 320, 320), True, {}, WD, True, 8, "from_t"),
    ((8, 127, 384), BOTH, {}, WS, None, None, "from_t"),
    ((8, 128, 384), BOTH, {}, WD, True, 8, "from_t"),
    # ... and not folded
    ((32, 1199, 128), False, {}, WL, None, None, "from_t-unfolded"),
    ((32, 1200, 128), False, {}, WD, True, 16, "from_t-unfolded"),
    ((16, 1099, 192), False, {}, WL, None, None, "from_t-unfolded"),
    ((16, 1100, 192), False, {}, WD, True, 16, "from_t-unfolded"),
    ((16, 639, 256), False, {}, WL, None, None, "from_t-unfolded"),
    ((16, 640, 256), False, {}, WD, True, 8, "from_t-unfolded"),
    ((16, 399, 320), False, {}, WL, None, None, "from_t-unfolded"),
    ((16, 400, 320), False, {}, WD, True, 8, "from_t-unfolded"),
    # from_t2 (two workgroups per CU: 256 < 2N * column blocks <= 512): two and three column blocks never
    ((64, 1400, 256), BOTH, {}, WD, True, 16, "from_t2"),
    ((48, 799, 320), BOTH, {}, WL, None, None, "from_t2"),
    ((48, 800, 320), BOTH, {}, WD, True, 8, "from_t2"),
    ((40, 127, 384), BOTH, {}, WS, None, None, "from_t2"),
    ((40, 128, 384), BOTH, {}, WD, True, 8, "from_t2"),
    ((128, 3000, 128), BOTH, {}, WL, None, None, "from_t2-never"),
    ((64, 3000, 192), BOTH, {}, WL, None, None, "from_t2-never"),
    # the workgroup counts themselves: 2N * column blocks against 256 and 512
    ((64, 900, 128), True, {}, WD, True, 8, "cus"),
    ((65, 900, 128), True, {}, WL, None, None, "cus"),
    ((65, 1500, 256), BOTH, {}, WL, None, None, "2cus"),
    # one / two, five / six and eight / nine column blocks
    ((16, 150, 64), BOTH, {}, WD, False, 8, "nA=1"),
    ((16, 150, 65), BOTH, {}, WL, None, None, "nA=2"),
    ((16, 100, 320), BOTH, {}, WL, None, None, "nA=5"),
    ((16, 100, 321), BOTH, {}, WS, None, None, "nA=6"),
    ((4, 100, 512), BOTH, {}, WS, None, None, "nA=8"),
    ((4, 100, 513), BOTH, {}, WD, True, 8, "nA=9"),
    ((4, 100, 512), BOTH, NONE, WS, None, None, "nA=8"),
    ((4, 100, 513), BOTH, NONE, SINGLE, None, None, "nA=9"),
    # N = 96 / 97 beyond two column blocks; two column blocks at any batch
    ((96, 300, 320), BOTH, {}, WL, None, None, "N=96"),
    ((97, 300, 320), BOTH, {}, WS, None, None, "N=97"),
    ((300, 300, 128), BOTH, {}, WL, None, None, "wl-two"),
    # blocks of 16 diagonals: T = 1024, and T = 320 on one column block while 2N <= 256
    ((16, 1023, 300), BOTH, {}, WD, True, 8, "k16"),
    ((16, 1024, 300), BOTH, {}, WD, True, 16, "k16"),
    ((16, 319, 64), BOTH, {}, WD, False, 8, "lone-k16"),
    ((16, 320, 64), BOTH, {}, WD, False, 16, "lone-k16"),
    ((128, 500, 64), BOTH, {}, WD, False, 16, "lone-k16-cus"),
    ((129, 500, 64), BOTH, {}, WD, False, 8, "lone-k16-cus"),
    ((129, 1024, 64), BOTH, {}, WD, False, 16, "k16"),
]


def _rows():
    for shape, folded, other, kernel, rings, diagonals, clause in TABLE:
        for f in (folded if isinstance(folded, tuple) else (folded,)):
            yield shape, f, other, kernel, rings, diagonals, clause


def _wrong(plan_of):
    wrong = []
    for shape, folded, other, kernel, rings, diagonals, clause in _rows():
        kw = dict(dict(cus=256, pin="auto"), **other)
        got = plan_of(*shape, folded=folded, **kw)
        want = (kernel, diagonals, rings) if kernel == WD else (kernel,)
        if tuple(got[:len(want)]) != want:
            wrong.append((clause, shape, folded, other, want, tuple(got)))
    return wrong


def test_the_plan_is_the_one_the_parent_commit_computed():
    from warp_rnnt_amd import debug
    assert not [v for v in KNOB_VARIABLES if v in os.environ], "the table holds for the default environment"
    wrong = _wrong(debug.lattice_plan)
    assert not wrong, wrong
    # cus = 0: not given, answered as 256 without touching a device; pin = None: the process's current pin
    for shape in ((16, 1500, 300), (64, 1500, 256), (65, 1500, 256), (128, 500, 64)):
        assert debug.lattice_plan(*shape) == debug.lattice_plan(*shape, cus=256, pin="auto")
    with debug.lattice_kernel("ws"):
        assert debug.lattice_plan(16, 150, 40).kernel == WS and debug.lattice_plan(16, 150, 40, pin="auto").kernel == WD
    L = debug.load()
    assert L.rnnt_amd_debug_lattice_plan(0, 100, 100, 0, 3, 0, -1, 1) == -1
    assert L.rnnt_amd_debug_lattice_plan(16, 1500, 300, 0, 3, 256, 0, 1) == 2 | 16 << 8 | 1 << 16
    assert L.rnnt_amd_debug_lattice_plan(16, 150, 40, 0, 3, 256, 0, 1) == 2 | 8 << 8


CHILD = r'''
import json, sys
sys.path.insert(0, %r)
from warp_rnnt_amd import debug
print("PLANS " + json.dumps([list(debug.lattice_plan(*shape, folded=folded, **kw)) for shape, folded, kw in json.loads(sys.argv[1])]))
'''


def _plans_in_child(env_extra, calls):
    env = {k: v for k, v in os.environ.items() if k not in KNOB_VARIABLES and k != "WARP_RNNT_AMD_LIB"}
    env.update(env_extra)
    out = subprocess.run([sys.executable, "-c", CHILD % ROOT, json.dumps(calls)], env=env, stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, timeout=300)
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    return json.loads(out.stdout.decode().split("PLANS ")[-1])


def test_the_knobs_reach_the_plan():
    """RNNT_WD_K16_FROM_T=1 (read by the shipped library): blocks of 16 diagonals on every row, the kernels as in the
    table.  RNNT_WL_MAX_BLOCKS=0 (read by the `ab` build only, -DRNNT_AB_KNOBS): lattice_wl is never chosen, pinned or not --
    its rows go to lattice_ws -- and nothing else moves."""
    from warp_rnnt_amd import _build
    rows = list(_rows())
    calls = [(shape, folded, dict(dict(cus=256, pin="auto"), **other)) for shape, folded, other, *_ in rows]
    got = _plans_in_child({"RNNT_WD_K16_FROM_T": "1"}, calls)
    assert [g[0] for g in got] == [r[3] for r in rows]
    assert {g[1] for g in got} == {16}
    got = _plans_in_child({"RNNT_WL_MAX_BLOCKS": "0", "WARP_RNNT_AMD_LIB": _build.build(variant="ab")}, calls)
    assert WL in {r[3] for r in rows} and WL not in {g[0] for g in got}
    assert [g[0] for g in got] == [WS if r[3] == WL else r[3] for r in rows]
    assert [g[1:] for g, r in zip(got, rows) if r[3] == WD] == [[r[5], r[4]] for r in rows if r[3] == WD]
