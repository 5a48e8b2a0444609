"""Which forward log-softmax kernel the library plans for a call, and in which shape (csrc/lsm_plan.h through
rnnt_amd_debug_lsm_plan: host only, no launch).  A wrong threshold is a silent loss of speed; a plan that differed between
the storage types would break the promise that half-precision logits give the bits of their fp32 upcast.

The table was derived by hand from the source of the commit before the planner existed (dispatch_lsm_map and
lsm_regs_rows_per_group of csrc/lsm.h, launch_log_softmax_backward of csrc/lsm_backward.hip), not from the code under test.
Unless a row says otherwise: 85 rows (N=1, T=17, U=5), the dense map, aligned tensors, no plane, fp32."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOB_VARIABLES = ("RNNT_LSM_NO_REGS", "RNNT_LSM_REGS_XCD", "RNNT_LSM_NO_LGR", "RNNT_LSM_NO_ROWS", "RNNT_LSM_NO_DIAG",
                  "RNNT_LSM_ROWS_ANY", "RNNT_LSM_NO_WP", "RNNT_LSM_WP_FUSED", "RNNT_LG_XCD", "RNNT_LG_XCD_FUSED",
                  "RNNT_LSMBWD_XCD", "RNNT_LSMBWD_SMALLEST_COVER")
NORM, GATHER, BWD, LSMBWD = "norm", "gather", "bwd", "log_softmax_backward"
DEFAULTS = dict(KR=0, L=0, Q=0, WP=False, TH=0, NV=0, grid_y=1, grid_z=1, lds=0, R=0, q=0, xcd=0, head_rows=0, tail=None)
INT_MAX = (1 << 31) - 1


def regs(KR, grid, head_rows, tail=None, xcd=1):
    return dict(family="regs", KR=KR, grid=grid, head_rows=head_rows, tail=tail, xcd=xcd)


def small(L, q, R, lds, grid, WP=False):
    return dict(family="small", L=L, q=q, R=R, lds=lds, grid=grid, WP=WP)


def rows_(L, Q, grid):
    return dict(family="rows", L=L, Q=Q, grid=grid)


def diag(Q, grid, grid_y=1, grid_z=1):
    return dict(family="rows_diag", L=8, Q=Q, grid=grid, grid_y=grid_y, grid_z=grid_z)


def lgr(TH, NV, grid=85):
    return dict(family="lgr", TH=TH, NV=NV, grid=grid)


def large(TH, NV, xcd, grid=None):
    return dict(family="large", TH=TH, NV=NV, xcd=xcd, grid=(88 if xcd else 85) if grid is None else grid)


def generic(grid=22):
    return dict(family="generic", grid=grid)


# (mode, V, other facts) -> the plan
TABLE = [
    # ---- plain log-softmax: the register kernel from V = 32 on where whole rows pack into 16-byte groups of <= 32 lanes
    (NORM, 3, {}, small(1, 3, 256, 3072, 8, WP=True)),
    (NORM, 28, {}, small(2, 14, 128, 14336, 8, WP=True)),
    (NORM, 31, {}, small(2, 16, 128, 15872, 8, WP=True)),
    (NORM, 32, {}, regs(4, 8, 84, tail="small")),
    (NORM, 32, dict(plane=True), regs(4, 8, 84, tail="small")),
    (NORM, 32, dict(rows=84), regs(4, 8, 84)),
    (NORM, 32, dict(rows=3), small(2, 16, 128, 16384, 8, WP=True)),           # fewer rows than a group
    (NORM, 33, {}, small(4, 9, 64, 8448, 8, WP=True)),
    (NORM, 50, {}, regs(2, 8, 84, tail="small")),
    (NORM, 50, dict(plane=True), regs(2, 8, 84, tail="small")),
    (NORM, 50, dict(rows=1), small(4, 13, 64, 12800, 8, WP=True)),
    (NORM, 50, dict(aligned=False), generic()),
    (NORM, 64, {}, regs(2, 8, 84, tail="small")),
    (NORM, 96, {}, regs(1, 8, 85)),
    (NORM, 100, {}, regs(1, 8, 85)),
    (NORM, 128, {}, regs(1, 8, 85)),
    # the register kernel's grid must stay below 2^31 (rounded up to the eight XCDs): else the LDS tiles
    (NORM, 128, dict(rows=(1 << 35) - 128), regs(1, (1 << 31) - 8, INT_MAX)),
    (NORM, 128, dict(rows=(1 << 35) - 112), small(8, 16, 32, 16384, 1 << 30, WP=True)),
    # 128 < V <= 1024: a row per small workgroup where >= 94 % of a cover's lanes are busy (one wave: >= 63 of 64)
    (NORM, 132, {}, small(16, 9, 16, 8448, 8, WP=True)),
    (NORM, 244, {}, small(16, 16, 16, 15616, 8, WP=True)),
    (NORM, 252, {}, lgr(64, 1)),
    (NORM, 256, {}, lgr(64, 1)),
    (NORM, 256, dict(rows=(1 << 22) + 1), lgr(64, 1, grid=1 << 22)),
    (NORM, 256, dict(rows=(1 << 22) - 1), lgr(64, 1, grid=(1 << 22) - 1)),
    (NORM, 256, dict(aligned=False), generic()),
    (NORM, 448, {}, small(32, 14, 8, 14336, 16)),
    (NORM, 484, {}, lgr(128, 1)),
    (NORM, 500, {}, lgr(128, 1)),
    (NORM, 512, {}, lgr(64, 2)),
    (NORM, 600, {}, small(64, 10, 4, 9600, 24)),
    (NORM, 768, {}, lgr(64, 3)),
    (NORM, 1000, {}, lgr(256, 1)),
    (NORM, 1024, {}, lgr(128, 2)),
    # 1024 < V <= 16384, V % 4 == 0: a row per workgroup; the three-pass covers keep the plain XCD order
    (NORM, 1028, {}, large(256, 2, 1)),
    (NORM, 1030, {}, generic()),
    (NORM, 2048, {}, large(256, 2, 1)),
    (NORM, 2052, {}, large(384, 2, 1)),
    (NORM, 3076, {}, large(512, 2, 1)),
    (NORM, 4096, {}, large(512, 2, 1)),
    (NORM, 4100, {}, large(512, 3, 1)),
    (NORM, 5000, {}, large(512, 3, 1)),
    (NORM, 5000, dict(rows=(1 << 22) - 1), large(512, 3, 1, grid=1 << 22)),
    (NORM, 5000, dict(rows=(1 << 22) + 1), large(512, 3, 1, grid=1 << 22)),
    (NORM, 5000, dict(aligned=False), generic()),
    (NORM, 5632, {}, large(512, 3, 1)),
    (NORM, 5636, {}, large(768, 2, 1)),
    (NORM, 6144, {}, large(768, 2, 1)),
    (NORM, 6148, {}, large(1024, 2, 1)),
    (NORM, 8192, {}, large(1024, 2, 1)),
    (NORM, 8196, {}, large(768, 3, 0)),
    (NORM, 10000, {}, large(896, 3, 0)),
    (NORM, 12288, {}, large(1024, 3, 0)),
    (NORM, 12292, {}, large(512, 8, 1)),
    (NORM, 16384, {}, large(512, 8, 1)),
    (NORM, 16388, {}, generic()),
    # ---- fused gather: L lanes per row for V = 32, 64, 128, 256 and every V % 4 == 0 from 448 on; along the diagonals
    #      for V = 32, 64 on the dense map from T = 16 on
    (GATHER, 3, {}, small(1, 3, 1024, 20480, 8)),
    (GATHER, 28, {}, small(2, 14, 128, 15360, 8)),
    (GATHER, 31, {}, small(2, 16, 128, 16896, 8)),
    (GATHER, 32, {}, diag(1, 5)),
    (GATHER, 32, dict(rows=80, T=16), diag(1, 4)),
    (GATHER, 32, dict(rows=75, T=15), rows_(8, 1, 8)),
    (GATHER, 32, dict(compact=True), rows_(8, 1, 8)),
    (GATHER, 32, dict(aligned=False), generic()),
    (GATHER, 32, dict(rows=3 * 40 * 33, T=40, U=33), diag(1, 10, 3, 3)),
    (GATHER, 32, dict(rows=65536 * 16, T=16, U=1), rows_(8, 1, 16384)),        # N = 65536: no grid z for it
    (GATHER, 32, dict(rows=65535 * 16, T=16, U=1), diag(1, 4, 1, 65535)),
    (GATHER, 33, {}, small(4, 9, 64, 8960, 8)),
    (GATHER, 50, {}, small(4, 13, 64, 13312, 8)),
    (GATHER, 64, {}, diag(2, 5)),
    (GATHER, 64, dict(rows=80, T=16), diag(2, 4)),
    (GATHER, 64, dict(rows=75, T=15), rows_(8, 2, 8)),
    (GATHER, 96, {}, small(8, 12, 32, 12544, 8)),
    (GATHER, 100, {}, small(8, 13, 32, 13056, 8)),
    (GATHER, 128, {}, rows_(8, 4, 8)),
    (GATHER, 132, {}, small(16, 9, 16, 8576, 8)),
    (GATHER, 244, {}, small(16, 16, 16, 15744, 8)),
    (GATHER, 256, {}, rows_(16, 4, 8)),
    (GATHER, 444, {}, small(32, 14, 8, 14272, 16)),
    (GATHER, 448, {}, rows_(32, 4, 16)),
    (GATHER, 484, {}, rows_(32, 4, 16)),
    (GATHER, 500, {}, rows_(32, 4, 16)),
    (GATHER, 600, {}, rows_(64, 3, 24)),
    (GATHER, 1000, {}, rows_(64, 4, 24)),
    (GATHER, 1024, {}, rows_(64, 4, 24)),
    (GATHER, 1024, dict(compact=True), rows_(64, 4, 24)),
    (GATHER, 1028, {}, large(256, 4, 0)),
    (GATHER, 1030, {}, generic()),
    (GATHER, 4096, {}, large(256, 4, 0)),
    (GATHER, 4100, {}, large(256, 8, 0)),
    (GATHER, 5000, {}, large(256, 8, 0)),
    (GATHER, 6148, {}, large(256, 8, 0)),
    (GATHER, 8192, {}, large(256, 8, 0)),
    (GATHER, 8196, {}, large(512, 8, 0)),
    (GATHER, 10000, {}, large(512, 8, 0)),
    (GATHER, 12288, {}, large(512, 8, 0)),
    (GATHER, 12292, {}, large(512, 8, 0)),
    (GATHER, 16384, {}, large(512, 8, 0)),
    (GATHER, 16384, dict(compact=True), large(512, 8, 0)),
    (GATHER, 16388, {}, generic()),
    # ---- fused d/d logits: tiles, a row per workgroup, generic -- nothing else
    (BWD, 3, {}, small(1, 3, 1024, 12288, 8)),
    (BWD, 32, {}, small(2, 16, 128, 16384, 8)),
    (BWD, 50, {}, small(4, 13, 64, 12800, 8)),
    (BWD, 50, dict(compact=True), small(4, 13, 64, 12800, 8)),
    (BWD, 50, dict(aligned=False), generic()),
    (BWD, 64, {}, small(4, 16, 64, 16384, 8)),
    (BWD, 256, {}, small(16, 16, 16, 16384, 8)),
    (BWD, 600, {}, small(64, 10, 4, 9600, 24)),
    (BWD, 1024, {}, small(64, 16, 4, 16384, 24)),
    (BWD, 1028, {}, large(256, 4, 0)),
    (BWD, 1030, {}, generic()),
    (BWD, 5000, {}, large(256, 8, 0)),
    (BWD, 10000, {}, large(512, 8, 0)),
    (BWD, 16384, {}, large(512, 8, 0)),
    (BWD, 16388, {}, generic()),
    # ---- the backward of the plain log-softmax (fp32): two tiles per workgroup; two or three passes per row
    (LSMBWD, 3, {}, small(1, 3, 1064, 25536, 8)),
    (LSMBWD, 50, {}, small(4, 13, 64, 25600, 8)),
    (LSMBWD, 50, dict(aligned=False), generic()),
    (LSMBWD, 1024, {}, small(64, 16, 4, 32768, 24)),
    (LSMBWD, 1028, {}, large(256, 2, 1)),
    (LSMBWD, 1030, {}, generic()),
    (LSMBWD, 5000, {}, large(640, 2, 1)),
    (LSMBWD, 6148, {}, large(896, 2, 1)),
    (LSMBWD, 8192, {}, large(1024, 2, 1)),
    (LSMBWD, 8196, {}, large(768, 3, 1)),
    (LSMBWD, 10000, {}, large(896, 3, 1)),
    (LSMBWD, 12288, {}, large(1024, 3, 1)),
    (LSMBWD, 12292, {}, large(512, 8, 1)),
    (LSMBWD, 16384, {}, large(512, 8, 1)),
    (LSMBWD, 16388, {}, generic()),
]

# half-precision logits: twice the rows per LDS tile in the fused gather (the same HBM bytes per tile), nothing else
HALF_GATHER_TILES = [
    (3, small(1, 3, 2048, 40960, 8)),
    (50, small(4, 13, 128, 26624, 8)),
    (96, small(8, 12, 64, 25088, 8)),
    (132, small(16, 9, 48, 25728, 8)),
]


def _facts(mode, V, other):
    return dict(dict(mode=mode, dtype="f32", rows=85, V=V, T=17, U=5, compact=False, aligned=True, plane=False), **other)


def _full(plan):
    return dict(DEFAULTS, **plan)


def test_the_plan_is_the_one_the_parent_commit_computed():
    from warp_rnnt_amd import debug
    assert not [v for v in KNOB_VARIABLES if v in os.environ], "the table holds for the default environment"
    wrong = []
    for mode, V, other, want in TABLE:
        got = debug.lsm_plan(**_facts(mode, V, other))
        if got != _full(want):
            wrong.append((mode, V, other, _full(want), got))
    assert not wrong, wrong
    for dtype in ("bf16", "f16"):
        for V, want in HALF_GATHER_TILES:
            assert debug.lsm_plan(**_facts(GATHER, V, dict(dtype=dtype))) == _full(want), (dtype, V)
    # every family the planner can name is reached
    assert {w["family"] for *_, w in TABLE} == set(debug.LSM_FAMILIES)
    L = debug.load()
    assert L.rnnt_amd_debug_lsm_plan(0, 0, 85, 50, 17, 5, 0, 1, 0, None, 0) == 0           # the family alone
    assert L.rnnt_amd_debug_lsm_plan(3, 0, 85, 5000, 1, 1, 0, 1, 0, None, 0) == 5
    for bad in ((-1, 0, 85, 50), (4, 0, 85, 50), (0, -1, 85, 50), (0, 3, 85, 50), (0, 0, -1, 50), (0, 0, 85, 0)):
        assert L.rnnt_amd_debug_lsm_plan(*bad, 17, 5, 0, 1, 0, None, 0) == -1, bad
    with pytest.raises(ValueError):
        debug.lsm_plan(NORM, "f32", -1, 50)


def test_a_vocabulary_takes_the_same_plan_at_every_storage_type():
    """the same kernel, lanes per row and reduction tree at every E -- only the rows per tile (and with them
    the LDS bytes and the grid) of the fused gather's LDS tiles may differ, where half doubles them."""
    from warp_rnnt_amd import debug
    for mode, V, other, _ in TABLE:
        f32 = debug.lsm_plan(**_facts(mode, V, other))
        for dtype in ("bf16", "f16"):
            half = debug.lsm_plan(**_facts(mode, V, dict(other, dtype=dtype)))
            if mode == GATHER and f32["family"] == "small":
                # (whole passes of the tile's 256 threads inside twice the budget: at least as many rows per tile)
                assert half["R"] >= f32["R"] and half["lds"] == half["R"] * (4 * V + 8), (V, other)
                half = dict(half, R=f32["R"], lds=f32["lds"], grid=f32["grid"])
            assert half == f32, (mode, V, other, dtype)


# knob -> (value, facts, what the plan becomes): each on a row of the table that it moves
KNOB_ROWS = [
    ("RNNT_LSM_NO_REGS", "1", (NORM, 50, {}), small(4, 13, 64, 12800, 8, WP=True)),
    ("RNNT_LSM_REGS_XCD", "0", (NORM, 50, {}), regs(2, 3, 84, tail="small", xcd=0)),
    ("RNNT_LSM_NO_LGR", "1", (NORM, 256, {}), small(16, 16, 16, 16384, 8, WP=True)),
    ("RNNT_LSM_NO_ROWS", "1", (GATHER, 128, {}), small(8, 16, 32, 16640, 8)),
    ("RNNT_LSM_NO_DIAG", "1", (GATHER, 32, {}), rows_(8, 1, 8)),
    ("RNNT_LSM_ROWS_ANY", "1", (GATHER, 96, {}), rows_(8, 3, 8)),
    ("RNNT_LSM_NO_WP", "1", (NORM, 28, {}), small(2, 14, 128, 14336, 8)),
    ("RNNT_LSM_WP_FUSED", "1", (GATHER, 28, {}), small(2, 14, 128, 15360, 8, WP=True)),
    ("RNNT_LG_XCD", "0", (NORM, 5000, {}), large(512, 3, 0)),
    ("RNNT_LG_XCD_FUSED", "1", (GATHER, 5000, {}), large(256, 8, 1)),
    ("RNNT_LSMBWD_XCD", "0", (LSMBWD, 5000, {}), large(640, 2, 0)),
    ("RNNT_LSMBWD_SMALLEST_COVER", "1", (LSMBWD, 5000, {}), large(256, 8, 1)),
]

CHILD = r'''
import json, sys
sys.path.insert(0, %r)
from warp_rnnt_amd import debug
print("PLANS " + json.dumps([debug.lsm_plan(**facts) for facts in json.loads(sys.argv[1])]))
'''


def _plans_in_child(env_extra, calls):
    env = {k: v for k, v in os.environ.items() if k not in KNOB_VARIABLES and k != "WARP_RNNT_AMD_LIB"}
    env.update(env_extra)
    out = subprocess.run([sys.executable, "-c", CHILD % ROOT, json.dumps(calls)], env=env, stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, timeout=300)
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    return json.loads(out.stdout.decode().split("PLANS ")[-1])


def test_the_knobs_reach_the_plan_of_the_ab_build_only():
    """The knobs are read once per process, so each setting gets a child.  The shipped library ignores all twelve variables;
    the `ab` build (-DRNNT_AB_KNOBS) honours each one on a row where it changes the plan, and leaves that row alone when
    the variable is not set."""
    from warp_rnnt_amd import _build
    assert [k for k, *_ in KNOB_ROWS] == list(KNOB_VARIABLES)
    calls = [_facts(*facts) for _, _, facts, _ in KNOB_ROWS]
    table = {(m, V, json.dumps(o, sort_keys=True)): w for m, V, o, w in TABLE}
    default = [_full(table[(m, V, json.dumps(o, sort_keys=True))]) for _, _, (m, V, o), _ in KNOB_ROWS]
    everything = {k: v for k, v, _, _ in KNOB_ROWS}
    assert _plans_in_child(everything, calls) == default
    ab = {"WARP_RNNT_AMD_LIB": _build.build(variant="ab")}
    assert _plans_in_child(ab, calls) == default
    for i, (knob, value, _, want) in enumerate(KNOB_ROWS):
        got = _plans_in_child(dict(ab, **{knob: value}), calls)
        assert got[i] == _full(want) != default[i], (knob, got[i])
