"""prune_ranges_hip without a GPU: the additive contract of include/warp_rnnt_amd_prune_ranges.h and its table, the C
entry's refusals with pointers that are never dereferenced, and the front end's argument errors."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "warp_rnnt_amd_prune_ranges.h"
INVALID, SUCCESS = 5, 0


def _lib():
    import warp_rnnt_amd
    from warp_rnnt_amd import _build
    _build.build()          # hipcc cross-compiles for gfx950 without a GPU; no-op when up to date
    return warp_rnnt_amd.load()


def test_header_declares_what_the_table_binds_and_the_version_did_not_move():
    from warp_rnnt_amd import _build, _lib as lib
    L = _lib()
    table = lib.PRUNE_RANGES_SYMBOLS
    assert lib.ADDITIVE_PRUNE_RANGES == ((table, HEADER),)
    with open(os.path.join(ROOT, "include", HEADER)) as f:
        declared = set(re.findall(r"\b(rnnt_amd_\w+)\s*\(", f.read().split("#ifndef")[1]))
    assert declared == set(table) == {"rnnt_amd_prune_ranges"}
    for name, (res, args) in table.items():
        fn = getattr(L, name)
        assert fn.restype is res and list(fn.argtypes) == list(args)
    assert L.rnnt_amd_version() == lib.ABI_VERSION == 110
    assert "prune_ranges.hip" in _build.SOURCES and any(os.path.basename(h) == HEADER for h in _build.HEADERS)
    assert len(lib.ADDITIVE) == 5 and lib.ADDITIVE_PRUNED_JOINT == ((lib.PRUNED_JOINT_SYMBOLS, "warp_rnnt_amd_pruned_joint.h"),)
    assert lib.ADDITIVE_TOPOLOGY == ((lib.TOPOLOGY_SYMBOLS, "warp_rnnt_amd_topology.h"),) and len(lib.PRUNED_SYMBOLS) == 2


def test_refusals_before_any_hip_call():
    L = _lib()
    p, odd = ctypes.c_void_p(256), ctypes.c_void_p(260)

    def call(pairs=p, pitch=None, xn=p, yn=p, starts=p, N=2, T=3, U=6, S=2):
        return L.rnnt_amd_prune_ranges(None, pairs, T * U if pitch is None else pitch, xn, yn, starts, N, T, U, S)

    for kw in (dict(pairs=None), dict(xn=None), dict(yn=None), dict(starts=None), dict(pairs=odd), dict(T=0), dict(U=0),
               dict(S=1), dict(S=7), dict(pitch=17), dict(U=4097, S=5), dict(N=-1), dict(N=70000), dict(T=1 << 20, U=1 << 10)):
        assert call(**kw) == INVALID, kw
    assert call(N=0) == SUCCESS


def test_front_end_argument_errors():
    from warp_rnnt_amd.pruned import prune_ranges_hip
    g, xn, yn = torch.zeros(2, 4, 6, 2), torch.tensor([4, 3], dtype=torch.int32), torch.tensor([5, 2], dtype=torch.int32)
    with pytest.raises(ValueError, match="s_range must be >= 2"):
        prune_ranges_hip(g, xn, yn, 1)
    with pytest.raises(RuntimeError, match="pair_grads must be located in the CUDA"):
        prune_ranges_hip(g, xn, yn, 3)
    with pytest.raises(RuntimeError, match="pair_grads must be a float32 tensor"):
        prune_ranges_hip(g.double(), xn, yn, 3)
