"""The pruned joiner's hidden activations without a GPU: the header against the table, the C entries' refusals, the Python
checks."""
import ctypes
import glob
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "warp_rnnt_amd_pruned_hidden.h"
INVALID, SUCCESS = 5, 0


def _lib():
    import warp_rnnt_amd
    from warp_rnnt_amd import _build
    _build.build()          # hipcc cross-compiles for gfx950 without a GPU; no-op when up to date
    return warp_rnnt_amd.load()


def test_header_declares_what_the_table_binds_and_the_version_did_not_move():
    from warp_rnnt_amd import _build, _lib as lib
    L = _lib()
    table = lib.PRUNED_HIDDEN_SYMBOLS
    assert lib.ADDITIVE_PRUNED_HIDDEN == ((table, HEADER),)
    declared = {}
    for path in glob.glob(os.path.join(ROOT, "include", "*.h")):
        with open(path) as f:
            declared[os.path.basename(path)] = set(re.findall(r"\b(rnnt_amd_\w+)\s*\(", f.read().split("#ifndef")[1]))
    assert declared[HEADER] == set(table) == {"rnnt_amd_pruned_hidden_workspace_size", "rnnt_amd_pruned_hidden",
                                              "rnnt_amd_pruned_hidden_backward"}
    for name, (res, args) in table.items():
        fn = getattr(L, name)
        assert fn.restype is res and list(fn.argtypes) == list(args)
    assert L.rnnt_amd_version() == lib.ABI_VERSION == 110
    assert "pruned_hidden.hip" in _build.SOURCES and any(os.path.basename(h) == HEADER for h in _build.HEADERS)
    # the names are this header's and this table's alone
    assert all(not (names & set(table)) for header, names in declared.items() if header != HEADER)
    others = [v for k, v in vars(lib).items() if k.endswith("SYMBOLS") and k != "PRUNED_HIDDEN_SYMBOLS"]
    assert len(others) >= 16 and all(not (set(t) & set(table)) for t in others)
    assert all(table is not t for family in lib.ADDITIVE for t in family)


def test_refusals_before_any_hip_call():
    """Made-up pointers and a null stream: every call is refused by a host-side check or is an empty batch."""
    L = _lib()
    p, odd, ws = ctypes.c_void_p(4096), ctypes.c_void_p(4104), ctypes.c_void_p(8192)

    def fwd(dtype=1, act=0, f=p, g=p, starts=p, xn=p, h=p, N=2, T=3, U=4, S=2, H=16):
        return L.rnnt_amd_pruned_hidden(None, dtype, act, f, g, starts, xn, h, N, T, U, S, H)

    def bwd(ws=ws, dtype=1, act=0, dh=p, h=p, starts=p, xn=p, df=p, dg=p, N=2, T=3, U=4, S=2, H=16):
        return L.rnnt_amd_pruned_hidden_backward(None, ws, dtype, act, dh, h, starts, xn, df, dg, N, T, U, S, H)

    shapes = [dict(H=0), dict(H=4), dict(H=12), dict(H=4104), dict(S=0), dict(U=0), dict(T=0), dict(N=-1),
              dict(N=2, T=1 << 20, S=1 << 13)]          # (the last: N*T*S >= 2^32, a product an empty batch does not reach)
    for call, refused in ((fwd, [dict(f=None), dict(g=None), dict(starts=None), dict(h=None), dict(f=odd), dict(g=odd),
                                 dict(h=odd), dict(starts=ctypes.c_void_p(4098)), dict(xn=ctypes.c_void_p(4098))]),
                          (bwd, [dict(dh=None), dict(h=None), dict(starts=None), dict(ws=None), dict(ws=odd), dict(dh=odd),
                                 dict(h=odd), dict(df=odd), dict(dg=odd), dict(xn=ctypes.c_void_p(4098))])):
        for kw in refused + shapes + [dict(dtype=3), dict(dtype=-1), dict(act=2), dict(act=-1)]:
            assert call(**kw) == INVALID, (call.__name__, kw)
            if "N" not in kw:                    # a refused argument is not answered as an empty batch
                assert call(N=0, **kw) == INVALID, (call.__name__, kw)
        assert call(N=0) == SUCCESS and call(N=0, xn=None) == SUCCESS and call(N=0, S=9, U=1, H=4096) == SUCCESS
    assert bwd(N=0, ws=None, dg=None) == SUCCESS and bwd(ws=None, df=None, dg=None) == SUCCESS
    size = L.rnnt_amd_pruned_hidden_workspace_size
    assert [size(2, 3, 4, 2, 16), size(16, 1500, 300, 5, 512)] == [256, 8 * 16 * 300]
    for kw in shapes:
        assert size(*({**dict(N=2, T=3, U=4, S=2, H=16), **kw}[k] for k in "NTUSH")) == 0, kw


def test_python_checks():
    from warp_rnnt_amd.pruned import pruned_joint_hidden
    f, g, starts = torch.zeros(2, 3, 16), torch.zeros(2, 4, 16), torch.zeros(2, 3, dtype=torch.int32)
    with pytest.raises(ValueError, match="H % 8 == 0, 8 <= H <= 4096"):
        pruned_joint_hidden(torch.zeros(2, 3, 12), torch.zeros(2, 4, 12), starts, s_range=2)
    with pytest.raises(ValueError, match="8 <= H <= 4096"):
        pruned_joint_hidden(torch.zeros(2, 3, 4104), torch.zeros(2, 4, 4104), starts, s_range=2)
    with pytest.raises(ValueError, match="activation must be one of"):
        pruned_joint_hidden(f, g, starts, s_range=2, activation="gelu")
    with pytest.raises(ValueError, match="needs s_range"):
        pruned_joint_hidden(f, g, starts)
    with pytest.raises(RuntimeError, match="f must be located in the CUDA"):
        pruned_joint_hidden(f, g, starts, s_range=2)
