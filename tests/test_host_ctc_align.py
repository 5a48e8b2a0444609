"""The CTC best-path alignment without a GPU: the header against the table, the C entry's refusals, the Python checks."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "warp_rnnt_amd_ctc_align.h"
INVALID, SUCCESS = 5, 0


def _lib():
    import warp_rnnt_amd
    from warp_rnnt_amd import _build
    _build.build()          # hipcc cross-compiles for gfx950 without a GPU; no-op when up to date
    return warp_rnnt_amd.load()


def test_header_declares_what_the_table_binds_and_the_version_did_not_move():
    from warp_rnnt_amd import _build, _lib as lib
    L = _lib()
    table = lib.CTC_ALIGN_SYMBOLS
    assert lib.ADDITIVE_CTC_ALIGN == ((table, HEADER),)
    with open(os.path.join(ROOT, "include", HEADER)) as f:
        declared = set(re.findall(r"\b(rnnt_amd_\w+)\s*\(", f.read().split("#ifndef")[1]))
    assert declared == set(table) == {"rnnt_amd_ctc_align_workspace_size", "rnnt_amd_ctc_align"}
    for name, (res, args) in table.items():
        fn = getattr(L, name)
        assert fn.restype is res and list(fn.argtypes) == list(args)
    assert L.rnnt_amd_version() == lib.ABI_VERSION == 110
    assert "ctc_align.hip" in _build.SOURCES and "ctc_align.h" in _build.HEADERS
    assert any(os.path.basename(h) == HEADER for h in _build.HEADERS)
    others = [v for k, v in vars(lib).items() if k.endswith("SYMBOLS") and k != "CTC_ALIGN_SYMBOLS"]
    assert len(others) >= 18 and all(not (set(t) & set(table)) for t in others)
    assert all(table is not t for family in lib.ADDITIVE for t in family)


def test_refusals_before_any_hip_call():
    """Made-up pointers and a null stream: every call is refused by a host-side check or is an empty batch."""
    L = _lib()
    p, odd, ws = ctypes.c_void_p(4096), ctypes.c_void_p(4097), ctypes.c_void_p(8192)

    def call(ws=ws, kind=1, dtype=1, x=p, labels=p, xn=p, yn=p, scores=p, ft=p, ef=p, N=2, T=3, L_=4, V=16, blank=0):
        return L.rnnt_amd_ctc_align(None, ws, kind, dtype, x, labels, xn, yn, scores, ft, ef, N, T, L_, V, blank)

    shapes = [dict(L_=0), dict(L_=1024), dict(V=1), dict(V=16385), dict(T=0), dict(N=-1), dict(blank=16), dict(blank=-1),
              dict(N=2, T=1 << 20, L_=1023)]            # (the last: N*T*(L+1) = 2^31, a product an empty batch does not reach)
    off4 = ctypes.c_void_p(4098)
    pointers = [dict(ws=None), dict(ws=ctypes.c_void_p(4224)), dict(x=None), dict(labels=None), dict(xn=None), dict(yn=None),
                dict(scores=None), dict(ft=None), dict(ef=None), dict(x=odd), dict(labels=off4), dict(xn=off4),
                dict(yn=off4), dict(scores=off4), dict(ft=off4), dict(ef=off4)]
    for kw in pointers + shapes + [dict(dtype=3), dict(dtype=-1), dict(kind=2), dict(kind=-1)]:
        assert call(**kw) == INVALID, kw
        if "N" not in kw:                        # a refused argument is not answered as an empty batch
            assert call(N=0, **kw) == INVALID, kw
    for kind in (0, 1):
        assert call(N=0, kind=kind) == SUCCESS and call(N=0, kind=kind, L_=1023, V=16384, T=1 << 20) == SUCCESS
    assert call(dtype=0, x=off4) == INVALID and call(N=0, dtype=2, x=off4) == SUCCESS
    size = L.rnnt_amd_ctc_align_workspace_size
    assert size(2, 3, 4, 16) == 256 + 256 + 6 * 256           # 48 and 120 bytes; 6 rows of 64 words of 4 bytes
    up = lambda n: -(-n // 256) * 256
    assert size(16, 1500, 300, 500) == up(8 * 24000) + up(4 * 24000 * 301) + 24000 * 64 * 4
    assert size(1, 10, 512, 8) == up(80) + up(4 * 10 * 513) + 10 * 64 * 8        # 513 positions: 64-bit words
    for kw in shapes[:6] + shapes[8:]:
        assert size(*({**dict(N=2, T=3, L_=4, V=16), **kw}[k] for k in ("N", "T", "L_", "V"))) == 0, kw


def test_python_checks():
    from warp_rnnt_amd.ctc import ctc_align
    z, lab, n = torch.zeros(2, 3, 16), torch.zeros(2, 4, dtype=torch.int32), torch.ones(2, dtype=torch.int32)
    for bad, match in (((torch.zeros(2, 3, 1), lab, n, n), "2 <= V <= 16384"),
                       ((z, torch.zeros(2, 1024, dtype=torch.int32), n, n), "1 <= L <= 1023"),
                       ((torch.zeros(2, 1 << 20, 2), torch.zeros(2, 1023, dtype=torch.int32), n, n),
                        r"N\*T\*\(L\+1\) < 2\^31")):
        with pytest.raises(ValueError, match=match):
            ctc_align(*bad)
    with pytest.raises(ValueError, match="blank=16 is outside"):
        ctc_align(z, lab, n, n, blank=16)
    with pytest.raises(ValueError, match="kind must be one of"):
        ctc_align(z, lab, n, n, kind="probs")
    with pytest.raises(RuntimeError, match="logits must be a float32, bfloat16 or float16"):
        ctc_align(z.double(), lab, n, n, kind="log_probs")
    with pytest.raises(RuntimeError, match="labels must be a Int tensor"):
        ctc_align(z, lab.long(), n, n)
    with pytest.raises(RuntimeError, match="frames_lengths shape must be equal"):
        ctc_align(z, lab, torch.ones(3, dtype=torch.int32), n)
    with pytest.raises(RuntimeError, match="logits must be located in the CUDA"):
        ctc_align(z, lab, n, n, blank=-1)
