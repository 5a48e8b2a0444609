"""The CTC loss without a GPU: the header against the table, the C entries' refusals, the Python checks."""
import ctypes
import glob
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "warp_rnnt_amd_ctc.h"
INVALID, SUCCESS = 5, 0


def _lib():
    import warp_rnnt_amd
    from warp_rnnt_amd import _build
    _build.build()          # hipcc cross-compiles for gfx950 without a GPU; no-op when up to date
    return warp_rnnt_amd.load()


def test_header_declares_what_the_table_binds_and_the_version_did_not_move():
    from warp_rnnt_amd import _build, _lib as lib
    L = _lib()
    table = lib.CTC_SYMBOLS
    assert lib.ADDITIVE_CTC == ((table, HEADER),)
    declared = {}
    for path in glob.glob(os.path.join(ROOT, "include", "*.h")):
        with open(path) as f:
            declared[os.path.basename(path)] = set(re.findall(r"\b(rnnt_amd_\w+)\s*\(", f.read().split("#ifndef")[1]))
    assert declared[HEADER] == set(table) == {"rnnt_amd_ctc_workspace_size", "rnnt_amd_ctc_loss_logits",
                                              "rnnt_amd_ctc_logits_backward"}
    for name, (res, args) in table.items():
        fn = getattr(L, name)
        assert fn.restype is res and list(fn.argtypes) == list(args)
    assert L.rnnt_amd_version() == lib.ABI_VERSION == 110
    assert "ctc.hip" in _build.SOURCES and "ctc.h" in _build.HEADERS
    assert any(os.path.basename(h) == HEADER for h in _build.HEADERS)
    # the names are this header's and this table's alone
    assert all(not (names & set(table)) for header, names in declared.items() if header != HEADER)
    others = [v for k, v in vars(lib).items() if k.endswith("SYMBOLS") and k != "CTC_SYMBOLS"]
    assert len(others) >= 17 and all(not (set(t) & set(table)) for t in others)
    assert all(table is not t for family in lib.ADDITIVE for t in family)


def test_refusals_before_any_hip_call():
    """Made-up pointers and a null stream: every call is refused by a host-side check or is an empty batch."""
    L = _lib()
    p, odd, ws = ctypes.c_void_p(4096), ctypes.c_void_p(4097), ctypes.c_void_p(8192)

    def fwd(ws=ws, dtype=1, logits=p, labels=p, xn=p, yn=p, out=p, N=2, T=3, L_=4, V=16, blank=0):
        return L.rnnt_amd_ctc_loss_logits(None, ws, dtype, logits, labels, xn, yn, out, N, T, L_, V, blank)

    def bwd(ws=ws, dtype=1, logits=p, labels=p, xn=p, yn=p, dcosts=p, out=p, N=2, T=3, L_=4, V=16, blank=0):
        return L.rnnt_amd_ctc_logits_backward(None, ws, dtype, logits, labels, xn, yn, dcosts, out, N, T, L_, V, blank)

    shapes = [dict(L_=0), dict(L_=1024), dict(V=1), dict(V=16385), dict(T=0), dict(N=-1), dict(blank=16), dict(blank=-1),
              dict(N=2, T=1 << 20, L_=1023)]            # (the last: N*T*(L+1) = 2^31, a product an empty batch does not reach)
    pointers = [dict(ws=None), dict(ws=ctypes.c_void_p(4224)), dict(logits=None), dict(labels=None), dict(xn=None),
                dict(yn=None), dict(out=None), dict(logits=odd), dict(out=odd), dict(labels=ctypes.c_void_p(4098)),
                dict(xn=ctypes.c_void_p(4098)), dict(yn=ctypes.c_void_p(4098))]
    for call in (fwd, bwd):
        for kw in pointers + shapes + [dict(dtype=3), dict(dtype=-1)]:
            assert call(**kw) == INVALID, (call.__name__, kw)
            if "N" not in kw:                    # a refused argument is not answered as an empty batch
                assert call(N=0, **kw) == INVALID, (call.__name__, kw)
        assert call(N=0) == SUCCESS and call(N=0, L_=1023, V=16384, T=1 << 20) == SUCCESS
    assert bwd(dcosts=ctypes.c_void_p(4098)) == INVALID and bwd(N=0, dcosts=None) == SUCCESS
    assert fwd(dtype=0, logits=ctypes.c_void_p(4098)) == INVALID and fwd(N=0, dtype=2, logits=ctypes.c_void_p(4098)) == SUCCESS
    size = L.rnnt_amd_ctc_workspace_size
    assert size(2, 3, 4, 16) == 6 * 256                    # six pieces, each within one unit of 256 bytes
    assert size(16, 1500, 300, 500) == sum(-(-4 * n // 256) * 256 for n in
                                           (2 * 24000, 24000 * 301, 48000 * 301, 48000 * 301, 16, 16 * 300))
    for kw in shapes[:6] + shapes[8:]:
        assert size(*({**dict(N=2, T=3, L_=4, V=16), **kw}[k] for k in ("N", "T", "L_", "V"))) == 0, kw


def test_python_checks():
    from warp_rnnt_amd.ctc import ctc_loss_from_logits
    z, lab, n = torch.zeros(2, 3, 16), torch.zeros(2, 4, dtype=torch.int32), torch.ones(2, dtype=torch.int32)
    for bad, match in (((torch.zeros(2, 3, 1), lab, n, n), "2 <= V <= 16384"),
                       ((torch.zeros(2, 3, 16385), lab, n, n), "2 <= V <= 16384"),
                       ((z, torch.zeros(2, 0, dtype=torch.int32), n, n), "1 <= L <= 1023"),
                       ((z, torch.zeros(2, 1024, dtype=torch.int32), n, n), "1 <= L <= 1023"),
                       ((torch.zeros(2, 1 << 20, 2), torch.zeros(2, 1023, dtype=torch.int32), n, n),
                        r"N\*T\*\(L\+1\) < 2\^31")):
        with pytest.raises(ValueError, match=match):
            ctc_loss_from_logits(*bad)
    with pytest.raises(ValueError, match="blank=16 is outside"):
        ctc_loss_from_logits(z, lab, n, n, blank=16)
    with pytest.raises(ValueError, match="reduction must be one of"):
        ctc_loss_from_logits(z, lab, n, n, reduction="batchmean")
    with pytest.raises(RuntimeError, match="logits must be a float32, bfloat16 or float16"):
        ctc_loss_from_logits(z.double(), lab, n, n)
    with pytest.raises(RuntimeError, match="labels must be a Int tensor"):
        ctc_loss_from_logits(z, lab.long(), n, n)
    with pytest.raises(RuntimeError, match="labels_lengths shape must be equal"):
        ctc_loss_from_logits(z, lab, n, torch.ones(3, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="logits must be contiguous"):
        ctc_loss_from_logits(z.transpose(0, 1).contiguous().transpose(0, 1), lab, n, n)
    with pytest.raises(RuntimeError, match="logits must be located in the CUDA"):
        ctc_loss_from_logits(z, lab, n, n, blank=-1)
