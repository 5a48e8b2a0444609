"""The contract of an additive header of the C ABI, once for every family of warp_rnnt_amd._lib.ADDITIVE (gradient clamp,
dropout in the joint, HAT loss, alignments, TDT loss): entries that came after version 110 and did not move it are declared in a
header of their own, bound in a table of their own, exported, and a library built before them is told apart by its exports.
What is particular to a family -- how its argument lists relate to its twins', its constants, its sources -- is in that
family's test_host_*.py."""
import ctypes
import os
import re
import subprocess

import pytest

from warp_rnnt_amd import _lib as lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADERS = ("warp_rnnt_amd_clamp.h", "warp_rnnt_amd_joint_dropout.h", "warp_rnnt_amd_hat.h", "warp_rnnt_amd_align.h",
           "warp_rnnt_amd_tdt.h")
FAMILIES = pytest.mark.parametrize("table,header", lib.ADDITIVE, ids=[h[len("warp_rnnt_amd_"):-2] for _, h in lib.ADDITIVE])


def _load():
    import warp_rnnt_amd
    from warp_rnnt_amd import _build
    _build.build()          # hipcc cross-compiles for gfx950 without a GPU; no-op when up to date
    return warp_rnnt_amd.load()


def test_every_family_is_in_the_table_load_walks():
    families = (lib.CLAMP_SYMBOLS, lib.DROPOUT_SYMBOLS, lib.HAT_SYMBOLS, lib.ALIGN_SYMBOLS, lib.TDT_SYMBOLS)
    assert lib.ADDITIVE == tuple(zip(families, HEADERS)) and len(HEADERS) == 5


@FAMILIES
def test_header_declares_what_the_table_binds_and_the_library_exports(table, header):
    import warp_rnnt_amd
    from warp_rnnt_amd import _build
    L = _load()
    text = open(os.path.join(ROOT, "include", header)).read()
    declared = set(re.findall(r"\b(run_[a-z_]+|rnnt_amd_[a-z_]+)\s*\(", text))
    assert declared == set(table)
    assert '#include "warp_rnnt_amd.h"' in text
    main = open(os.path.join(ROOT, "include", "warp_rnnt_amd.h")).read()
    others = [lib.SYMBOLS] + [t for t, _ in lib.ADDITIVE if t is not table]
    syms = subprocess.check_output(["nm", "-D", "--defined-only", warp_rnnt_amd.lib_path()]).decode()
    for name in declared:
        assert name not in main                                           # a header of their own
        assert not any(name in other for other in others)                 # ... and a table of their own
        assert re.search(r"\bT " + name + r"\b", syms), name
        fn = getattr(L, name)
        res, args = table[name]
        assert fn.restype is res and list(fn.argtypes) == list(args)      # bound by load()
    assert L.rnnt_amd_version() == lib.ABI_VERSION == 110                 # the version did not move
    # part of the build's fingerprint
    assert any(os.path.basename(h) == header for h in _build.HEADERS)
    for h in _build.HEADERS:
        assert os.path.exists(os.path.join(_build.CSRC, h)), h


@FAMILIES
def test_library_without_an_entry_of_the_table_is_refused_with_the_rebuild_message(table, header, monkeypatch):
    """A stale library (same version number, built before the entries existed) must not surface as an AttributeError."""
    _load()
    monkeypatch.setattr(lib, "_lib", None)
    monkeypatch.setitem(table, "rnnt_amd_no_such_entry", (ctypes.c_int, [ctypes.c_float]))
    with pytest.raises(RuntimeError, match=r"rnnt_amd_no_such_entry \(include/" + re.escape(header) + r"\).*rebuild it"):
        lib.load()
