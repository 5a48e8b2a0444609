"""The host-side decisions of the C ABI, replayed from tests/golden/host_decisions.json (tests/golden/make_host_decisions.py
wrote it from a build of the commit before the C ABI's entries were folded onto one workspace, one tail and one compact
core; the rows of rnnt_amd_align_workspace_size from the commit before the host layer was split by entry family, the
rows of rnnt_amd_tdt_workspace_size from the commit before its table joined _lib.ADDITIVE, which is how this test reaches
that entry): every
workspace size and offset over a grid of shapes, and for every status-returning entry the calls it answers without a
launch -- each rejection reason one at a time, and the early successes."""
import json
import os

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))


def test_sizes_offsets_and_launch_free_answers_are_the_recorded_ones():
    """Runs only where no GPU is visible: the recorded calls carry made-up pointers, and an entry that stopped rejecting
    one of them has to fail on the missing device here (a status other than the recorded one) rather than launch on a
    shared card."""
    if torch.cuda.is_available():
        pytest.skip("host-only table: replayed where no GPU is visible (its pointers are made up)")
    from warp_rnnt_amd import _lib
    L = _lib.load()
    with open(os.path.join(HERE, "golden", "host_decisions.json")) as f:
        table = json.load(f)
    assert table["abi_version"] == L.rnnt_amd_version()
    entries = {fn for fn, (res, _) in _lib.SYMBOLS.items() if res is _lib._i and fn.startswith(("rnnt_amd_", "run_warp"))}
    no_rows = {"rnnt_amd_version", "rnnt_amd_compact_last_status", "rnnt_amd_debug_set_lattice_kernel",
               "rnnt_amd_debug_get_lattice_kernel", "rnnt_amd_debug_last_lattice_kernel",
               "rnnt_amd_debug_lattice_plan", "rnnt_amd_debug_lsm_plan"}     # (no status, or no arguments)
    assert {row[0] for row in table["calls"]} == entries - no_rows
    tables = [_lib.SYMBOLS] + [t for t, _ in _lib.ADDITIVE]       # (the size entries of the additive headers as well)
    assert {row[0] for row in table["sizes"]} == {fn for t in tables for fn, (res, _) in t.items() if res is _lib._sz}
    wrong = [(fn, args, want, getattr(L, fn)(*args)) for fn, args, want in table["sizes"]
             if getattr(L, fn)(*args) != want]
    assert not wrong, wrong
    assert L.rnnt_amd_workspace_size(16, 1500, 300) == 117084928
    wrong = []
    for fn, why, args, want in table["calls"]:
        got = getattr(L, fn)(*args)
        if got != want:
            wrong.append((fn, why, want, got))
    assert not wrong, wrong
