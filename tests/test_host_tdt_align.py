"""Best-path alignments over the TDT lattice without a GPU: the definition of include/warp_rnnt_amd_tdt_align.h
(tests/tdt_align_reference.py) against exhaustive path enumeration -- the score, the tie rule, lattices without a path --
the additive contract of the new header and its table, the two C entries' refusals with pointers that are never
dereferenced, the workspace size and its offsets, the unit's source, and the public signature."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import tdt_align_reference as ta

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "warp_rnnt_amd_tdt_align.h"
ENTRIES = {"rnnt_amd_tdt_align_workspace_size", "rnnt_amd_tdt_align"}
INVALID, SUCCESS = 5, 0
SETS = [(0, 1), (1,), (0, 1, 2, 3, 4), (2, 0, 1), (1, 2), (0, 1, 8), (1, 0, 3)]
LATTICES = 420          # at most 7 x 4 cells each


def _lib():
    import warp_rnnt_amd
    from warp_rnnt_amd import _build
    _build.build()          # hipcc cross-compiles for gfx950 without a GPU; no-op when up to date
    return warp_rnnt_amd.load()


def lattice(k):
    """Lattice k: (durations, T_n, U_n, tb, tl, dur, on_grid).  Even k: values on the grid {0, -1/2, -1}, whose sums are
    exact in fp32; odd k: real values.  Every tenth has the label row of frame 0 at -inf."""
    rng = np.random.RandomState(1000 + k)
    durations = SETS[k % len(SETS)]
    T_n, U_n, D = int(rng.randint(1, 8)), int(rng.randint(0, 4)), len(durations)
    grid = k % 2 == 0
    shape = (T_n, U_n + 1)
    if grid:
        tb, tl, dur = (-rng.randint(0, 3, size=s) / 2.0 for s in (shape, shape, shape + (D,)))
    else:
        tb, tl, dur = (-np.abs(rng.randn(*s)) * 2.0 for s in (shape, shape, shape + (D,)))
    if k % 10 == 3 or k % 10 == 8:
        tl[0, :] = -np.inf
    return durations, T_n, U_n, tb, tl, dur, grid


# ---- (a) the definition against exhaustive enumeration ----

def test_definition_against_exhaustive_enumeration():
    with_path = {True: 0, False: 0}
    several, without, masked = 0, 0, 0
    for k in range(LATTICES):
        durations, T_n, U_n, tb, tl, dur, grid = lattice(k)
        masked += bool(np.isneginf(tl[0]).all())
        top, want, count = ta.best_by_enumeration(tb, tl, dur, T_n, U_n, durations)
        s32, codes32, e32, _ = ta.viterbi32(tb, tl, dur, T_n, U_n, durations)
        s64, codes64, e64, _ = ta.viterbi64(tb, tl, dur, T_n, U_n, durations)
        assert s32.dtype == np.float32 and s64.dtype == np.float64
        assert codes32.shape == (T_n + 1, U_n + 1) and codes32[0, 0] == ta.NO_EDGE
        if want is None:                        # no path: -inf and no path
            without += 1
            assert s32 == -np.inf and s64 == -np.inf and e32 is None and e64 is None, k
            assert codes32[T_n, U_n] == ta.NO_EDGE
            continue
        with_path[grid] += 1
        ta.check_path(e64, T_n, U_n, durations)
        if grid:
            # sums are exact: the score IS the maximum, in either precision, and of the maximal paths the rule returns
            # the one whose codes, read from the last edge to the first, are lexicographically smallest
            several += count > 1
            assert float(s32) == top and s64 == top, k
            assert e32 == want and e64 == want, (k, count)
            assert (codes32 == codes64).all()
        else:
            assert count == 1, k
            assert abs(s64 - top) <= 1e-12, (k, s64, top)
            assert e64 == want, k
            assert abs(ta.path_score64(e64, tb, tl, dur) - top) <= 1e-12
        frames, lengths = ta.rows_of(e64, durations, 5)
        assert (frames[U_n:] == -1).all() and (lengths[U_n:] == -1).all() and (frames[:U_n] >= 0).all()
        assert ta.trace(codes64, T_n, U_n, durations) == e64
    print(f"{LATTICES} lattices: {with_path[True]} on the grid and {with_path[False]} real ones have a path, {several} of "
          f"the grid ones more than one maximal path; {without} have none; {masked} with frame 0's labels masked")
    assert LATTICES >= 400 and with_path[True] >= 100 and with_path[False] >= 100
    assert 10 * several >= with_path[True]      # the tie rule is exercised: at least 10 % of the grid lattices with a path
    assert without >= 10 and masked >= LATTICES // 10


def test_rows_of_an_edge_list():
    edges = [(0, 0, 1, 0), (1, 0, 2, 1), (3, 1, 0, 1), (3, 2, 1, 0)]          # durations (0, 1, 2): T_n = 4, U_n = 2
    ta.check_path(edges, 4, 2, (0, 1, 2))
    frames, lengths = ta.rows_of(edges, (0, 1, 2), 4)
    assert frames.tolist() == [1, 3, -1, -1] and lengths.tolist() == [2, 0, -1, -1]
    assert ta.codes_from_the_end(edges) == (2, 1, 5, 2)
    none = ta.rows_of(None, (0, 1, 2), 3)
    assert (none[0] == -1).all() and (none[1] == -1).all()


# ---- (b) the additive contract for the new header ----

def test_header_declares_what_the_table_binds_and_the_library_exports():
    import warp_rnnt_amd
    from warp_rnnt_amd import _build, _lib as lib
    L = _lib()
    table = lib.TDT_ALIGN_SYMBOLS
    assert set(table) == ENTRIES and lib.ADDITIVE_NEXT == ((table, HEADER),)
    text = open(os.path.join(ROOT, "include", HEADER)).read()
    declared = set(re.findall(r"\b(run_[a-z_]+|rnnt_amd_[a-z_]+)\s*\(", text))
    assert declared == set(table)
    assert '#include "warp_rnnt_amd.h"' in text
    main = open(os.path.join(ROOT, "include", "warp_rnnt_amd.h")).read()
    others = [lib.SYMBOLS] + [t for t, _ in lib.ADDITIVE]
    syms = subprocess.check_output(["nm", "-D", "--defined-only", warp_rnnt_amd.lib_path()]).decode()
    for name in declared:
        assert name not in main                                           # a header of their own
        assert not any(name in other for other in others)                 # ... and a table of their own
        assert re.search(r"\bT " + name + r"\b", syms), name
        fn = getattr(L, name)
        res, args = table[name]
        assert fn.restype is res and list(fn.argtypes) == list(args)      # bound by load()
    for other, header in lib.ADDITIVE:                                    # no other header declares them either
        assert not declared & set(re.findall(r"\b(rnnt_amd_[a-z_]+)\s*\(", open(os.path.join(ROOT, "include", header)).read()))
    assert L.rnnt_amd_version() == lib.ABI_VERSION == 110                 # the version did not move
    assert len(lib.ADDITIVE) == 5 and [h for _, h in lib.ADDITIVE] == [
        "warp_rnnt_amd_clamp.h", "warp_rnnt_amd_joint_dropout.h", "warp_rnnt_amd_hat.h", "warp_rnnt_amd_align.h",
        "warp_rnnt_amd_tdt.h"]
    # part of the build's fingerprint
    assert any(os.path.basename(h) == HEADER for h in _build.HEADERS) and "tdt_align.h" in _build.HEADERS
    assert "tdt_align.hip" in _build.SOURCES
    # the argument list: the loss's up to D, then scores and the two rows in place of costs and grads, no fastemit_lambda
    loss = lib.TDT_SYMBOLS["rnnt_amd_tdt_loss_logits"][1]
    assert table["rnnt_amd_tdt_align"][1] == loss[:9] + [ctypes.c_void_p] * 3 + loss[11:-1]
    assert table["rnnt_amd_tdt_align_workspace_size"] == lib.TDT_SYMBOLS["rnnt_amd_tdt_workspace_size"]


def test_library_without_an_entry_of_the_table_is_refused_with_the_rebuild_message(monkeypatch):
    from warp_rnnt_amd import _lib as lib
    _lib()
    monkeypatch.setattr(lib, "_lib", None)
    monkeypatch.setitem(lib.TDT_ALIGN_SYMBOLS, "rnnt_amd_no_such_entry", (ctypes.c_int, [ctypes.c_float]))
    with pytest.raises(RuntimeError, match=r"rnnt_amd_no_such_entry \(include/" + re.escape(HEADER) + r"\).*rebuild it"):
        lib.load()


# ---- (c) refusals and early successes ----

def _entry():
    L = _lib()
    p = ctypes.c_void_p(256)                 # aligned, non-null, never dereferenced
    good = (ctypes.c_int * 5)(0, 1, 2, 3, 4)

    def call(ws=p, dtype=0, logits=p, labels=p, xn=p, yn=p, durations=good, D=5, scores=p, frames=p, lengths=p, N=2, T=3,
             U=2, V=5, blank=0, sigma=0.0):
        if isinstance(durations, (tuple, list)):
            durations = (ctypes.c_int * max(len(durations), 1))(*durations)
        return L.rnnt_amd_tdt_align(None, ws, dtype, logits, labels, xn, yn, durations, D, scores, frames, lengths, N, T, U,
                                    V, blank, sigma)

    return L, call


def test_entry_refuses_before_any_hip_call():
    """Dummy device pointers that are never dereferenced: each call is refused by the host-side check it names; what is
    not refused is an empty batch, which succeeds without a launch.  The list is the TDT loss's
    (tests/test_host_tdt.py), plus the output rows."""
    if torch.cuda.is_available():
        pytest.skip("host-only table: replayed where no GPU is visible (its pointers are made up)")
    L, call = _entry()
    odd = ctypes.c_void_p(258)
    shared = [dict(dtype=-1), dict(dtype=3), dict(V=1), dict(V=0), dict(blank=5), dict(blank=-1), dict(logits=None),
              dict(labels=None), dict(N=-1), dict(N=70000), dict(T=0), dict(U=0), dict(U=1025), dict(U=1025, T=1),
              dict(T=1 << 20, U=1 << 10), dict(D=0), dict(D=10), dict(logits=ctypes.c_void_p(257)),
              dict(labels=odd)]
    for kw in shared:
        assert call(**kw) == INVALID, kw
        if "N" not in kw:       # a refused argument is not answered as an empty batch
            assert call(N=0, **kw) == INVALID, kw
    for durations in ((0, 2, 3), (0, 1, 1), (0, 1, 9), (-1, 0, 1), (1, 1)):
        assert call(durations=durations, D=len(durations)) == INVALID, durations
    assert call(durations=None) == INVALID
    for sigma in (-0.01, float("inf"), float("nan")):
        assert call(sigma=sigma) == INVALID, sigma
    for kw in (dict(ws=None), dict(ws=ctypes.c_void_p(264)), dict(scores=None), dict(xn=None), dict(yn=None),
               dict(scores=odd), dict(xn=odd), dict(yn=odd),
               dict(frames=None), dict(lengths=None), dict(frames=None, lengths=None), dict(frames=odd), dict(lengths=odd)):
        assert call(**kw) == INVALID, kw
        assert call(N=0, **kw) == INVALID, kw
    assert call(dtype=1, logits=odd, N=0) == SUCCESS and call(dtype=0, logits=odd) == INVALID      # two-byte elements
    for dtype in (0, 1, 2):
        assert call(dtype=dtype, N=0) == SUCCESS
        assert call(dtype=dtype, N=0, U=1, labels=None, frames=None, lengths=None) == SUCCESS      # NULL rows iff U == 1
        assert call(dtype=dtype, N=0, U=1024, sigma=0.05) == SUCCESS
    for durations in ((1,), (0, 1), (2, 0, 1), (1, 2), (0, 1, 8), tuple(range(9))):
        assert call(durations=durations, D=len(durations), N=0) == SUCCESS, durations


# ---- (d) the workspace ----

def test_workspace_size_is_a_function_of_the_shape_monotone_and_laid_out_as_restated():
    L = _lib()
    size, loss_size = L.rnnt_amd_tdt_align_workspace_size, L.rnnt_amd_tdt_workspace_size
    assert len(size.argtypes) == 4          # (N, T, U, D) and nothing else
    base = (3, 20, 7, 4)
    assert size(*base) == size(*base) > 0
    for shape in (base, (1, 1, 1, 1), (2, 3, 6, 5), (1, 6, 1024, 2), (7, 126, 5, 5), (16, 1500, 300, 5), (2, 5, 3, 9)):
        N, T, U, D = shape
        off = ta.workspace_offsets(*shape)
        assert size(*shape) == off["size"], shape
        assert off["plane"] == 0 and off["dec"] % 256 == 0 and off["dec"] >= 4 * (2 + D) * N * T * U
        assert size(*shape) >= 4 * (2 + D) * N * T * U + (T + U) * U * N         # the plane and the decision bytes
    for k, hi in enumerate((40, 200, 1024, 9)):
        sizes = [size(*(base[:k] + (v,) + base[k + 1:])) for v in range(1, hi + 1)]
        assert all(s > 0 for s in sizes), k
        assert all(a <= b for a, b in zip(sizes, sizes[1:])), k
    # 0 for every shape the loss's size entry refuses, and only for those
    for bad in ((-1, 20, 7, 4), (3, 0, 7, 4), (3, 20, 0, 4), (3, 20, 7, 0), (3, 20, 7, 10), (3, 20, 1025, 4), (70000, 20, 7, 4),
                (1, 4, 1025, 5), (1, 1 << 20, 1 << 10, 5), (65535, 1 << 10, 1 << 10, 2)):
        assert loss_size(*bad) == 0 and size(*bad) == 0, bad
    for good in ((1, 4, 1024, 5), (65535, 1, 1, 1), (1, 1 << 18, 1 << 10, 9)):
        assert loss_size(*good) > 0 and size(*good) > 0, good
    from warp_rnnt_amd import ops
    with pytest.raises(RuntimeError, match="status 5.*unsupported sizes.*U=1025"):
        ops._workspace("cpu", size, "N T U D", 1, 4, 1025, 5)


def test_plane_and_codes_are_read_from_the_workspace_as_laid_out():
    """planes_of_plane and codes_of_dec, which the GPU tests trust: a plane and decision bytes written by their addresses."""
    N, T, U, D = 2, 3, 4, 2
    flat = np.zeros(((2 + D) * N * T * U,), np.float32)
    for c in range(2 + D):
        for n in range(N):
            for t in range(T):
                for u in range(U):
                    flat[c * N * T * U + (n * T + (t + u) % T) * U + u] = 1000 * c + 100 * n + 10 * t + u
    tb, tl, dur = ta.planes_of_plane(flat, N, T, U, D)
    idx = 100 * np.arange(N)[:, None, None] + 10 * np.arange(T)[None, :, None] + np.arange(U)[None, None, :]
    assert (tb == idx).all() and (tl == 1000 + idx).all()
    assert all((dur[..., i] == 1000 * (2 + i) + idx).all() for i in range(D))
    dec = np.full((N * (T + U) * U,), 77, np.uint8)
    T_n, U_n = 2, 3
    for t in range(T_n):
        for u in range(U_n + 1):
            dec[(1 * (T + U) + t + u) * U + u] = 10 * t + u
    dec[(1 * (T + U) + T_n + U_n) * U + U_n] = 99
    codes = ta.codes_of_dec(dec, 1, T, U, T_n, U_n)
    assert codes[:T_n].tolist() == [[0, 1, 2, 3], [10, 11, 12, 13]] and codes[T_n].tolist() == [255, 255, 255, 99]


# ---- (e) the source ----

def test_the_unit_holds_no_assembly_no_atomics_and_no_polled_loads():
    from warp_rnnt_amd import _build
    assert "tdt_align.hip" not in _build.HAZARD_CHECKED and "tdt_align.hip" not in _build.RELOAD_CHECKED
    text = open(os.path.join(_build.CSRC, "tdt_align.hip")).read()
    for word in ("asm", "atomic", "volatile"):
        assert word not in text, word
    assert "k_tdt_align_sweep" in text and "k_tdt_align_trace" in text
    # the definition stands in the unit's header verbatim, as in the C header
    definition = [l.strip(" */") for l in open(os.path.join(ROOT, "include", HEADER)).read().splitlines()
                  if "v(0,0) = 0" in l or "if c > best" in l or "scores[n] = v(T_n, U_n)" in l]
    assert len(definition) == 4
    unit = open(os.path.join(_build.CSRC, "tdt_align.h")).read()
    assert all(l in unit for l in definition)


# ---- (f) Python ----

def test_public_signature_and_argument_errors_on_cpu_tensors():
    from warp_rnnt_amd import ops, tdt
    params = inspect.signature(tdt.tdt_align).parameters
    assert list(params) == ["logits", "labels", "frames_lengths", "labels_lengths", "durations", "sigma", "blank"]
    assert [params[k].default for k in list(params)[4:]] == [(0, 1, 2, 3, 4), 0.0, 0]
    assert list(inspect.signature(ops.tdt_align).parameters) == ["logits", "labels", "xn", "yn", "durations", "blank", "sigma"]
    batch = (torch.zeros((2, 3, 2, 7 + 5)), torch.ones((2, 1), dtype=torch.int32), torch.tensor([3, 2], dtype=torch.int32),
             torch.tensor([1, 1], dtype=torch.int32))
    with pytest.raises(AssertionError):
        tdt.tdt_align(*batch, blank=1.0)
    with pytest.raises(RuntimeError, match="must be located in the CUDA"):
        tdt.tdt_align(*batch)
    with pytest.raises(RuntimeError, match="ys must be a Int tensor"):
        tdt.tdt_align(batch[0], batch[1].long(), batch[2], batch[3])
    for word in ("emit_frames + emit_durations", "no_grad", "-1", "NaN", "graph", "U > 1024"):
        assert word in tdt.tdt_align.__doc__, word
    import warp_rnnt_amd
    assert "tdt_align" in warp_rnnt_amd.__doc__ and not hasattr(warp_rnnt_amd, "tdt_align")
