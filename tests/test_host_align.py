"""Best-path alignments without a GPU: the two C entries of include/warp_rnnt_amd_align.h (their input kinds and
argument lists, sized by the shape, refusing bad arguments before any HIP call), the NumPy reference
against exhaustive enumeration -- the tie rule included -- and the public functions' signatures, argument errors and the
path mask."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import align_reference as ar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"rnnt_amd_align_workspace_size", "rnnt_amd_align"}
HEADER = os.path.join(ROOT, "include", "warp_rnnt_amd_align.h")
INVALID, SUCCESS = 5, 0
DENSE, GATHERED, LOGITS, HAT = 0, 1, 2, 3


def _lib():
    import warp_rnnt_amd
    from warp_rnnt_amd import _build
    _build.build()          # hipcc cross-compiles for gfx950 without a GPU; no-op when up to date
    return warp_rnnt_amd.load()


# ---- header and table ----

def test_align_entries_input_kinds_argument_lists_and_units():
    """(What every additive header owes -- declared, bound, exported, a stale library refused: test_host_additive_abi.py.)"""
    from warp_rnnt_amd import _build, _lib as lib
    assert set(lib.ALIGN_SYMBOLS) == ENTRIES
    assert re.search(r"#define\s+RNNT_ALIGN_IN_HAT_LOGITS\s+3\b", open(HEADER).read()) and lib.ALIGN_IN_HAT_LOGITS == HAT
    assert (lib.IN_LOG_PROBS_DENSE, lib.IN_LOG_PROBS_GATHERED, lib.IN_LOGITS_DENSE) == (DENSE, GATHERED, LOGITS)
    assert lib.ALIGN_SYMBOLS["rnnt_amd_align_workspace_size"] == lib.SYMBOLS["rnnt_amd_workspace_size"]
    assert len(lib.ALIGN_SYMBOLS["rnnt_amd_align"][1]) == 15
    assert "align.h" in _build.HEADERS
    assert "align.hip" in _build.SOURCES and "align.hip" not in _build.HAZARD_CHECKED


def test_the_unit_polls_nothing_and_includes_what_it_may():
    """align.hip: no inline assembly, no atomics, no volatile reads -- nothing that could wait on memory -- and only the
    headers the unit is allowed."""
    text = re.sub(r"//[^\n]*", "", open(os.path.join(ROOT, "warp_rnnt_amd", "csrc", "align.hip")).read())
    for word in ("asm", "atomic", "volatile", "__hip_atomic", "s_sleep"):
        assert not re.search(r"\b" + word, text), word
    includes = set(re.findall(r'#include\s+[<"]([^>"]+)[>"]', text))
    assert includes <= {"align.h", "common.h", "kernels.h", "streaming.h", "../../include/warp_rnnt_amd_align.h"}, includes
    assert text.count("__syncthreads()") == 1          # the one barrier every wave of a workgroup reaches, phase by phase


# ---- sizes ----

def test_workspace_size_is_the_loss_carve_plus_the_decision_words():
    L = _lib()
    for N, T, U in ((16, 1500, 300), (2, 100, 1100), (1, 5, 1)):
        words = N * (T + U - 1) * ((U + 63) // 64) * 8
        base, size = L.rnnt_amd_workspace_size(N, T, U), L.rnnt_amd_align_workspace_size(N, T, U)
        assert base > 0 and size >= base + words, (N, T, U)
        assert size < base + words + (1 << 20), (N, T, U)          # (and not much more: the parked stripe columns)
        assert size % 256 == 0
    assert L.rnnt_amd_align_workspace_size(1, 0, 3) == 0
    for bad in ((-1, 4, 4), (70000, 4, 4), (1, 4, 0), (1, 1 << 15, 1 << 14), (65535, 1 << 10, 1 << 7)):
        assert L.rnnt_amd_align_workspace_size(*bad) == 0 == L.rnnt_amd_workspace_size(*bad), bad


# ---- refusals before any HIP call ----

def test_align_refuses_before_any_hip_call():
    """Dummy device pointers that are never dereferenced: each call is refused by the host-side check it names."""
    if torch.cuda.is_available():
        pytest.skip("host-only table: replayed where no GPU is visible (its pointers are made up)")
    L = _lib()
    p = ctypes.c_void_p(256)                 # aligned, non-null, never dereferenced

    def call(ws=p, kind=LOGITS, dtype=0, x=p, labels=p, xn=p, yn=p, scores=p, emit=p, N=2, T=3, U=2, V=5, blank=0):
        return L.rnnt_amd_align(None, ws, kind, dtype, x, labels, xn, yn, scores, emit, N, T, U, V, blank)

    def refused(**kw):
        assert call(**kw) == INVALID, kw
        if "N" not in kw:          # ... whatever else is asked: a refused argument is not answered as an empty batch
            assert call(N=0, **kw) == INVALID, kw

    for kind in (-1, 4, 17):
        refused(kind=kind)
    for kind in (DENSE, GATHERED, LOGITS, HAT):
        for kw in (dict(dtype=-1), dict(dtype=3), dict(N=-1), dict(N=70000), dict(T=0), dict(U=0),
                   dict(T=1 << 15, U=1 << 14), dict(N=65535, T=1 << 10, U=1 << 7), dict(ws=None),
                   dict(ws=ctypes.c_void_p(264)), dict(x=None), dict(xn=None), dict(yn=None), dict(scores=None),
                   dict(emit=None)):
            refused(kind=kind, **kw)
    for kind in (DENSE, GATHERED):          # fp32 only on the two log-prob kinds
        refused(kind=kind, dtype=1)
        refused(kind=kind, dtype=2)
    for kind in (DENSE, LOGITS, HAT):       # vocabulary, blank, labels
        for kw in (dict(V=0), dict(V=-3), dict(blank=5), dict(blank=-1), dict(labels=None)):
            refused(kind=kind, **kw)
    refused(kind=HAT, V=1)
    # ... which the gathered kind does not read
    for kw in (dict(V=0), dict(blank=5), dict(blank=-1), dict(labels=None), dict(V=1)):
        assert call(kind=GATHERED, N=0, **kw) == SUCCESS, kw
    # no utterances: success without a launch, per kind and dtype; a column of blanks needs no labels and no emit frames
    for kind, dtypes in ((DENSE, (0,)), (GATHERED, (0,)), (LOGITS, (0, 1, 2)), (HAT, (0, 1, 2))):
        for dtype in dtypes:
            assert call(kind=kind, dtype=dtype, N=0) == SUCCESS, (kind, dtype)
            assert call(kind=kind, dtype=dtype, N=0, U=1, labels=None, emit=None) == SUCCESS, (kind, dtype)
    assert call(kind=DENSE, N=0, V=1) == SUCCESS and call(kind=LOGITS, N=0, V=1) == SUCCESS


# ---- the reference against enumeration ----

def _lattice(rng, grid, T, U):
    """(T,U) planes of values in (-1, 0] on a grid of 1/grid: sums of a handful are exact in fp32 and fp64 alike, and on
    the grid of 1/4 -- four values -- paths of equal score are common."""
    b = -rng.randint(0, grid, size=(T, U)).astype(np.float64) / grid
    l = -rng.randint(0, grid, size=(T, U)).astype(np.float64) / grid
    return b, l


def _check_against_enumeration(b, l, T_n, U_n):
    s32, e32 = ar.viterbi32(b, l, T_n, U_n)
    s64, e64 = ar.viterbi64(b, l, T_n, U_n)
    best, emit, n_best = ar.best_by_enumeration(b, l, T_n, U_n)
    assert s32.dtype == np.float32 and s64.dtype == np.float64 and e32.dtype == np.int32 and e32.shape == (U_n,)
    assert float(s32) == s64 == best, (T_n, U_n, s32, s64, best)
    assert e32.tolist() == e64.tolist() == emit.tolist(), (T_n, U_n, e32, emit)
    if np.isfinite(best):
        assert ar.path_score64(e32, b, l, T_n) == best
    return n_best


def test_viterbi_is_the_best_path_by_enumeration_and_the_tie_rule_picks_the_earliest_emissions():
    rng = np.random.RandomState(2024)
    tied = 0
    for grid in (4, 64):
        for k in range(200):
            T_n, U_n = rng.randint(2, 6), rng.randint(1, 4)      # (more than one path: the edges come below)
            T, U = min(T_n + rng.randint(0, 2), 5), min(U_n + 1 + rng.randint(0, 2), 4)
            b, l = _lattice(rng, grid, T, U)
            n_best = _check_against_enumeration(b, l, T_n, U_n)
            if grid == 4 and n_best > 1:
                tied += 1
    assert tied >= 50, tied          # the 1/4 grid makes real ties: the rule is under test, not assumed
    # the edges: no labels, a single frame, -inf in every label of frame 0
    b, l = _lattice(rng, 4, 5, 4)
    _check_against_enumeration(b, l, 5, 0)
    s, e = ar.viterbi32(b, l, 4, 0)
    assert s == np.float32(b[:4, 0].sum()) and e.shape == (0,)
    _check_against_enumeration(b, l, 1, 3)
    s, e = ar.viterbi32(b, l, 1, 3)
    assert e.tolist() == [0, 0, 0] and float(s) == l[0, :3].sum() + b[0, 3]
    l[0, :] = -np.inf
    for T_n, U_n in ((5, 3), (2, 2), (3, 1)):
        _check_against_enumeration(b, l, T_n, U_n)
        s, e = ar.viterbi32(b, l, T_n, U_n)
        assert np.isfinite(s) and (e >= 1).all()
    s, e = ar.viterbi32(b, l, 1, 2)          # every path goes through frame 0: the score is -inf, the path still a path
    assert s == -np.inf and e.tolist() == [0, 0]
    _check_against_enumeration(b, l, 1, 2)


# ---- the public functions ----

def test_public_signatures_and_argument_errors_on_cpu_tensors():
    import warp_rnnt_amd
    from warp_rnnt_amd import align, ops
    params = inspect.signature(align.rnnt_align).parameters
    assert list(params) == ["inputs", "labels", "frames_lengths", "labels_lengths", "blank", "kind"]
    assert [params[k].default for k in list(params)[4:]] == [0, "logits"]
    params = inspect.signature(ops.align).parameters
    assert list(params) == ["input", "labels", "xn", "yn", "input_kind", "blank"] and params["blank"].default == 0
    assert list(inspect.signature(align.alignment_mask).parameters) == ["emit_frames", "frames_lengths", "labels_lengths",
                                                                       "T", "U"]
    assert align.KINDS == ("logits", "hat_logits", "log_probs", "gathered")
    batch = (torch.zeros((2, 3, 2, 7)), torch.ones((2, 1), dtype=torch.int32), torch.tensor([3, 2], dtype=torch.int32),
             torch.tensor([1, 1], dtype=torch.int32))
    for bad in ("dense", "", None, "LOGITS"):
        with pytest.raises(ValueError, match="kind must be one of"):
            align.rnnt_align(*batch, kind=bad)
    with pytest.raises(AssertionError):
        align.rnnt_align(*batch, blank=1.0)
    # the input checks, with their texts: these tensors are not on the GPU
    for kind in align.KINDS:
        with pytest.raises(RuntimeError, match="must be located in the CUDA"):
            align.rnnt_align(*batch, kind=kind)
        with pytest.raises(RuntimeError, match="ys must be a Int tensor"):
            align.rnnt_align(batch[0], batch[1].long(), batch[2], batch[3], kind=kind)
    for kind in ("logits", "hat_logits"):
        with pytest.raises(RuntimeError, match="float32, bfloat16 or float16"):
            align.rnnt_align(batch[0].double(), *batch[1:], kind=kind)
    for kind in ("log_probs", "gathered"):          # fp32 only
        with pytest.raises(RuntimeError, match="xs must be a Float tensor"):
            align.rnnt_align(batch[0].bfloat16(), *batch[1:], kind=kind)
    assert "align.py" in warp_rnnt_amd.__doc__ and not hasattr(warp_rnnt_amd, "rnnt_align")


def _monotone_and_complete(mask, T_n, U_n):
    cells = np.argwhere(mask)
    assert len(cells) == T_n + U_n
    order = cells[np.lexsort((cells[:, 1], cells[:, 0] + cells[:, 1]))]          # by diagonal: one cell on each
    assert (order[:, 0] + order[:, 1] == np.arange(T_n + U_n)).all()
    steps = np.diff(order, axis=0)
    assert ((steps == (1, 0)).all(1) | (steps == (0, 1)).all(1)).all()
    assert tuple(order[0]) == (0, 0) and tuple(order[-1]) == (T_n - 1, U_n)


def test_alignment_mask_marks_the_cells_of_the_path():
    from warp_rnnt_amd.align import alignment_mask
    # by hand: 3 frames, 2 labels, emitted at frames 0 and 2
    mask = alignment_mask(torch.tensor([[0, 2]], dtype=torch.int32), torch.tensor([3]), torch.tensor([2]), 3, 3)
    assert mask.dtype == torch.bool and mask.shape == (1, 3, 3)
    assert mask[0].int().tolist() == [[1, 1, 0],
                                      [0, 1, 0],
                                      [0, 1, 1]]
    # a ragged batch, straight from the reference: -1 behind U_n, rows beyond T_n and columns beyond U_n stay empty
    rng = np.random.RandomState(7)
    T, U = 9, 6
    lens = [(9, 5), (4, 2), (1, 3), (6, 0), (1, 0)]
    emit = np.full((len(lens), U - 1), -1, np.int32)
    for n, (T_n, U_n) in enumerate(lens):
        b, l = rng.randn(T, U), rng.randn(T, U)
        emit[n, :U_n] = ar.viterbi32(b, l, T_n, U_n)[1]
    mask = alignment_mask(torch.tensor(emit), torch.tensor([x for x, _ in lens], dtype=torch.int32),
                          torch.tensor([y for _, y in lens], dtype=torch.int32), T, U).numpy()
    assert mask.shape == (len(lens), T, U)
    for n, (T_n, U_n) in enumerate(lens):
        _monotone_and_complete(mask[n], T_n, U_n)
        assert not mask[n, T_n:].any() and not mask[n, :, U_n + 1:].any()
        for u in range(U_n):          # label u is emitted from the last cell of column u
            assert mask[n, emit[n, u], u] and mask[n, emit[n, u], u + 1]
