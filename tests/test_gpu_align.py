"""Best-path alignments on the GPU: rnnt_amd_align / warp_rnnt_amd.align.rnnt_align.

The sweep has one add per edge and one compare per cell, in fp32 and nothing else, so the NumPy restatement of the
definition (tests/align_reference.py: viterbi32) run on the pair plane the producer left in the workspace gives the
kernels' bits: scores and emit frames are compared exactly, for every producer, at the smallest shapes at which each piece
can go wrong -- a skew that wraps, the edges of the 64-column blocks, the trace's chunks of 64 diagonals, more columns than
a workgroup has lanes, a lattice of one column, the wide-row producer.  Then what the path means (against fp64), the loss
as an upper bound, bits that depend on the utterance alone, refused lengths, graph capture and the public function.

Every figure is printed before it is asserted (pytest -s)."""
import functools
import math

import numpy as np
import pytest
import torch

import align_reference as ar
import dense_layout_reference as dl
from helpers import make_case, np_log_softmax32
from oracle import transduce_np

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 2.0 ** -24
GUARD = 64                 # elements in front of and behind each output
SENTINEL = -123456789      # what the guards of emit_frames hold

SHAPES = [(3, 12, 6, 5),        # a full utterance, one of a single frame, one without labels
          (2, 3, 6, 7),         # U > T: the skew wraps
          (2, 21, 64, 4), (2, 21, 65, 4), (2, 11, 129, 3),        # column-block edges
          (7, 126, 5, 3),       # last diagonals 62, 63, 64, 65, 127, 128, 129: the trace's chunk edges
          (1, 6, 1030, 3),      # more than a workgroup's columns: two stripes
          (1, 300, 1, 3),       # U = 1: emit_frames of zero columns
          (2, 9, 5, 5000)]      # the wide-row producer
IDS = ["N%d-T%d-U%d-V%d" % s for s in SHAPES]
HALF = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
DENSE, GATHERED, LOGITS, HAT = 0, 1, 2, 3
# (kind, variant, which blank of (0, V//2, V-1))
KINDS = ([("logits", d, 0) for d in ("f32", "bf16", "f16")] +
         [("hat_logits", d, b) for d in ("f32", "bf16") for b in (0, 1, 2)] +
         [("log_probs", "f32", 0), ("gathered", "real", 0), ("gathered", "grid", 0)])
KIND_IDS = ["%s-%s-b%d" % k for k in KINDS]


def blank_of(V, which):
    return (0, V // 2, V - 1)[which]


@functools.lru_cache(maxsize=None)
def case(shape, blank=0, seed=0):
    """fp32 logits, labels, lengths on the host (read-only, shared)."""
    N, T, U, V = shape
    logits, labels, xn, yn = make_case(7000 * seed + 100 * V + 10 * T + U + blank, N, T, U, V, ragged=True, blank=blank)
    if shape == SHAPES[0]:
        xn[:], yn[:] = (12, 1, 6), (5, 2, 0)
    if shape == (7, 126, 5, 3):
        xn[:], yn[:] = (59, 60, 61, 62, 124, 125, 126), 4
    for a in (logits, labels, xn, yn):
        a.setflags(write=False)
    return logits, labels, xn, yn


def dev(a, dtype=None):
    return torch.tensor(np.asarray(a), device=DEV, dtype=dtype)


def producer_input(shape, kind, variant, blank):
    """(input_kind, device tensor) of a case for one producer."""
    from warp_rnnt_amd import ops
    N, T, U, V = shape
    logits, labels, xn, yn = case(shape, blank)
    if kind == "logits":
        return LOGITS, dev(logits).to(HALF[variant])
    if kind == "hat_logits":
        return HAT, dev(logits).to(HALF[variant])
    if kind == "log_probs":
        return DENSE, ops.log_softmax(dev(logits))
    if variant == "real":
        return GATHERED, dev(dl.gather(np_log_softmax32(logits), labels if U > 1 else None, blank))
    rng = np.random.RandomState(N * T + U)          # a grid of 1/4: ties everywhere, sums exact in fp32
    return GATHERED, dev((-rng.randint(0, 16, size=(N, T, U, 2)) / 4.0).astype(np.float32))


def raw_align(input_kind, x, labels, xn, yn, blank):
    """rnnt_amd_align through ctypes on a NaN-filled workspace, outputs embedded in poisoned guards.  Returns scores (N,)
    fp32, emit_frames (N,U-1) int32 and the pair plane turned back to row-major (N,T,U,2), all on the host; asserts that
    the guards are untouched."""
    import warp_rnnt_amd
    from warp_rnnt_amd import ops
    L = warp_rnnt_amd.load()
    N, T, U, V = x.shape
    size = L.rnnt_amd_align_workspace_size(N, T, U)
    assert size > 0 and size % 4 == 0
    ws = torch.full((size // 4,), float("nan"), dtype=torch.float32, device=DEV)
    sbuf = torch.full((N + 2 * GUARD,), float("nan"), dtype=torch.float32, device=DEV)
    ebuf = torch.full((N * (U - 1) + 2 * GUARD,), SENTINEL, dtype=torch.int32, device=DEV)
    tl = None if U == 1 else dev(labels)
    txn, tyn = dev(xn), dev(yn)
    st = L.rnnt_amd_align(torch.cuda.current_stream().cuda_stream, ws.data_ptr(), input_kind, ops.LOGITS_DTYPES[x.dtype],
                          x.data_ptr(), None if tl is None else tl.data_ptr(), txn.data_ptr(), tyn.data_ptr(),
                          sbuf[GUARD:].data_ptr(), None if U == 1 else ebuf[GUARD:].data_ptr(), N, T, U, V, blank)
    assert st == 0, st
    torch.cuda.synchronize()
    sbuf, ebuf = sbuf.cpu().numpy(), ebuf.cpu().numpy()
    assert np.isnan(sbuf[:GUARD]).all() and np.isnan(sbuf[GUARD + N:]).all()
    assert (ebuf[:GUARD] == SENTINEL).all() and (ebuf[GUARD + N * (U - 1):] == SENTINEL).all()
    off = dl.workspace_offsets(N, T, U)
    plane = ws[off["pairs"] // 4: off["pairs"] // 4 + 2 * off["cells"]].cpu().numpy().reshape(N, T, U, 2)
    return sbuf[GUARD:GUARD + N], ebuf[GUARD:GUARD + N * (U - 1)].reshape(N, U - 1), dl.from_diagonal(plane)


def expected(pairs, xn, yn):
    """viterbi32 per utterance on row-major pairs: scores (N,) and emit_frames (N,U-1) with the -1 tail; NaN and -1 for
    lengths outside [1,T] x [0,U-1]."""
    N, T, U, _ = pairs.shape
    scores = np.full((N,), np.nan, np.float32)
    emit = np.full((N, U - 1), -1, np.int32)
    for n in range(N):
        if 1 <= xn[n] <= T and 0 <= yn[n] < U:
            scores[n], emit[n, :yn[n]] = ar.viterbi32(pairs[n, :, :, 0], pairs[n, :, :, 1], xn[n], yn[n])
    return scores, emit


def assert_bits(scores, emit, want_scores, want_emit):
    ok = ~np.isnan(want_scores)
    assert np.isnan(scores[~ok]).all()
    assert (scores[ok].view(np.int32) == want_scores[ok].view(np.int32)).all(), (scores, want_scores)
    assert (emit == want_emit).all(), np.argwhere(emit != want_emit)[:5]


# ---- 1. bit for bit, every producer ----

@pytest.mark.parametrize("kind,variant,which", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_scores_and_emit_frames_are_the_reference_bits(shape, kind, variant, which):
    blank = blank_of(shape[3], which)
    _, labels, xn, yn = case(shape, blank)
    input_kind, x = producer_input(shape, kind, variant, blank)
    scores, emit, pairs = raw_align(input_kind, x, labels, xn, yn, blank)
    assert not np.isnan(pairs).any()                      # the producer wrote every cell of the plane, and it is still there
    if kind == "gathered":
        assert (pairs.view(np.int32) == x.cpu().numpy().view(np.int32)).all()
    want_scores, want_emit = expected(pairs, xn, yn)
    assert np.isfinite(want_scores).all()
    assert_bits(scores, emit, want_scores, want_emit)
    for n in range(shape[0]):                             # a path: non-decreasing frames inside the utterance
        frames = emit[n, :yn[n]]
        assert (np.diff(frames) >= 0).all() and (frames >= 0).all() and (frames < xn[n]).all()


def test_minus_infinity_is_legal_input():
    """-inf in every label of frame 0, and an utterance whose only frame it is: the path stays a path, the score may be
    -inf."""
    shape = (3, 12, 6, 5)
    _, labels, xn, yn = case(shape)
    pairs = producer_input(shape, "gathered", "grid", 0)[1].clone()
    pairs[:, 0, :, 1] = float("-inf")
    scores, emit, plane = raw_align(GATHERED, pairs, labels, xn, yn, 0)
    want_scores, want_emit = expected(plane, xn, yn)
    assert want_scores[1] == -np.inf and np.isfinite(want_scores[[0, 2]]).all()      # (utterance 1 has one frame)
    assert_bits(scores, emit, want_scores, want_emit)
    assert (emit[0, :yn[0]] >= 1).all() and (emit[1, :yn[1]] == 0).all()


# ---- 2. what the path means, against fp64 ----

@pytest.mark.parametrize("kind", ["logits", "log_probs"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_the_path_is_the_best_path_in_fp64_up_to_the_log_softmax_bar(shape, kind):
    N, T, U, V = shape
    logits, labels, xn, yn = case(shape)
    input_kind, x = producer_input(shape, kind, "f32", 0)
    scores, emit, _ = raw_align(input_kind, x, labels, xn, yn, 0)
    lp64 = transduce_np.log_softmax(logits)
    pairs64 = np.zeros((N, T, U, 2))
    pairs64[..., 0] = lp64[..., 0]
    if U > 1:
        index = np.broadcast_to(labels.astype(np.int64)[:, None, :, None], (N, T, U - 1, 1))
        pairs64[:, :, :U - 1, 1] = np.take_along_axis(lp64[:, :, :U - 1], index, axis=3)[..., 0]
    for n in range(N):
        b, l = pairs64[n, :, :, 0], pairs64[n, :, :, 1]
        # (the fp64 optimum, scored by the routine that scores the returned path: equal paths give equal sums)
        best64 = ar.path_score64(ar.viterbi64(b, l, xn[n], yn[n])[1], b, l, xn[n])
        s = ar.path_score64(emit[n, :yn[n]], b, l, xn[n])
        length = int(xn[n] + yn[n])
        # the project's per-value log-softmax bar (tests/test_gpu_lsm_routes.py) on every edge, and the rounding of
        # `length` fp32 adds on either path
        bar = length * 2e-6 * max(1.0, math.log(V)) + 2 * length * EPS * abs(s)
        print(f"{shape} {kind} n={n}: best64 - s = {best64 - s:.3e}, |score - s| = {abs(float(scores[n]) - s):.3e}, bar {bar:.3e}")
        assert 0 <= best64 - s <= bar, (shape, kind, n)
        assert abs(float(scores[n]) - s) <= bar, (shape, kind, n)


# ---- 3. against the loss ----

@pytest.mark.parametrize("kind", ["logits", "hat_logits"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_the_best_path_cannot_beat_the_sum_over_paths(shape, kind):
    from warp_rnnt_amd.align import rnnt_align
    from warp_rnnt_amd.fused import rnnt_loss_from_logits
    from warp_rnnt_amd.hat import hat_loss_from_logits
    blank = blank_of(shape[3], 1)
    logits, labels, xn, yn = case(shape, blank)
    x, tl, txn, tyn = dev(logits), dev(labels), dev(xn), dev(yn)
    loss = rnnt_loss_from_logits if kind == "logits" else hat_loss_from_logits
    with torch.no_grad():
        cost = loss(x, tl, txn, tyn, blank=blank).double().cpu().numpy()
    score = rnnt_align(x, tl, txn, tyn, blank=blank, kind=kind)[0].double().cpu().numpy()
    print(f"{shape} {kind}: score {score.tolist()} -cost {(-cost).tolist()}")
    assert np.isfinite(score).all() and (cost > 0).all()
    assert (score <= -cost * (1 - 1e-5)).all()          # (1e-5: the cost tolerance of the loss's own tests)
    for n in np.flatnonzero(yn == 0):                   # without labels there is one path
        assert abs(score[n] + cost[n]) <= 1e-5 * abs(cost[n]), n


# ---- 4. bits depend on the utterance alone ----

def _bits(t):
    return t.view(torch.int32)


@pytest.mark.parametrize("kind", ["gathered", "log_probs", "hat_logits", "logits"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_bits_depend_on_the_utterance_alone(shape, kind):
    """Each utterance alone gives the bits of its row in the batch, and a second call gives the same bits.

    Every producer, through the C entry (pair plane, score, emit frames) and through the public function.  The utterance
    alone is a tensor of its own (`clone()`): a slice of the batch is a view at `base + n * T*U*V * 4`, which at V = 3
    and V = 7 is not a multiple of 16 bytes for odd n, and the fused log-softmax serves an input that is not 16-byte
    aligned with another kernel family (lsm_plan.h) whose fp32 rounding it does not promise to be the same."""
    from warp_rnnt_amd.align import rnnt_align
    N = shape[0]
    _, labels, xn, yn = case(shape)
    input_kind, x = producer_input(shape, kind, "real" if kind == "gathered" else "f32", 0)
    scores, emit, pairs = raw_align(input_kind, x, labels, xn, yn, 0)
    again = raw_align(input_kind, x, labels, xn, yn, 0)
    assert (again[0].view(np.int32) == scores.view(np.int32)).all() and (again[1] == emit).all()
    tl, txn, tyn = dev(labels), dev(xn), dev(yn)
    for n in range(N):
        one = slice(n, n + 1)
        alone = x[one].clone()
        assert alone.data_ptr() % 16 == 0
        s1, e1, p1 = raw_align(input_kind, alone, labels[one], xn[one], yn[one], 0)
        assert (p1.view(np.int32) == pairs[one].view(np.int32)).all(), n
        assert s1.view(np.int32)[0] == scores.view(np.int32)[n] and (e1[0] == emit[n]).all(), n
        s2, e2 = rnnt_align(alone, tl[one].clone(), txn[one].clone(), tyn[one].clone(), kind=kind)
        assert s2.cpu().numpy().view(np.int32)[0] == scores.view(np.int32)[n] and (e2.cpu().numpy()[0] == emit[n]).all(), n


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_half_precision_logits_give_the_bits_of_their_upcast(shape):
    from warp_rnnt_amd.align import rnnt_align
    logits, labels, xn, yn = case(shape)
    x, tl, txn, tyn = dev(logits), dev(labels), dev(xn), dev(yn)
    for kind in ("logits", "hat_logits"):
        for dtype in (torch.bfloat16, torch.float16):
            xh = x.to(dtype)
            sh, eh = rnnt_align(xh, tl, txn, tyn, kind=kind)
            sf, ef = rnnt_align(xh.float(), tl, txn, tyn, kind=kind)
            assert sh.dtype == torch.float32 and torch.equal(_bits(sh), _bits(sf)) and torch.equal(eh, ef), (kind, dtype)


# ---- 5. refused lengths ----

@pytest.mark.parametrize("kind", ["logits", "gathered"])
def test_refused_lengths_get_nan_and_minus_one_and_touch_nothing_else(kind):
    shape = (5, 12, 6, 5)
    N, T, U, V = shape
    _, labels, _, _ = case(shape)
    xn = np.array([0, T + 1, 5, 5, T], np.int32)
    yn = np.array([3, 3, -1, U, U - 1], np.int32)
    input_kind, x = producer_input(shape, kind, "f32" if kind == "logits" else "real", 0)
    scores, emit, pairs = raw_align(input_kind, x, labels, xn, yn, 0)          # (asserts the guards)
    want_scores, want_emit = expected(pairs, xn, yn)
    assert np.isnan(want_scores[:4]).all() and np.isfinite(want_scores[4]) and (want_emit[:4] == -1).all()
    assert_bits(scores, emit, want_scores, want_emit)
    alone = raw_align(input_kind, x[4:].clone(), labels[4:], xn[4:], yn[4:], 0)
    assert alone[0].view(np.int32)[0] == scores.view(np.int32)[4] and (alone[1][0] == emit[4]).all()


# ---- 6. graph capture ----

def test_align_replays_from_a_graph():
    from warp_rnnt_amd.align import rnnt_align
    shape = (3, 30, 70, 50)
    _, labels, xn, yn = case(shape)
    tl, txn, tyn = dev(labels), dev(xn), dev(yn)
    batches = [dev(case(shape, seed=s)[0]) for s in (1, 2, 3)]
    want = [tuple(t.clone() for t in rnnt_align(b, tl, txn, tyn)) for b in batches]
    assert not torch.equal(want[0][1], want[1][1])
    x = batches[0].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            rnnt_align(x, tl, txn, tyn)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        scores, emit = rnnt_align(x, tl, txn, tyn)
    for rep in range(6):
        k = rep % len(batches)
        x.copy_(batches[k])
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(scores, want[k][0]), f"replay {rep}"
        assert torch.equal(emit, want[k][1]), f"replay {rep}"


# ---- 7. the public function ----

@pytest.mark.parametrize("shape", [SHAPES[0], (1, 300, 1, 3), (2, 11, 129, 3)], ids=["ragged", "U1", "wide"])
def test_public_function_shapes_dtypes_and_the_path_mask(shape):
    from warp_rnnt_amd.align import alignment_mask, rnnt_align
    N, T, U, V = shape
    logits, labels, xn, yn = case(shape)
    x = dev(logits).requires_grad_(True)
    tl, txn, tyn = dev(labels), dev(xn), dev(yn)
    for kind, inp in (("logits", x), ("log_probs", torch.log_softmax(x, -1))):
        scores, emit = rnnt_align(inp, tl, txn, tyn, kind=kind)
        assert scores.dtype == torch.float32 and scores.shape == (N,) and not scores.requires_grad
        assert emit.dtype == torch.int32 and emit.shape == (N, U - 1) and not emit.requires_grad
        assert scores.device == x.device and emit.device == x.device
        mask = alignment_mask(emit, txn, tyn, T, U)
        assert mask.dtype == torch.bool and mask.shape == (N, T, U) and mask.device == x.device
        assert mask.sum(dim=(1, 2)).tolist() == (xn + yn).tolist()
        for n in range(N):
            assert mask[n, 0, 0] and mask[n, xn[n] - 1, yn[n]]
            assert not mask[n, xn[n]:].any() and not mask[n, :, yn[n] + 1:].any()
    with pytest.raises(RuntimeError, match="status 5"):
        rnnt_align(x, tl, txn, tyn, blank=V)
    with pytest.raises(RuntimeError, match="status 5"):
        rnnt_align(x[..., :1].contiguous(), tl, txn, tyn, kind="hat_logits")
    empty = rnnt_align(x[:0].contiguous(), tl[:0].contiguous(), txn[:0].contiguous(), tyn[:0].contiguous())
    assert empty[0].shape == (0,) and empty[1].shape == (0, U - 1)
