"""Best-path alignments over the TDT lattice on the GPU: rnnt_amd_tdt_align / warp_rnnt_amd.tdt.tdt_align.

The sweep has, per incoming edge, one fp32 add for the weight, one for v + weight and one compare, and nothing else, so the
NumPy restatement of the definition (tests/tdt_align_reference.py: viterbi32, itself held to exhaustive enumeration by
tests/test_host_tdt_align.py) run on the plane the producer left in the workspace gives the kernels' bits: scores, both
rows and every decision byte inside each window and at each end cell are compared exactly, at the smallest shapes at
which each mechanism can go wrong -- a skew that wraps, durations longer than the utterance, the edges of the 64-column
waves, a ring that wraps, nine durations, the trace over more than a hundred diagonals, the widest lattice, a lattice of
one column, the producer's row groups.  Then ties, -inf, what the path means against fp64 with derived bars, the loss as an
upper bound, bits that depend on the utterance alone, refused lengths, graph capture and the public function.

Every figure is printed before it is asserted (pytest -s)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import tdt_align_reference as ta
import tdt_reference as tr
from helpers import make_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 2.0 ** -24
GUARD = 64                 # elements in front of and behind each output
SENTINEL = -123456789      # what the guards of the two rows hold

D5 = (0, 1, 2, 3, 4)
D4 = (0, 1, 2, 3)
FIRST = (3, 12, 6, 5, (0, 1))
NO_PATH = (3, 12, 6, 5, (1, 2))                     # FIRST's lengths: utterance 1 (one frame, two labels) has no path
WAVE_EDGES = [(2, 21, 64, 4, D5), (2, 21, 65, 4, D5), (2, 11, 129, 3, (2, 0, 1))]
WIDEST = (1, 6, 1024, 3, (0, 1))
ROW_GROUPS = [(2, 15, 9, 252, D4), (2, 9, 5, 253, D4), (2, 9, 5, 5000, D5)]
SHAPES = ([FIRST, NO_PATH,
           (2, 3, 6, 7, D5)] +          # U > T: the skew wraps, T below the longest duration
          WAVE_EDGES +
          [(2, 60, 9, 5, (0, 1, 8)),    # the ring wraps
           (2, 5, 3, 6, tuple(range(9))),
           (7, 126, 5, 3, D5),          # T_n = 59 .. 62, 124 .. 126, U_n = 4
           WIDEST,
           (1, 300, 1, 3, D5)] +        # no emit columns
          ROW_GROUPS)
SIGMAS = (0.0, 0.05)
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}


def name(shape):
    return "N%d-T%d-U%d-V%d-d%s" % (*shape[:4], "".join(map(str, shape[4])))


# (shape, which blank of (0, V//2, V-1), dtype): every blank on the first and the last three shapes, the half types on
# the first, the wave-edge, the widest and the row-group shapes
CASES = ([(s, 0, "f32") for s in SHAPES] +
         [(s, b, "f32") for s in [FIRST] + ROW_GROUPS for b in (1, 2)] +
         [(s, 0, d) for s in [FIRST] + WAVE_EDGES + [WIDEST] + ROW_GROUPS for d in ("bf16", "f16")])
CASE_IDS = ["%s-b%d-%s" % (name(s), b, d) for s, b, d in CASES]


def blank_of(V, which):
    return (0, V // 2, V - 1)[which]


@functools.lru_cache(maxsize=None)
def case(shape, blank=0, seed=0):
    """fp32 logits (N,T,U,V+D), labels, lengths on the host (read-only, shared)."""
    N, T, U, V, durations = shape
    D = len(durations)
    tokens, labels, xn, yn = make_case(9000 * seed + 100 * V + 10 * T + U + blank, N, T, U, V, ragged=True, blank=blank)
    extra = np.random.RandomState(7 * V + T + D + seed).randn(N, T, U, D).astype(np.float32)
    logits = np.ascontiguousarray(np.concatenate([tokens, extra], axis=-1))
    if shape[:4] == FIRST[:4]:
        xn[:], yn[:] = (12, 1, 6), (5, 2, 0)
    if shape[:4] == (7, 126, 5, 3):
        xn[:], yn[:] = (59, 60, 61, 62, 124, 125, 126), 4
    for a in (logits, labels, xn, yn):
        a.setflags(write=False)
    return logits, labels, xn, yn


def dev(a, dtype=None):
    return torch.tensor(np.asarray(a), device=DEV, dtype=dtype)


def _durations(durations):
    return (ctypes.c_int * len(durations))(*durations)


def raw_align(x, labels, xn, yn, durations, blank, sigma):
    """rnnt_amd_tdt_align through ctypes on a NaN-filled workspace, outputs embedded in poisoned guards.  Returns scores
    (N,) fp32, emit_frames and emit_durations (N,U-1) int32, the plane as it lies at offset 0 (flat fp32) and the decision
    bytes (flat uint8), all on the host; asserts that the guards are untouched."""
    import warp_rnnt_amd
    from warp_rnnt_amd import ops
    L = warp_rnnt_amd.load()
    N, T, U, W = x.shape
    D = len(durations)
    off = ta.workspace_offsets(N, T, U, D)
    size = L.rnnt_amd_tdt_align_workspace_size(N, T, U, D)
    assert size == off["size"] and size % 4 == 0
    ws = torch.full((size // 4,), float("nan"), dtype=torch.float32, device=DEV)
    sbuf = torch.full((N + 2 * GUARD,), float("nan"), dtype=torch.float32, device=DEV)
    rows = [torch.full((N * (U - 1) + 2 * GUARD,), SENTINEL, dtype=torch.int32, device=DEV) for _ in range(2)]
    tl = None if U == 1 else dev(labels)
    txn, tyn = dev(xn), dev(yn)
    st = L.rnnt_amd_tdt_align(torch.cuda.current_stream().cuda_stream, ws.data_ptr(), ops.LOGITS_DTYPES[x.dtype],
                              x.data_ptr(), None if tl is None else tl.data_ptr(), txn.data_ptr(), tyn.data_ptr(),
                              _durations(durations), D, sbuf[GUARD:].data_ptr(),
                              None if U == 1 else rows[0][GUARD:].data_ptr(),
                              None if U == 1 else rows[1][GUARD:].data_ptr(), N, T, U, W - D, blank, sigma)
    assert st == 0, st
    torch.cuda.synchronize()
    sbuf = sbuf.cpu().numpy()
    assert np.isnan(sbuf[:GUARD]).all() and np.isnan(sbuf[GUARD + N:]).all()
    out = []
    for r in rows:
        r = r.cpu().numpy()
        assert (r[:GUARD] == SENTINEL).all() and (r[GUARD + N * (U - 1):] == SENTINEL).all()
        out.append(r[GUARD:GUARD + N * (U - 1)].reshape(N, U - 1))
    host = ws.cpu().numpy()
    plane = host[:(2 + D) * off["cells"]].copy()
    dec = host.view(np.uint8)[off["dec"]:off["dec"] + N * (T + U) * U].copy()
    return sbuf[GUARD:GUARD + N], out[0], out[1], plane, dec


def loss_plane(x, labels, xn, yn, durations, blank, sigma):
    """The plane rnnt_amd_tdt_loss_logits leaves at offset 0 of its own (NaN-filled) workspace, flat fp32 on the host."""
    import warp_rnnt_amd
    from warp_rnnt_amd import ops
    L = warp_rnnt_amd.load()
    N, T, U, W = x.shape
    D = len(durations)
    size = L.rnnt_amd_tdt_workspace_size(N, T, U, D)
    assert size > 0 and size % 4 == 0
    ws = torch.full((size // 4,), float("nan"), dtype=torch.float32, device=DEV)
    costs = torch.empty((N,), dtype=torch.float32, device=DEV)
    tl = None if U == 1 else dev(labels)
    txn, tyn = dev(xn), dev(yn)
    st = L.rnnt_amd_tdt_loss_logits(torch.cuda.current_stream().cuda_stream, ws.data_ptr(), ops.LOGITS_DTYPES[x.dtype],
                                    x.data_ptr(), None if tl is None else tl.data_ptr(), txn.data_ptr(), tyn.data_ptr(),
                                    _durations(durations), D, costs.data_ptr(), None, N, T, U, W - D, blank, sigma, 0.0)
    assert st == 0, st
    torch.cuda.synchronize()
    return ws[:(2 + D) * N * T * U].cpu().numpy()


def expected(plane, xn, yn, N, T, U, durations):
    """viterbi32 per utterance on the plane read back: scores (N,), both rows (N,U-1), and per utterance (codes, edges,
    ties) or None for lengths outside [1,T] x [0,U-1] -- which get NaN and -1."""
    tb, tl, dur = ta.planes_of_plane(plane, N, T, U, len(durations))
    scores = np.full((N,), np.nan, np.float32)
    frames = np.full((N, U - 1), -1, np.int32)
    lengths = np.full((N, U - 1), -1, np.int32)
    detail = [None] * N
    for n in range(N):
        if 1 <= xn[n] <= T and 0 <= yn[n] < U:
            scores[n], codes, edges, ties = ta.viterbi32(tb[n], tl[n], dur[n], xn[n], yn[n], durations)
            frames[n], lengths[n] = ta.rows_of(edges, durations, U - 1)
            detail[n] = (codes, edges, ties)
    return scores, frames, lengths, detail


def assert_bits(got, want, xn, yn, T, U):
    """Scores, both rows and every decision byte inside each window and at each end cell: exactly."""
    scores, frames, lengths, _, dec = got
    want_scores, want_frames, want_lengths, detail = want
    ok = ~np.isnan(want_scores)
    assert np.isnan(scores[~ok]).all()
    assert (scores[ok].view(np.int32) == want_scores[ok].view(np.int32)).all(), (scores, want_scores)
    assert (frames == want_frames).all(), np.argwhere(frames != want_frames)[:5]
    assert (lengths == want_lengths).all(), np.argwhere(lengths != want_lengths)[:5]
    for n, d in enumerate(detail):
        if d is not None:
            codes = ta.codes_of_dec(dec, n, T, U, int(xn[n]), int(yn[n]))
            assert (codes == d[0]).all(), (n, np.argwhere(codes != d[0])[:5])


def run_and_compare(x, labels, xn, yn, durations, blank, sigma):
    N, T, U, _ = x.shape
    got = raw_align(x, labels, xn, yn, durations, blank, sigma)
    assert not np.isnan(got[3]).any()            # the producer wrote every cell of the plane, and it is still there
    want = expected(got[3], xn, yn, N, T, U, durations)
    assert_bits(got, want, xn, yn, T, U)
    return got, want


def assert_path_properties(frames, lengths, xn, yn, durations):
    """What the rows of a path satisfy: frames non-decreasing, emit + duration <= the next emit, the last emit + duration
    < T_n, durations drawn from the set, -1 tails."""
    for n in range(len(xn)):
        f, d, Un = frames[n], lengths[n], int(yn[n])
        assert (f[Un:] == -1).all() and (d[Un:] == -1).all()
        if Un and f[0] >= 0:
            assert (f[:Un] >= 0).all() and (np.diff(f[:Un]) >= 0).all() and all(int(k) in durations for k in d[:Un])
            assert (f[:Un - 1] + d[:Un - 1] <= f[1:Un]).all() and f[Un - 1] + d[Un - 1] < xn[n]
        else:
            assert (f == -1).all() and (d == -1).all()


# ---- 1. bit for bit ----

@pytest.mark.parametrize("sigma", SIGMAS)
@pytest.mark.parametrize("shape,which,dname", CASES, ids=CASE_IDS)
def test_scores_rows_and_decision_bytes_are_the_reference_bits(shape, which, dname, sigma):
    N, T, U, V, durations = shape
    blank = blank_of(V, which)
    logits, labels, xn, yn = case(shape, blank)
    x = dev(logits).to(DTYPES[dname])
    got, want = run_and_compare(x, labels, xn, yn, durations, blank, sigma)
    scores, frames, lengths, plane, dec = got
    # the plane's bits are those the loss leaves in its own workspace
    assert (plane.view(np.int32) == loss_plane(x, labels, xn, yn, durations, blank, sigma).view(np.int32)).all()
    if shape == NO_PATH:
        assert scores[1] == -np.inf and (frames[1] == -1).all() and (lengths[1] == -1).all()
        assert np.isfinite(scores[[0, 2]]).all()
    else:
        assert np.isfinite(scores).all()
    assert_path_properties(frames, lengths, xn, yn, durations)
    if dname != "f32":                           # a half type gives the bits of its fp32 upcast
        up = raw_align(x.float(), labels, xn, yn, durations, blank, sigma)
        assert (up[3].view(np.int32) == plane.view(np.int32)).all()
        assert (up[0].view(np.int32) == scores.view(np.int32)).all()
        assert (up[1] == frames).all() and (up[2] == lengths).all()
        assert_bits(up, want, xn, yn, T, U)


# ---- 2. ties ----

@pytest.mark.parametrize("durations", [D5, (0, 1)], ids=["d01234", "d01"])
@pytest.mark.parametrize("fill", ["zeros", "one-row"])
def test_ties_go_to_the_earlier_candidate(fill, durations):
    """Equal rows: every cell has the same weights.  The reference, on the plane read back, must see a cell where two
    candidates equal the maximum on every returned path.

    All-zero logits: every edge of the lattice has the same weight, bit for bit, so a path's score depends on its number
    of edges alone and every cell that two shortest ways reach holds a tie.  One random row: the weights differ by the
    edge's kind and duration, and two orders of the same edges meet with the same bits only where the sum is exact --
    behind the first two edges of a path, (0 + a) + b = (0 + b) + a by commutativity; further on, (v + a) + b and
    (v + b) + a round apart.  The tie rule puts a path's small codes at its end, so its first two edges are alike unless
    the edge of its largest code is there once: the lengths of the random-row case are those at which it is, for both
    duration sets (worked out on the host from the row; T_n = 12 and 10 with one label, T_n = 2 with five)."""
    N, T, U, V = FIRST[:4]
    W = V + len(durations)
    if fill == "zeros":
        logits = np.zeros((N, T, U, W), np.float32)
        xn, yn = np.array([12, 7, 9], np.int32), np.array([5, 3, 4], np.int32)
    else:
        logits = np.broadcast_to(np.random.RandomState(2).randn(W).astype(np.float32), (N, T, U, W)).copy()
        xn, yn = np.array([12, 2, 10], np.int32), np.array([1, 5, 1], np.int32)
    labels = np.full((N, U - 1), 3, np.int32)        # one label: every cell's label weight is the same
    for sigma in SIGMAS:
        got, want = run_and_compare(dev(logits), labels, xn, yn, durations, 0, sigma)
        for n, (codes, edges, ties) in enumerate(want[3]):
            if edges is None:
                continue
            on_path = [ties[t + durations[i], u + kind] for t, u, i, kind in edges]
            print(f"{fill} {durations} sigma {sigma} n={n}: {sum(on_path)} of {len(on_path)} cells of the path hold a tie")
            assert any(on_path), (fill, durations, n)
        assert_path_properties(got[1], got[2], xn, yn, durations)


# ---- 3. -inf ----

@pytest.mark.parametrize("durations", [(0, 1), D5], ids=["d01", "d01234"])
def test_minus_infinity_is_legal_input(durations):
    """The label logits of frame 0 masked: no label is emitted at frame 0, and the utterance whose only frame it is has no
    path."""
    shape = FIRST[:4] + (durations,)
    N, T, U, V, _ = shape
    logits, labels, xn, yn = case(shape)
    logits = logits.copy()
    for n in range(N):
        for u in range(U - 1):
            logits[n, 0, u, labels[n, u]] = -np.inf
    got, want = run_and_compare(dev(logits), labels, xn, yn, durations, 0, 0.0)
    scores, frames, lengths = got[:3]
    assert scores[1] == -np.inf and (frames[1] == -1).all() and (lengths[1] == -1).all()      # one frame, two labels
    assert np.isfinite(scores[[0, 2]]).all()
    assert (frames[0, :yn[0]] >= 1).all()
    assert_path_properties(frames, lengths, xn, yn, durations)


# ---- 4. what the path means, with derived bars ----

MEANING = [FIRST, NO_PATH, (2, 3, 6, 7, D5), (2, 21, 65, 4, D5), (2, 60, 9, 5, (0, 1, 8)), (2, 5, 3, 6, tuple(range(9))),
           (2, 9, 5, 253, D4)]


def bars(plane, frames_row, codes_dec, n, xn, yn, N, T, U, durations):
    """fp64 on the upcast plane for utterance n: (s, best64, ll64, bar) -- the fp64 score of the returned path (read back
    along the kernel's decision bytes), the fp64 optimum, the fp64 log-likelihood, and the bar: every edge advances the
    diagonal, so a path has at most E = T_n + U_n edges of two fp32 adds each, each within 2^-24 relative of a partial sum
    that is at most |best64| in magnitude -- bar = 2 E 2^-24 |best64| (1 + 2 E 2^-24)."""
    tb, tl, dur = (a.astype(np.float64) for a in ta.planes_of_plane(plane, N, T, U, len(durations)))
    Tn, Un = int(xn[n]), int(yn[n])
    best64 = float(ta.viterbi64(tb[n], tl[n], dur[n], Tn, Un, durations)[0])
    tok = np.stack([tb[n], tl[n]], axis=-1)                   # a two-token vocabulary: blank 0, every label 1
    with np.errstate(invalid="ignore"):                       # (an utterance without a path: -inf - -inf in its occupancies)
        ll64 = float(tr.utterance(tok, dur[n], np.ones((U,), np.int64), Tn, Un, durations, 0)[0])
    if not np.isfinite(best64):
        return None, best64, ll64, 0.0
    edges = ta.trace(ta.codes_of_dec(codes_dec, n, T, U, Tn, Un), Tn, Un, durations)
    ta.check_path(edges, Tn, Un, durations)
    assert (ta.rows_of(edges, durations, U - 1)[0] == frames_row).all()
    E = Tn + Un
    return ta.path_score64(edges, tb[n], tl[n], dur[n]), best64, ll64, 2 * E * EPS * abs(best64) * (1 + 2 * E * EPS)


@pytest.mark.parametrize("sigma", SIGMAS)
@pytest.mark.parametrize("shape", MEANING, ids=[name(s) for s in MEANING])
def test_the_path_is_the_best_path_in_fp64_up_to_the_rounding_of_its_adds(shape, sigma):
    N, T, U, V, durations = shape
    logits, labels, xn, yn = case(shape)
    scores, frames, lengths, plane, dec = raw_align(dev(logits), labels, xn, yn, durations, 0, sigma)
    for n in range(N):
        s, best64, ll64, bar = bars(plane, frames[n], dec, n, xn, yn, N, T, U, durations)
        if s is None:
            assert scores[n] == -np.inf and ll64 == -np.inf
            continue
        score = float(scores[n])
        print(f"{name(shape)} sigma {sigma} n={n}: |score - s| = {abs(score - s):.3e}, best64 - s = {best64 - s:.3e}, "
              f"ll64 - score = {ll64 - score:.3e}, bar {bar:.3e}")
        assert abs(score - s) <= bar, (shape, n)
        assert 0 <= best64 - s <= 2 * bar, (shape, n)
        assert score <= ll64 + bar, (shape, n)


# ---- 5. through the public functions ----

@pytest.mark.parametrize("shape", MEANING, ids=[name(s) for s in MEANING])
def test_the_best_path_cannot_beat_the_sum_over_paths(shape):
    """score + cost <= COST_BAR |cost| + bar: COST_BAR is the bar the TDT loss's cost is held to against fp64
    (tests/test_gpu_tdt.py, cited), bar the rounding of the path's adds (above)."""
    from test_gpu_tdt import COST_BAR
    from warp_rnnt_amd.tdt import tdt_align, tdt_loss_from_logits
    N, T, U, V, durations = shape
    blank = blank_of(V, 1)
    logits, labels, xn, yn = case(shape, blank)
    x, tl, txn, tyn = dev(logits), dev(labels), dev(xn), dev(yn)
    for sigma in SIGMAS:
        with torch.no_grad():
            cost = tdt_loss_from_logits(x, tl, txn, tyn, durations=durations, sigma=sigma, blank=blank).double().cpu().numpy()
        scores, frames, lengths = (t.cpu().numpy() for t in tdt_align(x, tl, txn, tyn, durations=durations, sigma=sigma,
                                                                      blank=blank))
        raw = raw_align(x, labels, xn, yn, durations, blank, sigma)
        assert (raw[0].view(np.int32) == scores.view(np.int32)).all() and (raw[1] == frames).all() and (raw[2] == lengths).all()
        for n in range(N):
            _, best64, _, bar = bars(raw[3], frames[n], raw[4], n, xn, yn, N, T, U, durations)
            if not np.isfinite(best64):
                assert scores[n] == -np.inf and cost[n] == np.inf
                continue
            margin = COST_BAR * abs(cost[n]) + bar - (float(scores[n]) + cost[n])
            print(f"{name(shape)} sigma {sigma} n={n}: score {scores[n]:.6f} -cost {-cost[n]:.6f} margin {margin:.3e}")
            assert margin >= 0, (shape, sigma, n)
        assert_path_properties(frames, lengths, xn, yn, durations)


# ---- 6. other behaviour ----

ALONE = [FIRST, NO_PATH, (2, 21, 65, 4, D5), (7, 126, 5, 3, D5), (2, 9, 5, 5000, D5)]


@pytest.mark.parametrize("shape", ALONE, ids=[name(s) for s in ALONE])
def test_bits_depend_on_the_utterance_alone(shape):
    """Each utterance alone gives the bits of its row in the batch, through the C entry and the public function, and a
    second call gives the same bits."""
    from warp_rnnt_amd.tdt import tdt_align
    N, T, U, V, durations = shape
    logits, labels, xn, yn = case(shape)
    x = dev(logits)
    scores, frames, lengths, plane, dec = raw_align(x, labels, xn, yn, durations, 0, 0.05)
    again = raw_align(x, labels, xn, yn, durations, 0, 0.05)
    assert (again[0].view(np.int32) == scores.view(np.int32)).all() and (again[1] == frames).all() and (again[2] == lengths).all()
    tl, txn, tyn = dev(labels), dev(xn), dev(yn)
    for n in range(N):
        one = slice(n, n + 1)
        alone = x[one].clone()
        s1, f1, l1, _, _ = raw_align(alone, labels[one], xn[one], yn[one], durations, 0, 0.05)
        assert s1.view(np.int32)[0] == scores.view(np.int32)[n] and (f1[0] == frames[n]).all() and (l1[0] == lengths[n]).all(), n
        s2, f2, l2 = tdt_align(alone, tl[one].clone(), txn[one].clone(), tyn[one].clone(), durations=durations, sigma=0.05)
        assert s2.cpu().numpy().view(np.int32)[0] == scores.view(np.int32)[n], n
        assert (f2.cpu().numpy()[0] == frames[n]).all() and (l2.cpu().numpy()[0] == lengths[n]).all(), n


def test_refused_lengths_get_nan_and_minus_one_and_touch_nothing_else():
    shape = (5, 12, 6, 5, D5)
    N, T, U, V, durations = shape
    logits, labels, _, _ = case(shape)
    xn = np.array([0, T + 1, 5, 5, T], np.int32)
    yn = np.array([3, 3, -1, U, U - 1], np.int32)
    x = dev(logits)
    got, want = run_and_compare(x, labels, xn, yn, durations, 0, 0.0)          # (asserts the guards)
    assert np.isnan(want[0][:4]).all() and np.isfinite(want[0][4]) and (want[1][:4] == -1).all()
    assert np.isnan(got[0][:4]).all() and (got[1][:4] == -1).all() and (got[2][:4] == -1).all()
    # nothing of a refused utterance's decision bytes is written: they still hold the workspace's NaN fill
    refused = 4 * (T + U) * U
    assert (got[4][:refused] == np.full((refused // 4,), np.nan, np.float32).view(np.uint8)).all()
    alone = raw_align(x[4:].clone(), labels[4:], xn[4:], yn[4:], durations, 0, 0.0)
    assert alone[0].view(np.int32)[0] == got[0].view(np.int32)[4]
    assert (alone[1][0] == got[1][4]).all() and (alone[2][0] == got[2][4]).all()


def test_align_replays_from_a_graph():
    from warp_rnnt_amd.tdt import tdt_align
    shape = (3, 30, 70, 50, D5)
    _, labels, xn, yn = case(shape)
    tl, txn, tyn = dev(labels), dev(xn), dev(yn)
    batches = [dev(case(shape, seed=s)[0]) for s in (1, 2, 3)]
    want = [tuple(t.clone() for t in tdt_align(b, tl, txn, tyn, sigma=0.05)) for b in batches]
    assert not torch.equal(want[0][1], want[1][1])
    x = batches[0].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            tdt_align(x, tl, txn, tyn, sigma=0.05)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = tdt_align(x, tl, txn, tyn, sigma=0.05)
    for rep in range(6):
        k = rep % len(batches)
        x.copy_(batches[k])
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out[0].view(torch.int32), want[k][0].view(torch.int32)), f"replay {rep}"
        assert torch.equal(out[1], want[k][1]) and torch.equal(out[2], want[k][2]), f"replay {rep}"


@pytest.mark.parametrize("shape", [FIRST, (1, 300, 1, 3, D5), (2, 11, 129, 3, (2, 0, 1))], ids=["ragged", "U1", "wide"])
def test_public_function_shapes_and_dtypes(shape):
    from warp_rnnt_amd.tdt import tdt_align
    N, T, U, V, durations = shape
    logits, labels, xn, yn = case(shape)
    x = dev(logits).requires_grad_(True)
    tl, txn, tyn = dev(labels), dev(xn), dev(yn)
    scores, frames, lengths = tdt_align(x, tl, txn, tyn, durations=durations)
    assert scores.dtype == torch.float32 and scores.shape == (N,) and not scores.requires_grad
    for rows in (frames, lengths):
        assert rows.dtype == torch.int32 and rows.shape == (N, U - 1) and not rows.requires_grad and rows.device == x.device
    assert scores.device == x.device and torch.isfinite(scores).all()
    assert_path_properties(frames.cpu().numpy(), lengths.cpu().numpy(), xn, yn, durations)
    for dtype in (torch.bfloat16, torch.float16):
        sh = tdt_align(x.detach().to(dtype), tl, txn, tyn, durations=durations)
        sf = tdt_align(x.detach().to(dtype).float(), tl, txn, tyn, durations=durations)
        assert sh[0].dtype == torch.float32 and all(torch.equal(a, b) for a, b in zip(sh, sf))
    with pytest.raises(RuntimeError, match="status 5.*blank"):
        tdt_align(x, tl, txn, tyn, durations=durations, blank=V)
    with pytest.raises(RuntimeError, match="status 5.*durations"):
        tdt_align(x, tl, txn, tyn, durations=(0, 2))
    with pytest.raises(RuntimeError, match="status 5.*sigma"):
        tdt_align(x, tl, txn, tyn, durations=durations, sigma=-1.0)
    empty = tdt_align(x[:0].contiguous(), tl[:0].contiguous(), txn[:0].contiguous(), tyn[:0].contiguous(), durations=durations)
    assert empty[0].shape == (0,) and empty[1].shape == (0, U - 1) and empty[2].shape == (0, U - 1)
