"""Best-path alignments on the pruned band on the GPU: rnnt_amd_pruned_align / warp_rnnt_amd.pruned.pruned_rnnt_align.

The pairs the producer leaves in the workspace are held to the definition in fp64 (want_pairs); the NumPy restatement of
the sweep (tests/pruned_align_reference.py) on those pairs gives the kernel's bits.  Every figure is printed before it is
asserted (pytest -s)."""
import functools
import math

import numpy as np
import pytest
import torch

import hat_reference as hr
import pruned_align_reference as par
import pruned_reference as pr
from oracle import transduce_np

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 2.0 ** -24
GUARD, SENTINEL = 64, -123456789
KINDS = {"logits": 0, "hat_logits": 1, "pairs": 2}
TOPOLOGY = {"regular": 0, "modified": 1}
HALF = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
CHUNK = 64                      # PA_CHUNK of csrc/pruned_align.h: frames staged ahead of the sweep
# (N,T,U,S,V): the first has an utterance of one frame, one without labels and a full one
SHAPES = ([(3, 12, 6, 2, 5), (2, 9, 4, 1, 5), (2, 10, 6, 6, 5), (2, 7, 1, 1, 5), (4, 8, 9, 3, 5)] +
          [(2, 20, S + 3, S, 5) for S in (5, 16, 17, 32, 33, 64)] +
          [(2, T, 8, 3, 5) for T in (CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK - 1, 2 * CHUNK, 2 * CHUNK + 1)] +
          [(2, 9, 5, 3, V) for V in (64, 65, 1030)])
STEPS = (4, 8, 9, 3, 5)         # starts with steps of 0, 1, S-1, S (disconnects), a decreasing step, a row outside [0,U)


def dev(a, dtype=None):
    return torch.tensor(np.asarray(a), device=DEV, dtype=dtype)


@functools.lru_cache(maxsize=None)
def case(shape, blank=0):
    N, T, U, S, V = shape
    logits, labels, starts, xn, yn = pr.make_band_case(sum(a * b for a, b in zip(shape, (7, 5, 3, 11, 1))), N, T, U, S, V,
                                                       blank=blank)
    if shape == SHAPES[0]:
        xn[:], yn[:] = (12, 1, 6), (5, 0, 0)
        starts = pr.feasible_starts(np.random.RandomState(1), T, U, S, xn, yn)
    if S == U:
        starts[:] = 0
    if shape == STEPS:
        xn[:], yn[:] = 8, 8
        starts = np.array([[0, 0, 1, 3, 3, 4, 6, 6], [0, 0, 3, 3, 4, 6, 6, 6], [0, 1, 0, 2, 4, 5, 6, 6],
                           [0, 2, 20, 2, 4, 6, 6, 6]], np.int32)
    for a in (logits, labels, starts, xn, yn):
        a.setflags(write=False)
    return logits, labels, starts, xn, yn


def grid_pairs(shape):
    N, T, U, S, V = shape                                 # a grid of 1/4: ties everywhere, sums exact in fp32
    return (-np.random.RandomState(N * T + S).randint(0, 16, size=(N, T, S, 2)) / 4.0).astype(np.float32)


def raw_align(kind, x, labels, starts, xn, yn, U, blank, topology, dp):
    """The C entry on a NaN-filled workspace, outputs in poisoned guards: scores, emit_frames, the band pairs left."""
    import warp_rnnt_amd
    from warp_rnnt_amd import ops
    L = warp_rnnt_amd.load()
    N, T, S, V = x.shape
    topo = TOPOLOGY[topology]
    size = L.rnnt_amd_pruned_align_workspace_size(N, T, S, topo)
    assert size > 0 and size % 4 == 0
    ws = torch.full((size // 4,), float("nan"), dtype=torch.float32, device=DEV)
    sbuf = torch.full((N + 2 * GUARD,), float("nan"), dtype=torch.float32, device=DEV)
    ebuf = torch.full((N * (U - 1) + 2 * GUARD,), SENTINEL, dtype=torch.int32, device=DEV)
    tl, ts, txn, tyn = (dev(labels) if U > 1 else None), dev(starts), dev(xn), dev(yn)
    st = L.rnnt_amd_pruned_align(torch.cuda.current_stream().cuda_stream, ws.data_ptr(), KINDS[kind],
                                 ops.LOGITS_DTYPES[x.dtype], x.data_ptr(), None if tl is None else tl.data_ptr(),
                                 ts.data_ptr(), txn.data_ptr(), tyn.data_ptr(), sbuf[GUARD:].data_ptr(),
                                 None if U == 1 else ebuf[GUARD:].data_ptr(), N, T, U, S, V, blank, topo, dp)
    assert st == 0, st
    torch.cuda.synchronize()
    sbuf, ebuf = sbuf.cpu().numpy(), ebuf.cpu().numpy()
    assert np.isnan(sbuf[:GUARD]).all() and np.isnan(sbuf[GUARD + N:]).all()
    assert (ebuf[:GUARD] == SENTINEL).all() and (ebuf[GUARD + N * (U - 1):] == SENTINEL).all()
    pairs = ws[:2 * N * T * S].cpu().numpy().reshape(N, T, S, 2)
    return sbuf[GUARD:GUARD + N], ebuf[GUARD:GUARD + N * (U - 1)].reshape(N, U - 1), pairs


def want_pairs(kind, x, labels, starts, xn, yn, U, blank, dp):
    """The definition's band pairs (N,T,S,2) in fp64, from the input as the entry receives it (a half tensor: its upcast):
    log-softmax or HAT log-probs of the row's blank and label, the delay penalty, -inf off the band and from column U_n."""
    z = x.double().cpu().numpy()
    N, T, S = z.shape[:3]
    t, Tn, Un = np.arange(T)[None, :, None], xn[:, None, None], yn[:, None, None]
    u = starts[:, :, None].astype(np.int64) + np.arange(S)
    live = (u >= 0) & (u < U) & (t < Tn) & (u <= Un)
    if kind == "pairs":
        b, l = z[..., 0], z[..., 1]
    else:
        lp = hr.hat_log_probs64(z, blank) if kind == "hat_logits" else transduce_np.log_softmax(z)
        label = np.concatenate([labels, np.full((N, 1), blank, labels.dtype)], axis=1)[np.arange(N)[:, None, None],
                                                                                      np.clip(u, 0, U - 1)]
        b, l = lp[..., blank], np.take_along_axis(lp, label[..., None].astype(np.int64), axis=-1)[..., 0]
    l = l + float(np.float32(dp)) * ((Tn - 1) / 2.0 - t)
    return np.stack([np.where(live, b, -np.inf), np.where(live & (u < Un), l, -np.inf)], axis=-1)


def pair_bar(V, magnitude):
    """Of one pair against fp64: the project's per-value log-softmax bar (tests/test_gpu_lsm_routes.py), and eight more
    roundings at most -- HAT's softplus (exp, log1p, add) and its sum with log q, the penalty's product and its add --
    each within an ulp (2 EPS) of a magnitude that |pair| + 1 bounds.
    The largest error measured on this file's cases: 9.9e-7, HAT at (2,9,5,3,1030), where the bar is 1.5e-5."""
    return 2e-6 * max(1.0, math.log(V)) + 16 * EPS * (1.0 + magnitude)


def expected(pairs, starts, xn, yn, U, topology):
    scores = np.zeros((len(pairs),), np.float32)
    emit = np.full((len(pairs), U - 1), -1, np.int32)
    for n in range(len(pairs)):
        scores[n], e = par.VITERBI32[topology](*par.scatter(pairs[n], starts[n], U), xn[n], yn[n])
        if np.isfinite(scores[n]):
            emit[n, :yn[n]] = e
    return scores, emit


def assert_bits(got, want):
    (scores, emit), (want_scores, want_emit) = got[:2], want
    assert (scores.view(np.int32)[~np.isnan(want_scores)] == want_scores.view(np.int32)[~np.isnan(want_scores)]).all() and \
        np.isnan(scores[np.isnan(want_scores)]).all(), (scores, want_scores)
    assert (emit == want_emit).all(), np.argwhere(emit != want_emit)[:5]


def check_bits(shape, kind, topology, dp, dtype="f32", which=0):
    N, T, U, S, V = shape
    blank = (0, V // 2, V - 1)[which]
    logits, labels, starts, xn, yn = case(shape, blank)
    x = dev(grid_pairs(shape)) if kind == "pairs" else dev(logits).to(HALF[dtype])
    got = raw_align(kind, x, labels, starts, xn, yn, U, blank, topology, dp)
    ref = want_pairs(kind, x, labels, starts, xn, yn, U, blank, dp)
    there = np.isfinite(ref)
    assert (np.isneginf(got[2]) == ~there).all()          # every row written, and still there; -inf exactly off the band
    err, bar = np.abs(got[2][there] - ref[there]), pair_bar(V, np.abs(ref[there]))
    want = expected(got[2], starts, xn, yn, U, topology)
    print(f"{shape} {kind} {topology} dp={dp} {dtype} b{which}: pairs off fp64 by {err.max():.3e} (bar {bar.min():.3e}), "
          f"scores {got[0].tolist()}")
    assert (err <= bar).all()
    assert_bits(got, want)
    return want[0]


# ---- 1. the pairs against fp64, the path on them bit for bit ----

@pytest.mark.parametrize("dp", [0.0, 0.01])
@pytest.mark.parametrize("topology", list(TOPOLOGY))
@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("shape", SHAPES, ids=["N%d-T%d-U%d-S%d-V%d" % s for s in SHAPES])
def test_scores_and_emit_frames_are_the_reference_bits(shape, kind, topology, dp):
    want = check_bits(shape, kind, topology, dp)
    if shape == STEPS:                                    # a step of S and a row outside the grid disconnect the band;
        assert np.isinf(want[[1, 3]]).all() and np.isfinite(want[[0, 2]]).all()          # cell (t,t) is in the other two
    elif topology == "regular":
        assert np.isfinite(want).all()


@pytest.mark.parametrize("dtype,which", [("f32", 1), ("f32", 2), ("bf16", 0), ("f16", 0)])
@pytest.mark.parametrize("kind", ["logits", "hat_logits"])
def test_blank_positions_and_half_precision_are_the_reference_bits(kind, dtype, which):
    for topology in TOPOLOGY:
        check_bits((2, 9, 5, 3, 65), kind, topology, 0.01, dtype, which)


# ---- 2. the tie rule, and the references against enumeration ----

@pytest.mark.parametrize("topology", list(TOPOLOGY))
def test_ties_are_broken_as_the_enumeration_says(topology):
    N, T, U, S = 12, 6, 4, 4
    rng = np.random.RandomState(5)
    xn, yn = rng.randint(4, T + 1, size=N).astype(np.int32), rng.randint(2, U, size=N).astype(np.int32)
    starts, labels = np.zeros((N, T), np.int32), np.zeros((N, U - 1), np.int32)
    x = (-rng.randint(0, 2, size=(N, T, S, 2)) / 4.0).astype(np.float32)          # two values: most lattices tie
    scores, emit, pairs = raw_align("pairs", dev(x), labels, starts, xn, yn, U, 0, topology, 0.0)
    tied = 0
    for n in range(N):
        b, l = par.scatter(pairs[n], starts[n], U)
        s, e, count = par.ENUMERATION[topology](b, l, xn[n], yn[n])
        tied += count > 1
        assert float(scores[n]) == s and (emit[n, :yn[n]] == e).all(), (n, emit[n], e)
        for viterbi in (par.VITERBI32, par.VITERBI64):    # (the references themselves, on the same lattices)
            sv, ev = viterbi[topology](b, l, xn[n], yn[n])
            assert float(sv) == s == par.PATH_SCORE64[topology](e, b, l, xn[n]) and (ev == e).all(), n
    print(f"{topology}: {tied} of {N} lattices have more than one maximal path")
    assert tied >= 3


# ---- 3. what the path means, against fp64; 5. the loss as an upper bound ----

@pytest.mark.parametrize("topology", list(TOPOLOGY))
@pytest.mark.parametrize("kind", ["logits", "hat_logits"])
@pytest.mark.parametrize("shape,which", [(SHAPES[0], 0), ((2, 20, 19, 16, 5), 1), ((2, 129, 8, 3, 5), 0),
                                         ((2, 9, 5, 3, 1030), 2)])
def test_the_path_is_the_best_path_in_fp64_and_cannot_beat_the_loss(shape, which, kind, topology):
    from warp_rnnt_amd.pruned import pruned_rnnt_align, pruned_rnnt_loss_from_logits
    N, T, U, S, V = shape
    dp, blank = 0.01, (0, V // 2, V - 1)[which]
    logits, labels, starts, xn, yn = case(shape, blank)
    args = (dev(logits), dev(labels), dev(starts), dev(xn), dev(yn))
    scores, emit = (a.cpu().numpy() for a in pruned_rnnt_align(*args, blank=blank, kind=kind, rnnt_type=topology,
                                                               delay_penalty=dp))
    with torch.no_grad():
        cost = pruned_rnnt_loss_from_logits(*args, blank=blank, rnnt_type=topology, delay_penalty=dp,
                                            use_hat_loss=kind == "hat_logits").double().cpu().numpy()
    ref = want_pairs(kind, args[0], labels, starts, xn, yn, U, blank, dp)
    for n in range(N):
        Tn, Un = int(xn[n]), int(yn[n])
        b, l = par.scatter(ref[n], starts[n], U)
        best64, frames64 = par.VITERBI64[topology](b, l, Tn, Un)
        if not np.isfinite(scores[n]):                    # (modified: T_n < U_n, or a band the modified path cannot climb)
            assert np.isinf(best64) and np.isinf(cost[n]) and (emit[n] == -1).all()
            continue
        best64 = par.PATH_SCORE64[topology](frames64, b, l, Tn)
        s = par.PATH_SCORE64[topology](emit[n, :Un], b, l, Tn)
        # pair_bar on every edge (the magnitudes of a path's pairs sum to |s|, but for the penalties above zero), and the
        # rounding of T_n + U_n fp32 adds on either path: the form of tests/test_gpu_align.py
        bar = pair_bar(V, 0.0) * (Tn + Un) + 16 * EPS * (abs(s) + dp * Tn * Un) + 2 * (Tn + Un) * EPS * abs(s)
        print(f"{shape} b{which} {kind} {topology} n={n}: best64 - s = {best64 - s:.3e}, |score - s| = "
              f"{abs(float(scores[n]) - s):.3e}, score + cost = {float(scores[n]) + cost[n]:.3e}, bar {bar:.3e}")
        assert 0 <= best64 - s <= bar and abs(float(scores[n]) - s) <= bar, n
        assert float(scores[n]) + cost[n] <= bar, n


# ---- 4. the dense entry ----

def test_the_whole_lattice_as_band_gives_the_dense_entry_bits():
    from warp_rnnt_amd.align import rnnt_align
    from warp_rnnt_amd.pruned import pruned_rnnt_align
    _, labels, starts, xn, yn = case((3, 12, 6, 2, 5))
    x, tl, txn, tyn = dev(grid_pairs((3, 12, 6, 6, 2))), dev(labels), dev(xn), dev(yn)
    got = pruned_rnnt_align(x, tl, torch.zeros((3, 12), dtype=torch.int32, device=DEV), txn, tyn, kind="pairs")
    want = rnnt_align(x, tl, txn, tyn, kind="gathered")
    assert torch.equal(got[0].view(torch.int32), want[0].view(torch.int32)) and torch.equal(got[1], want[1])


# ---- 6. bits depend on the utterance alone; refused lengths ----

@pytest.mark.parametrize("topology", list(TOPOLOGY))
def test_bits_depend_on_the_utterance_alone_and_refused_lengths_touch_nothing_else(topology):
    N, T, U, S, V = shape = (4, 10, 5, 3, 5)
    logits, labels = case(shape)[:2]
    xn, yn = np.array([10, 9, 8, 7], np.int32), np.array([4, 3, 4, 2], np.int32)
    # a ramp up to U_n + 1 - S: u(t) = min((t + 1) // 2, U_n) is a path of either topology in every utterance
    starts = np.minimum(np.arange(T) // 2, np.maximum(yn + 1 - S, 0)[:, None]).astype(np.int32)
    x = dev(logits)
    batch = raw_align("logits", x, labels, starts, xn, yn, U, 0, topology, 0.01)
    assert np.isfinite(batch[0]).all() and (batch[1][np.arange(U - 1) < yn[:, None]] >= 0).all()
    for rows in ([2, 0, 3, 1], [0], [1], [2], [3]):       # shuffled, and every utterance in a batch of its own
        got = raw_align("logits", x[dev(rows)].contiguous(), labels[rows], starts[rows], xn[rows], yn[rows], U, 0,
                        topology, 0.01)
        assert_bits(got, (batch[0][rows], batch[1][rows]))
    for n, (bad_xn, bad_yn) in enumerate([(0, yn[0]), (T + 1, yn[1]), (xn[2], -1), (xn[3], U)]):
        xr, yr = xn.copy(), yn.copy()                     # one refused utterance at a time, the others as they were
        xr[n], yr[n] = bad_xn, bad_yn
        got = raw_align("logits", x, labels, starts, xr, yr, U, 0, topology, 0.01)          # (asserts the guards)
        want = (batch[0].copy(), batch[1].copy())
        want[0][n], want[1][n] = np.nan, -1
        assert_bits(got, want)


# ---- 7. graph capture ----

def test_align_replays_from_a_graph():
    from warp_rnnt_amd.pruned import pruned_rnnt_align
    _, labels, starts, xn, yn = case((2, 129, 8, 3, 5))
    rest = (dev(labels), dev(starts), dev(xn), dev(yn))
    batches = [dev(np.random.RandomState(s).randn(2, 129, 3, 5).astype(np.float32)) for s in (1, 2, 3)]
    want = [tuple(t.clone() for t in pruned_rnnt_align(b, *rest, delay_penalty=0.01)) for b in batches]
    assert not torch.equal(want[0][1], want[1][1])
    x = batches[0].clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        scores, emit = pruned_rnnt_align(x, *rest, delay_penalty=0.01)
    for rep in range(6):
        x.copy_(batches[rep % 3])
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(scores, want[rep % 3][0]) and torch.equal(emit, want[rep % 3][1]), f"replay {rep}"
