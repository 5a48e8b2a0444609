"""ctc_align (csrc/ctc_align.hip) against its restatement in NumPy (tests/ctc_align_reference.py), bit for bit, and against
float64 where the emissions are the kernel's own.

Every batch is ragged, and every utterance meant to have a path has T_n >= L_n + its adjacent repeats (make() asserts it).
Two kinds of values: the log-softmax of Gaussian logits, and multiples of 1/4 in [-3, 0], whose sums are exact in fp32, so
ties between paths are real and the tie rule decides.

The float64 bars (test_logits_*): an emission is off float64 by at most the project's per-value log-softmax bar,
2e-6 max(1, log V) (tests/test_gpu_lsm_routes.py; used as in tests/test_gpu_pruned_align.py).  The returned path is the best
one of the kernel's plane, so on the float64 plane it can fall short of the best score by the emission errors of two paths
of T_n frames: 2 T_n bars."""
import functools
import itertools
import math

import numpy as np
import pytest
import torch

import ctc_align_reference as ref      # (tests/ is on the path: conftest.py's rootdir insert and pytest's own)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
B = 128                                # frames per block of the walk back at 32-bit decision words
# (N, T, L, V), blank, frames_lengths, labels_lengths
CASES = {
    "small": ((3, 7, 3, 5), 0, (7, 4, 1), (3, 0, 1)),               # one utterance without labels, one of a single frame
    "wave": ((2, 70, 63, 4), 3, (70, 61), (63, 50)),                # L + 1 = 64: a full wave at one position per lane
    "k2": ((2, 140, 64, 4), 0, (140, 90), (64, 33)),                # the first shape with two positions per lane
    "k3": ((2, 300, 130, 3), 1, (300, 177), (130, 65)),             # three positions, served by four: lanes partly filled
    "k16": ((1, 1100, 1023, 64), 0, (1100,), (1023,)),              # sixteen positions, 64-bit decision words
    "block-1": ((2, B - 1, 5, 6), 0, (B - 1, 9), (5, 4)),
    "block": ((2, B, 5, 6), 0, (B, B - 1), (5, 2)),
    "block+1": ((2, B + 1, 5, 6), 0, (B + 1, B), (5, 3)),
    "2block+1": ((2, 2 * B + 1, 5, 6), 0, (2 * B + 1, 2 * B), (5, 5)),
    "one-token": ((2, 12, 5, 2), 1, (12, 5), (5, 3)),               # every label the same token: no skip, every blank needed
}


@functools.lru_cache(maxsize=None)
def make(case, quantised):
    """values (N,T,V) float32, labels (N,L), frames_lengths, labels_lengths (int32 tensors on the CPU), blank."""
    (N, T, L, V), blank, xn, yn = CASES[case]
    gen = torch.Generator().manual_seed(1000 * T + L)
    others = [v for v in range(V) if v != blank]
    labels = torch.zeros(N, L, dtype=torch.int64)
    for n in range(N):
        for l in range(L):              # no two neighbours alike where the vocabulary allows it ...
            pick = [v for v in others if l == 0 or v != labels[n, l - 1]] or others
            labels[n, l] = pick[int(torch.randint(len(pick), (1,), generator=gen))]
        for l in (1, 3):                # ... but for two planted repeats, where the frames allow them
            if l < yn[n] and xn[n] >= yn[n] + ref.repeats(labels[n], yn[n]) + 2:
                labels[n, l] = labels[n, l - 1]
        assert xn[n] >= yn[n] + ref.repeats(labels[n], yn[n]), (case, n)
    if quantised:
        values = -torch.randint(0, 13, (N, T, V), generator=gen).float() / 4
    else:
        values = torch.log_softmax(2.0 * torch.randn(N, T, V, generator=gen), -1)
    return values, labels.int(), torch.tensor(xn, dtype=torch.int32), torch.tensor(yn, dtype=torch.int32), blank


def plane_of(values, labels, V, blank):
    """The emission plane (N,T,L+1) of values (N,T,V) as a NumPy array of their dtype."""
    tok = torch.where((labels >= 0) & (labels < V), labels, blank).long()
    cols = torch.cat([torch.full_like(tok[:, :1], blank), tok], 1)
    return torch.gather(values, 2, cols[:, None, :].expand(-1, values.shape[1], -1)).numpy()


@functools.lru_cache(maxsize=None)
def expected(case, quantised):
    values, labels, xn, yn, blank = make(case, quantised)
    return ref.align_fp32(plane_of(values, labels, values.shape[2], blank), labels.numpy(), xn, yn, values.shape[2], blank)


def run(values, labels, xn, yn, blank, kind="log_probs"):
    from warp_rnnt_amd.ctc import ctc_align
    out = ctc_align(values.to(DEV), labels.to(DEV), xn.to(DEV), yn.to(DEV), blank=blank, kind=kind)
    return tuple(x.cpu().numpy() for x in out)


def assert_bits(got, want):
    for g, w, name in zip(got, want, ("scores", "frame_tokens", "emit_frames")):
        assert g.dtype == w.dtype and g.shape == w.shape, name
        assert np.array_equal(g.view(np.int32), w.view(np.int32)), (name, g, w)


@pytest.mark.parametrize("quantised", [False, True], ids=["softmax", "quarters"])
@pytest.mark.parametrize("case", list(CASES))
def test_bits(case, quantised):
    want = expected(case, quantised)
    assert np.isfinite(want[0]).all() and (want[1][:, 0] >= 0).all()        # every utterance of these has a path
    assert_bits(run(*make(case, quantised)), want)


def test_meaning_by_enumeration():
    """T = 5, L = 2, V = 3 in quarters: every frame sequence that collapses to the labels, its exact score, and of the best
    ones the one the tie rule names: the greatest state sequence read from the last frame backwards."""
    T, V, blank = 5, 3, 0
    gen = torch.Generator().manual_seed(5)
    values = -torch.randint(0, 3, (2, T, V), generator=gen).float() / 4      # (three levels: many equal paths)
    labels, xn, yn = torch.tensor([[1, 2], [2, 2]], dtype=torch.int32), torch.tensor([5, 4]), torch.tensor([2, 2])
    scores, frame_tokens, _ = run(values, labels, xn.int(), yn.int(), blank)
    for n in range(2):
        Tn, want, best = int(xn[n]), labels[n].tolist(), {}
        for seq in itertools.product(range(V), repeat=Tn):
            if [k for k, _ in itertools.groupby(seq) if k != blank] != want:
                continue
            states, l = [], -1
            for t, k in enumerate(seq):
                l += k != blank and (t == 0 or seq[t - 1] != k)
                states.append(2 * l + 1 if k != blank else 2 * (l + 1))
            best[seq] = (sum(float(values[n, t, k]) for t, k in enumerate(seq)), states[::-1])
        top = max(best.values())
        assert tuple(frame_tokens[n, :Tn]) in best and float(scores[n]) == top[0]
        assert best[tuple(frame_tokens[n, :Tn])] == top


@pytest.mark.parametrize("name", list(DTYPES))
@pytest.mark.parametrize("case", ["small", "k2"])
def test_logits_give_the_loss_emissions_and_the_float64_best_path(case, name):
    from warp_rnnt_amd import _lib, ops
    from warp_rnnt_amd.ctc import ctc_loss_from_logits
    _, labels, xn, yn, blank = make(case, False)
    (N, T, L, V), gen = CASES[case][0], torch.Generator().manual_seed(7)
    logits = (2.0 * torch.randn(N, T, V, generator=gen)).to(DTYPES[name])
    dev = [x.to(DEV) for x in (logits, labels, xn, yn)]
    *out, ws = ops.ctc_align(*dev, _lib.CTC_ALIGN_IN_LOGITS, blank)
    off = ops.ctc_align_emissions_offset(N, T)
    plane = ws[off:off + 4 * N * T * (L + 1)].view(torch.float32).view(N, T, L + 1).cpu().numpy()
    got = tuple(x.cpu().numpy() for x in out)
    assert_bits(got, ref.align_fp32(plane, labels.numpy(), xn, yn, V, blank))
    plane64 = plane_of(torch.log_softmax(logits.double(), -1), labels, V, blank)
    cost = ctc_loss_from_logits(*dev, blank=blank, reduction="none").cpu().numpy()
    bar = 2e-6 * max(1.0, math.log(V))
    for n in range(N):
        Tn, Ln = int(xn[n]), int(yn[n])
        best64 = ref.best_score64(plane64[n], labels[n].numpy(), Tn, Ln, V, blank)
        path64 = ref.path_score64(plane64[n], got[1][n], labels[n].numpy(), Tn, Ln, V, blank)
        print(f"{case} {name} n={n}: best64 - path64 = {best64 - path64:.3e} (bar {2 * Tn * bar:.3e}), score + cost = "
              f"{float(got[0][n]) + float(cost[n]):.3e} (bar {bar:.3e})")
        assert -1e-9 <= best64 - path64 <= 2 * Tn * bar, n
        assert float(got[0][n]) + float(cost[n]) <= bar, n


def test_edges_no_path_and_refused_lengths_leave_the_others_alone():
    values, labels, xn, yn, blank = make("k2", True)
    values, labels = values[[0, 1, 0, 1, 0]].contiguous(), labels[[0, 1, 0, 1, 0]].contiguous()
    need = int(yn[0]) + ref.repeats(labels[0], int(yn[0]))
    xn5 = torch.tensor([int(xn[0]), 0, need - 1, int(xn[1]), 141], dtype=torch.int32)     # 1: refused; 2: no path; 4: refused
    yn5 = torch.tensor([int(yn[0]), 3, int(yn[0]), int(yn[1]), 2], dtype=torch.int32)
    scores, frame_tokens, emit_frames = run(values, labels, xn5, yn5, blank)
    assert np.isnan(scores[[1, 4]]).all() and scores[2] == -np.inf
    assert (frame_tokens[[1, 2, 4]] == -1).all() and (emit_frames[[1, 2, 4]] == -1).all()
    assert_bits((scores[[0, 3]], frame_tokens[[0, 3]], emit_frames[[0, 3]]), expected("k2", True))
    yn5[4] = 65                                                                          # labels_lengths past L
    assert np.isnan(run(values, labels, xn5.clamp(max=140), yn5, blank)[0][4])


def test_graph_replay_gives_the_eager_bits():
    from warp_rnnt_amd.ctc import ctc_align
    values, labels, xn, yn, blank = (x.to(DEV) if isinstance(x, torch.Tensor) else x for x in make("k3", False))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ctc_align(values, labels, xn, yn, blank=blank, kind="log_probs")      # (warm-up outside the capture)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ctc_align(values, labels, xn, yn, blank=blank, kind="log_probs")
    for _ in range(3):                                  # several replays, each against the eager result
        for x in out:
            x.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert_bits(tuple(x.cpu().numpy() for x in out), expected("k3", False))
