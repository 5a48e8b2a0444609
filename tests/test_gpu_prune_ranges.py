"""prune_ranges_hip on the GPU against a loop form of its definition in fp64 NumPy.  The bar is equality: occupancies on a
grid of 2^-12, at most 1, windows below 2048 terms -- every partial sum is exact in fp32, so both sides see the same ties.
Shapes: every lane-group width (U <= 128, <= 256, a wave), a row of several passes, the scans' chunk of 512 frames."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def reference(occ, xn, yn, S):
    """The definition, utterance by utterance and frame by frame; occ (N,T,U) fp64."""
    N, T, U = occ.shape
    out = np.zeros((N, T), np.int64)
    if S >= U:
        return out
    for n in range(N):
        hi = min(max(int(yn[n]) + 1 - S, 0), U - S)
        raw = np.full(T, hi, np.int64)
        w = np.lib.stride_tricks.sliding_window_view(occ[n], S, axis=1).sum(-1)          # (T, U-S+1)
        for t in range(min(max(int(xn[n]) - 1, 0), T)):
            if not np.isnan(occ[n, t, :hi + S]).any():
                raw[t] = int(np.argmax(w[t, :hi + 1]))                                   # (numpy: the first of equal maxima)
        for scan in (lambda a, b: min(a, b), lambda a, b: max(a, b - (S - 1))):
            for t in range(T - 2, -1, -1):
                raw[t] = scan(raw[t], raw[t + 1])
        out[n] = raw
    return out


dyadic = lambda rng, *shape: rng.randint(0, 4097, shape) / 4096.0  # noqa: E731


def pairs_of(occ, rng):
    """(N,T,U,2) fp32 with -(g0 + g1) = occ exactly: split unevenly on the grid, a third each with a zero blank / label channel."""
    k = np.round(occ * 4096)
    kind = rng.randint(0, 3, occ.shape)
    kb = np.where(kind == 0, 0, np.where(kind == 1, k, np.floor(np.nan_to_num(k) * rng.rand(*occ.shape))))
    return torch.tensor(-np.stack([kb, k - kb], -1) / 4096, dtype=torch.float32)


def run(pairs, xn, yn, S):
    from warp_rnnt_amd.pruned import prune_ranges_hip
    got = prune_ranges_hip(pairs.to(DEV), torch.tensor(xn, dtype=torch.int32, device=DEV),
                           torch.tensor(yn, dtype=torch.int32, device=DEV), S)
    assert got.dtype == torch.int32 and tuple(got.shape) == tuple(pairs.shape[:2]) and got.is_contiguous()
    return got.cpu().numpy()


CASES = sorted({(U, 65, S) for U in (63, 64, 65, 130, 300, 1100) for S in (2, 5, 8, U - 1)} |
               {(S + d, 65, S) for S in (2, 5, 8) for d in (0, 1)} |
               {(130, T, S) for T in (1, 2, 63, 64, 65, 200) for S in (2, 5)} |
               {(65, T, 5) for T in (511, 512, 513, 1030)} | {(4096, 2, 5)})          # (4096: the entry's limit)


@pytest.mark.parametrize("U,T,S", CASES)
def test_dyadic_occupancies_equal_fp64(U, T, S):
    """N = 3, ragged: full length; a single frame (infeasible where U > S: start[0] = hi > 0); U_n = 0 or S - 2 (hi = 0)."""
    rng = np.random.RandomState(1000 * U + 10 * T + S)
    occ = dyadic(rng, 3, T, U)
    xn, yn = [T, 1, max(T - 3, 1)], [U - 1, U - 1, (0, S - 2)[(U + T) % 2]]
    np.testing.assert_array_equal(run(pairs_of(occ, rng), xn, yn, S), reference(occ, xn, yn, S))


@pytest.mark.parametrize("U", (100, 130, 300, 1100))
def test_rows_built_to_tie_and_lengths_of_every_kind(U):
    """Frame 0 of utterances 0 to 3: a constant row (0); a plateau of equal best windows (20); one best window across u = 64
    (62: two lanes, two passes); equal best windows at 63 and 64, in different lanes and passes (63).  The frames behind hold
    one best window at the same place, so the scans hand frame 0's choice to start[0].  Utterance 4 is infeasible over
    several frames, 5 to 7 have T_n above T, zero and negative."""
    S, T, N, first = 5, 40, 8, [0, 20, 62, 63]
    rng = np.random.RandomState(U)
    occ = dyadic(rng, N, T, U) / 8
    for n, e in enumerate(first):
        occ[n, 1:, e:e + S] = 1.0
    occ[0, 0], occ[1, 0, 20:40], occ[2, 0, 62:67] = 0.25, 0.5, 1.0
    occ[3, 0, 63], occ[3, 0, 64:68], occ[3, 0, 68] = 1.0, 0.5, 1.0
    xn, yn = [T] * 4 + [4, T + 5, 0, -3], [e + S - 1 + 30 for e in first] + [U - 1, U - 2, U - 1, 7]
    want = reference(occ, xn, yn, S)
    assert want[:4, 0].tolist() == first and want[4, 0] == U - S - 12 > 0 and (want[6] == U - S).all()
    np.testing.assert_array_equal(run(pairs_of(occ, rng), xn, yn, S), want)


def test_nan_inside_and_outside_the_cells_a_window_can_touch():
    N, T, U, S = 2, 6, 130, 5
    rng = np.random.RandomState(3)
    occ = dyadic(rng, N, T, U)
    xn, yn = [T, T], [40, U - 1]                   # utterance 0: hi = 36, windows touch u < 41
    clean = reference(occ, xn, yn, S)
    occ[0, 1, 41] = occ[0, 3, 129] = np.nan        # outside: nothing changes
    np.testing.assert_array_equal(run(pairs_of(occ, rng), xn, yn, S), clean)
    occ[0, 2, 40] = occ[1, 0, 77] = np.nan         # inside: those frames' raw start is hi
    want = reference(occ, xn, yn, S)
    assert (want != clean).any()
    np.testing.assert_array_equal(run(pairs_of(occ, rng), xn, yn, S), want)


def test_strided_view_of_the_modified_pairs_is_read_in_place():
    N, T, U, S = 3, 70, 66, 5
    rng = np.random.RandomState(4)
    occ = dyadic(rng, N, T, U)
    buf = torch.full((N, T + 1, U, 2), -3e30)      # row T: garbage that would win every window
    buf[:, :T] = pairs_of(occ, rng)
    xn, yn = [T, T - 9, 33], [U - 1, 30, U - 7]
    np.testing.assert_array_equal(run(buf.to(DEV)[:, :T], xn, yn, S), reference(occ, xn, yn, S))


@pytest.mark.parametrize("U,S", [(66, 5), (300, 5), (300, 2)])
def test_real_valued_occupancies_batch_independence_and_invariants(U, S):
    T = 90
    rng = np.random.RandomState(U + S)
    occ = rng.rand(4, T, U).astype(np.float32)
    g = torch.tensor(-np.stack([occ * 0.3, occ * 0.7], -1))
    xn, yn = np.array([T, T - 11, 40, 3]), np.array([U - 1, U // 2, S - 2, U - 1])      # (utterance 3 is infeasible)
    alone = [run(g[n:n + 1], xn[n:n + 1], yn[n:n + 1], S)[0] for n in range(4)]
    for order in ([0, 1, 2], [2, 0, 1], [1, 3, 0]):
        np.testing.assert_array_equal(run(g[order], xn[order], yn[order], S), np.stack([alone[n] for n in order]))
    for n in range(4):
        hi, d = min(max(yn[n] + 1 - S, 0), U - S), np.diff(alone[n])
        assert (d >= 0).all() and (d <= S - 1).all() and (alone[n][xn[n] - 1:] == hi).all()
        if (xn[n] - 1) * (S - 1) >= yn[n] + 1 - S:
            assert alone[n].min() >= 0 and alone[n].max() + S <= max(yn[n] + 1, S)


@pytest.mark.parametrize("rnnt_type", ["regular", "modified"])
def test_the_recipe_end_to_end(rnnt_type):
    from warp_rnnt_amd.pruned import prune_joint_inputs, prune_ranges_hip, pruned_rnnt_loss_from_logits
    from warp_rnnt_amd.simple import simple_rnnt_loss
    N, T, U, S, V, H = 3, 40, 12, 5, 33, 32
    gen = torch.Generator().manual_seed(12)
    f, g = (torch.randn(N, T, H, generator=gen) * 0.7).to(DEV), (torch.randn(N, U, H, generator=gen) * 0.7).to(DEV)
    am_w, lm_w, w = ((torch.randn(H, V, generator=gen) / H ** 0.5).to(DEV).requires_grad_(True) for _ in range(3))
    labels = torch.randint(1, V, (N, U - 1), generator=gen, dtype=torch.int32).to(DEV)
    xn, yn = torch.tensor([T, T - 7, 25], dtype=torch.int32).to(DEV), torch.tensor([U - 1, U - 4, 6], dtype=torch.int32).to(DEV)
    simple, pair_grads = simple_rnnt_loss((f @ am_w).contiguous(), (g @ lm_w).contiguous(), labels, xn, yn,
                                          lm_only_scale=0.25, return_grad=True, rnnt_type=rnnt_type)
    starts = prune_ranges_hip(pair_grads, xn, yn, S)
    fp, gp = prune_joint_inputs(f, g, starts, S)
    loss = pruned_rnnt_loss_from_logits((torch.tanh(fp + gp) @ w).contiguous(), labels, starts, xn, yn, rnnt_type=rnnt_type)
    (0.5 * simple.sum() + loss.sum()).backward()
    assert torch.isfinite(loss).all() and torch.isfinite(w.grad).all() and (w.grad != 0).any() and (am_w.grad != 0).any()


def test_graph_replay_gives_the_eager_starts():
    from warp_rnnt_amd.pruned import prune_ranges_hip
    N, T, U, S = 3, 130, 300, 5
    rng = np.random.RandomState(6)
    batches = [pairs_of(dyadic(rng, N, T, U), rng).to(DEV) for _ in range(2)]
    xn, yn = torch.tensor([T, 77, 64], dtype=torch.int32).to(DEV), torch.tensor([U - 1, 150, 3], dtype=torch.int32).to(DEV)
    want = [prune_ranges_hip(b, xn, yn, S) for b in batches]
    static, graph = batches[0].clone(), torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = prune_ranges_hip(static, xn, yn, S)
    for rep in range(4):
        static.copy_(batches[rep % 2])
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(got, want[rep % 2]), f"replay {rep}"
