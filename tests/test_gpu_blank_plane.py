"""The blank column as a plane of its own: ops.log_softmax keeps column 0 of the log-probs as a contiguous
(N*T*U,) plane beside them and a dense loss that is handed the same, unchanged tensor reads the blank from it -- the gather
then fetches one dword per row instead of two.  Everything here is an equality of bits: the plane holds the floats of the
column, and costs and gradients with the plane are those without it.

No counterpart in the reference (its gather is torch.gather on an int64 index, warp_rnnt/__init__.py:118-128)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GUARD = 64           # floats behind the plane that must stay untouched


def _lib_and_stream(torch):
    from warp_rnnt_amd import _lib
    return _lib.load(), torch.cuda.current_stream().cuda_stream


# V -> the body dispatch_lsm_map<LSM_NORM> chooses (csrc/lsm.h), every one of them at least once:
#   k_lsm_regs, rows per group 1 / 2 / 3 / 4: V = 100 / 50 / 36 / 32 (V >= 32, KR*V % 4 == 0, 20 <= KR*V/4 <= 32)
#   k_lsm_small wave-private, L = 1 / 2 / 4 / 16 lanes per row: V = 6 / 28 / 51 / 200 (51: odd, q = 13 straight-line pass)
#   k_lsm_small, whole workgroup per tile (L = 32 / 64): V = 300 / 600
#   k_lsm_large as one row per small workgroup (128 < V <= 1024, >= 94 % of the lanes busy): V = 256 (64 x 1), 1000 (256 x 1)
#   k_lsm_large, V > 1024: 1028 (256 x 2), 5000 (512 x 3), 10000 (896 x 3: the predicated loads)
#   k_lsm_generic: V = 1030 (V > 1024, not a multiple of 4)
# (k_lsm_rows serves the fused gather only: the plain log-softmax never takes it.)
# Rows: N*T*U = 2*33*34 = 2244, no multiple of a tile (and 1*33*35 = 1155, odd: rows left over behind k_lsm_regs' groups of
# 2 and 4, which the LDS-staged kernel then serves WITH its slice of the plane); V > 1024: 2*5*4 = 40 rows.
SMALL_V = [6, 28, 32, 36, 50, 51, 100, 200, 256, 300, 600, 1000]
LARGE_V = [1028, 1030, 5000, 10000]
CASES = [(2244, V) for V in SMALL_V] + [(1155, V) for V in (32, 50)] + [(40, V) for V in LARGE_V]


@pytest.mark.parametrize("rows,V", CASES)
def test_plane_is_the_column_and_rows_are_unchanged(rows, V):
    import torch
    L, stream = _lib_and_stream(torch)
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(1000 + V + rows)
    x = (torch.randn(rows, V, generator=g) * 3.0).to(dev)
    want = torch.empty_like(x)
    assert L.rnnt_amd_log_softmax(stream, x.data_ptr(), want.data_ptr(), rows, V) == 0
    for col in (0, V - 1):
        out = torch.full_like(x, float("nan"))
        plane = torch.full((rows + GUARD,), -7.0, device=dev)
        assert L.rnnt_amd_log_softmax_plane(stream, x.data_ptr(), out.data_ptr(), plane.data_ptr(), rows, V, col) == 0
        assert torch.equal(out, want), f"col {col}: rows differ from rnnt_amd_log_softmax"
        assert torch.equal(plane[:rows], out[:, col]), f"col {col}: plane != out[:, col]"
        assert bool((plane[rows:] == -7.0).all()), f"col {col}: written behind the plane"
    # in place
    xi = x.clone()
    plane = torch.full((rows + GUARD,), -7.0, device=dev)
    assert L.rnnt_amd_log_softmax_plane(stream, xi.data_ptr(), xi.data_ptr(), plane.data_ptr(), rows, V, 0) == 0
    assert torch.equal(xi, want) and torch.equal(plane[:rows], want[:, 0])
    assert bool((plane[rows:] == -7.0).all())


@pytest.mark.parametrize("dtype", ["bfloat16", "float16"])
def test_typed_entry_keeps_the_plane_too(dtype):
    import torch
    from warp_rnnt_amd import _lib
    L, stream = _lib_and_stream(torch)
    dev = torch.device("cuda:0")
    rows, V = 1155, 50
    x = (torch.randn(rows, V, generator=torch.Generator().manual_seed(3)) * 3.0).to(dev).to(getattr(torch, dtype))
    code = {"bfloat16": _lib.DTYPE_BF16, "float16": _lib.DTYPE_F16}[dtype]
    want = torch.empty((rows, V), device=dev)
    assert L.rnnt_amd_log_softmax_typed(stream, code, x.data_ptr(), want.data_ptr(), rows, V) == 0
    out = torch.empty_like(want)
    plane = torch.full((rows + GUARD,), -7.0, device=dev)
    assert L.rnnt_amd_log_softmax_plane_typed(stream, code, x.data_ptr(), out.data_ptr(), plane.data_ptr(), rows, V,
                                              V - 1) == 0
    assert torch.equal(out, want) and torch.equal(plane[:rows], out[:, V - 1])
    assert bool((plane[rows:] == -7.0).all())


def _batch(torch, N, T, U, V, blank, seed):
    """Ragged: a full-length utterance, one of a single frame and no label, one in between; labels that include the blank."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    logits = torch.randn(N, T, U, V, generator=g) * 2.0
    labels = torch.randint(0, V, (N, U - 1), generator=g, dtype=torch.int32)
    labels[:, ::3] = blank
    xn = torch.tensor([T, 1, max(1, T // 2)] + [T] * (N - 3), dtype=torch.int32)[:N]
    yn = torch.tensor([U - 1, 0, (U - 1) // 2] + [U - 1] * (N - 3), dtype=torch.int32)[:N]
    dev = torch.device("cuda:0")
    return logits.to(dev), labels.to(dev), xn.to(dev), yn.to(dev)


def _both_ways(torch, logits, labels, xn, yn, blank, lam):
    """(with the plane, without) for every gradient layout of the dense entry, and whether the plane was taken."""
    from warp_rnnt_amd import debug, ops
    planed = ops.log_softmax(logits, blank_plane=True)
    plain = ops.log_softmax(logits, blank_plane=False)
    assert getattr(plain, ops.PLANE_ATTR, None) is None and torch.equal(planed, plain)
    note = getattr(planed, ops.PLANE_ATTR)
    assert torch.equal(note[0], plain[..., 0].reshape(-1))
    res = []
    for kind in (ops.GRADS_GATHERED, ops.GRADS_GATHERED_DIAGONAL, ops.GRADS_DENSE):
        a = ops.loss(planed, labels, xn, yn, ops.IN_LOG_PROBS_DENSE, kind, blank, lam)
        took = debug.last_loss_used_blank_plane()
        b = ops.loss(plain, labels, xn, yn, ops.IN_LOG_PROBS_DENSE, kind, blank, lam)
        assert not debug.last_loss_used_blank_plane()
        res.append((kind, a, b, took))
    return res


# the edges of both axes of the gather's 32 x 32 tiles (and of the 8-frame tiles small problems take); V = 50: rows of 200
# bytes, V = 130: rows that are not 8-byte multiples of a line either
@pytest.mark.parametrize("V", [50, 130])
@pytest.mark.parametrize("U", [2, 33, 34])
@pytest.mark.parametrize("T", [31, 32, 33, 65])
def test_loss_with_the_plane_is_the_loss_without_it(T, U, V):
    import torch
    N = 3
    lam = 0.01 if (T, U, V) == (33, 34, 50) else 0.0
    for blank in (0, 3):
        logits, labels, xn, yn = _batch(torch, N, T, U, V, blank, seed=T * 1000 + U * 10 + blank)
        for kind, (ca, ga), (cb, gb), took in _both_ways(torch, logits, labels, xn, yn, blank, lam):
            # the plane holds column 0: a loss with another blank must not take it
            assert took == (blank == 0), (kind, blank, took)
            assert torch.equal(ca, cb), f"costs differ (grads_kind {kind}, blank {blank})"
            assert torch.equal(ga, gb), f"gradients differ (grads_kind {kind}, blank {blank})"


def test_the_32_frame_tiles_take_the_plane_too():
    """512 tiles of 32 x 32 and more: k_to_diagonal's 32-frame form (the shapes above all run its 8-frame form)."""
    import torch
    N, T, U, V = 22, 65, 257, 50
    assert N * ((T + 31) // 32) * ((U + 31) // 32) >= 512
    logits, labels, xn, yn = _batch(torch, N, T, U, V, 0, seed=11)
    for kind, (ca, ga), (cb, gb), took in _both_ways(torch, logits, labels, xn, yn, 0, 0.0):
        assert took
        assert torch.equal(ca, cb) and torch.equal(ga, gb), f"grads_kind {kind}"


def _loss_and_grad(torch, lp, labels, xn, yn):
    import warp_rnnt
    lp = lp.requires_grad_(True)
    warp_rnnt.rnnt_loss(lp, labels, xn, yn, gather=True, reduction="sum").backward()
    return lp.grad


def test_a_stale_or_foreign_plane_is_never_used():
    import torch
    import warp_rnnt
    from warp_rnnt_amd import debug, ops
    N, T, U, V = 3, 33, 34, 50
    logits, labels, xn, yn = _batch(torch, N, T, U, V, 0, seed=5)
    other = torch.log_softmax(logits.flip(0) * 0.5, -1)

    def check(lp, takes_plane, what):
        """rnnt_loss(lp) against a clone of lp that never had a plane; which path ran is asked, not timed."""
        fresh = lp.detach().clone()
        got = warp_rnnt.rnnt_loss(lp, labels, xn, yn, gather=True)
        assert debug.last_loss_used_blank_plane() == takes_plane, what
        want = warp_rnnt.rnnt_loss(fresh, labels, xn, yn, gather=True)
        assert not debug.last_loss_used_blank_plane(), what
        assert torch.equal(got, want), what

    check(ops.log_softmax(logits, blank_plane=True), True, "untouched")
    lp = ops.log_softmax(logits, blank_plane=True)
    lp.add_(1.0)
    check(lp, False, "add_")
    lp = ops.log_softmax(logits, blank_plane=True)
    lp.copy_(other)
    check(lp, False, "copy_")
    lp = ops.log_softmax(logits, blank_plane=True)
    ops.log_softmax(logits.flip(0).contiguous(), out=lp, blank_plane=False)       # a raw-pointer write: no version bump
    assert ops.blank_plane_of(lp, 0) is None
    check(lp, False, "log_softmax(out=lp) without a plane")
    ops.log_softmax(logits * 0.25, out=lp, blank_plane=True)                      # ... and with a fresh one
    check(lp, True, "log_softmax(out=lp) with a fresh plane")
    lp = ops.log_softmax(logits, blank_plane=True)
    check(lp.view(N, T, U, V), False, "a view")
    check(lp[:], False, "a slice")
    check(lp.clone(), False, "a clone")
    check(lp, True, "the tensor itself, afterwards")
    # the other entries that write through a raw pointer drop the note as well
    for write in (lambda t: ops.log_softmax_backward(other, other, grad_in=t),
                  lambda t: ops.logits_backward(logits, labels, torch.zeros(N, T, U, 2, device=t.device),
                                                torch.ones(N, device=t.device), out=t)):
        lp = ops.log_softmax(logits, blank_plane=True)
        write(lp)
        assert ops.blank_plane_of(lp, 0) is None
    # gather=False keeps today's path
    lp = ops.log_softmax(logits, blank_plane=True)
    warp_rnnt.rnnt_loss(lp, labels, xn, yn, gather=False)
    assert not debug.last_loss_used_blank_plane()
    # and the gradients through the plane are those without it
    g1 = _loss_and_grad(torch, ops.log_softmax(logits, blank_plane=True), labels, xn, yn)
    assert debug.last_loss_used_blank_plane()
    g2 = _loss_and_grad(torch, ops.log_softmax(logits, blank_plane=False), labels, xn, yn)
    assert torch.equal(g1, g2)


def test_log_softmax_and_loss_replay_from_a_graph():
    import torch
    import warp_rnnt
    from warp_rnnt_amd import debug, ops
    N, T, U, V = 3, 65, 34, 50
    logits, labels, xn, yn = _batch(torch, N, T, U, V, 0, seed=9)
    batches = [logits, logits.flip(1).contiguous() * 0.5, logits.roll(1, 2) + 0.25]

    def step(x):
        return warp_rnnt.rnnt_loss(ops.log_softmax(x, blank_plane=True), labels, xn, yn, gather=True)

    eager = [step(b).clone() for b in batches]
    assert debug.last_loss_used_blank_plane()
    static = batches[0].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step(static)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        costs = step(static)
    assert debug.last_loss_used_blank_plane()
    for k in (1, 2):
        static.copy_(batches[k])
        graph.replay()
        torch.cuda.synchronize()
        np.testing.assert_array_equal(costs.cpu().numpy(), eager[k].cpu().numpy(), err_msg=f"replay with batch {k}")
