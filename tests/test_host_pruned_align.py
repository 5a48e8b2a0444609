"""Best-path alignments on the pruned band without a GPU: the C entry's refusals and sizes, the Python checks.  (The
references of tests/pruned_align_reference.py meet enumeration in tests/test_gpu_pruned_align.py, on the lattices of its
tie test.)"""
import ctypes

import pytest
import torch

INVALID, SUCCESS = 5, 0


def _lib():
    import warp_rnnt_amd
    from warp_rnnt_amd import _build
    _build.build()          # hipcc cross-compiles for gfx950 without a GPU; no-op when up to date
    return warp_rnnt_amd.load()


def test_entry_refuses_before_any_hip_call_and_the_size_is_the_shapes():
    """Made-up pointers and a null stream: every call is refused by a host-side check or is an empty batch."""
    L = _lib()
    p = ctypes.c_void_p(256)

    def call(ws=p, kind=0, dtype=0, x=p, labels=p, starts=p, xn=p, yn=p, scores=p, emit=p, N=2, T=3, U=4, S=2, V=5, blank=0,
             topology=0, dp=0.1):
        return L.rnnt_amd_pruned_align(None, ws, kind, dtype, x, labels, starts, xn, yn, scores, emit, N, T, U, S, V, blank,
                                       topology, dp)

    refused = [dict(kind=3), dict(kind=-1), dict(topology=2), dict(dtype=3), dict(kind=2, dtype=1), dict(V=1), dict(blank=5),
               dict(labels=None), dict(N=-1), dict(T=0), dict(S=0), dict(S=5), dict(S=65, U=70), dict(dp=-1.0),
               dict(dp=float("nan")), dict(ws=None), dict(ws=ctypes.c_void_p(264)), dict(x=None), dict(starts=None),
               dict(xn=None), dict(yn=None), dict(scores=None), dict(emit=None)]
    for kw in refused:
        assert call(**kw) == INVALID, kw
        if "N" not in kw:                        # a refused argument is not answered as an empty batch
            assert call(N=0, **kw) == INVALID, kw
    for topology in (0, 1):
        assert call(N=0, topology=topology) == SUCCESS and call(N=0, S=64, U=64, topology=topology) == SUCCESS
    assert call(N=0, kind=2, labels=None) == SUCCESS and call(N=0, U=1, S=1, labels=None, emit=None) == SUCCESS
    size = L.rnnt_amd_pruned_align_workspace_size
    up = lambda x: (x + 255) // 256 * 256
    for N, T, S in ((2, 3, 2), (16, 1500, 5), (1, 7, 64)):
        assert [size(N, T, S, k) for k in (0, 1)] == [up(8 * N * T * S) + up(8 * N * (T + k)) for k in (0, 1)]
    assert [size(2, 3, 65, 0), size(2, 0, 2, 0), size(-1, 3, 2, 0), size(2, 3, 2, 2), size(1 << 15, 1 << 15, 4, 0)] == [0] * 5


def test_python_checks_and_their_texts():
    from warp_rnnt_amd.pruned import pruned_rnnt_align
    x, labels, starts = torch.zeros(2, 3, 2, 5), torch.zeros(2, 3, dtype=torch.int32), torch.zeros(2, 3, dtype=torch.int32)
    n = torch.ones(2, dtype=torch.int32)
    with pytest.raises(ValueError, match="constrained"):
        pruned_rnnt_align(x, labels, starts, n, n, rnnt_type="constrained")
    with pytest.raises(ValueError, match="kind must be one of"):
        pruned_rnnt_align(x, labels, starts, n, n, kind="log_probs")
    with pytest.raises(ValueError, match="delay_penalty must be finite"):
        pruned_rnnt_align(x, labels, starts, n, n, delay_penalty=-1.0)
    with pytest.raises(RuntimeError, match="ranges must be an integer tensor"):
        pruned_rnnt_align(x, labels, starts.float(), n, n)
