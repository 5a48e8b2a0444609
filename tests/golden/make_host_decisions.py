#!/usr/bin/env python
"""Generates tests/golden/host_decisions.json: what the C ABI decides on the host alone.

Two tables, recorded from a build of the library (the in-tree one, or the path given as the first argument):
  sizes  every workspace size / offset entry over a grid of shapes -- padded, compact, bounded, joint, align, TDT; valid and invalid,
         including both sides of each limit of the size checks;
  calls  for every status-returning entry the calls it answers WITHOUT launching anything: each reason it has to reject a
         call, one at a time (status 5), and its early successes (N == 0, STU == 0 where that is one, nothing requested).
         Calls that touch the device even when they refuse (STU == 0 on the bounded entries, a bad vocabulary on
         rnnt_amd_loss_compact_bounded, N == 0 on entries without that early return) are left out.

Needs no GPU and must not see one: the pointers are made-up addresses that only a call which returns before its first
launch may be given.  tests/test_host_decisions.py replays both tables against the library under test.

    python tests/golden/make_host_decisions.py [path/to/libwarp_rnnt_amd.so]
"""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from warp_rnnt_amd import _lib  # noqa: E402

P = 1 << 40                     # "a device pointer": non-null, 256-byte aligned, never dereferenced
DTYPES = (0, 1, 2)              # RNNT_DTYPE_F32 / BF16 / F16

# (N, T, U): both sides of every limit of the padded size check, and U on both sides of one 64-column block (the rings)
PADDED = [(0, 1, 1), (1, 1, 1), (2, 5, 3), (16, 150, 40), (16, 1500, 300), (3, 37, 64), (3, 37, 65), (1, 100, 513),
          (65535, 1, 1), (65536, 1, 1), (-1, 1, 1), (1, 0, 1), (1, 1, 0), (1, 1 << 15, (1 << 14) - 1),
          (1, 1 << 15, 1 << 14), (15, 1 << 14, 1 << 14), (16, 1 << 14, 1 << 14)]
# (N, STU, Tmax, Umax)
COMPACT = [(0, 0, 0, 0), (2, 0, 5, 3), (2, 23, 5, 3), (2, 23, 0, 0), (16, 5000000, 1500, 300), (3, 1000, 37, 64),
           (3, 1000, 37, 65), (65535, 65535, 1, 1), (65536, 65536, 1, 1), (-1, 1, 1, 1), (1, -1, 1, 1),
           (1, (1 << 32) - 1, 1 << 15, (1 << 14) - 1), (1, 1 << 32, 1 << 15, (1 << 14) - 1), (1, 100, 1 << 15, 1 << 14),
           (15, 100, 1 << 14, 1 << 14), (16, 100, 1 << 14, 1 << 14)]
# (N, T, U, H, V)
JOINT = [(2, 5, 3, 64, 8), (16, 150, 40, 640, 1024), (1, 1, 1, 32, 2), (1, 1, 1, 1024, 1 << 24), (3, 37, 65, 128, 100),
         (0, 5, 3, 64, 8), (65536, 5, 3, 64, 8), (2, 5, 3, 16, 8), (2, 5, 3, 48, 8), (2, 5, 3, 1056, 8), (2, 5, 3, 64, 1),
         (2, 5, 3, 64, (1 << 24) + 1), (16, 1 << 14, 1 << 14, 64, 8)]
# (N, T, U, D): both sides of every limit of the TDT size check -- the padded ones with U <= 1024 on top (one workgroup's
# columns: T * U < 2^29 and N * T * U < 2^32 are shown at U = 1024), and 1 <= D <= 9
TDT = [(2, 5, 3, 5), (16, 1500, 300, 5), (3, 20, 7, 4), (3, 37, 65, 2), (0, 5, 3, 5), (65535, 1, 1, 5), (65536, 1, 1, 5),
       (-1, 5, 3, 5), (2, 0, 3, 5), (2, 5, 0, 5), (1, 4, 1024, 5), (1, 4, 1025, 5), (2, 5, 3, 0), (2, 5, 3, 1), (2, 5, 3, 9),
       (2, 5, 3, 10), (1, (1 << 19) - 1, 1024, 1), (1, 1 << 19, 1024, 1), (15, 1 << 18, 1024, 9), (16, 1 << 18, 1024, 9)]
SIZES = [("rnnt_amd_workspace_size", PADDED), ("rnnt_amd_workspace_mismatch_offset", PADDED),
         ("rnnt_amd_debug_redo_offset", PADDED), ("rnnt_amd_workspace_size_compact", COMPACT),
         ("rnnt_amd_workspace_size_compact_bounded", COMPACT), ("rnnt_amd_joint_workspace_size", JOINT),
         ("rnnt_amd_align_workspace_size", PADDED), ("rnnt_amd_tdt_workspace_size", TDT)]

BAD_DIMS = [dict(N=-1), dict(T=0), dict(U=0), dict(N=65536), dict(T=1 << 15, U=1 << 14), dict(N=16, T=1 << 14, U=1 << 14)]
BAD_COMPACT_DIMS = [dict(N=-1), dict(N=65536), dict(STU=-1), dict(STU=1 << 32), dict(Tmax=1 << 15, Umax=1 << 14),
                    dict(N=16, Tmax=1 << 14, Umax=1 << 14)]
BAD_WORKSPACE = [dict(workspace=0), dict(workspace=P + 8)]
BAD_DTYPE = [dict(dtype=-1), dict(dtype=3)]
BAD_PLANE = [dict(rows=-1), dict(V=0), dict(col=-1), dict(col=7), dict(col_out=0)]


def bad_vocab(V):
    return [dict(V=0), dict(blank=-1), dict(blank=V)]


def entry(names, base, rejected, accepted):
    """One entry's rows: its valid `base` call (never made: it would launch) with each change of `rejected` / `accepted`."""
    names = names.split()
    assert set(base) == set(names), set(base) ^ set(names)
    return names, base, rejected, accepted


DIMS = dict(N=2, T=5, U=3)
CDIMS = dict(N=2, STU=23, Tmax=5, Umax=3)
LOSS = dict(stream=0, workspace=P, labels=P, xn=P, yn=P, costs=P, grads=P, grads_kind=1, V=7, blank=0, fastemit_lambda=0.0,
            **DIMS)
BAD_GRADS = [dict(grads_kind=-1), dict(grads_kind=4), dict(grads=0), dict(grads_kind=2, input_kind=1),
             dict(grads_kind=2, input_kind=2)]
COMPACT_LOSS = dict(stream=0, workspace=P, ys=P, xn=P, yn=P, costs=P, grads2=P, V=7, blank=0, fastemit_lambda=0.0, **CDIMS)
JOINT_IN = dict(stream=0, workspace=P, dtype=0, activation=0, f=P, g=P, weight=P, bias=P, labels=P, xn=P, yn=P, H=64, V=8,
                blank=0, **DIMS)
BAD_JOINT = (BAD_DTYPE + [dict(activation=-1), dict(activation=2)] + BAD_DIMS +
             [dict(H=16), dict(H=48), dict(H=1056), dict(V=1), dict(V=(1 << 24) + 1), dict(blank=-1), dict(blank=8)] +
             BAD_WORKSPACE + [dict(f=0), dict(g=0), dict(weight=0), dict(xn=0), dict(yn=0), dict(labels=0),
                              dict(f=P + 4), dict(g=P + 8), dict(weight=P + 4), dict(bias=P + 2)])

ENTRIES = {
    "run_warp_rnnt": entry(
        "stream counts alphas betas labels log_probs grads costs xn yn N T U V blank fastemit_lambda",
        dict(stream=0, counts=P, alphas=P, betas=P, labels=P, log_probs=P, grads=P, costs=P, xn=P, yn=P, V=7, blank=0,
             fastemit_lambda=0.0, **DIMS),
        BAD_DIMS + bad_vocab(7), [dict(N=0)]),
    "run_warp_rnnt_gather": entry(
        "stream counts alphas betas log_probs grads costs xn yn N T U fastemit_lambda",
        dict(stream=0, counts=P, alphas=P, betas=P, log_probs=P, grads=P, costs=P, xn=P, yn=P, fastemit_lambda=0.0, **DIMS),
        BAD_DIMS, [dict(N=0)]),
    "rnnt_amd_loss": entry(
        "stream workspace input_kind input labels xn yn costs grads grads_kind N T U V blank fastemit_lambda",
        dict(LOSS, input_kind=0, input=P),
        BAD_DIMS + BAD_WORKSPACE + bad_vocab(7) + [dict(labels=0), dict(input_kind=-1), dict(input_kind=3)] + BAD_GRADS[:4],
        [dict(N=0), dict(N=0, input_kind=3), dict(N=0, input_kind=1, V=0, labels=0)]),
    "rnnt_amd_loss_logits": entry(
        "stream workspace dtype logits labels xn yn costs grads grads_kind N T U V blank fastemit_lambda",
        dict(LOSS, dtype=1, logits=P),
        BAD_DTYPE + BAD_DIMS + BAD_WORKSPACE + bad_vocab(7) + [dict(labels=0), dict(grads_kind=2)] + BAD_GRADS[:3],
        [dict(N=0, dtype=d) for d in DTYPES]),
    "rnnt_amd_expand_grads": entry(
        "stream grads_diagonal labels xn yn grad_costs dense_grads N T U V blank overwrite",
        dict(stream=0, grads_diagonal=P, labels=P, xn=P, yn=P, grad_costs=P, dense_grads=P, V=7, blank=0, overwrite=1, **DIMS),
        BAD_DIMS + bad_vocab(7) + [dict(N=1, T=1, U=1 << 11, V=1 << 20), dict(N=65535, T=1 << 16, U=1)], []),
    "rnnt_amd_logits_backward": entry(
        "stream logits labels grads_diagonal grad_costs dlogits N T U V blank",
        dict(stream=0, logits=P, labels=P, grads_diagonal=P, grad_costs=P, dlogits=P, V=7, blank=0, **DIMS),
        BAD_DIMS + bad_vocab(7) + [dict(labels=0)], []),
    "rnnt_amd_logits_backward_typed": entry(
        "stream dtype logits labels grads_diagonal grad_costs dlogits N T U V blank",
        dict(stream=0, dtype=2, logits=P, labels=P, grads_diagonal=P, grad_costs=P, dlogits=P, V=7, blank=0, **DIMS),
        BAD_DTYPE + BAD_DIMS + bad_vocab(7) + [dict(labels=0), dict(labels=0, dtype=0), dict(V=0, dtype=0), dict(N=-1, dtype=0)],
        []),
    "rnnt_amd_log_softmax": entry("stream x out rows V", dict(stream=0, x=P, out=P, rows=4, V=7),
                                  [dict(rows=-1), dict(V=0)], []),
    "rnnt_amd_log_softmax_typed": entry(
        "stream dtype x out rows V", dict(stream=0, dtype=1, x=P, out=P, rows=4, V=7),
        BAD_DTYPE + [dict(rows=-1), dict(V=0), dict(rows=-1, dtype=0), dict(V=0, dtype=0), dict(V=0, dtype=2)], []),
    "rnnt_amd_log_softmax_backward": entry("stream grad_out out grad_in rows V",
                                           dict(stream=0, grad_out=P, out=P, grad_in=P, rows=4, V=7),
                                           [dict(rows=-1), dict(V=0)], []),
    "rnnt_amd_gather": entry("stream log_probs labels gathered N T U V blank",
                             dict(stream=0, log_probs=P, labels=P, gathered=P, V=7, blank=0, **DIMS),
                             BAD_DIMS + bad_vocab(7), []),
    "rnnt_amd_compact_offsets": entry(
        "stream xn yn N cell_offsets label_offsets stats",
        dict(stream=0, xn=P, yn=P, N=2, cell_offsets=P, label_offsets=P, stats=P),
        [dict(N=-1), dict(N=65536), dict(cell_offsets=0), dict(label_offsets=0), dict(stats=0), dict(xn=0), dict(yn=0)], []),
    "rnnt_amd_loss_compact": entry(
        "stream workspace xs ys xn yn cell_offsets label_offsets costs grads2 loc N STU Tmax Umax V blank fastemit_lambda",
        dict(COMPACT_LOSS, xs=P, cell_offsets=P, label_offsets=P, loc=P),
        BAD_COMPACT_DIMS + BAD_WORKSPACE + bad_vocab(7),
        [dict(N=0), dict(STU=0), dict(N=0, STU=0, Tmax=0, Umax=0)]),
    "rnnt_amd_loss_compact_bounded": entry(
        "stream workspace xs ys n_labels xn yn costs grads2 loc N STU Tmax Umax V blank fastemit_lambda",
        dict(COMPACT_LOSS, xs=P, n_labels=4, loc=P),
        BAD_COMPACT_DIMS + BAD_WORKSPACE + [dict(Tmax=0), dict(Umax=0), dict(n_labels=-1), dict(N=0, Tmax=0), dict(N=0, V=0, workspace=0)],
        [dict(N=0), dict(N=0, V=0), dict(N=0, blank=7)]),
    "rnnt_amd_loss_compact_logits": entry(
        "stream workspace dtype logits ys xn yn cell_offsets label_offsets costs grads2 N STU Tmax Umax V blank fastemit_lambda",
        dict(COMPACT_LOSS, dtype=1, logits=P, cell_offsets=P, label_offsets=P),
        BAD_DTYPE + BAD_COMPACT_DIMS + BAD_WORKSPACE + bad_vocab(7) + [dict(ys=0), dict(ys=0, N=0)],
        [dict(N=0, dtype=d) for d in DTYPES] + [dict(STU=0), dict(STU=0, ys=0, Umax=1)]),
    "rnnt_amd_loss_compact_logits_bounded": entry(
        "stream workspace dtype logits ys n_labels xn yn costs grads2 N STU Tmax Umax V blank fastemit_lambda",
        dict(COMPACT_LOSS, dtype=2, logits=P, n_labels=4),
        BAD_DTYPE + BAD_COMPACT_DIMS + BAD_WORKSPACE + bad_vocab(7) +
        [dict(Tmax=0), dict(Umax=0), dict(n_labels=-1), dict(ys=0), dict(N=0, V=0), dict(N=0, ys=0)],
        [dict(N=0, dtype=d) for d in DTYPES] + [dict(N=0, ys=0, n_labels=0)]),
    "rnnt_amd_compact_logits_backward": entry(
        "stream dtype logits ys n_labels xn yn cell_offsets label_offsets grads2 grad_costs dlogits N STU V blank",
        dict(stream=0, dtype=1, logits=P, ys=P, n_labels=4, xn=P, yn=P, cell_offsets=P, label_offsets=P, grads2=P,
             grad_costs=P, dlogits=P, N=2, STU=23, V=7, blank=0),
        BAD_DTYPE + BAD_COMPACT_DIMS[:4] + bad_vocab(7) + [dict(n_labels=-1), dict(ys=0), dict(STU=0, V=0)],
        [dict(STU=0, dtype=d) for d in DTYPES] + [dict(STU=0, N=0)]),
    "rnnt_amd_compact_scatter_grads": entry(
        "stream grad_costs grads2 loc cum_lens dense_grads STU N V blank",
        dict(stream=0, grad_costs=P, grads2=P, loc=P, cum_lens=P, dense_grads=P, STU=23, N=2, V=7, blank=0),
        [dict(N=-1), dict(STU=-1)] + bad_vocab(7), []),
    "rnnt_amd_joint_loss": entry(
        "stream workspace dtype activation f g weight bias labels xn yn costs lse grads N T U H V blank fastemit_lambda",
        dict(JOINT_IN, costs=P, lse=P, grads=P, fastemit_lambda=0.0),
        BAD_JOINT + [dict(costs=0), dict(lse=0), dict(N=0, workspace=0), dict(lse=P + 4)],
        [dict(N=0), dict(N=0, dtype=2, activation=1, bias=0, lse=0, grads=0)]),
    "rnnt_amd_joint_backward": entry(
        "stream workspace dtype activation f g weight bias labels xn yn lse grads grad_costs df dg dweight dbias N T U H V blank",
        dict(JOINT_IN, lse=P, grads=P, grad_costs=P, df=P, dg=P, dweight=P, dbias=P),
        BAD_JOINT + [dict(lse=0), dict(grads=0), dict(grads=P + 4), dict(df=0, dg=0, dweight=0, dbias=0, workspace=P + 8),
                     dict(lse=P + 4)],
        [dict(N=0), dict(df=0, dg=0, dweight=0, dbias=0), dict(df=0, dg=0, dweight=0, dbias=0, bias=0, grad_costs=0, dtype=1)]),
    "rnnt_amd_debug_lattice_only": entry("stream workspace xn yn N T U", dict(stream=0, workspace=P, xn=P, yn=P, **DIMS),
                                         BAD_DIMS + [dict(workspace=0)], []),
    "rnnt_amd_debug_gather_only": entry(
        "stream workspace log_probs labels N T U V blank",
        dict(stream=0, workspace=P, log_probs=P, labels=P, V=7, blank=0, **DIMS),
        BAD_DIMS + [dict(workspace=0)] + bad_vocab(7) + [dict(labels=0)], []),
    # the blank column as a plane of its own: what tests/test_host_blank_plane.py asks of these entries, one row each
    "rnnt_amd_log_softmax_plane": entry("stream x out col_out rows V col",
                                        dict(stream=0, x=P, out=P, col_out=P, rows=4, V=7, col=0), BAD_PLANE, []),
    "rnnt_amd_log_softmax_plane_typed": entry(
        "stream dtype x out col_out rows V col", dict(stream=0, dtype=1, x=P, out=P, col_out=P, rows=4, V=7, col=0),
        BAD_DTYPE + [dict(bad, dtype=d) for bad in BAD_PLANE for d in DTYPES], []),
    "rnnt_amd_loss_blank_plane": entry(
        "stream workspace log_probs blank_plane labels xn yn costs grads grads_kind N T U V blank fastemit_lambda",
        dict(LOSS, log_probs=P, blank_plane=P),
        [dict(blank_plane=0)] + BAD_DIMS[:4] + BAD_WORKSPACE + bad_vocab(7) + [dict(labels=0)] + BAD_GRADS[:3], [dict(N=0)]),
    "rnnt_amd_debug_gather_only_blank_plane": entry(
        "stream workspace log_probs blank_plane labels N T U V blank",
        dict(stream=0, workspace=P, log_probs=P, blank_plane=P, labels=P, V=7, blank=0, **DIMS),
        [dict(blank_plane=0), dict(workspace=0), dict(N=-1), dict(T=0), dict(V=0), dict(blank=7), dict(labels=0)], []),
}


def load(path):
    L = ctypes.CDLL(path)
    for table in [_lib.SYMBOLS] + [t for t, _ in _lib.ADDITIVE]:
        for name, (res, args) in table.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = res, args
    return L


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else _lib.lib_path()
    L = load(path)
    sizes = [[fn, list(a), getattr(L, fn)(*a)] for fn, grid in SIZES for a in grid]
    calls = []
    for fn, (names, base, rejected, accepted) in ENTRIES.items():
        assert len(names) == len(_lib.SYMBOLS[fn][1]), fn
        for expect, changes in ((5, rejected), (0, accepted)):
            for change in changes:
                assert set(change) <= set(names), (fn, change)
                args = [dict(base, **change)[k] for k in names]
                status = getattr(L, fn)(*args)
                # a row is only worth recording when no launch was attempted: a launch cannot succeed here, and what
                # it fails with is not a decision of the host code
                assert status == expect, (fn, change, status)
                calls.append([fn, " ".join(f"{k}={v}" for k, v in change.items()), args, status])
    out = os.path.join(HERE, "host_decisions.json")
    with open(out, "w") as f:
        json.dump({"abi_version": L.rnnt_amd_version(), "sizes": sizes, "calls": calls}, f, indent=None, separators=(",", ":"))
        f.write("\n")
    print("wrote", out, len(sizes), "sizes,", len(calls), "calls,", os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
