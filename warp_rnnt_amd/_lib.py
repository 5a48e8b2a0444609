"""ctypes binding of the C ABI in include/warp_rnnt_amd.h.

Import torch before calling :func:`load` in a process that also uses torch:
the library depends on ``libamdhip64.so.7`` and must share the HIP runtime
torch already loaded (same SONAME, so the dynamic loader reuses it), otherwise
stream handles would belong to a different runtime.
"""
import ctypes
import os

HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_NAME = "libwarp_rnnt_amd.so"
_lib = None

STATUS_NAMES = {
    0: "RNNT_STATUS_SUCCESS", 1: "RNNT_STATUS_WARP_FAILED", 2: "RNNT_STATUS_GRADS_BLANK_FAILED",
    3: "RNNT_STATUS_GRADS_LABEL_FAILED", 4: "RNNT_STATUS_COSTS_FAILED",
    5: "RNNT_STATUS_INVALID_ARGUMENT", 6: "RNNT_STATUS_PROLOGUE_FAILED", 7: "RNNT_STATUS_EXPAND_FAILED",
}

# input_kind / grads_kind enums of rnnt_amd_loss
IN_LOG_PROBS_DENSE, IN_LOG_PROBS_GATHERED, IN_LOGITS_DENSE = 0, 1, 2
GRADS_GATHERED, GRADS_GATHERED_DIAGONAL, GRADS_DENSE, GRADS_NONE = 0, 1, 2, 3
# element type of the logits for the typed entries (rnnt_amd_loss_logits, ..._typed)
DTYPE_F32, DTYPE_BF16, DTYPE_F16 = 0, 1, 2
# activation of rnnt_amd_joint_loss / _backward
ACT_TANH, ACT_RELU = 0, 1

# every symbol include/warp_rnnt_amd.h declares: (restype, argtypes)
_vp, _i, _f, _sz, _i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_size_t, ctypes.c_int64


SYMBOLS = {
    "run_warp_rnnt": (_i, [_vp] * 10 + [_i] * 5 + [_f]),
    "run_warp_rnnt_gather": (_i, [_vp] * 9 + [_i] * 3 + [_f]),
    "run_gather_for_compact": (None, [_vp] * 8 + [ctypes.c_uint] * 5),
    "run_warp_rnnt_compact": (None, [_vp] * 10 + [ctypes.c_uint] * 3 + [_f, ctypes.c_bool]),
    "run_scatter_grad_for_compact": (None, [_vp] * 5 + [ctypes.c_uint] * 4),
    "rnnt_amd_compact_last_status": (_i, []),
    "rnnt_amd_workspace_size": (_sz, [_i, _i, _i]),
    "rnnt_amd_workspace_mismatch_offset": (_sz, [_i, _i, _i]),
    "rnnt_amd_debug_redo_offset": (_sz, [_i, _i, _i]),
    "rnnt_amd_loss": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _f]),
    "rnnt_amd_expand_grads": (_i, [_vp] * 7 + [_i] * 6),
    "rnnt_amd_logits_backward": (_i, [_vp] * 6 + [_i] * 5),
    "rnnt_amd_log_softmax": (_i, [_vp, _vp, _vp, _i64, _i]),
    "rnnt_amd_loss_logits": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _f]),
    "rnnt_amd_logits_backward_typed": (_i, [_vp, _i] + [_vp] * 5 + [_i] * 5),
    "rnnt_amd_log_softmax_typed": (_i, [_vp, _i, _vp, _vp, _i64, _i]),
    "rnnt_amd_log_softmax_backward": (_i, [_vp, _vp, _vp, _vp, _i64, _i]),
    "rnnt_amd_gather": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i]),
    "rnnt_amd_workspace_size_compact": (_sz, [_i, _i64, _i, _i]),
    "rnnt_amd_loss_compact": (_i, [_vp] * 11 + [_i, _i64, _i, _i, _i, _i, _f]),
    "rnnt_amd_workspace_size_compact_bounded": (_sz, [_i, _i64, _i, _i]),
    "rnnt_amd_loss_compact_bounded": (_i, [_vp] * 4 + [_i64] + [_vp] * 5 + [_i, _i64, _i, _i, _i, _i, _f]),
    "rnnt_amd_loss_compact_logits": (_i, [_vp, _vp, _i] + [_vp] * 8 + [_i, _i64, _i, _i, _i, _i, _f]),
    "rnnt_amd_loss_compact_logits_bounded": (_i, [_vp, _vp, _i, _vp, _vp, _i64] + [_vp] * 4 + [_i, _i64, _i, _i, _i, _i, _f]),
    "rnnt_amd_compact_logits_backward": (_i, [_vp, _i, _vp, _vp, _i64] + [_vp] * 7 + [_i, _i64, _i, _i]),
    "rnnt_amd_joint_workspace_size": (_sz, [_i] * 5),
    "rnnt_amd_joint_loss": (_i, [_vp, _vp, _i, _i] + [_vp] * 10 + [_i] * 6 + [_f]),
    "rnnt_amd_joint_backward": (_i, [_vp, _vp, _i, _i] + [_vp] * 14 + [_i] * 6),
    "rnnt_amd_compact_scatter_grads": (_i, [_vp] * 6 + [_i64, _i, _i, _i]),
    "rnnt_amd_compact_offsets": (_i, [_vp, _vp, _vp, _i, _vp, _vp, _vp]),
    "rnnt_amd_debug_lattice_only": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i]),
    "rnnt_amd_debug_gather_only": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i]),
    "rnnt_amd_debug_set_lattice_kernel": (_i, [_i]),
    "rnnt_amd_debug_get_lattice_kernel": (_i, []),
    "rnnt_amd_mismatch_flag": (ctypes.POINTER(ctypes.c_uint), [_i]),
    "rnnt_amd_debug_last_lattice_kernel": (_i, []),
    "rnnt_amd_debug_lattice_plan": (_i, [_i] * 8),
    "rnnt_amd_debug_lsm_plan": (_i, [_i, _i, _i64] + [_i] * 6 + [ctypes.POINTER(_i), _i]),
    "rnnt_amd_version": (_i, []),
    # the blank column as a plane of its own (version 108, additive)
    "rnnt_amd_log_softmax_plane": (_i, [_vp, _vp, _vp, _vp, _i64, _i, _i]),
    "rnnt_amd_log_softmax_plane_typed": (_i, [_vp, _i, _vp, _vp, _vp, _i64, _i, _i]),
    "rnnt_amd_loss_blank_plane": (_i, [_vp] * 9 + [_i] * 6 + [_f]),
    "rnnt_amd_debug_gather_only_blank_plane": (_i, [_vp] * 5 + [_i] * 5),
}


# every symbol include/warp_rnnt_amd_clamp.h declares (the gradient clamp of the fused backward; additive: it did not
# move the version): the arguments of the unclamped twin and a float clamp behind them
CLAMP_SYMBOLS = {
    "rnnt_amd_logits_backward_clamped": (_i, SYMBOLS["rnnt_amd_logits_backward_typed"][1] + [_f]),
    "rnnt_amd_compact_logits_backward_clamped": (_i, SYMBOLS["rnnt_amd_compact_logits_backward"][1] + [_f]),
}


# every symbol include/warp_rnnt_amd_joint_dropout.h declares (dropout inside the fused joint; additive: it did not move
# the version): the arguments of the twin with `float p, const uint64_t *seed` (a device pointer) behind them, and the
# mask's definition on the host
_u64 = ctypes.c_uint64
DROPOUT_SYMBOLS = {
    "rnnt_amd_joint_loss_dropout": (_i, SYMBOLS["rnnt_amd_joint_loss"][1] + [_f, _vp]),
    "rnnt_amd_joint_backward_dropout": (_i, SYMBOLS["rnnt_amd_joint_backward"][1] + [_f, _vp]),
    "rnnt_amd_joint_dropout_mask_host": (_i, [_u64, _f, _i, _i, _i, _i, _vp]),
}
# every symbol include/warp_rnnt_amd_hat.h declares (the factorised-blank loss on the fused path; additive: it did not move
# the version): the forward is rnnt_amd_loss_logits without its grads_kind, the backward rnnt_amd_logits_backward_typed
HAT_SYMBOLS = {
    "rnnt_amd_hat_loss_logits": (_i, [_vp, _vp, _i] + [_vp] * 6 + [_i] * 5 + [_f]),
    "rnnt_amd_hat_logits_backward": (_i, [_vp, _i] + [_vp] * 5 + [_i] * 5),
}
# every symbol include/warp_rnnt_amd_align.h declares (best-path alignments from the loss lattice; additive: it did not move
# the version): the size is rnnt_amd_workspace_size's, the call is (stream, workspace, input_kind, dtype, input, labels,
# xn, yn, scores, emit_frames, N, T, U, V, blank)
ALIGN_IN_HAT_LOGITS = 3      # input_kind of rnnt_amd_align beside the three IN_* above
ALIGN_SYMBOLS = {
    "rnnt_amd_align_workspace_size": (_sz, [_i, _i, _i]),
    "rnnt_amd_align": (_i, [_vp, _vp, _i, _i] + [_vp] * 6 + [_i] * 5),
}
# every symbol include/warp_rnnt_amd_tdt.h declares (the token-and-duration loss; additive: it did not move the version):
# the size is a function of (N, T, U, D); the forward is (stream, workspace, dtype, logits, labels, xn, yn, durations, D,
# costs, grads, N, T, U, V, blank, sigma, fastemit_lambda) with durations in host memory; the backward is (stream, dtype,
# logits, labels, grads, grad_costs, dlogits, N, T, U, V, D, blank)
TDT_SYMBOLS = {
    "rnnt_amd_tdt_workspace_size": (_sz, [_i, _i, _i, _i]),
    "rnnt_amd_tdt_loss_logits": (_i, [_vp, _vp, _i] + [_vp] * 5 + [_i, _vp, _vp] + [_i] * 5 + [_f, _f]),
    "rnnt_amd_tdt_logits_backward": (_i, [_vp, _i] + [_vp] * 5 + [_i] * 6),
}
# the additive table: (symbols, the header that declares them) of every family that came after version 110 and did not
# move it.  load() walks it; tests/test_host_additive_abi.py holds every family to the one contract, and
# tests/test_host_decisions.py reaches their size entries through it.
ADDITIVE = ((CLAMP_SYMBOLS, "warp_rnnt_amd_clamp.h"), (DROPOUT_SYMBOLS, "warp_rnnt_amd_joint_dropout.h"),
            (HAT_SYMBOLS, "warp_rnnt_amd_hat.h"), (ALIGN_SYMBOLS, "warp_rnnt_amd_align.h"),
            (TDT_SYMBOLS, "warp_rnnt_amd_tdt.h"))
# every symbol include/warp_rnnt_amd_tdt_align.h declares (best-path alignments over the TDT lattice; additive: it did not
# move the version): the size is a function of (N, T, U, D); the call is (stream, workspace, dtype, logits, labels, xn, yn,
# durations, D, scores, emit_frames, emit_durations, N, T, U, V, blank, sigma) with durations in host memory
TDT_ALIGN_SYMBOLS = {
    "rnnt_amd_tdt_align_workspace_size": (_sz, [_i, _i, _i, _i]),
    "rnnt_amd_tdt_align": (_i, [_vp, _vp, _i] + [_vp] * 5 + [_i] + [_vp] * 3 + [_i] * 5 + [_f]),
}
# the families that came after the five of ADDITIVE, under the same contract; load() walks them behind it
# (tests/test_host_tdt_align.py holds this one to it).  Folding the two tuples into one is for a change that may touch the
# tests which pin ADDITIVE to its five.
ADDITIVE_NEXT = ((TDT_ALIGN_SYMBOLS, "warp_rnnt_amd_tdt_align.h"),)
# every symbol include/warp_rnnt_amd_tdt_joint.h declares (the joint network fused into the TDT loss; additive: it did not
# move the version): the size is a function of (N, T, U, H, V, D); the forward is (stream, workspace, dtype, activation, f,
# g, weight, bias, labels, xn, yn, durations, D, costs, stats, grads, N, T, U, H, V, blank, sigma, fastemit_lambda, p,
# seed) with durations in host memory and seed a device pointer; the backward is (stream, workspace, dtype, activation, f,
# g, weight, bias, labels, xn, yn, stats, grads, grad_costs, df, dg, dweight, dbias, N, T, U, H, V, D, blank, p, seed)
TDT_JOINT_SYMBOLS = {
    "rnnt_amd_tdt_joint_workspace_size": (_sz, [_i] * 6),
    "rnnt_amd_tdt_joint_loss": (_i, [_vp, _vp, _i, _i] + [_vp] * 8 + [_i] + [_vp] * 3 + [_i] * 6 + [_f, _f, _f, _vp]),
    "rnnt_amd_tdt_joint_backward": (_i, [_vp, _vp, _i, _i] + [_vp] * 14 + [_i] * 7 + [_f, _vp]),
}
# the families behind ADDITIVE_NEXT, under the same contract (tests/test_host_tdt_joint.py holds this one to it); a tuple
# of its own because tests pin the two above to their contents
ADDITIVE_TDT_JOINT = ((TDT_JOINT_SYMBOLS, "warp_rnnt_amd_tdt_joint.h"),)
# every symbol include/warp_rnnt_amd_pruned.h declares (the pruned transducer loss over a band of S label positions per
# frame; additive: it did not move the version): HAT's two argument lists with `starts` (a device pointer, (N,T) int32)
# behind the labels and S between U and V -- the forward is (stream, workspace, dtype, logits, labels, starts, xn, yn,
# costs, grads, N, T, U, S, V, blank, fastemit_lambda), the backward (stream, dtype, logits, labels, starts,
# grads_diagonal, grad_costs, dlogits, N, T, U, S, V, blank)
PRUNED_SYMBOLS = {
    "rnnt_amd_pruned_loss_logits": (_i, [_vp, _vp, _i] + [_vp] * 7 + [_i] * 6 + [_f]),
    "rnnt_amd_pruned_logits_backward": (_i, [_vp, _i] + [_vp] * 6 + [_i] * 6),
}
# behind ADDITIVE_TDT_JOINT, under the same contract (tests/test_host_pruned.py holds this one to it); a tuple of its own
# for the same reason
ADDITIVE_PRUNED = ((PRUNED_SYMBOLS, "warp_rnnt_amd_pruned.h"),)
# every symbol include/warp_rnnt_amd_simple.h declares (the smoothed first pass of the pruned recipe over the trivial joiner
# am + lm; additive: it did not move the version): the size is a function of (N, T, U); the forward is (stream, workspace,
# dtype, am, lm, q, labels, xn, yn, costs, pair_grads, znorm, N, T, U, V, blank, lm_only_scale, am_only_scale,
# fastemit_lambda), the backward (stream, workspace, dtype, am, lm, q, labels, xn, yn, pair_grads, znorm, grad_costs, dam,
# dlm, dq_partials, N, T, U, V, blank, lm_only_scale, am_only_scale)
SIMPLE_SYMBOLS = {
    "rnnt_amd_simple_workspace_size": (_sz, [_i, _i, _i]),
    "rnnt_amd_simple_loss": (_i, [_vp, _vp, _i] + [_vp] * 9 + [_i] * 5 + [_f] * 3),
    "rnnt_amd_simple_backward": (_i, [_vp, _vp, _i] + [_vp] * 12 + [_i] * 5 + [_f] * 2),
}
# behind ADDITIVE_PRUNED, under the same contract (tests/test_host_simple.py holds this one to it); a tuple of its own for
# the same reason
ADDITIVE_SIMPLE = ((SIMPLE_SYMBOLS, "warp_rnnt_amd_simple.h"),)
# every symbol include/warp_rnnt_amd_multiblank.h declares (the multi-blank transducer loss; additive: it did not move the
# version): the size is a function of (N, T, U, B); the forward is (stream, workspace, dtype, logits, labels, xn, yn,
# blank_ids, blank_durations, B, costs, grads, N, T, U, V, sigma, fastemit_lambda) with the ids and durations in host
# memory; the backward is (stream, dtype, logits, labels, grads, grad_costs, dlogits, N, T, U, V, blank_ids, B)
MULTIBLANK_SYMBOLS = {
    "rnnt_amd_multiblank_workspace_size": (_sz, [_i, _i, _i, _i]),
    "rnnt_amd_multiblank_loss_logits": (_i, [_vp, _vp, _i] + [_vp] * 6 + [_i, _vp, _vp] + [_i] * 4 + [_f, _f]),
    "rnnt_amd_multiblank_logits_backward": (_i, [_vp, _i] + [_vp] * 5 + [_i] * 4 + [_vp, _i]),
}
# behind ADDITIVE_SIMPLE, under the same contract (tests/test_host_multiblank.py holds this one to it); a tuple of its own
# for the same reason
ADDITIVE_MULTIBLANK = ((MULTIBLANK_SYMBOLS, "warp_rnnt_amd_multiblank.h"),)
# every symbol include/warp_rnnt_amd_topology.h declares (k2's modified topology and delay penalty for the pruned and the
# simple loss; additive: it did not move the version): the sizes are functions of (topology, N, T, U); each entry has the
# argument list of its namesake without the suffix with `topology` behind it, the forwards `delay_penalty` behind that, and
# the pruned backward takes xn, yn behind `starts`
TOPOLOGY_REGULAR, TOPOLOGY_MODIFIED = 0, 1
TOPOLOGY_SYMBOLS = {
    "rnnt_amd_pruned_topology_workspace_size": (_sz, [_i, _i, _i, _i]),
    "rnnt_amd_simple_topology_workspace_size": (_sz, [_i, _i, _i, _i]),
    "rnnt_amd_pruned_loss_logits_topology": (_i, PRUNED_SYMBOLS["rnnt_amd_pruned_loss_logits"][1] + [_i, _f]),
    "rnnt_amd_pruned_logits_backward_topology": (_i, [_vp, _i] + [_vp] * 8 + [_i] * 6 + [_i]),
    "rnnt_amd_simple_loss_topology": (_i, SIMPLE_SYMBOLS["rnnt_amd_simple_loss"][1] + [_i, _f]),
    "rnnt_amd_simple_backward_topology": (_i, SIMPLE_SYMBOLS["rnnt_amd_simple_backward"][1] + [_i]),
}
# behind ADDITIVE_MULTIBLANK, under the same contract (tests/test_host_modified.py holds this one to it); a tuple of its own
# for the same reason
ADDITIVE_TOPOLOGY = ((TOPOLOGY_SYMBOLS, "warp_rnnt_amd_topology.h"),)


ABI_VERSION = 110   # rnnt_amd_version() of the library these argument lists belong to


class RNNTStatusError(RuntimeError):
    pass


def lib_path():
    """The in-tree library; WARP_RNNT_AMD_LIB selects another build of the same C ABI (the A/B variants
    of _build.VARIANTS used for the parity table) -- still a HIP build, still no fallback."""
    return os.environ.get("WARP_RNNT_AMD_LIB") or os.path.join(HERE, _LIB_NAME)


def load():
    """Load libwarp_rnnt_amd.so; fail loudly if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    path = lib_path()
    if not os.path.exists(path):
        raise RuntimeError(
            f"{path} is missing: the HIP extension has not been built. Run "
            "`python -c 'import __graft_entry__ as g; g.build()'` (or `python warp_rnnt_amd/_build.py`). "
            "There is no CPU fallback.")
    L = ctypes.CDLL(path)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(L, name)   # AttributeError if the library does not export a declared symbol
        fn.restype = res
        fn.argtypes = args
    # the argument lists above are this version's: an older build of the library (a stale prebuilt .so, a
    # WARP_RNNT_AMD_LIB variant built from older sources) would accept the calls and misread them
    if L.rnnt_amd_version() != ABI_VERSION:
        raise RuntimeError(f"{path} reports C-ABI version {L.rnnt_amd_version()}, this package binds version "
                           f"{ABI_VERSION}: rebuild it (`python warp_rnnt_amd/_build.py`)")
    # additive entries do not move the version: a library built before them has to be told apart by its exports
    for table, header in (ADDITIVE + ADDITIVE_NEXT + ADDITIVE_TDT_JOINT + ADDITIVE_PRUNED + ADDITIVE_SIMPLE +
                          ADDITIVE_MULTIBLANK + ADDITIVE_TOPOLOGY):
        for name, (res, args) in table.items():
            fn = getattr(L, name, None)
            if fn is None:
                raise RuntimeError(f"{path} does not export {name} (include/{header}): it was built from older "
                                   "sources: rebuild it (`python warp_rnnt_amd/_build.py`)")
            fn.restype = res
            fn.argtypes = args
    _lib = L
    return L
