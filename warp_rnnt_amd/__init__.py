"""MI355X-native RNN-Transducer loss: HIP kernels + C ABI + thin torch plumbing.

Layout
  csrc/            hand-written HIP kernels for gfx950 and the extern "C" entry points
  _build.py        hipcc build of libwarp_rnnt_amd.so (in-tree)
  _lib.py          ctypes loader for the C ABI declared in include/warp_rnnt_amd.h
  ops.py           torch-tensor front ends of the native entry points
  fused.py         rnnt_loss_from_logits: logits -> loss -> d/d logits, log-probabilities never in HBM
  hat.py           hat_loss_from_logits / HATLoss / hat_log_probs: the factorised-blank (HAT) loss on the same path
  pruned.py        pruned_rnnt_loss_from_logits / PrunedRNNTLoss: k2-style pruned loss, logits (N,T,S,V) on a band of S label
                   positions per frame; simple_pairs / prune_ranges / prune_joint_inputs: the rest of that recipe
  simple.py        simple_rnnt_loss / SimpleRNNTLoss / batch_log_unigram: that recipe's smoothed first pass over the trivial
                   joiner am + lm (k2's rnnt_loss_smoothed), an MFMA GEMM in front of the lattice, two behind it
  tdt.py           tdt_loss_from_logits / TDTLoss / tdt_log_probs: the token-and-duration (TDT) loss, a lattice of its own;
                   tdt_align: best-path token frames and durations of that lattice;
                   tdt_loss_from_joint / TDTJointLoss: the joint network fused into the TDT loss
  multiblank.py    multiblank_loss_from_logits / MultiblankLoss: the multi-blank transducer loss (big blanks that consume
                   2, 4, 8 ... frames), a lattice of its own
  align.py         rnnt_align / alignment_mask: best-path (Viterbi) alignments from the same lattice, any of its inputs
  joint.py         rnnt_loss_from_joint / JointLoss: the joint network (act, dropout, projection) fused into the loss
  compat.py        the same under torchaudio's / warp-transducer's signatures (rnnt_loss, RNNTLoss; gradient clamp)
  functional.py    log_softmax whose result rnnt_loss(..., gather=True) recognises and fuses with (lazy)
  debug.py         kernel pin for A/B runs, last_lattice_kernel()
  distributed.py   batch-sharded loss over RCCL (one rank per GPU)

The drop-in package that mirrors the reference's Python interface is the
top-level ``warp_rnnt`` (``warp_rnnt.rnnt_loss``, ``warp_rnnt._C.rnnt_loss``).
There is no CPU fallback anywhere in these packages.
"""
from ._lib import load, lib_path, RNNTStatusError  # noqa: F401
from ._mismatch import last_mismatch  # noqa: F401
from . import compat  # noqa: F401

__version__ = "0.2.0"
