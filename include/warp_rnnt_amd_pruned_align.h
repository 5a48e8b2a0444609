/* Best-path alignments on the pruned band: additive entries of libwarp_rnnt_amd.so (they did not move the C-ABI version --
 * nothing that was there moves).
 *
 * What the dense align entry of warp_rnnt_amd_align.h gives a dense model -- the score of the best path and the frame at which every
 * label is emitted -- for the pruned recipe of warp_rnnt_amd_pruned.h, warp_rnnt_amd_topology.h and
 * warp_rnnt_amd_pruned_hat.h: band logits (N,T,S,V), both topologies, the delay penalty.  No (N,T,U) plane is formed.
 *
 * Cells and weights.  Utterance n has T_n = xn[n] frames and U_n = yn[n] labels; c(t) = starts[n,t].  Cell (t,u) is in the
 * band iff 0 <= u - c(t) < S, 0 <= u < U, t < T_n and u <= U_n.  Its pair (b(t,u), l(t,u)) is what the pruned loss puts in
 * that cell -- the log-softmax pair, or HAT's -- from row (n, t, u - c(t)) of the logits, with
 * delay_penalty * (0.5f * (float)(T_n - 1) - (float)t) added to the finished label channel (fp32: the bracket, one multiply,
 * one add; delay_penalty == 0 adds nothing).  l(t,u) = -inf for u >= U_n.  A cell outside the band has both weights -inf:
 * edges leave band cells only.  starts is device data nobody validates: non-monotone starts, jumps of S or more and rows
 * outside [0,U) are legal, they remove edges.
 *
 * RNNT_TOPOLOGY_REGULAR -- the recurrence of warp_rnnt_amd_align.h on those weights:
 *
 *     v(0,0) = 0
 *     cb = v(t-1,u) + b(t-1,u)            (t > 0)
 *     cl = v(t,u-1) + l(t,u-1)            (u > 0)
 *     by_label(t,u) = u > 0 and (t == 0 or cl > cb)        a tie goes to the blank
 *     v(t,u) = cl if by_label(t,u) else cb
 *     score = v(T_n-1, U_n) + b(T_n-1, U_n)
 *
 * and emit_frames[n,u-1] = t for every by_label cell on the walk back from (T_n-1, U_n).
 *
 * RNNT_TOPOLOGY_MODIFIED -- every edge consumes a frame:
 *
 *     v(0,0) = 0
 *     cb = v(t,u) + b(t,u),   cl = v(t,u-1) + l(t,u-1)     (a term with a negative index: -inf)
 *     by_label(t+1,u) = u > 0 and cl > cb
 *     v(t+1,u) = cl if by_label(t+1,u) else cb
 *     score = v(T_n, U_n)                                  no terminal blank
 *
 * and emit_frames[n,u-1] = t, the frame the label's edge consumes, on the walk back from (T_n, U_n).
 *
 * Everything is fp32, one add per edge and one compare per cell, every add rounded on its own.  emit_frames (N,U-1) is
 * int32 with -1 from column U_n on.  An utterance whose score is -inf -- no path in the band; T_n < U_n in the modified
 * topology -- gets -inf and a row of -1.  Lengths outside [1,T] x [0,U-1] give a NaN score and a row of -1, and nothing
 * outside that utterance's own outputs is written.  -inf logits are masks, as in the pruned loss; NaN input is unspecified.
 *
 * Refused with RNNT_STATUS_INVALID_ARGUMENT before any HIP call: what rnnt_amd_pruned_loss_logits_topology refuses for the
 * same arguments (an unknown dtype or topology, a delay_penalty that is negative, NaN or infinite, V < 2, a blank outside
 * [0,V), sizes it refuses, S < 1, S > U, N*T*S >= 2^32, a null or misaligned workspace, a null inputs / starts / xn / yn),
 * an unknown input_kind, S > 64, RNNT_PRUNED_ALIGN_IN_PAIRS with another dtype than RNNT_DTYPE_F32, a null scores, U > 1
 * without emit_frames or -- for the two logits kinds -- without labels.  N == 0 succeeds without a launch.  A failed
 * producer launch: RNNT_STATUS_PROLOGUE_FAILED; a failed sweep launch: RNNT_STATUS_WARP_FAILED.  The call only enqueues (no
 * read-back, no allocation): it can be captured into a graph.
 */
#ifndef WARP_RNNT_AMD_PRUNED_ALIGN_H
#define WARP_RNNT_AMD_PRUNED_ALIGN_H

#include "warp_rnnt_amd.h"
#include "warp_rnnt_amd_topology.h"

/* input_kind: what `inputs` holds */
#define RNNT_PRUNED_ALIGN_IN_LOGITS 0     /* (N,T,S,V) of `dtype`, read as rnnt_amd_pruned_loss_logits reads them */
#define RNNT_PRUNED_ALIGN_IN_HAT_LOGITS 1 /* (N,T,S,V) of `dtype`, read as rnnt_amd_pruned_hat_loss_logits reads them */
#define RNNT_PRUNED_ALIGN_IN_PAIRS 2      /* (N,T,S,2) fp32: channel 0 the blank's weight of row (n,t,s), channel 1 the
                                             label's; labels are not read, V and blank only checked; the delay penalty and
                                             the -inf of the cells outside the band and of column U_n still apply */

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of workspace: a function of the shape alone; 0 for N < 0, T < 1, S outside [1,64], N*T*S >= 2^32 or an unknown
 * topology.  Every piece on a multiple of 256 bytes:
 *     offset 0:                        the band pairs (N,T,S,2) fp32, pair of row (n,t,s) at ((n*T + t)*S + s): the weights
 *                                      above, still there when the call returns;
 *     offset round_up(8*N*T*S, 256):   one 64-bit decision word per (n, frame), N*T of them (modified: N*(T+1), frame T_n
 *                                      holds the end cell in bit 0): bit s is by_label of cell (t, c(t) + s); written for the
 *                                      frames t < T_n of an utterance with lengths the entry takes, unspecified elsewhere. */
size_t rnnt_amd_pruned_align_workspace_size(int N, int T, int S, int topology);

rnntStatus_t rnnt_amd_pruned_align(rnntStream_t stream, void *workspace, int input_kind, int dtype, const void *inputs,
                                   const int *labels, const int *starts, const int *xn, const int *yn,
                                   float *scores /* (N,) */, int *emit_frames /* (N,U-1); NULL iff U == 1 */, int N, int T,
                                   int U, int S, int V, int blank, int topology, float delay_penalty);

#ifdef __cplusplus
}
#endif
#endif /* WARP_RNNT_AMD_PRUNED_ALIGN_H */
