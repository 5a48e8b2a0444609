/* Best-path (Viterbi) alignments from the fused loss lattice: additive entries of libwarp_rnnt_amd.so (they did not move
 * the C-ABI version -- nothing that was there moves).
 *
 * A producer of the loss fills the diagonal-major (blank, label) pair plane -- dense log-probs, gathered pairs, logits
 * through the fused log-softmax, or logits through the factorised-blank (HAT) form -- and a max-plus sweep over that plane
 * takes the place of the alpha / beta sweeps.  For utterance n with T_n = xn[n], U_n = yn[n] and b(t,u), l(t,u) the two
 * channels of its plane, in fp32, one IEEE add and one compare per edge, nothing fused:
 *
 *     v(0,0) = 0
 *     cb = v(t-1,u) + b(t-1,u)          (t > 0)
 *     cl = v(t,u-1) + l(t,u-1)          (u > 0)
 *     by_label(t,u) = u > 0 and (t == 0 or cl > cb)       a tie goes to the blank predecessor
 *     v(t,u) = by_label ? cl : cb
 *     scores[n] = v(T_n-1, U_n) + b(T_n-1, U_n)
 *
 * The path is read back from (T_n-1, U_n) along by_label; emit_frames[n, u] is the frame t of the label step
 * (t,u) -> (t,u+1) for u < U_n, and -1 for U_n <= u < U-1.  Among all paths of maximal score this is the one whose emit
 * frames are smallest when compared from the last label to the first.  Log-probs of -inf are legal (the score may be
 * -inf, the path stays a path); NaN input is unspecified.  An utterance with xn[n] outside [1,T] or yn[n] outside [0,U-1]
 * gets scores[n] = NaN and a row of -1, and nothing outside its own outputs is read or written.
 *
 * Refused with RNNT_STATUS_INVALID_ARGUMENT before any HIP call: an unknown input_kind or dtype, a dtype other than
 * RNNT_DTYPE_F32 on the two log-prob kinds, sizes rnnt_amd_workspace_size refuses, a null or misaligned workspace, a null
 * input / xn / yn / scores, a null emit_frames with U > 1, and -- except for RNNT_IN_LOG_PROBS_GATHERED, which reads
 * neither V, blank nor labels -- V < 1 (V < 2 for RNNT_ALIGN_IN_HAT_LOGITS), a blank outside [0,V), U > 1 without labels.
 * N == 0 succeeds without a launch.  A failed producer launch: RNNT_STATUS_PROLOGUE_FAILED; a failed sweep or trace
 * launch: RNNT_STATUS_WARP_FAILED.  The call only enqueues (no read-back, no allocation): it can be captured into a graph.
 */
#ifndef WARP_RNNT_AMD_ALIGN_H
#define WARP_RNNT_AMD_ALIGN_H

#include "warp_rnnt_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* input_kind: RNNT_IN_LOG_PROBS_DENSE 0, RNNT_IN_LOG_PROBS_GATHERED 1, RNNT_IN_LOGITS_DENSE 2 of rnnt_amd_loss, or logits
 * (N,T,U,V) read the way rnnt_amd_hat_loss_logits reads them: */
#define RNNT_ALIGN_IN_HAT_LOGITS 3

/* Bytes of workspace for (N,T,U); 0 for sizes rnnt_amd_workspace_size refuses.  A function of the shape alone.  It begins
 * with what rnnt_amd_workspace_size carves for (N,T,U) -- its pair plane still holds the producer's pairs when
 * rnnt_amd_align returns -- followed by the decision words, W[n][d][u/64] with bit u mod 64 = by_label at cell (d-u, u),
 * and the boundary columns that the sweep hands between column stripes. */
size_t rnnt_amd_align_workspace_size(int N, int T, int U);

rnntStatus_t rnnt_amd_align(rnntStream_t stream, void *workspace, int input_kind, int dtype, const void *input,
                            const int *labels, const int *xn, const int *yn,
                            float *scores /* (N,) */, int *emit_frames /* (N,U-1) row-major; may be NULL iff U == 1 */,
                            int N, int T, int U, int V, int blank);

#ifdef __cplusplus
}
#endif
#endif /* WARP_RNNT_AMD_ALIGN_H */
