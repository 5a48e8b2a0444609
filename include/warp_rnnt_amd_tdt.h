/* The token-and-duration transducer (TDT) loss on the fused logits path: additive entries of libwarp_rnnt_amd.so (they did
 * not move the C-ABI version -- nothing that was there moves).
 *
 * TDT is the transducer of Xu et al. 2023: beside the token the model predicts how many frames the step consumes.
 * Logits (N,T,U,V+D): columns [0,V) are token logits, the blank among them (any index; NeMo's convention is V-1), V >= 2;
 * column V+i is the logit of durations[i].  durations: D distinct integers in [0,8] in any order, 1 among them.
 * Per cell, with sigma >= 0:
 *
 *     tok = log_softmax(z[:V]) - sigma          dur = log_softmax(z[V:])          (fp32 from the load on)
 *
 * Edges out of cell (t,u) of an utterance with T_n frames and U_n labels, d = durations[i]:
 *
 *     blank, d >  0, weight tok[blank] + dur[i]:       to (t+d, u) if t+d < T_n;  to the end if t+d == T_n and u == U_n
 *     label, d >= 0, weight tok[labels[u]] + dur[i]:   to (t+d, u+1) if u < U_n and t+d < T_n
 *
 * and no other: nothing jumps past T_n, a label never lands on frame T_n.  alpha(0,0) = 0, alpha of a cell is the log sum
 * exp over its incoming edges of alpha(source) + weight, ll the same over the edges to the end, costs[n] = -ll; beta is the
 * mirror image.  An edge from (t,u) has the occupancy exp(alpha(t,u) + weight + beta(destination) - ll); label edges are
 * multiplied by 1 + fastemit_lambda (the costs do not change).  Per cell G_b and G_l are the sums over the blank and the
 * label edges, G_dur[i] = blank_i + label_i, S = G_b + G_l, and with p = softmax(z[:V]), q = softmax(z[V:]):
 *
 *     dz[v]   = grad_costs[n] (p_v S - [v == blank] G_b - [v == label] G_l)        v < V
 *     dz[V+i] = grad_costs[n] (q_i S - G_dur[i])
 *
 * rounded once to the logits' type.  A token or duration logit of -inf is a masked entry: probability zero, gradient
 * exactly zero; every row needs a finite blank, label and duration-1 logit.  Cells outside an utterance's (T_n, U_n + 1)
 * window get exactly zero dz; so does every cell of an utterance whose lengths lie outside [1,T] x [0,U-1], and its cost
 * is NaN.
 *
 * Not here: the mix with the standard loss (NeMo's omega), a gradient clamp, a forward/backward mismatch guard, the
 * compact layout.  The joint network in front of the logits, fused into this loss, is warp_rnnt_amd_tdt_joint.h.  A lattice
 * has at most 1024 columns: U <= 1024 (the sweeps hold a column per lane of one workgroup); a wider one is refused.
 *
 * Everything refused -- an unknown dtype, durations that are not as above, V < 2, a blank outside [0,V), U > 1024 or sizes
 * rnnt_amd_workspace_size refuses, sigma < 0 or not finite, a null or misaligned workspace, a null or misaligned logits /
 * costs / grads / dlogits, a null xn / yn / durations, U > 1 without labels -- comes back as RNNT_STATUS_INVALID_ARGUMENT
 * before any HIP call.  N == 0 succeeds without a launch.  A failed launch: RNNT_STATUS_PROLOGUE_FAILED (the producer),
 * RNNT_STATUS_WARP_FAILED (the sweeps), RNNT_STATUS_GRADS_BLANK_FAILED (the gradient kernel), RNNT_STATUS_EXPAND_FAILED
 * (the backward).
 */
#ifndef WARP_RNNT_AMD_TDT_H
#define WARP_RNNT_AMD_TDT_H

#include "warp_rnnt_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of workspace for rnnt_amd_tdt_loss_logits: a function of (N,T,U,D) alone; 0 for sizes that are refused. */
size_t rnnt_amd_tdt_workspace_size(int N, int T, int U, int D);

/* durations: D integers in HOST memory, read during the call.  grads: (2+D, N, T, U) fp32 -- G_b, G_l, G_dur[0..D) as
 * planes, each in the diagonal-major cell order -- what rnnt_amd_tdt_logits_backward reads.  grads == NULL: costs only;
 * the beta sweep and the gradient kernel do not run. */
rnntStatus_t rnnt_amd_tdt_loss_logits(rnntStream_t stream, void *workspace, int dtype, const void *logits,
                                      const int *labels, const int *xn, const int *yn, const int *durations, int D,
                                      float *costs, float *grads /* or NULL: costs only */, int N, int T, int U, int V,
                                      int blank, float sigma, float fastemit_lambda);

/* d(sum_n grad_costs[n] * cost[n]) / d logits, (N,T,U,V+D) of type `dtype`, every element written. */
rnntStatus_t rnnt_amd_tdt_logits_backward(rnntStream_t stream, int dtype, const void *logits, const int *labels,
                                          const float *grads, const float *grad_costs /* or NULL: 1 */, void *dlogits,
                                          int N, int T, int U, int V, int D, int blank);

#ifdef __cplusplus
}
#endif
#endif /* WARP_RNNT_AMD_TDT_H */
