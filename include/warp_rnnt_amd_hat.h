/* The factorised-blank (HAT) transducer loss on the fused logits path: additive entries of libwarp_rnnt_amd.so (they did
 * not move the C-ABI version -- nothing that was there moves).
 *
 * HAT is the Hybrid Autoregressive Transducer of Variani et al. 2020.  The blank probability of a lattice cell is a
 * Bernoulli, sigmoid(z[blank]); the labels share 1 - sigmoid(z[blank]) through a softmax over the NON-BLANK logits only.
 * With b = blank and sp(x) = max(x,0) + log1p(exp(-|x|)), per cell with logits z[0..V):
 *
 *     lpB   = -sp(-z_b)                          log sigmoid(z_b)
 *     lnb   = -sp( z_b)                          log(1 - sigmoid(z_b))
 *     m     = max_{v != b} z_v,   s = sum_{v != b} exp(z_v - m)
 *     lp[v] = ((z_v - m) - log s) + lnb          v != b
 *
 * The loss is the ordinary transducer lattice over these log-probs (FastEmit included).  From the gradient pair (gB, gL)
 * of a cell, sig = sigmoid(z_b) and q_v = exp((z_v - m) - log s):
 *
 *     u_b = gB (1 - sig) - gL sig,     u_v = gL ([v == label] - q_v)   (v != b),     dz = grad_costs[n] * u
 *
 * rounded once to the logits' type.  A non-blank logit of -inf is a masked entry: it adds nothing to m or s and gets an
 * exactly zero gradient; a row needs one finite non-blank logit.  Cells outside an utterance's (T_n, U_n + 1) window get
 * exactly zero dz.
 *
 * Both entries take logits (N,T,U,V) of type `dtype` (RNNT_DTYPE_*), V >= 2; all arithmetic is fp32 from the load on,
 * costs and gradient pairs are fp32.  Everything refused -- an unknown dtype, V < 2, a blank outside [0,V), sizes
 * rnnt_amd_workspace_size refuses, a null or misaligned workspace, a null logits / xn / yn / costs / grads_diagonal /
 * dlogits, U > 1 without labels -- comes back as RNNT_STATUS_INVALID_ARGUMENT before any HIP call.  N == 0 succeeds
 * without a launch.  A failed launch: RNNT_STATUS_PROLOGUE_FAILED (forward), RNNT_STATUS_EXPAND_FAILED (backward).
 */
#ifndef WARP_RNNT_AMD_HAT_H
#define WARP_RNNT_AMD_HAT_H

#include "warp_rnnt_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* workspace: what rnnt_amd_workspace_size answers for (N,T,U), in bytes.  grads: the gradient pairs d cost / d (lpB, lp[label]) in the
 * diagonal-major layout of RNNT_GRADS_GATHERED_DIAGONAL -- what rnnt_amd_hat_logits_backward reads. */
rnntStatus_t rnnt_amd_hat_loss_logits(rnntStream_t stream, void *workspace, int dtype, const void *logits,
                                      const int *labels, const int *xn, const int *yn, float *costs,
                                      float *grads /* (N,T,U,2) diagonal-major pairs, or NULL: costs only */,
                                      int N, int T, int U, int V, int blank, float fastemit_lambda);

/* d(sum_n grad_costs[n] * cost[n]) / d logits, (N,T,U,V) of type `dtype`, every element written. */
rnntStatus_t rnnt_amd_hat_logits_backward(rnntStream_t stream, int dtype, const void *logits, const int *labels,
                                          const float *grads_diagonal, const float *grad_costs /* or NULL: 1 */,
                                          void *dlogits, int N, int T, int U, int V, int blank);

#ifdef __cplusplus
}
#endif
#endif /* WARP_RNNT_AMD_HAT_H */
