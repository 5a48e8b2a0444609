/* The multi-blank transducer loss on the fused logits path: additive entries of libwarp_rnnt_amd.so (they did not move
 * the C-ABI version -- nothing that was there moves).
 *
 * The multi-blank transducer is the one of Xu et al. 2022, "Multi-blank Transducers for Speech Recognition" (NeMo's
 * MultiblankRNNTLossNumba), TDT's predecessor: beside the standard blank the vocabulary holds "big blanks" that consume
 * 2, 4, 8 ... frames at once.
 *
 * Inputs.  Logits (N,T,U,V) in fp32, bf16 or fp16, with one softmax over all V columns.  B blanks, given as blank_ids[i]
 * and blank_durations[i] for i < B: the ids are distinct and lie in [0,V); the durations are distinct integers in [1,8],
 * in any order, with 1 among them (the standard blank); so 1 <= B <= 8, and V >= B + 1.  sigma >= 0.
 *
 * Per cell.  lp = log_softmax(z) - sigma, in fp32 from the load on.
 *
 * Edges out of (t,u), for an utterance with T_n frames and U_n labels:
 *
 *     blank i, d = blank_durations[i], weight lp[blank_ids[i]]:  to (t+d, u) if t+d < T_n;  to the end if t+d == T_n and u == U_n
 *     label,                            weight lp[labels[u]]:     to (t, u+1) if u < U_n
 *
 * There are no other edges.  This is NeMo's lattice: a big blank reaches the end only when it lands exactly on T_n.
 *
 * Costs.  alpha(0,0) = 0.  alpha of a cell is the log-sum-exp over its incoming edges of alpha(source) + weight.  ll is
 * the same sum over the edges to the end.  costs[n] = -ll.  beta is the mirror image.
 *
 * The operation order of a cell, in both sweeps: the maximum of the terms, then one sum of exponentials with blanks
 * i = 0..B-1 followed by the label, then one log.  A term is alpha(source) + weight (beta: weight + beta(destination)),
 * every sum rounded on its own.
 *
 * Gradients.  An edge has the occupancy exp(alpha(t,u) + w + beta(dest) - ll).  Label edges are multiplied by
 * 1 + fastemit_lambda.  The costs do not move.  Per cell: G_l, G_blank[i], and S = G_l + sum_i G_blank[i].  With
 * p = softmax(z):
 *
 *     dz[v] = grad_costs[n] (p_v S - [v == labels[u]] G_l - sum_i [v == blank_ids[i]] G_blank[i])
 *
 * This is the true derivative of the cost.  It is rounded once to the logits' type.  The label is subtracted first, then
 * i ascending.
 *
 * Special cases.  -inf is a masked entry: probability zero, gradient exactly zero.  Every row needs a finite
 * standard-blank logit and a finite label logit.  A label that equals a blank id is the caller's business.  The lattice
 * above is still what is computed.  A cell outside an utterance's window gets exactly zero dz.  An utterance with lengths
 * outside [1,T] x [0,U-1] gets a NaN cost and zero dz.  With B = 1 the cost is the standard loss plus sigma (T_n + U_n).
 *
 * Not here: the compact layout, a joint entry, an align entry, a gradient clamp, the forward/backward mismatch guard.  A
 * lattice has at most 1024 columns: U <= 1024 (the sweeps hold a column per lane of one workgroup); a wider one is refused.
 *
 * Everything refused -- an unknown dtype, V < B + 1, ids or durations that are not as above, B outside [1,8], U > 1024 or
 * sizes rnnt_amd_workspace_size refuses, sigma < 0 or not finite, a null or misaligned workspace, a null or misaligned
 * logits / costs / grads / dlogits, a null xn / yn / blank_ids / blank_durations, U > 1 without labels -- comes back as
 * RNNT_STATUS_INVALID_ARGUMENT before any HIP call.  N == 0 succeeds without a launch.  A failed launch:
 * RNNT_STATUS_PROLOGUE_FAILED (the producer), RNNT_STATUS_WARP_FAILED (the sweeps), RNNT_STATUS_GRADS_BLANK_FAILED (the
 * gradient kernel), RNNT_STATUS_EXPAND_FAILED (the backward).
 */
#ifndef WARP_RNNT_AMD_MULTIBLANK_H
#define WARP_RNNT_AMD_MULTIBLANK_H

#include "warp_rnnt_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of workspace for rnnt_amd_multiblank_loss_logits: a function of (N,T,U,B) alone; 0 for sizes that are refused. */
size_t rnnt_amd_multiblank_workspace_size(int N, int T, int U, int B);

/* blank_ids, blank_durations: B integers each in HOST memory, read during the call (they travel to the kernels by value,
 * so a captured call keeps them).  grads: (1+B, N, T, U) fp32 -- G_l, G_blank[0..B) as planes, each in the diagonal-major
 * cell order -- what rnnt_amd_multiblank_logits_backward reads.  grads == NULL: costs only; the beta sweep and the
 * gradient kernel do not run. */
rnntStatus_t rnnt_amd_multiblank_loss_logits(rnntStream_t stream, void *workspace, int dtype, const void *logits,
                                             const int *labels, const int *xn, const int *yn, const int *blank_ids,
                                             const int *blank_durations, int B, float *costs,
                                             float *grads /* or NULL: costs only */, int N, int T, int U, int V,
                                             float sigma, float fastemit_lambda);

/* d(sum_n grad_costs[n] * cost[n]) / d logits, (N,T,U,V) of type `dtype`, every element written.  blank_ids: as above. */
rnntStatus_t rnnt_amd_multiblank_logits_backward(rnntStream_t stream, int dtype, const void *logits, const int *labels,
                                                 const float *grads, const float *grad_costs /* or NULL: 1 */,
                                                 void *dlogits, int N, int T, int U, int V, const int *blank_ids, int B);

#ifdef __cplusplus
}
#endif
#endif /* WARP_RNNT_AMD_MULTIBLANK_H */
