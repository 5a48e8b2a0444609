/* The pruned transducer loss on the fused logits path: additive entries of libwarp_rnnt_amd.so (they did not move the
 * C-ABI version -- nothing that was there moves).
 *
 * The pruned loss is that of Kuang et al. 2022 ("Pruned RNN-T for fast, memory-efficient ASR training"; k2's
 * rnnt_loss_pruned with rnnt_type = "regular"): a cheap first pass picks, per frame t of utterance n, a band of S label
 * positions that begins at starts[n,t]; the joint network runs on the band only, and the loss is the ordinary transducer
 * lattice restricted to it.
 *
 *     logits (N,T,S,V), row (n,t,s)  =  lattice cell (t, u = starts[n,t] + s) of utterance n
 *     lp = log_softmax(logits[n,t,s,:]),   pair of the cell = (lp[blank], lp[labels[n,u]])
 *
 * In the last column of the lattice, and for a label outside [0,V), the label is the blank (the convention of
 * rnnt_amd_loss_logits).  Every cell of the (N,T,U) grid that no row maps to holds (F, F), F = -1e30f, and the cost is the
 * standard transducer cost of that pair plane, FastEmit included.  F is finite on purpose: the sweeps' interior computes
 * lse(-inf,-inf) = NaN; lse(x, y) with y <= F returns x bit for bit, and a gradient that passes through F is exactly 0.
 * An utterance whose band holds no path from (0,0) to (T_n - 1, U_n) comes back with a cost >= 1e29 and gradient pairs
 * without meaning: give the backward grad_costs[n] = 0 for it.
 *
 * From the gradient pair (gB, gL) of a row's cell and p = softmax(z):
 *
 *     dz[v] = grad_costs[n] * ([v == blank] gB + [v == label] gL - p[v] (gB + gL))
 *
 * rounded once to the logits' type.  A row whose u lies outside [0,U) produces nothing in the forward and gets an exactly
 * zero row in the backward (starts is device data that nobody validates on the host).  An utterance with
 * grad_costs[n] == 0 gets exactly zero rows whatever its pairs hold, and so do the rows outside an utterance's
 * (T_n, U_n + 1) window.  A logit of -inf is a masked entry: it adds nothing to the normaliser and gets an exactly zero
 * gradient; a row needs one finite logit, and the blank's and the label's must be finite.
 *
 * Both entries take logits of type `dtype` (RNNT_DTYPE_*); all arithmetic is fp32 from the load on, costs and gradient
 * pairs are fp32; V >= 2.  Everything refused -- an unknown dtype, V < 2, a blank outside [0,V), sizes
 * rnnt_amd_workspace_size refuses for (N,T,U), S < 1, S > U, N*T*S >= 2^32, a null or misaligned workspace, a null
 * logits / starts / xn / yn / costs / grads_diagonal / dlogits, grads_diagonal off a multiple of 8 bytes, U > 1 without
 * labels -- comes back as RNNT_STATUS_INVALID_ARGUMENT before any HIP call.
 * N == 0 succeeds without a launch.  A failed launch: RNNT_STATUS_PROLOGUE_FAILED (forward), RNNT_STATUS_EXPAND_FAILED
 * (backward).
 */
#ifndef WARP_RNNT_AMD_PRUNED_H
#define WARP_RNNT_AMD_PRUNED_H

#include "warp_rnnt_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* workspace: what rnnt_amd_workspace_size answers for (N,T,U), in bytes.  starts: (N,T) int32, the first lattice column of
 * every frame's band.  grads: the gradient pairs d cost / d (lp[blank], lp[label]) of the (N,T,U) grid in the
 * diagonal-major layout of RNNT_GRADS_GATHERED_DIAGONAL -- what rnnt_amd_pruned_logits_backward reads. */
rnntStatus_t rnnt_amd_pruned_loss_logits(rnntStream_t stream, void *workspace, int dtype, const void *logits,
                                         const int *labels, const int *starts, const int *xn, const int *yn, float *costs,
                                         float *grads /* (N,T,U,2) diagonal-major pairs, or NULL: costs only */,
                                         int N, int T, int U, int S, int V, int blank, float fastemit_lambda);

/* d(sum_n grad_costs[n] * cost[n]) / d logits, (N,T,S,V) of type `dtype`, every element written. */
rnntStatus_t rnnt_amd_pruned_logits_backward(rnntStream_t stream, int dtype, const void *logits, const int *labels,
                                             const int *starts, const float *grads_diagonal,
                                             const float *grad_costs /* or NULL: 1 */, void *dlogits, int N, int T, int U,
                                             int S, int V, int blank);

#ifdef __cplusplus
}
#endif
#endif /* WARP_RNNT_AMD_PRUNED_H */
