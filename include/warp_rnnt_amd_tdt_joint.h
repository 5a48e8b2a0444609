/* The joint network fused into the token-and-duration transducer (TDT) loss: additive entries of libwarp_rnnt_amd.so (they
 * did not move the C-ABI version -- nothing that was there moves).
 *
 * The logits of warp_rnnt_amd_tdt.h are z[n,t,u,:] = weight act(f[n,t] + g[n,u]) + bias with f (N,T,H), g (N,U,H),
 * weight (V+D, H) -- the nn.Linear layout; rows [0,V) are the tokens, the blank among them at any index, row V+i is
 * durations[i] -- and bias (V+D,) fp32 or NULL: the column order of rnnt_amd_tdt_loss_logits.  These entries take the
 * joint's inputs and form z tile by tile with MFMA, as rnnt_amd_joint_loss does for the standard loss; neither act(f+g)
 * (N,T,U,H) nor z (N,T,U,V+D) exists in memory.  The lattice, the costs and dz are those of warp_rnnt_amd_tdt.h:
 *
 *     dz[v]   = grad_costs[n] (p_v S - [v == blank] G_b - [v == label] G_l)        v < V,  p_v = exp((z_v - m) - ls)
 *     dz[V+i] = grad_costs[n] (q_i S - G_dur[i])                                           q_i = exp((z_{V+i} - md) - lsd)
 *
 * with (m, ls) the maximum and the log of the sum of exp(z - m) over the token logits and (md, lsd) the same over the
 * duration logits -- the normalisers are kept as two floats each, never added up.  f, g and weight share one element type
 * (dtype: RNNT_DTYPE_*), everything else is fp32; act(f+g) is computed in fp32 and rounded once to that type as the
 * matrix-core operand.  A token or duration bias of -inf is a masked entry.
 *
 * Dropout between the activation and the projection: p in [0,1) and a seed word in DEVICE memory, the mask that of
 * warp_rnnt_amd_joint_dropout.h (Philox4x32-10, counter (n, t, u, k >> 2); rnnt_amd_joint_dropout_mask_host describes it).
 * p == 0 means no dropout and the seed is unread.  Hand the backward the forward's p and seed.
 *
 * Limits: H % 32 == 0, 32 <= H <= 1024, V >= 2, 1 <= D <= 9 durations that are distinct integers in [0,8] with 1 among
 * them, U <= 1024 lattice columns, f, g and weight on 16-byte boundaries.  Not here: the mix with the standard loss
 * (NeMo's omega), a gradient clamp, the compact layout, a joint entry for rnnt_amd_tdt_align or for the HAT loss.
 *
 * Everything refused -- an unknown dtype or activation, sizes or durations outside the limits, a blank outside [0,V), sigma
 * < 0 or not finite, p outside [0,1), p > 0 without a seed, a null or misaligned workspace, a null f / g / weight / xn /
 * yn / costs / durations, U > 1 without labels, grads without stats, a backward without stats or grads, a misaligned
 * f / g / weight / stats / grads -- comes back as RNNT_STATUS_INVALID_ARGUMENT before any HIP call.  N == 0 succeeds
 * without a launch.  A failed launch: RNNT_STATUS_PROLOGUE_FAILED (the producer), RNNT_STATUS_WARP_FAILED (the sweeps),
 * RNNT_STATUS_GRADS_BLANK_FAILED (the gradient kernel), RNNT_STATUS_EXPAND_FAILED (the backward).  The calls only enqueue:
 * they can be captured into a graph.
 */
#ifndef WARP_RNNT_AMD_TDT_JOINT_H
#define WARP_RNNT_AMD_TDT_JOINT_H

#include <stdint.h>

#include "warp_rnnt_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of workspace for both entries: the TDT loss's layout for (N,T,U,D) (warp_rnnt_amd_tdt.h), then weight transposed
 * (H, V+D rounded up to 32) and the split-K partials of d weight and d bias -- that second part is a function of (H, V+D)
 * and of the split count alone.  0 for sizes that are refused. */
size_t rnnt_amd_tdt_joint_workspace_size(int N, int T, int U, int H, int V, int D);

/* durations: D integers in HOST memory, read during the call.  stats: (N,T,U,4) fp32 -- (m, ls, md, lsd) per cell -- needed
 * iff grads.  grads: (2+D, N, T, U) fp32 -- G_b, G_l, G_dur[0..D) as planes in the diagonal-major cell order -- or NULL:
 * costs only; the beta sweep and the gradient kernel do not run. */
rnntStatus_t rnnt_amd_tdt_joint_loss(rnntStream_t stream, void *workspace, int dtype, int activation, const void *f,
                                     const void *g, const void *weight, const float *bias /* or NULL */,
                                     const int *labels, const int *xn, const int *yn, const int *durations /* host */,
                                     int D, float *costs, float *stats, float *grads, int N, int T, int U, int H, int V,
                                     int blank, float sigma, float fastemit_lambda, float p, const uint64_t *seed);

/* d(sum_n grad_costs[n] * cost[n]) / d(f, g, weight, bias): df (N,T,H) and dg (N,U,H) in `dtype`, dweight (V+D,H) and
 * dbias (V+D,) fp32; each may be NULL and is then not computed.  Every element of what is asked for is written; rows of df
 * from xn[n] on and of dg behind yn[n] are zero.  The bits of dweight / dbias are a function of the shape and the inputs
 * alone (fixed split order, no atomics). */
rnntStatus_t rnnt_amd_tdt_joint_backward(rnntStream_t stream, void *workspace, int dtype, int activation, const void *f,
                                         const void *g, const void *weight, const float *bias, const int *labels,
                                         const int *xn, const int *yn, const float *stats, const float *grads,
                                         const float *grad_costs /* or NULL: 1 */, void *df, void *dg, float *dweight,
                                         float *dbias, int N, int T, int U, int H, int V, int D, int blank, float p,
                                         const uint64_t *seed);

#ifdef __cplusplus
}
#endif
#endif /* WARP_RNNT_AMD_TDT_JOINT_H */
