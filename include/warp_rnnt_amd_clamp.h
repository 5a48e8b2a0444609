/* Gradient clamp on the fused logits path: additive entries of libwarp_rnnt_amd.so (they did not move the C-ABI
 * version -- nothing that was there moves).
 *
 * torchaudio.functional.rnnt_loss and warp-transducer's RNNTLoss take logits and a `clamp`: the d/d logits of every
 * utterance are limited to [-clamp, +clamp] elementwise and only THEN multiplied by the upstream gradient.  On the fused
 * path the unscaled gradient never exists in memory, so the clamp has to sit inside the backward kernel:
 *
 *     u[v]  = [v==blank] gB + [v==label] gL - softmax(z)[v] (gB + gL)        (unit upstream)
 *     dz[v] = grad_costs[n] * min(max(u[v], -clamp), +clamp)
 *
 * Both entries take the arguments of their unclamped twin (warp_rnnt_amd.h) and a `float clamp` behind them:
 *   - clamp negative, NaN or infinite: RNNT_STATUS_INVALID_ARGUMENT, before any HIP call -- as is everything the twin
 *     refuses;
 *   - clamp == 0: the twin, bit for bit (the same kernels);
 *   - clamp > 0: the clamped kernels, launched under the plan of the unclamped call on the same facts.  With grad_costs
 *     of 1 and a clamp that nothing reaches the result is the twin's, bit for bit.
 * What the twin answers without a launch (N == 0; STU == 0) these answer too.  A masked logit (-inf) keeps an exactly
 * zero gradient; half-precision results are the fp32 result rounded once.
 */
#ifndef WARP_RNNT_AMD_CLAMP_H
#define WARP_RNNT_AMD_CLAMP_H

#include "warp_rnnt_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The dense twin is the typed dense backward of warp_rnnt_amd.h (logits and dlogits of type `dtype`, RNNT_DTYPE_*). */
rnntStatus_t rnnt_amd_logits_backward_clamped(rnntStream_t stream, int dtype, const void *logits, const int *labels,
                                              const float *grads_diagonal, const float *grad_costs, void *dlogits,
                                              int N, int T, int U, int V, int blank, float clamp);

/* The compact twin is the compact (packed rows) backward of warp_rnnt_amd.h; rows that belong to no utterance come back
 * zero. */
rnntStatus_t rnnt_amd_compact_logits_backward_clamped(rnntStream_t stream, int dtype, const void *logits, const int *ys,
                                                      int64_t n_labels, const int *xn, const int *yn,
                                                      const int64_t *cell_offsets, const int *label_offsets,
                                                      const float *grads2, const float *grad_costs, void *dlogits,
                                                      int N, int64_t STU, int V, int blank, float clamp);

#ifdef __cplusplus
}
#endif
#endif /* WARP_RNNT_AMD_CLAMP_H */
