/* Dropout inside the fused joint: additive entries of libwarp_rnnt_amd.so (they did not move the C-ABI version -- nothing
 * that was there moves).
 *
 * The joint most transducers train is  activation -> Dropout(p) -> Linear(H, V).  Dropout acts on act(f+g), (N,T,U,H),
 * the tensor the fused joint (warp_rnnt_amd.h: rnnt_amd_joint_loss) never forms, so it cannot be applied from outside;
 * these entries apply it where the kernels stage that operand:
 *
 *     h~[n,t,u,k] = E(m[n,t,u,k] * scale * act_fp32(f[n,t,k] + g[n,u,k]))    (one rounding to E = `dtype`)
 *     z  = weight @ h~ + bias,   dweight = sum dz^T h~,   d/d(f+g) = (dz weight) * m * scale * act'(h~ / scale)
 *
 * The mask is a pure function of (seed, p, n, t, u, k) -- Philox4x32-10 (multipliers 0xD2511F53, 0xCD9E8D57; key
 * increments 0x9E3779B9, 0xBB67AE85; ten rounds):
 *     key     = (low 32 bits of seed, high 32 bits of seed)
 *     counter = (n, t, u, k >> 2);   output word (k & 3) decides element k
 *     m = [word < thr],   thr = min(2^32 - 1, floor((1 - (double)p) * 2^32)),   scale = (float)(1 / (1 - (double)p))
 * The counter holds n, t, u themselves: the mask of an utterance does not change with the padding of the batch around
 * it, and forward and backward (whose kernels walk the cells in three different orders) see one mask.
 *
 * rnnt_amd_joint_loss_dropout / rnnt_amd_joint_backward_dropout take the arguments of their twin (warp_rnnt_amd.h) with
 * `float p, const uint64_t *seed` behind them; the workspace is the twin's (rnnt_amd_joint_workspace_size).
 *   - seed is a DEVICE pointer, 8-byte aligned, read by the kernels when they run: a captured graph replays with whatever
 *     the word holds at replay time.  Hand the backward the seed (and p) of its forward.
 *   - p == 0: the twin, bit for bit (the same kernels); seed is ignored and may be NULL.
 *   - p < 0, p >= 1, a NaN p, or p > 0 with a NULL or misaligned seed: RNNT_STATUS_INVALID_ARGUMENT before any HIP call --
 *     as is everything the twin refuses.
 * What the twin answers without a launch (N == 0; a backward with no output) these answer too.
 *
 * rnnt_amd_joint_dropout_mask_host: the same definition on the host, no HIP call: keep (N,T,U,H), one byte per element
 * (1 = kept).  RNNT_STATUS_INVALID_ARGUMENT for a p outside [0,1), a negative size or a NULL keep.  It exists so that the
 * mask can be checked, and reference results formed, without a GPU.
 */
#ifndef WARP_RNNT_AMD_JOINT_DROPOUT_H
#define WARP_RNNT_AMD_JOINT_DROPOUT_H

#include "warp_rnnt_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

rnntStatus_t rnnt_amd_joint_loss_dropout(rnntStream_t stream, void *workspace, int dtype, int activation, const void *f,
                                         const void *g, const void *weight, const float *bias, const int *labels,
                                         const int *xn, const int *yn, float *costs, float *lse, float *grads, int N,
                                         int T, int U, int H, int V, int blank, float fastemit_lambda, float p,
                                         const uint64_t *seed);

rnntStatus_t rnnt_amd_joint_backward_dropout(rnntStream_t stream, void *workspace, int dtype, int activation,
                                             const void *f, const void *g, const void *weight, const float *bias,
                                             const int *labels, const int *xn, const int *yn, const float *lse,
                                             const float *grads, const float *grad_costs, void *df, void *dg,
                                             float *dweight, float *dbias, int N, int T, int U, int H, int V, int blank,
                                             float p, const uint64_t *seed);

rnntStatus_t rnnt_amd_joint_dropout_mask_host(uint64_t seed, float p, int N, int T, int U, int H, unsigned char *keep);

#ifdef __cplusplus
}
#endif
#endif /* WARP_RNNT_AMD_JOINT_DROPOUT_H */
