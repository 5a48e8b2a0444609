/* The joint network fused into the pruned transducer loss: additive entries of libwarp_rnnt_amd.so (they did not move the
 * C-ABI version -- nothing that was there moves).
 *
 * The logits of warp_rnnt_amd_pruned.h are z[n,t,s,:] = weight act(f[n,t] + g[n,u]) + bias, u = starts[n,t] + s, with
 * f (N,T,H), g (N,U,H), weight (V,H) -- the nn.Linear layout -- and bias (V,) fp32 or NULL.  These entries take the joint's
 * inputs and form z tile by tile with MFMA: neither act(f+g) (N,T,S,H) nor z (N,T,S,V) exists in memory.  Everything
 * behind z is the definition of warp_rnnt_amd_pruned.h with the regular topology: the pair of cell (t,u), the floor -1e30
 * outside the band, FastEmit, the guard; an utterance whose band holds no path comes back with a cost >= 1e29: give the
 * backward grad_costs[n] = 0 for it and all its gradients are exactly zero.  A row is part of the call when the
 * utterance's lengths are in range, t < xn[n] and 0 <= u <= yn[n]; every other row is neither read nor written (starts is
 * device data that nobody validates on the host).  From the gradient pair (gB, gL) of a row's cell:
 *
 *     dz[v] = grad_costs[n] (([v == blank] gB + [v == label] gL) - p_v (gB + gL)),   p_v = exp((z_v - m) - ls)
 *
 * with (m, ls) the maximum and the log of the sum of exp(z - m) of the row, kept as two floats and never added up.  f, g
 * and weight share one element type (dtype: RNNT_DTYPE_*), everything else is fp32; act(f+g) is computed in fp32 and
 * rounded once to that type as the matrix-core operand, and so is dz in front of the backward's products.  A bias of -inf
 * is a masked column.  No floating-point atomics: the bits of every result are a function of the inputs and the shape.
 *
 * Memory: no (N,T,S,V) tensor at any point.  The forward's state is the loss layout of (N,T,U) plus `stats`, 8 bytes per
 * band row.  The backward's workspace adds one (N,T,S,H) buffer in `dtype` (d cost / d (f+g) per row, which d g is summed
 * from), weight transposed (H, V rounded up to 64) in `dtype`, and the split-K partials of d weight and d bias, splits x
 * (V rounded up to 64) x (H + 1) fp32 with splits <= 32 and splits <= N T S / (8 H): at most a quarter of the bf16 logits.
 * So a training step holds, beyond its inputs and the gradients it returns, at most
 *
 *     rnnt_amd_pruned_joint_workspace_size(...)  +  8 N T S (stats)  +  8 N T U (the gradient pairs)  bytes.
 *
 * The Python front end adds two terms of its own: V H elements of `dtype` where it stages a master weight of another type
 * in the activations' (these entries take f, g and weight in one type), and the (N,) vectors of a call -- costs, the
 * upstream gradient, the no-path mask -- in the allocator's granules, 64 KiB at most.
 *
 * Limits: H % 32 == 0, 32 <= H <= 1024, V >= 2, 1 <= S <= U, N T S < 2^32, N T < 2^31, f, g and weight on 16-byte
 * boundaries.  Not here: the modified topology and the delay penalty of warp_rnnt_amd_topology.h, dropout, a gradient
 * clamp, band forms of the HAT and TDT losses, the compact layout.
 *
 * Everything refused -- an unknown dtype or activation, sizes outside the limits, a blank outside [0,V), a null or
 * misaligned workspace, a null f / g / weight / starts / xn / yn / costs, U > 1 without labels, grads without stats, a
 * backward without stats or grads, a misaligned f / g / weight / stats / grads -- comes back as
 * RNNT_STATUS_INVALID_ARGUMENT before any HIP call.  N == 0 succeeds without a launch.  A failed launch:
 * RNNT_STATUS_PROLOGUE_FAILED (the producer), RNNT_STATUS_WARP_FAILED (the sweeps), RNNT_STATUS_GRADS_BLANK_FAILED (the
 * gradient kernel), RNNT_STATUS_EXPAND_FAILED (the backward).  The calls only enqueue: they can be captured into a graph.
 */
#ifndef WARP_RNNT_AMD_PRUNED_JOINT_H
#define WARP_RNNT_AMD_PRUNED_JOINT_H

#include "warp_rnnt_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of workspace for both entries: the loss layout of (N,T,U), then what the backward adds (above).  0 for sizes and
 * a dtype that are refused. */
size_t rnnt_amd_pruned_joint_workspace_size(int dtype, int N, int T, int U, int S, int H, int V);

/* starts: (N,T) int32, the first lattice column of every frame's band.  stats: (N,T,S,2) fp32 -- (m, ls) per band row --
 * needed iff grads.  grads: the gradient pairs of the (N,T,U) grid in the diagonal-major layout of
 * RNNT_GRADS_GATHERED_DIAGONAL, or NULL: costs only. */
rnntStatus_t rnnt_amd_pruned_joint_loss(rnntStream_t stream, void *workspace, int dtype, int activation, const void *f,
                                        const void *g, const void *weight, const float *bias /* or NULL */,
                                        const int *labels, const int *starts, const int *xn, const int *yn, float *costs,
                                        float *stats, float *grads, int N, int T, int U, int S, int H, int V, int blank,
                                        float fastemit_lambda);

/* d(sum_n grad_costs[n] * cost[n]) / d(f, g, weight, bias): df (N,T,H) and dg (N,U,H) in `dtype`, dweight (V,H) and dbias
 * (V,) fp32; each may be NULL and is then not computed.  Every element of what is asked for is written; rows of df from
 * xn[n] on and of dg behind yn[n] are zero. */
rnntStatus_t rnnt_amd_pruned_joint_backward(rnntStream_t stream, void *workspace, int dtype, int activation,
                                            const void *f, const void *g, const void *weight, const float *bias,
                                            const int *labels, const int *starts, const int *xn, const int *yn,
                                            const float *stats, const float *grads,
                                            const float *grad_costs /* or NULL: 1 */, void *df, void *dg, float *dweight,
                                            float *dbias, int N, int T, int U, int S, int H, int V, int blank);

#ifdef __cplusplus
}
#endif
#endif /* WARP_RNNT_AMD_PRUNED_JOINT_H */
