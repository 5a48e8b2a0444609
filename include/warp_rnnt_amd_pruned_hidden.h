/* The pruned joiner's hidden activations: additive entries of libwarp_rnnt_amd.so (they did not move the C-ABI version --
 * nothing that was there moves).
 *
 * Between the band selection (warp_rnnt_amd_prune_ranges.h) and the output projection of the pruned recipe's joiner stands
 * h = act(f + g on the band).  With f (N,T,H), g (N,U,H), starts (N,T) int32 and a band of S positions, for a live frame
 *
 *     h[n,t,s,:] = act( (float)f[n,t,:] + (float)g[n, clamp(starts[n,t] + s, 0, U-1), :] )
 *
 * the sum in fp32 (no contraction), the activation in fp32, rounded once to `dtype`; the index sum in 64 bits.  xn (N,)
 * int32 may be NULL: every frame is live.  Otherwise frame t of utterance n is live iff t < xn[n] (any xn[n]: below 1 none
 * is, above T all are); a frame that is not live is not read -- neither f, g nor its start -- and its S rows of h are
 * exactly zero.
 *
 * The backward takes dh and the h the forward wrote, both (N,T,S,H) of `dtype`.  With p = (float)dh * act'((float)h) --
 * act' from the rounded output: 1 - h^2 for tanh, [h > 0] for relu -- over live frames,
 *
 *     df[n,t,:] = sum_s p[n,t,s,:]
 *     dg[n,u,:] = sum over (t,s) with clamp(starts[n,t] + s, 0, U-1) == u of p[n,t,s,:]
 *
 * each sum in fp32 in ascending t, then ascending s, rounded once.  df rows of frames that are not live and dg rows no live
 * (t,s) maps to are exactly zero.  df or dg may be NULL: that gradient is not computed (dg == NULL: the workspace is not
 * touched and may be NULL).  No atomics, no (N,T,S,H) temporary: two calls give the same bits.  dh and h are read once for
 * df and once for dg.  starts is device data nobody validates: any values are legal, monotone or not.
 *
 * Shapes: N >= 0, T >= 1, U >= 1, S >= 1, H % 8 == 0, 8 <= H <= 4096, the (N,T,U) sizes rnnt_amd_workspace_size takes,
 * N*T*S < 2^32, N*T*S*H < 2^40 and N*U*H < 2^40.  Everything else -- and an unknown dtype or activation, a null f / g /
 * starts / h (forward), a null dh / h / starts or a dg without a workspace on a multiple of 256 bytes (backward), f, g, h,
 * dh, df or dg off a multiple of 16 bytes, starts or xn off a multiple of 4 -- comes back as RNNT_STATUS_INVALID_ARGUMENT
 * before any HIP call.  N == 0 succeeds without a launch.  A failed launch: RNNT_STATUS_PROLOGUE_FAILED (forward),
 * RNNT_STATUS_EXPAND_FAILED (backward).  The calls only enqueue (no read-back, no allocation, no memset): they can be
 * captured into a graph.
 */
#ifndef WARP_RNNT_AMD_PRUNED_HIDDEN_H
#define WARP_RNNT_AMD_PRUNED_HIDDEN_H

#include "warp_rnnt_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of the backward's workspace, a function of the shape alone; 0 for a shape the entries refuse.  One piece: per
 * (n,u) the range [lo,hi) of frames the dg kernel walks, two int32 -- 8*N*U bytes rounded up to 256. */
size_t rnnt_amd_pruned_hidden_workspace_size(int N, int T, int U, int S, int H);

rnntStatus_t rnnt_amd_pruned_hidden(rnntStream_t stream, int dtype, int activation, const void *f, const void *g,
                                    const int *starts, const int *xn /* or NULL */, void *h /* (N,T,S,H) */, int N, int T,
                                    int U, int S, int H);

rnntStatus_t rnnt_amd_pruned_hidden_backward(rnntStream_t stream, void *workspace, int dtype, int activation,
                                             const void *dh, const void *h, const int *starts, const int *xn /* or NULL */,
                                             void *df /* (N,T,H) or NULL */, void *dg /* (N,U,H) or NULL */, int N, int T,
                                             int U, int S, int H);

#ifdef __cplusplus
}
#endif
#endif /* WARP_RNNT_AMD_PRUNED_HIDDEN_H */
