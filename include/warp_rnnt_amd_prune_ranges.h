/* The band selection of the pruned recipe: an additive entry of libwarp_rnnt_amd.so (it did not move the C-ABI version --
 * nothing that was there moves).
 *
 * Between the two passes of the pruned transducer loss (Kuang et al. 2022; k2's get_rnnt_prune_ranges) the gradient pairs
 * of the first pass -- rnnt_amd_simple_loss's pair_grads, minus the edge occupancies -- are turned into the first lattice
 * column of every frame's band of S label positions, the `starts` of include/warp_rnnt_amd_pruned.h.  Per utterance n, with
 * g = pair_grads + 2 * n * pitch, T_n = xn[n], U_n = yn[n]:
 *
 *     occ[t,u] = -(g[t,u,0] + g[t,u,1])                                            (fp32)
 *     hi       = clamp(U_n + 1 - S, 0, U - S)
 *     raw[t]   = the lowest u0 in [0,hi] at which w(t,u0) = occ[t,u0] + ... + occ[t,u0+S-1] is largest,   t <  T_n - 1
 *              = hi,                                                                                       t >= T_n - 1
 *     raw[t]   = min(raw[t], raw[t+1])                 from the last frame backwards, then
 *     start[t] = max(raw[t], start[t+1] - (S - 1))     from the last frame backwards.
 *
 * The S terms of w are added left to right from u0 -- ((occ[t,u0] + occ[t,u0+1]) + occ[t,u0+2]) + ... -- every sum rounded
 * to fp32 on its own: a window's bits are a function of S, u0 and its S values, not of U, T, N or the place in the batch.
 * A frame with a NaN among occ[t,u], u < hi + S, gets raw[t] = hi.  Any T_n is taken -- zero, negative, above T: the rule
 * above is all there is -- and cells u >= hi + S and rows t >= T_n - 1 are not read.  So 0 <= start[t+1] - start[t] <= S - 1,
 * start[t] = hi for t >= T_n - 1, and an utterance with (T_n - 1)(S - 1) < U_n + 1 - S, whose frames cannot climb its
 * labels in steps of S - 1, comes back with start[0] > 0 (the pruned loss then answers +inf for it).
 *
 * Two launches, no workspace, no atomics, no memset: two calls give the same starts, and the call can be captured into a
 * graph.  Everything refused -- a null pair_grads / xn / yn / starts, pair_grads off a multiple of 8 bytes or an int
 * pointer off a multiple of 4, sizes rnnt_amd_workspace_size refuses for (N,T,U), S < 2, S > U, U > 4096 (a frame's
 * occupancies are staged whole on chip), pitch < T * U -- comes back as RNNT_STATUS_INVALID_ARGUMENT before any HIP call.
 * N == 0 succeeds without a launch.  A failed launch: RNNT_STATUS_PROLOGUE_FAILED.
 */
#ifndef WARP_RNNT_AMD_PRUNE_RANGES_H
#define WARP_RNNT_AMD_PRUNE_RANGES_H

#include <stdint.h>

#include "warp_rnnt_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* pair_grads: N planes of (T,U,2) floats, rows and cells contiguous, plane n at pair_grads + 2 * n * pitch -- pitch in
 * cells, T * U for a contiguous (N,T,U,2) tensor, (T + 1) * U for the first T frames of the modified topology's
 * (N,T+1,U,2) pairs.  starts: (N,T) int32, every element written. */
rnntStatus_t rnnt_amd_prune_ranges(rnntStream_t stream, const float *pair_grads, int64_t pitch, const int *xn,
                                   const int *yn, int *starts, int N, int T, int U, int S);

#ifdef __cplusplus
}
#endif
#endif /* WARP_RNNT_AMD_PRUNE_RANGES_H */
