/* The "simple" transducer loss, the smoothed first pass of the pruned recipe: additive entries of libwarp_rnnt_amd.so
 * (they did not move the C-ABI version -- nothing that was there moves).
 *
 * The pruned loss of Kuang et al. 2022 is the second half of a two-pass recipe.  The first half is the transducer loss
 * over the trivial joiner am[n,t,:] + lm[n,u,:], smoothed towards the two marginal models -- in exact arithmetic k2's
 * rnnt_loss_smoothed(lm, am, symbols, termination_symbol = blank, lm_only_scale, am_only_scale, boundary) with the
 * "regular" topology.  Per utterance n (the index dropped), am (T,V), lm (U,V), labels y_0 .. y_{U-2}, blank b,
 * c1 = lm_only_scale, c2 = am_only_scale, c0 = 1 - c1 - c2, q (V,) the log of a unigram distribution:
 *
 *     sym(u,0) = b,   sym(u,1) = y_u for u < U-1 and 0 <= y_u < V, else b
 *     Z(t,u)   = log(max(sum_v exp(am[t,v] + lm[u,v]), tiny))       (tiny: FLT_MIN after the two row maxima are taken out)
 *     ZL(u)    = log sum_v exp(lm[u,v]),     ZA(t) = log sum_v exp(am[t,v] + q[v])
 *     pair(t,u,c) = c0 (am[t,s] + lm[u,s] - Z(t,u)) + c1 (lm[u,s] - ZL(u)) + c2 (am[t,s] + q[s] - ZA(t)),   s = sym(u,c)
 *     cost = the standard transducer cost of that (T,U,2) pair plane, FastEmit included
 *
 * q is read only when am_only_scale != 0 and is an input: k2's batch unigram, log(mean over the batch's (n,u) rows of
 * softmax(lm[n,u,:]) + tiny), is the caller's to form (and to differentiate).  With am_only_scale == 0 an utterance's
 * result does not depend on its batch.  am and lm are finite: a -inf entry is not a masked entry here.
 *
 * The backward, with G(t,u,c) = grad_costs[n] * pair_grads[n,t,u,c], S = G(.,.,0) + G(.,.,1),
 * P(t,u,v) = exp(am[t,v] + lm[u,v] - Z(t,u)), PA(t,:) = softmax(am[t,:] + q), PL(u,:) = softmax(lm[u,:]):
 *
 *     d am[t,v] = (c0+c2) sum_u sum_c [v == sym(u,c)] G(t,u,c) - c0 sum_u S(t,u) P(t,u,v) - c2 PA(t,v) sum_u S(t,u)
 *     d lm[u,v] = (c0+c1) sum_t sum_c [v == sym(u,c)] G(t,u,c) - c0 sum_t S(t,u) P(t,u,v) - c1 PL(u,v) sum_t S(t,u)
 *     d q[v]    = c2 sum_n (sum_{t,u,c} [v == sym(u,c)] G(t,u,c) - sum_t PA(t,v) sum_u S(t,u))      (lm held fixed)
 *
 * rounded once to the inputs' type.  Rows t >= T_n of d am, rows u > U_n of d lm and every row of an utterance with
 * grad_costs[n] == 0 are exactly zero.  No floating-point atomics: the same bits from run to run.
 *
 * Both entries take am and lm of type `dtype` (RNNT_DTYPE_*); all arithmetic is fp32 from the load on; costs, gradient
 * pairs, znorm, q and d q are fp32.  Everything refused -- an unknown dtype, V < 2 or V > 2^24, a blank outside [0,V),
 * sizes rnnt_amd_workspace_size refuses for (N,T,U), T or U above 65535 * 64, a scale that is negative, not finite or a
 * sum of the two above 1 (in fp32), am_only_scale != 0 without q, a null or misaligned workspace, a null am / lm / xn / yn /
 * costs (forward) or am / lm / xn / yn / pair_grads / znorm / d am / d lm (backward), pair_grads without znorm, am / lm /
 * d am / d lm off a multiple of their element size, pair_grads off a multiple of 8 bytes, any other pointer off a
 * multiple of 4, U > 1 without labels -- comes back as RNNT_STATUS_INVALID_ARGUMENT before any HIP call.  N == 0 succeeds
 * without a launch.  A failed launch: RNNT_STATUS_PROLOGUE_FAILED (the producer), RNNT_STATUS_EXPAND_FAILED (backward).
 */
#ifndef WARP_RNNT_AMD_SIMPLE_H
#define WARP_RNNT_AMD_SIMPLE_H

#include "warp_rnnt_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of the workspace of both entries for (N,T,U): what rnnt_amd_workspace_size answers, then the row statistics of am
 * and lm and the backward's row sums (O(N (T + U)) floats).  0: sizes the entries refuse.  The workspace carries nothing
 * from the forward to the backward. */
size_t rnnt_amd_simple_workspace_size(int N, int T, int U);

/* pair_grads: d cost[n] / d pair, (N,T,U,2) row-major, every element written, zero outside an utterance's
 * (T_n, U_n + 1) window -- not scaled by any upstream gradient.  znorm: Z(t,u) minus the row maxima of am[t,:] and lm[u,:],
 * (N,T,U) row-major, every element written: what the backward needs of Z.  Both NULL: costs only. */
rnntStatus_t rnnt_amd_simple_loss(rnntStream_t stream, void *workspace, int dtype, const void *am, const void *lm,
                                  const float *q /* (V,), or NULL with am_only_scale == 0 */, const int *labels,
                                  const int *xn, const int *yn, float *costs, float *pair_grads /* or NULL */,
                                  float *znorm /* or NULL; required with pair_grads */, int N, int T, int U, int V,
                                  int blank, float lm_only_scale, float am_only_scale, float fastemit_lambda);

/* d(sum_n grad_costs[n] * cost[n]) / d am (N,T,V) and / d lm (N,U,V) of type `dtype`, every element written, and the
 * per-utterance partial vectors of d q, (N,V) fp32, every element written when am_only_scale != 0 (otherwise untouched; may
 * be NULL): d q is their sum over n.  pair_grads and znorm: what the forward wrote. */
rnntStatus_t rnnt_amd_simple_backward(rnntStream_t stream, void *workspace, int dtype, const void *am, const void *lm,
                                      const float *q, const int *labels, const int *xn, const int *yn,
                                      const float *pair_grads, const float *znorm,
                                      const float *grad_costs /* or NULL: 1 */, void *dam, void *dlm,
                                      float *dq_partials /* (N,V), or NULL */, int N, int T, int U, int V, int blank,
                                      float lm_only_scale, float am_only_scale);

#ifdef __cplusplus
}
#endif
#endif /* WARP_RNNT_AMD_SIMPLE_H */
