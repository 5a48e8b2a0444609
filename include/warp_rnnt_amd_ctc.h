/* The CTC loss (Graves et al. 2006) from logits: additive entries of libwarp_rnnt_amd.so (they did not move the C-ABI
 * version -- nothing that was there moves).
 *
 * logits (N,T,V) of `dtype`, batch-major and contiguous; labels (N,L) int32, padded; xn, yn (N,) int32: the frames T_n and
 * the labels L_n of utterance n.  A label that is no index of [0,V) is read as the blank.
 *
 * Emissions.  For a live row (t < T_n), with z the row as floats, m = max z and ls = log sum exp(z - m) (chunks of 8
 * elements, chunk c on lane c mod G of the row's G lanes, each lane's running maximum and sum in ascending order, the
 * lanes joined by an xor butterfly):
 *
 *     E[n,t,0]   = max(((float)z[blank]       - m) - ls, FLOOR)
 *     E[n,t,1+l] = max(((float)z[labels[n,l]] - m) - ls, FLOOR)        l < L_n            FLOOR = -1e30f
 *
 * Lattice.  T_n frames by 2 L_n + 1 states: B_l (the blank in front of label l, l = 0..L_n; B_{L_n} is the final blank) and
 * S_l (label l, l < L_n).  skip_l = l > 0 and labels[n,l] != labels[n,l-1].  With lse(a,b,c) = M + log(exp(a-M) + exp(b-M)
 * + exp(c-M)), M = max(a,b,c), the sum from the left, exp and log the hardware's base-2 forms scaled by log2(e) and ln 2:
 *
 *     alpha[0,B_0] = E[0,0]     alpha[0,S_0] = E[0,1]     every other state of frame 0: FLOOR
 *     alpha[t,B_l] = max(E[t,0]   + lse(alpha[t-1,B_l], alpha[t-1,S_{l-1}], FLOOR),                          FLOOR)
 *     alpha[t,S_l] = max(E[t,1+l] + lse(alpha[t-1,S_l], alpha[t-1,B_l], skip_l ? alpha[t-1,S_{l-1}] : FLOOR), FLOOR)
 *
 * (a state that does not exist counts as FLOOR).  beta is the same recursion on the utterance read backwards -- frames from
 * T_n - 1 down, the labels from L_n - 1 down, B_l in the place of B_{L_n - l} -- so beta[t,s] holds E[t,s] as alpha[t,s]
 * does.  Every value is finite: nothing is ever -inf, no difference of infinities is formed.
 *
 *     ll_n    = lse(alpha[T_n-1,B_{L_n}], alpha[T_n-1,S_{L_n-1}], FLOOR)
 *     costs[n] = -ll_n,  or +inf where ll_n <= FLOOR / 2: no path (T_n < L_n + the adjacent repeats)
 *
 * Lengths outside 1 <= xn[n] <= T, 0 <= yn[n] <= L: nothing of the utterance is read, costs[n] is NaN, its gradient zero.
 *
 * Backward.  occ(s) = exp(((alpha[t,s] + beta[t,s]) - E[t,s]) - ll_n).  The blank's: each lane adds its B_l in ascending l,
 * the lanes joined by the xor butterfly.  A token's: the label positions of an utterance are put in a stable order by token
 * (a function of the labels alone), and the positions that share a token are added in that order, from 0, by one lane.
 *
 *     dlogits[n,t,v] = (E) ( dcosts[n] * ( exp(((float)z[v] - m) - ls) - occ_token(v) - [v == blank] occ_blank ) )
 *
 * rounded once to `dtype`.  Rows t >= T_n, utterances without a path and utterances with lengths out of range are written
 * as zeros, and their logits are not read.  dcosts == NULL: ones.  No atomics anywhere: two calls give the same bits, and
 * an utterance's bits do not depend on the batch around it.
 *
 * The forward runs the emission kernel and the alpha sweep and leaves them in the workspace; the backward runs the beta
 * sweep, the label order and the gradient kernel on the workspace the forward of the same arguments left.
 *
 * Shapes: N >= 0, T >= 1, 1 <= L <= 1023, 2 <= V <= 16384, 0 <= blank < V, N*T*(L+1) < 2^31.  Everything else -- and an
 * unknown dtype, a null logits / labels / xn / yn / costs (forward) or dlogits (backward), a workspace that is null or off a
 * multiple of 256 bytes, logits or dlogits off a multiple of their element size, labels / xn / yn / costs / dcosts off a
 * multiple of 4 -- comes back as RNNT_STATUS_INVALID_ARGUMENT before any HIP call.  N == 0 succeeds without a launch.  A
 * failed launch: RNNT_STATUS_PROLOGUE_FAILED (forward), RNNT_STATUS_EXPAND_FAILED (backward).  The calls only enqueue (no
 * read-back, no allocation, no memset): they can be captured into a graph.
 */
#ifndef WARP_RNNT_AMD_CTC_H
#define WARP_RNNT_AMD_CTC_H

#include "warp_rnnt_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of the workspace, a function of the shape alone; 0 for a shape the entries refuse.  Pieces, each rounded up to 256
 * bytes, fp32 unless said: (m, ls) per row (N,T,2); E (N,T,L+1); alpha (N,T,2,L+1) -- channel 0 the B_l, channel 1 the
 * S_l; beta, the same; ll (N,); the label order (N,L) int32. */
size_t rnnt_amd_ctc_workspace_size(int N, int T, int L, int V);

rnntStatus_t rnnt_amd_ctc_loss_logits(rnntStream_t stream, void *workspace, int dtype, const void *logits,
                                      const int *labels, const int *xn, const int *yn, float *costs, int N, int T, int L,
                                      int V, int blank);

rnntStatus_t rnnt_amd_ctc_logits_backward(rnntStream_t stream, void *workspace, int dtype, const void *logits,
                                          const int *labels, const int *xn, const int *yn,
                                          const float *dcosts /* or NULL */, void *dlogits, int N, int T, int L, int V,
                                          int blank);

#ifdef __cplusplus
}
#endif
#endif /* WARP_RNNT_AMD_CTC_H */
