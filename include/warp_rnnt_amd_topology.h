/* k2's second lattice topology and its delay penalty for the pruned recipe -- the pruned loss
 * (warp_rnnt_amd_pruned.h) and the simple loss (warp_rnnt_amd_simple.h): additive entries of libwarp_rnnt_amd.so (they did
 * not move the C-ABI version -- nothing that was there moves).  Each entry is its namesake without the suffix with
 * `topology` (and the forwards: `delay_penalty`) behind its last argument; RNNT_TOPOLOGY_REGULAR with delay_penalty == 0
 * is that namesake, bit for bit.  What the namesakes' headers say holds here unless this one says otherwise.
 *
 * Utterance n has T_n = xn[n] frames and U_n = yn[n] labels; cell (t,u) holds the pair (lpB, lpL) as the regular entries
 * form it.
 *
 * delay_penalty dp >= 0 (Kang et al. 2022, "Delay-penalized transducer for low-latency streaming ASR"; k2's
 * px += delay_penalty * ((T_n - 1) / 2 - t)), both topologies: the label channel of every cell of frame t becomes
 *
 *     lpL + dp * (0.5f * (float)(T_n - 1) - (float)t)
 *
 * in fp32: the bracket first, one multiply, one add to the finished lpL.  The blank channel is untouched (the "log-probs" no
 * longer normalise).  The penalty is a constant with respect to the inputs: the backward entries apply the chain rule they
 * always applied, to the gradient pairs of the penalised lattice, and take no dp.  dp == 0 adds nothing.
 *
 * RNNT_TOPOLOGY_MODIFIED (k2's rnnt_type = "modified": a label consumes a frame, at most one symbol per frame):
 * alpha(0,0) = 0 and, for 1 <= t <= T_n, 0 <= u <= U_n,
 *
 *     alpha(t,u) = lse(alpha(t-1,u) + lpB(t-1,u), alpha(t-1,u-1) + lpL(t-1,u-1))      (a term with a negative index: absent)
 *     cost = -alpha(T_n, U_n)
 *
 * There is no terminal blank.  T_n < U_n has no path: the cost comes back >= 1e29 with gradient pairs without meaning, as
 * for a band without a path (give the backward grad_costs[n] = 0).  T_n == U_n is the single all-label path.
 *
 * The shear.  With t' = t - u the blank is (t',u) -> (t'+1,u) and the label (t',u) -> (t',u+1): the regular lattice with
 * T'_n = T_n - U_n + 1 frames, U_n + 1 columns and a virtual terminal cell (t' = T_n - U_n, u = U_n) whose blank is 0.  The
 * window t' in [0, T_n - U_n], u in [0, U_n] is exactly the set of modified cells that lie on a path; every other cell
 * holds the floor of warp_rnnt_amd_pruned.h.  The regular sweeps, costs, guard, FastEmit and gradient kernel run on that
 * lattice unchanged.  Its diagonals t' + u are the frames, so its diagonal-major plane with T + 1 rows is frame-major:
 *
 *     cell (t,u) of utterance n  at  ((n * (T+1) + t) * U + u),   0 <= t <= T,  row T_n: the terminal cell in column U_n
 *
 * That is the layout of the modified gradient pairs: `grads` of the pruned forward, `grads_diagonal` of its backward and
 * `pair_grads` of the simple entries are (N,T+1,U,2) fp32, d cost / d (lpB, lpL) of cell (t,u) at that address, exactly zero
 * outside the window.  The simple forward also zeroes the terminal cell's pair (d cost / d its blank is -1), so that rows
 * 0 .. T-1 of its pair_grads are the (T,U,2) pairs by frame with nothing else in them; the pruned forward leaves it.
 * Rows with t >= T_n, t < u or u > U_n -- a padding frame's band covers column U_n, whose row T_n has the terminal cell's
 * address -- are not read by the forwards and get an exactly zero gradient from the backwards; the pruned backward
 * therefore takes xn and yn.
 *
 * Workspaces: the sizes below.  RNNT_TOPOLOGY_MODIFIED takes the regular layout of (N, T+1, U) and N ints behind it.
 *
 * Refused with RNNT_STATUS_INVALID_ARGUMENT before any HIP call, besides what the namesakes refuse: an unknown topology; a
 * delay_penalty that is negative, NaN or infinite; with RNNT_TOPOLOGY_MODIFIED, sizes for which (N, T+1, U) is refused and,
 * in the pruned backward, a null xn or yn (with RNNT_TOPOLOGY_REGULAR they are not read and may be null).  The size
 * functions answer 0 for what is refused.
 */
#ifndef WARP_RNNT_AMD_TOPOLOGY_H
#define WARP_RNNT_AMD_TOPOLOGY_H

#include "warp_rnnt_amd.h"

#define RNNT_TOPOLOGY_REGULAR 0
#define RNNT_TOPOLOGY_MODIFIED 1

#ifdef __cplusplus
extern "C" {
#endif

/* the workspace of rnnt_amd_pruned_loss_logits_topology, in bytes (regular: what rnnt_amd_workspace_size answers) */
size_t rnnt_amd_pruned_topology_workspace_size(int topology, int N, int T, int U);

/* the workspace of the two simple entries below, in bytes (regular: what rnnt_amd_simple_workspace_size answers) */
size_t rnnt_amd_simple_topology_workspace_size(int topology, int N, int T, int U);

rnntStatus_t rnnt_amd_pruned_loss_logits_topology(rnntStream_t stream, void *workspace, int dtype, const void *logits,
                                                  const int *labels, const int *starts, const int *xn, const int *yn,
                                                  float *costs,
                                                  float *grads /* regular: (N,T,U,2) diagonal-major; modified:
                                                                  (N,T+1,U,2) frame-major; or NULL: costs only */,
                                                  int N, int T, int U, int S, int V, int blank, float fastemit_lambda,
                                                  int topology, float delay_penalty);

rnntStatus_t rnnt_amd_pruned_logits_backward_topology(rnntStream_t stream, int dtype, const void *logits,
                                                      const int *labels, const int *starts,
                                                      const int *xn /* modified only, else unread */,
                                                      const int *yn /* modified only, else unread */,
                                                      const float *grads_diagonal,
                                                      const float *grad_costs /* or NULL: 1 */, void *dlogits, int N,
                                                      int T, int U, int S, int V, int blank, int topology);

rnntStatus_t rnnt_amd_simple_loss_topology(rnntStream_t stream, void *workspace, int dtype, const void *am, const void *lm,
                                           const float *q, const int *labels, const int *xn, const int *yn, float *costs,
                                           float *pair_grads /* regular: (N,T,U,2); modified: (N,T+1,U,2); or NULL */,
                                           float *znorm /* (N,T,U) */, int N, int T, int U, int V, int blank,
                                           float lm_only_scale, float am_only_scale, float fastemit_lambda, int topology,
                                           float delay_penalty);

rnntStatus_t rnnt_amd_simple_backward_topology(rnntStream_t stream, void *workspace, int dtype, const void *am,
                                               const void *lm, const float *q, const int *labels, const int *xn,
                                               const int *yn, const float *pair_grads, const float *znorm,
                                               const float *grad_costs, void *dam, void *dlm, float *dq_partials, int N,
                                               int T, int U, int V, int blank, float lm_only_scale, float am_only_scale,
                                               int topology);

#ifdef __cplusplus
}
#endif
#endif /* WARP_RNNT_AMD_TOPOLOGY_H */
