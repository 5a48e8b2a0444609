/* The factorised-blank (HAT) loss on the pruned band: additive entries of libwarp_rnnt_amd.so (they did not move the C-ABI
 * version -- nothing that was there moves).
 *
 * k2's rnnt_loss_pruned(..., use_hat_loss=True), what icefall's zipformer_hat trains with: the pruned transducer loss of
 * warp_rnnt_amd_pruned.h and warp_rnnt_amd_topology.h with the log-probs of warp_rnnt_amd_hat.h in every cell of the band.
 *
 *     logits (N,T,S,V), row (n,t,s)  =  lattice cell (t, u = starts[n,t] + s) of utterance n
 *     lpB = -sp(-z_b),     lp[v] = ((z_v - m) - log s) + (-sp(z_b))  for v != b,     pair of the cell = (lpB, lp[labels[n,u]])
 *
 * with b = blank, sp(x) = max(x,0) + log1p(exp(-|x|)), m = max_{v != b} z_v and s = sum_{v != b} exp(z_v - m).  In the last
 * column of the lattice, and for a label outside [0,V), the label channel holds lpB.  delay_penalty is added to the finished
 * label channel as warp_rnnt_amd_topology.h says; every cell no row maps to holds the floor of warp_rnnt_amd_pruned.h.  From
 * the gradient pair (gB, gL) of a row's cell, sig = sigmoid(z_b) and q_v = exp((z_v - m) - log s):
 *
 *     u_b = gB (1 - sig) - gL sig,     u_v = gL ([v == label] - q_v)   (v != b),     dz = grad_costs[n] * u
 *
 * rounded once to the logits' type.  A row's result has the bits rnnt_amd_hat_loss_logits / rnnt_amd_hat_logits_backward
 * give the same row: with S == U, starts of zero and RNNT_TOPOLOGY_REGULAR the two entries below are those two.
 *
 * The two entries take the argument lists of rnnt_amd_pruned_loss_logits_topology and
 * rnnt_amd_pruned_logits_backward_topology, and what their headers say holds here: the layouts of `grads` /
 * `grads_diagonal` under the two topologies, the rows that are not read by the forward and come back exactly zero from
 * the backward (u outside [0,U); outside the modified window; grad_costs[n] == 0; a gradient pair of (0,0)) -- without a
 * look at the logits --, the cost >= 1e29 of an utterance whose band holds no path, and everything that is refused with
 * RNNT_STATUS_INVALID_ARGUMENT before any HIP call.  workspace: rnnt_amd_pruned_topology_workspace_size(topology, N, T, U)
 * bytes.  N == 0 succeeds without a launch.  A failed launch: RNNT_STATUS_PROLOGUE_FAILED (forward),
 * RNNT_STATUS_EXPAND_FAILED (backward).
 */
#ifndef WARP_RNNT_AMD_PRUNED_HAT_H
#define WARP_RNNT_AMD_PRUNED_HAT_H

#include "warp_rnnt_amd.h"
#include "warp_rnnt_amd_topology.h"

#ifdef __cplusplus
extern "C" {
#endif

rnntStatus_t rnnt_amd_pruned_hat_loss_logits(rnntStream_t stream, void *workspace, int dtype, const void *logits,
                                             const int *labels, const int *starts, const int *xn, const int *yn,
                                             float *costs,
                                             float *grads /* regular: (N,T,U,2) diagonal-major; modified: (N,T+1,U,2)
                                                             frame-major; or NULL: costs only */,
                                             int N, int T, int U, int S, int V, int blank, float fastemit_lambda,
                                             int topology, float delay_penalty);

/* d(sum_n grad_costs[n] * cost[n]) / d logits, (N,T,S,V) of type `dtype`, every element written. */
rnntStatus_t rnnt_amd_pruned_hat_logits_backward(rnntStream_t stream, int dtype, const void *logits, const int *labels,
                                                 const int *starts, const int *xn /* modified only, else unread */,
                                                 const int *yn /* modified only, else unread */,
                                                 const float *grads_diagonal, const float *grad_costs /* or NULL: 1 */,
                                                 void *dlogits, int N, int T, int U, int S, int V, int blank,
                                                 int topology);

#ifdef __cplusplus
}
#endif
#endif /* WARP_RNNT_AMD_PRUNED_HAT_H */
