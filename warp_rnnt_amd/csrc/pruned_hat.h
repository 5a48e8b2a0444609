// Launch interface of the factorised-blank (HAT) kernels on the pruned band (pruned_hat.hip) for the C ABI of
// include/warp_rnnt_amd_pruned_hat.h.
#pragma once
#include <hip/hip_runtime.h>

namespace rnnt {

// The pruned loss of pruned.h with HAT's pair in every cell of the band (hat.h): logits (N,T,S,V) of RNNT_DTYPE_*, row
// (n,t,s) is lattice cell (t, u = starts[n*T + t] + s); the plane, its floor, the topologies, the delay penalty, xn / yn and
// the rows that are not read or come back exactly zero are launch_pruned_pairs' and launch_pruned_logits_backward's.
//   pairs: PRUNED_FLOOR over the plane, then make_float2(lpB, lp[label] (+ penalty)) of every live row, lpB = log
//   sigmoid(z_b), lp[label] = log softmax over v != b + log(1 - sigmoid(z_b)), lpB again where the label channel is the
//   blank's;
//   backward: u_b = gB (1 - sig) - gL sig, u_v = gL ([v == l] - q_v), dz = scale[n] * u, rounded once to the logits' type.
// A row's bits are those of the same row under launch_hat_gather_skewed / launch_hat_logits_backward.
hipError_t launch_pruned_hat_pairs(hipStream_t stream, int dtype, const void* logits, const int* labels, const int* starts,
                                   const int* xn, const int* yn, float* ws2, int N, int T, int U, int S, int V, int blank,
                                   int topology, float delay_penalty);
hipError_t launch_pruned_hat_logits_backward(hipStream_t stream, int dtype, const void* logits, const int* labels,
                                             const int* starts, const int* xn, const int* yn, const float* g2_diagonal,
                                             const float* scale, void* dlogits, int N, int T, int U, int S, int V,
                                             int blank, int topology);

}  // namespace rnnt
