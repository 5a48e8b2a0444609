// Launch interface of the pruned transducer kernels (pruned.hip) for the C ABI of include/warp_rnnt_amd_pruned.h.
#pragma once
#include <hip/hip_runtime.h>

namespace rnnt {

// What a cell of the (N,T,U) grid that no row of the band maps to holds, in both channels: a finite floor, not -inf -- the
// interior of the sweeps computes lse(-inf,-inf) = NaN on purpose (lattice_step.h).  lse(x, y) with y <= F and x an
// ordinary log-probability is x bit for bit, and exp(alpha + lp + beta - b00) of anything that passed through a floor is +0.
constexpr float PRUNED_FLOOR = -1e30f;

// The pruned transducer loss (Kuang et al. 2022): logits (N,T,S,V) of RNNT_DTYPE_* (hipErrorInvalidValue for another
// dtype), row (n,t,s) is lattice cell (t, u = starts[n*T + t] + s) of utterance n; fp32 arithmetic from the load on.
//   pairs: the whole diagonal-major pair plane ws2 (N,T,U,2) -- PRUNED_FLOOR in both channels, then
//   make_float2(lp[blank], lp[label]) of every row whose u lies in [0,U) at map_cell's address of (n,t,u), with the "label
//   = blank in the last column" convention of launch_log_softmax_gather_skewed.  A row whose u lies outside [0,U) produces
//   nothing and touches nothing: `starts` is device data.
//   backward: d/d logits (N,T,S,V) in the logits' type from the gradient pairs at the same addresses, scaled by scale[n]
//   (nullptr: 1); every element written; exactly zero rows where u lies outside [0,U), where scale[n] == 0 (whatever the
//   pairs hold) and where the pair is (0,0).
hipError_t launch_pruned_pairs(hipStream_t stream, int dtype, const void* logits, const int* labels, const int* starts,
                               float* ws2, int N, int T, int U, int S, int V, int blank);
hipError_t launch_pruned_logits_backward(hipStream_t stream, int dtype, const void* logits, const int* labels,
                                         const int* starts, const float* g2_diagonal, const float* scale, void* dlogits,
                                         int N, int T, int U, int S, int V, int blank);

}  // namespace rnnt
