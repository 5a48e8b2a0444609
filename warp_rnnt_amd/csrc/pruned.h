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
//
// topology (include/warp_rnnt_amd_topology.h): TOPO_REGULAR is the above.  TOPO_MODIFIED -- a label consumes
// a frame -- is the regular lattice over the sheared cells (t' = t - u, u), whose diagonals are the frames: the plane is
// (N,T+1,U,2) and frame-major, cell (t,u) at ((n (T+1) + t) U + u); the sweeps run on it with xs[n] = T_n - U_n + 1 frames
// (launch_modified_terminal).  Only rows with t < xn[n], t >= u, u <= yn[n] are written (pairs) or get a gradient
// (backward: every other row is exactly zero): row (T_n, U_n) of a padding frame has the terminal cell's address.  xn, yn:
// needed by TOPO_MODIFIED and by a delay_penalty != 0, else unread.
// delay_penalty dp: the label channel of a row of frame t holds lp[label] + dp * (0.5f * (float)(T_n - 1) - (float)t); the
// backward is the same for every dp.  TOPO_REGULAR with dp == 0 launches the kernels that read no length.
constexpr int TOPO_REGULAR = 0, TOPO_MODIFIED = 1;
hipError_t launch_pruned_pairs(hipStream_t stream, int dtype, const void* logits, const int* labels, const int* starts,
                               const int* xn, const int* yn, float* ws2, int N, int T, int U, int S, int V, int blank,
                               int topology, float delay_penalty);
hipError_t launch_pruned_logits_backward(hipStream_t stream, int dtype, const void* logits, const int* labels,
                                         const int* starts, const int* xn, const int* yn, const float* g2_diagonal,
                                         const float* scale, void* dlogits, int N, int T, int U, int S, int V, int blank,
                                         int topology);

// PRUNED_FLOOR into both channels of `cells` cells of a pair plane (the simple loss's modified plane)
hipError_t launch_pruned_floor(hipStream_t stream, float* ws2, size_t cells);
// One launch, a thread per utterance, between a TOPO_MODIFIED producer and the sweeps: xs[n] = T_n - U_n + 1 (1 where
// T_n < U_n: no path; 0 for lengths the sweeps refuse) and the virtual terminal cell (row T_n, column U_n) = (0, floor).
hipError_t launch_modified_terminal(hipStream_t stream, const int* xn, const int* yn, int* xs, float* ws2, int N, int T,
                                    int U);
// ... and behind the gradient kernel: the terminal cell's gradient pair (-1, 0) set to (0, 0), for a reader of the
// frame-major pairs that masks nothing (the simple loss's backward, prune_ranges)
hipError_t launch_modified_clear_terminal(hipStream_t stream, const int* xn, const int* yn, float* g2, int N, int T, int U);

}  // namespace rnnt
