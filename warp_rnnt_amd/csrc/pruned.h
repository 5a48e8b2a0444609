// Launch interface of the pruned transducer kernels (pruned.hip) for the C ABI of include/warp_rnnt_amd_pruned.h.
#pragma once
#include <hip/hip_runtime.h>

#include "common.h"

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

// (device: shared by the row kernels of pruned.hip and pruned_hat.hip)
// Where row `row` of (N,T,S) lies in the lattice.  live: u in [0,U) -- starts is device data nobody validated, and the sum
// is formed in 64 bits so that no start wraps into the grid
//
// TOPO_MODIFIED (pruned.h): the plane has T + 1 rows per utterance and is frame-major, cell (t,u) at ((n (T+1) + t) U + u) --
// the diagonal-major address of cell (t' = t - u, u) of the sheared lattice.  live: also t < xn[n], t >= u, u <= yn[n], the
// cells a path can reach -- row (t = T_n, u = U_n) of a padding frame has the address of the virtual terminal cell.
struct BandCell {
    size_t sk;      // float2 index into the diagonal-major plane
    int label;      // vocabulary index of the label channel (the blank in the last column and for a label outside [0,V))
    int n;
    int t;
    bool live;
};
template <int TOPO>
__device__ __forceinline__ BandCell band_cell(size_t row, const int* __restrict__ labels, const int* __restrict__ starts,
                                              const int* __restrict__ xn, const int* __restrict__ yn, int T, int U, int S,
                                              int V, int blank) {
    // N*T*S < 2^32 is checked by the C ABI, so 32-bit divisions are enough
    const unsigned r32 = (unsigned)row;
    const unsigned frame = r32 / (unsigned)S;          // n*T + t
    const int s = (int)(r32 - frame * (unsigned)S);
    const unsigned n = frame / (unsigned)T;
    const int t = (int)(frame - n * (unsigned)T);
    const long long u64 = (long long)starts[frame] + s;
    BandCell c;
    c.n = (int)n;
    c.t = t;
    c.live = u64 >= 0 && u64 < (long long)U;
    c.sk = 0;
    c.label = blank;
    if constexpr (TOPO == TOPO_MODIFIED) c.live = c.live && t < xn[n] && (long long)t >= u64 && u64 <= (long long)yn[n];
    if (c.live) {
        const int u = (int)u64;
        if constexpr (TOPO == TOPO_MODIFIED) {
            c.sk = ((size_t)n * (T + 1) + t) * (size_t)U + u;
        } else {
            int r = t + u;
            r = r >= T ? r % T : r;
            c.sk = ((size_t)n * T + r) * (size_t)U + u;
        }
        if (u < U - 1) c.label = safe_label(labels[(size_t)n * (U - 1) + u], V, blank);
    }
    return c;
}

}  // namespace rnnt
