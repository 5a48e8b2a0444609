// Launch interface of the pruned joiner's hidden activations (pruned_hidden.hip) for the C ABI of
// include/warp_rnnt_amd_pruned_hidden.h: h = act(f + g on the band), and its backward to f and g.
#pragma once
#include <hip/hip_runtime.h>

namespace rnnt {

constexpr int PRUNED_HIDDEN_MIN_H = 8;       // a row is whole 16-byte chunks in every dtype: H % 8 == 0
constexpr int PRUNED_HIDDEN_MAX_H = 4096;    // a frame's lanes hold its f row in registers: 256 lanes x 4 chunks of fp32

// The shapes the launchers take (the header's list without the (N,T,U) sizes of the loss entries)
inline bool pruned_hidden_shape_ok(int N, int T, int U, int S, int H) {
    if (N < 0 || T < 1 || U < 1 || S < 1 || H < PRUNED_HIDDEN_MIN_H || H > PRUNED_HIDDEN_MAX_H || H % 8) return false;
    const long long rows = (long long)N * T * S;
    return rows < 1ll << 32 && rows * H < 1ll << 40 && (long long)N * U * H < 1ll << 40;
}

// One (lo, hi) pair of int32 per (n,u): the frames the dg kernel walks
inline size_t pruned_hidden_table_ints(int N, int U) { return (size_t)N * U * 2; }

// h (N,T,S,H) of the dtype from f (N,T,H), g (N,U,H), starts (N,T), xn (N,) or nullptr.  One launch.
// hipErrorInvalidValue for a shape pruned_hidden_shape_ok refuses or an unknown dtype / activation; N == 0 launches nothing.
hipError_t launch_pruned_hidden_fwd(hipStream_t stream, int dtype, int activation, const void* f, const void* g,
                                    const int* starts, const int* xn, void* h, int N, int T, int U, int S, int H);

// df (N,T,H) and / or dg (N,U,H) from dh and h; either may be nullptr.  df: one launch.  dg: the table kernel into
// `table` (pruned_hidden_table_ints(N,U) ints), then the label-major kernel.
hipError_t launch_pruned_hidden_bwd(hipStream_t stream, int dtype, int activation, const void* dh, const void* h,
                                    const int* starts, const int* xn, int* table, void* df, void* dg, int N, int T, int U,
                                    int S, int H);

}  // namespace rnnt
