// Launch interface of the band selection of the pruned recipe (prune_ranges.hip) for the C ABI of
// include/warp_rnnt_amd_prune_ranges.h: from the first pass's gradient pairs to the (N,T) band starts, two launches.
#pragma once
#include <hip/hip_runtime.h>

namespace rnnt {

// A frame's occupancies are staged whole in LDS, a workgroup holds up to four frames: 4 * U floats within 64 KiB.
constexpr int PRUNE_RANGES_MAX_U = 4096;

// Per utterance n, g = pairs + n * pitch (float2 cells; rows of U cells, T of them), occ[t,u] = -(g[t,u].x + g[t,u].y),
// hi = clamp(yn[n] + 1 - S, 0, U - S) (64-bit):
//   raw[t] = hi for t >= xn[n] - 1 (the row is not read), else the lowest u0 in [0,hi] with the largest
//   w(t,u0) = (..((occ[t,u0] + occ[t,u0+1]) + occ[t,u0+2]) + ..) + occ[t,u0+S-1] -- left to right from u0, every sum
//   rounded on its own: a function of (S, u0) and the S values alone; hi where an occ[t,u], u < hi + S, is a NaN (or
//   where no window compares: every sum a NaN).  Cells u >= hi + S are not read.
//   Then, from the last frame backwards, m[t] = min(raw[t], m[t+1]) and start[t] = max(m[t], start[t+1] - (S-1)), the
//   second as t (S-1) + max_{t' >= t} (m[t'] - t' (S-1)); the starts overwrite raw in `starts`.
// hipErrorInvalidValue unless N >= 0, T >= 1, 2 <= S <= U <= PRUNE_RANGES_MAX_U, pitch >= T U, T U < 2^29 (the ramp
// t (S-1) stays in 32 bits) and N T < 2^31.  N == 0 launches nothing.  No atomics, no workspace, no memset.
hipError_t launch_prune_ranges(hipStream_t stream, const float* pairs, long long pitch, const int* xn, const int* yn,
                               int* starts, int N, int T, int U, int S);

}  // namespace rnnt
