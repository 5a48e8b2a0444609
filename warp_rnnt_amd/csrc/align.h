// Launch interface of the best-path (Viterbi) kernels (align.hip) for the C ABI of include/warp_rnnt_amd_align.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

namespace rnnt {

// The decision words of one call: per utterance (T+U-1) diagonals x align_blocks(U) 64-bit words, W[n][d][u/64], bit
// u mod 64 = by_label at cell (d-u, u).
__host__ __device__ inline int align_blocks(int U) { return (U + 63) / 64; }
inline size_t align_word_count(int N, int T, int U) { return (size_t)N * ((size_t)T + U - 1) * (size_t)align_blocks(U); }
// What the sweep parks between column stripes (lattices of more than 1024 columns): per utterance two columns -- one read,
// one written -- of one float per diagonal, rounded up to whole chunks of 64 diagonals.
__host__ __device__ inline size_t align_park_pitch(int T, int U) { return ((size_t)T + U + 63) / 64 * 64; }
inline size_t align_park_count(int N, int T, int U) { return (size_t)N * 2 * align_park_pitch(T, U); }

// pairs: the diagonal-major (blank, label) plane of a loss call, every cell written.  The sweep writes the decision words
// of every valid utterance (diagonals 1 .. T_n-1+U_n, the column blocks that hold a column <= U_n) and its score; an
// utterance whose lengths are outside [1,T] x [0,U-1] is left to the trace.
hipError_t launch_align_sweep(hipStream_t stream, const float* pairs, const int* xn, const int* yn,
                              unsigned long long* words, float* park, float* scores, int N, int T, int U);
// Reads the path back from the words: emit_frames (N,U-1), -1 behind U_n; a refused utterance gets a NaN score and a row
// of -1.  emit_frames may be null when U == 1.
hipError_t launch_align_trace(hipStream_t stream, const unsigned long long* words, const int* xn, const int* yn,
                              float* scores, int* emit_frames, int N, int T, int U);

}  // namespace rnnt
