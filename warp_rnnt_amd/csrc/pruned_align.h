// Launch interface of the best-path kernels on the pruned band (pruned_align.hip) for the C ABI of
// include/warp_rnnt_amd_pruned_align.h, which has the definition; DESIGN.md 3.24.
#pragma once
#include <hip/hip_runtime.h>

namespace rnnt {

constexpr int PA_MAX_S = 64;             // a band position per lane of one wave
constexpr int PA_CHUNK = 64;             // frames whose pairs and starts are staged on chip ahead of the sweep
constexpr int PA_IN_LOGITS = 0, PA_IN_HAT_LOGITS = 1, PA_IN_PAIRS = 2;

// decision words per utterance: one per frame; the modified topology has the end cell's frame T_n as well
__host__ __device__ inline size_t pruned_align_words(int T, int topology) { return (size_t)T + (topology == 1 ? 1 : 0); }

// The band-compact pairs (N,T,S,2) fp32 of `input` -- band logits (N,T,S,V) of RNNT_DTYPE_* read as launch_pruned_pairs
// (PA_IN_LOGITS) or launch_pruned_hat_pairs (PA_IN_HAT_LOGITS) reads them, or ready-made fp32 pairs (PA_IN_PAIRS) -- every
// row written: (-inf, -inf) where the row's cell is not in the band, -inf in the label channel from column U_n on, the
// delay penalty in the label channel.
hipError_t launch_band_pairs(hipStream_t stream, int kind, int dtype, const void* input, const int* labels,
                             const int* starts, const int* xn, const int* yn, float* pairs, int N, int T, int U, int S, int V,
                             int blank, float delay_penalty);

// The frame-synchronous max-plus sweep over those pairs and the walk back, one wave per utterance: words (N, T or T+1)
// decision words, scores (N,), emit_frames (N,U-1) with the -1 tails.
hipError_t launch_band_sweep(hipStream_t stream, const float* pairs, const int* starts, const int* xn, const int* yn,
                             unsigned long long* words, float* scores, int* emit_frames, int N, int T, int U, int S,
                             int topology);

}  // namespace rnnt
