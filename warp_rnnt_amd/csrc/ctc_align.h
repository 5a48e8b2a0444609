// Launch interface of the CTC best-path alignment (ctc_align.hip) for the C ABI of include/warp_rnnt_amd_ctc_align.h.
#pragma once
#include <hip/hip_runtime.h>

#include "ctc.h"

namespace rnnt {

constexpr int CTC_ALIGN_LANES = 64;              // one wave per utterance
constexpr int CTC_ALIGN_MAX_K = 16;              // label positions per lane: 64 * 16 >= CTC_MAX_L + 1
constexpr int CTC_ALIGN_BLOCK_BYTES = 32768;     // decision words the trace stages in LDS: 128 frames of 32-bit words, 64 of 64-bit

// Label positions per lane as the kernels are instantiated: 1, 2, 4, 8 or 16
inline int ctc_align_k(int L) {
    const int need = (L + 1 + CTC_ALIGN_LANES - 1) / CTC_ALIGN_LANES;
    int k = 1;
    while (k < need) k *= 2;
    return k;
}
// Bytes of a decision word: 4 K bits per lane and frame
inline size_t ctc_align_word_bytes(int L) { return ctc_align_k(L) > 8 ? 8 : 4; }
// The decisions of a call: one word per (n, t, lane)
inline size_t ctc_align_decision_bytes(int N, int T, int L) {
    return (size_t)N * T * CTC_ALIGN_LANES * ctc_align_word_bytes(L);
}

// The emission plane E (N,T,L+1) from log-probs (N,T,V) of the dtype, taken as they are: the L_n + 1 columns of the rows
// t < T_n, nothing else
hipError_t launch_ctc_align_gather(hipStream_t stream, int dtype, const void* log_probs, const int* labels, const int* xn,
                                   const int* yn, float* E, int N, int T, int L, int V, int blank);

// The max-plus sweep and the walk back on E: scores (N,), frame_tokens (N,T), emit_frames (N,L); decisions: the words above
hipError_t launch_ctc_align_sweep(hipStream_t stream, const float* E, const int* labels, const int* xn, const int* yn,
                                  void* decisions, float* scores, int* frame_tokens, int* emit_frames, int N, int T, int L,
                                  int V, int blank);

}  // namespace rnnt
