// Launch interface of the factorised-blank (HAT) kernels (hat.hip) for the C ABI of include/warp_rnnt_amd_hat.h.
#pragma once
#include <hip/hip_runtime.h>

namespace rnnt {

// HAT (Variani et al. 2020): the blank is a Bernoulli, sigmoid(z[blank]); the labels share 1 - sigmoid(z[blank]) through a
// softmax over the non-blank logits.  Logits (N,T,U,V) of RNNT_DTYPE_* (hipErrorInvalidValue for another dtype), fp32
// arithmetic from the load on, V >= 2.
//   gather: make_float2(lpB, lp[label]) of EVERY cell of the (N,T,U) grid at map_cell(...).sk of the diagonal-major pair
//   plane -- the address and the "label = blank in the last column" convention of launch_log_softmax_gather_skewed;
//   backward: d/d logits (N,T,U,V) in the logits' type from the gradient pairs at the same addresses, scaled by scale[n]
//   (nullptr: 1).
hipError_t launch_hat_gather_skewed(hipStream_t stream, int dtype, const void* logits, const int* labels, float* ws2,
                                    int N, int T, int U, int V, int blank);
hipError_t launch_hat_logits_backward(hipStream_t stream, int dtype, const void* logits, const int* labels,
                                      const float* g2_diagonal, const float* scale, void* dlogits, int N, int T, int U,
                                      int V, int blank);

}  // namespace rnnt
