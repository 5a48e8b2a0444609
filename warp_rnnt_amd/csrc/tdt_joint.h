// Launch interface of the joint network fused into the token-and-duration (TDT) loss (tdt_joint.hip) for the C ABI of
// include/warp_rnnt_amd_tdt_joint.h.  The sweeps and the gradient kernel behind the producer are tdt.h's, unchanged.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rnnt {

// f (N,T,H), g (N,U,H) and w (V+D,H) of `dtype` (RNNT_DTYPE_*; hipErrorInvalidValue for another), bias (V+D,) fp32 or
// nullptr; rows [0,V) of w are tokens, row V+i is durations[i].  Writes the plane of tdt.h -- 2 + D channels of every cell
// of the grid, zeros outside the utterances' windows -- and, stats != nullptr, four floats per cell in (N,T,U) order:
// (max, log sum) of the token logits and (max, log sum) of the duration logits.  p > 0: dropout between activation and
// projection with the mask of philox.h under the device word *seed; p == 0: the kernels without (seed unread).
hipError_t launch_tdt_joint_fwd(hipStream_t stream, int dtype, int act, const void* f, const void* g, const void* w,
                                const float* bias, const int* labels, const int* xn, const int* yn, float* plane,
                                float* stats, int N, int T, int U, int H, int V, int D, int blank, float sigma, float p,
                                const uint64_t* seed);
// gplane: the 2 + D channels k_tdt_grads wrote; wt: (H, joint_vpad(V+D)) elements of dtype; dw_part / db_part:
// (splits - 1) x joint_vpad(V+D) x H and splits x joint_vpad(V+D) fp32, splits = joint_w_splits(N,T,U,H,V+D,dtype): split 0
// of d weight goes straight into dweight.  wt and dw_part may be the same storage (wt is read before dw_part is written).
// df, dg in dtype, dweight (V+D,H) and dbias (V+D,) fp32; each may be nullptr.
hipError_t launch_tdt_joint_bwd(hipStream_t stream, int dtype, int act, const void* f, const void* g, const void* w,
                                const float* bias, const int* labels, const int* xn, const int* yn, const float* stats,
                                const float* gplane, const float* grad_costs, void* wt, float* dw_part, float* db_part,
                                int splits, void* df, void* dg, float* dweight, float* dbias, int N, int T, int U, int H,
                                int V, int D, int blank, float p, const uint64_t* seed);

}  // namespace rnnt
