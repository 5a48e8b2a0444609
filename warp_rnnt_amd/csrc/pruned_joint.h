// Launch interface of the joint network fused into the pruned transducer loss (pruned_joint.hip) for the C ABI of
// include/warp_rnnt_amd_pruned_joint.h.  The floor fill in front of the producer is pruned.h's, the sweeps and the gradient
// kernel behind it are the standard ones, unchanged.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

namespace rnnt {

// W^T of the backward is (H, Vp), Vp = V rounded up to the 64 columns of a V chunk, zero-padded; the partials have Vp rows
int pruned_joint_vpad(int V);
// Splits of the weight kernel over row chunks: a function of the shape and the dtype alone
int pruned_joint_w_splits(int dtype, int N, int T, int S, int H, int V);

// f (N,T,H), g (N,U,H) and w (V,H) of `dtype` (RNNT_DTYPE_*; hipErrorInvalidValue for another), bias (V,) fp32 or nullptr,
// starts (N,T).  Row (n,t,s) is cell (t, u = starts[n,t] + s); it is live when the utterance's lengths are in range,
// t < T_n and 0 <= u <= U_n.  Writes make_float2(lp[blank], lp[label]) of every live row at pruned.hip's cell address of
// the diagonal-major plane `pairs` (which the caller has filled with the floor) and, stats != nullptr, (max, log sum) of
// the row's logits at row (n,t,s) of stats (N,T,S,2).  Dead rows touch nothing.
hipError_t launch_pruned_joint_fwd(hipStream_t stream, int dtype, int act, const void* f, const void* g, const void* w,
                                   const float* bias, const int* labels, const int* starts, const int* xn, const int* yn,
                                   float* pairs, float* stats, int N, int T, int U, int S, int H, int V, int blank);
// grads: the diagonal-major gradient pairs; dpre: (N,T,S,H) elements of dtype; wt: (H, Vp) elements of dtype; dw_part /
// db_part: splits x Vp x H and splits x Vp fp32.  df, dg in dtype, dweight (V,H) and dbias (V,) fp32; each may be nullptr.
hipError_t launch_pruned_joint_bwd(hipStream_t stream, int dtype, int act, const void* f, const void* g, const void* w,
                                   const float* bias, const int* labels, const int* starts, const int* xn, const int* yn,
                                   const float* stats, const float* grads, const float* grad_costs, void* dpre, void* wt,
                                   float* dw_part, float* db_part, void* df, void* dg, float* dweight, float* dbias, int N,
                                   int T, int U, int S, int H, int V, int blank);

}  // namespace rnnt
