// Launch interface of the "simple" transducer loss kernels (simple.hip) for the C ABI of include/warp_rnnt_amd_simple.h:
// the smoothed first pass of the pruned recipe over the trivial joiner am[n,t,:] + lm[n,u,:].
#pragma once
#include <hip/hip_runtime.h>

namespace rnnt {

// Row statistics and row sums the launches below hand to each other, all fp32, sized by simple_layout (api_fused.hip):
//   sa (N*T) float4: (ma = max_v am[t,v],  ZA = log sum_v exp(am[t,v] + q[v]) or 0 without q,  am[t,blank],  0)
//   sl (N*U) float4: (ml = max_v lm[u,v],  ZL = log sum_v exp(lm[u,v]),  lm[u,blank],  lm[u,sym(u,1)])
//   ra (N*T) float2: (sum_u S(t,u),  sum_u G(t,u,0))                          -- the backward only
//   rl (N*U) float4: (sum_t S(t,u),  sum_t G(t,u,0),  sum_t G(t,u,1),  0)      -- the backward's d q only (the d lm kernel
//                    forms these sums of its own columns on the way)
struct SimpleStats {
    float* sa;
    float* sl;
    float* ra;
    float* rl;
};

// Tiles of 64 rows are numbered in a grid dimension of at most 65535: T and U up to this
constexpr int SIMPLE_MAX_ROWS = 65535 * 64;

// The scales of the smoothed loss: c0 = 1 - c1 - c2 (not below 0), c1 = lm_only_scale, c2 = am_only_scale.
struct SimpleScales {
    float c0, c1, c2;
};
inline SimpleScales simple_scales(float lm_only_scale, float am_only_scale) {
    const float c0 = (1.0f - lm_only_scale) - am_only_scale;
    return SimpleScales{c0 > 0.0f ? c0 : 0.0f, lm_only_scale, am_only_scale};
}

// am (N,T,V), lm (N,U,V) of RNNT_DTYPE_* (hipErrorInvalidValue for another dtype), finite; q (V,) fp32 or nullptr (then
// c2 must be 0); fp32 arithmetic from the load on.
//   pairs: the statistics sa and sl, then one MFMA tile kernel over (64 t, 64 u) tiles of every utterance with K = V.  It
//   writes make_float2(pair(t,u,0), pair(t,u,1)) of EVERY cell of the (N,T,U) grid -- the cells outside an utterance's
//   (T_n, U_n + 1) window too: they are computed from the padding rows of am and lm, which are finite like the others --
//   at map_cell's address of the diagonal-major pair plane ws2, and, where znorm is given, znorm[n,t,u] =
//   log(max(sum_v exp(am[t,v] - ma) exp(lm[u,v] - ml), FLT_MIN)) = Z(t,u) - ma(t) - ml(u) of every cell, row-major.
//   topology, delay_penalty (pruned.h: TOPO_*; include/warp_rnnt_amd_topology.h): TOPO_MODIFIED fills the frame-major plane
//   ws2 (N,T+1,U,2) with the floor and writes the pairs of the cells with t < xn[n], t >= u, u <= yn[n] at
//   ((n (T+1) + t) U + u); znorm as above.  delay_penalty dp adds dp * (0.5f * (float)(T_n - 1) - (float)t) to the label
//   channel.  xn, yn: needed by TOPO_MODIFIED and by dp != 0, else unread; TOPO_REGULAR with dp == 0 is the kernel above.
hipError_t launch_simple_pairs(hipStream_t stream, int dtype, const void* am, const void* lm, const float* q,
                               const int* labels, const int* xn, const int* yn, const SimpleStats& st, float* ws2,
                               float* znorm, int N, int T, int U, int V, int blank, SimpleScales c, int topology,
                               float delay_penalty);

//   backward: from the row-major gradient pairs g2 (N,T,U,2) (zero outside the window, as k_grads writes them), znorm and
//   scale[n] (nullptr: 1): the statistics again, the row sums ra and rl, then the two MFMA tile kernels -- d am over
//   (64 t, 64 v) tiles with K = U, d lm over (64 u, 64 v) tiles with K = T -- and, with c2 != 0 and dq given, the (N,V)
//   partial vectors of d q.  Every element of d am and d lm is written, in the inputs' type, rounded once; rows t >= T_n,
//   rows u > U_n and the rows of an utterance with scale[n] == 0 are exactly zero.  No atomics: the same bits every run.
//   g2_frames: the frames per utterance of g2, its row pitch: T, or T + 1 for the frame-major pairs of the modified
//   topology (frames t < T are read; the kernels are blind to the topology given pairs by frame, zero outside the window).
hipError_t launch_simple_backward(hipStream_t stream, int dtype, const void* am, const void* lm, const float* q,
                                  const int* labels, const int* xn, const int* yn, const float* g2, const float* znorm,
                                  const float* scale, const SimpleStats& st, void* dam, void* dlm, float* dq, int N, int T,
                                  int U, int V, int blank, SimpleScales c, int g2_frames);

}  // namespace rnnt
