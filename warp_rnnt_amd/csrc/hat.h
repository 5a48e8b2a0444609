// Launch interface of the factorised-blank (HAT) kernels (hat.hip) for the C ABI of include/warp_rnnt_amd_hat.h, and the
// arithmetic of a HAT row, which hat.hip and pruned_hat.hip share.
#pragma once
#include <hip/hip_runtime.h>

#include "row_chunks.h"

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

// ---------------------------------------------------------------------------------------------------------
// The arithmetic of a row (device): what a kernel that maps rows to cells in its own way calls, so that a row's bits are a
// function of the row, V, the blank and the label (the backward: its pair and scale as well) in every such kernel.
// Every product and sum is rounded on its own (row_chunks.h has set that; hat.hip has the reasons).
// ---------------------------------------------------------------------------------------------------------
#pragma clang fp contract(off)

constexpr int HAT_SMALL_V = 1024;        // rows up to here are held in registers: 2 chunks per lane, 64 lanes at the most

__device__ __forceinline__ float hat_softplus(float x) { return fmaxf(x, 0.0f) + log1pf(expf(-fabsf(x))); }

// What the forward stores for a cell: lpB, and lp[label] -- lpB again where the label channel is the blank's (the last
// column; a padded label), as the standard gather does
__device__ __forceinline__ float2 hat_pair(float zb, float zl, int label, int blank, float m, float ls) {
    const float lpB = -hat_softplus(-zb);
    const float lnb = -hat_softplus(zb);
    return make_float2(lpB, label == blank ? lpB : ((zl - m) - ls) + lnb);
}

// What the backward needs of a cell behind its row statistics
struct HatCellGrad {
    float ub;      // scale * u_b
    float gL, sc;
    int label;
};
__device__ __forceinline__ HatCellGrad hat_cell_grad(float zb, float2 g, float sc, int label) {
    const float e = expf(-fabsf(zb)), den = 1.0f + e;
    const float big = 1.0f / den, small = e / den;            // sigmoid(|z_b|), sigmoid(-|z_b|)
    const float sig = zb >= 0.0f ? big : small, nsig = zb >= 0.0f ? small : big;
    return {sc * (g.x * nsig - g.y * sig), g.y, sc, label};
}
__device__ __forceinline__ float hat_dz(const HatCellGrad& c, float z, int idx, int blank, float m, float ls) {
    const float q = row_exp((z - m) - ls);                    // (z = -inf at the blank, past V and at masked logits: q = +0)
    const float u = c.gL * ((idx == c.label ? 1.0f : 0.0f) - q);
    return idx == blank ? c.ub : c.sc * u;
}

// Rows of up to 1024 elements: a group of G lanes per row, chunks `lane` and `G + lane` in 16 registers
// (a row of up to 8 G elements has no second chunk in any lane: it is neither loaded nor worked on -- what it would add,
//  -inf to the maximum and +0 to the sum, changes no bit)
template <int G> __device__ __forceinline__ int hat_small_chunks(int V) { return V > G * ROW_CHUNK ? 2 : 1; }

template <typename E, int G, int ACC>
__device__ __forceinline__ void hat_small_stats(const E* __restrict__ xr, int lane, int V, int blank, float (&z)[2][ROW_CHUNK],
                                                float& m, float& ls) {
    const int chunks = hat_small_chunks<G>(V);
    row_load8<E, ACC, true>(xr, lane * ROW_CHUNK, V, z[0]);
    if (chunks > 1) row_load8<E, ACC, true>(xr, (G + lane) * ROW_CHUNK, V, z[1]);
    m = ROW_NEG_INF;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        if (k < chunks) {
#pragma unroll
            for (int i = 0; i < ROW_CHUNK; ++i) {
                if ((k * G + lane) * ROW_CHUNK + i == blank) z[k][i] = ROW_NEG_INF;
                m = fmaxf(m, z[k][i]);
            }
        }
    }
    m = group_max<G>(m);
    float s = 0.0f;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        if (k < chunks) {
#pragma unroll
            for (int i = 0; i < ROW_CHUNK; ++i) s += row_exp(z[k][i] - m);
        }
    }
    ls = logf(group_sum<G>(s));
}

// Longer rows: a wave per row, chunks lane, 64 + lane, ...; running maximum and sum per lane in one pass
// (row_stats of row_chunks.h at G = 64 over the whole row, the blank masked)
template <typename E, int ACC, bool NT>
__device__ __forceinline__ void hat_wave_stats(const E* __restrict__ xr, int lane, int V, int blank, float& m, float& ls) {
    row_stats<E, WAVE, ACC, NT>(xr, lane, V, V, [blank](int idx) { return idx == blank; }, m, ls);
}

}  // namespace rnnt
