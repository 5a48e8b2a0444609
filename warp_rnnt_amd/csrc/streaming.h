// What the streaming kernel families share -- the forward log-softmax (lsm.h), its backward (lsm_backward.hip), the dense
// to-diagonal kernels (to_diagonal.hip) and the compact-layout helpers (compact.hip): wave and block reductions, the
// 16-byte load and store with their cache policy, the dense cell -> workspace map and a few constants.
#pragma once
#include "common.h"
#include "kernels.h"

namespace rnnt {

// ---------------------------------------------------------------------------
// wave / block reductions
// ---------------------------------------------------------------------------
template <int WIDTH>
__device__ __forceinline__ float group_max(float v) {
#pragma unroll
    for (int o = WIDTH / 2; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, WAVE));
    return v;
}
template <int WIDTH>
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
    for (int o = WIDTH / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, WAVE);
    return v;
}

template <int THREADS>
__device__ __forceinline__ float block_reduce(float v, bool is_max, float* red) {
    v = is_max ? group_max<WAVE>(v) : group_sum<WAVE>(v);
    const int w = threadIdx.x >> 6;
    __syncthreads();                      // protect `red` from the previous use
    if ((threadIdx.x & 63) == 0) red[w] = v;
    __syncthreads();
    float r = red[0];
#pragma unroll
    for (int i = 1; i < THREADS / WAVE; ++i) r = is_max ? fmaxf(r, red[i]) : r + red[i];
    return r;
}

// Where the (blank,label) pair of flat cell index `cell` (row-major over N,T,U) lives in the
// diagonal-major workspace, and which label the cell uses.
struct CellMap {
    size_t sk;   // float2 index into the workspace
    int label;   // vocabulary index of the label channel (blank for the last column)
    int n;       // utterance
};
__device__ __forceinline__ CellMap map_cell(size_t cell, const int* __restrict__ labels, int T, int U,
                                            int V, int blank) {
    // N*T*U < 2^32 is checked by the C ABI, so 32-bit divisions are enough
    const unsigned c32 = (unsigned)cell;
    const unsigned frame = c32 / (unsigned)U;         // n*T + t
    const int u = (int)(c32 - frame * (unsigned)U);
    const unsigned n = frame / (unsigned)T;
    const int t = (int)(frame - n * (unsigned)T);
    int r = t + u;
    r = r >= T ? r % T : r;
    CellMap m;
    m.sk = ((size_t)n * T + r) * (size_t)U + u;
    m.label = (u < U - 1) ? safe_label(labels[(size_t)n * (U - 1) + u], V, blank) : blank;
    m.n = (int)n;
    return m;
}

// One float4 from / to global memory, non-temporal (NT) or plain; which stream takes which is measured at its kernels.
typedef float rnnt_f4 __attribute__((ext_vector_type(4)));
template <bool NT> __device__ __forceinline__ float4 rnnt_load4(const float4* p) {
    if constexpr (NT) {
        const rnnt_f4 v = __builtin_nontemporal_load(reinterpret_cast<const rnnt_f4*>(p));
        return make_float4(v.x, v.y, v.z, v.w);
    } else {
        return *p;
    }
}
template <bool NT> __device__ __forceinline__ void rnnt_store4(float4* p, float4 v) {
    if constexpr (NT) {
        const rnnt_f4 w = {v.x, v.y, v.z, v.w};
        __builtin_nontemporal_store(w, reinterpret_cast<rnnt_f4*>(p));
    } else {
        *p = v;
    }
}

constexpr float LOG2E = 1.44269504088896340736f;
constexpr float LN2 = 0.693147180559945309417f;
constexpr int TD = 32;   // tile edge of the to-diagonal kernels, dense and compact

}  // namespace rnnt
