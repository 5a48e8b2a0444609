// Rows of logits in chunks of 8 elements, for the streaming kernels that hold a row by a group of lanes (hat.hip, tdt.hip):
// the load and the store of a chunk at every storage type and access width, and the choice of that width.
//
// The row is cut into chunks of 8 elements; which lane holds which chunk is the kernel's business, and does not depend
// on the access: a chunk is one 16-byte access (two for fp32) where the row pitch W * sizeof(E) and the tensors'
// addresses are multiples of 16; otherwise accesses of 8, 4 or 2 bytes, the widest that pitch and addresses allow
// (W = 50 in fp32: 8 bytes).  bf16 / fp16 elements become floats at the load, so a half-precision row gives the bits of
// its fp32 upcast.
#pragma once
#include <type_traits>

#include "streaming.h"

namespace rnnt {

constexpr int ROW_CHUNK = 8;             // elements per chunk
constexpr float ROW_NEG_INF = -__builtin_inff();

// An access moves ACC bytes = NV elements: 16, 8, 4 (or, in half precision, 2) -- the largest power of two that divides the
// row pitch W * sizeof(E) and the tensors' addresses, so every access of a row is aligned and lies below W whole or not
// at all.  Which elements a lane holds does not depend on it.
template <typename T, int NV> struct RowVec { typedef T type __attribute__((ext_vector_type(NV))); };
template <typename T> struct RowVec<T, 1> { typedef T type; };
template <typename T, int NV> using row_vec_t = typename RowVec<T, NV>::type;

// Elements e0 .. e0+7 of the row at xr as floats; -inf at and past W
template <typename E, int ACC, bool NT>
__device__ __forceinline__ void row_load8(const E* __restrict__ xr, int e0, int W, float (&z)[ROW_CHUNK]) {
    constexpr int NV = ACC / (int)sizeof(E);
    static_assert(NV == 1 || NV == 2 || NV == 4 || NV == 8, "2 to 16 bytes, whole elements");
#pragma unroll
    for (int k = 0; k < ROW_CHUNK; k += NV) {
        if constexpr (NV == 1) {
            z[k] = e0 + k < W ? (float)xr[e0 + k] : ROW_NEG_INF;
        } else {
#pragma unroll
            for (int i = 0; i < NV; ++i) z[k + i] = ROW_NEG_INF;
            if (e0 + k < W) {
                const row_vec_t<E, NV>* p = reinterpret_cast<const row_vec_t<E, NV>*>(xr + e0 + k);
                row_vec_t<E, NV> h;
                if constexpr (NT) h = __builtin_nontemporal_load(p); else h = *p;
                const row_vec_t<float, NV> v = __builtin_convertvector(h, row_vec_t<float, NV>);
#pragma unroll
                for (int i = 0; i < NV; ++i) z[k + i] = v[i];
            }
        }
    }
}

// ... and d[0..7] to elements e0 .. e0+7 of the row at o, below W only, converted to E (round to nearest even) as stored
template <typename E, int ACC>
__device__ __forceinline__ void row_store8(E* __restrict__ o, int e0, int W, const float (&d)[ROW_CHUNK]) {
    constexpr int NV = ACC / (int)sizeof(E);
#pragma unroll
    for (int k = 0; k < ROW_CHUNK; k += NV) {
        if (e0 + k >= W) continue;
        if constexpr (NV > 1) {
            row_vec_t<float, NV> v;
#pragma unroll
            for (int i = 0; i < NV; ++i) v[i] = d[k + i];
            __builtin_nontemporal_store(__builtin_convertvector(v, row_vec_t<E, NV>),
                                        reinterpret_cast<row_vec_t<E, NV>*>(o + e0 + k));
        } else if constexpr (std::is_same_v<E, float>) {
            o[e0 + k] = d[k];
        } else {
            // (the median of d, d, d is d: an instruction between the multiply that made d and the cast.  Without it a
            //  scalar fp16 cast takes that multiply with it -- v_fma_mixlo_f16, one rounding of the exact product -- and
            //  a half result is no longer the fp32 result rounded once.  The packed conversions above take none.)
            o[e0 + k] = (E)__builtin_amdgcn_fmed3f(d[k], d[k], d[k]);
        }
    }
}

__device__ __forceinline__ float row_exp(float d) { return __builtin_amdgcn_exp2f(d * LOG2E); }   // d <= 0; exp(-inf) = +0

// The widest access of row_load8 / row_store8 that the row pitch and the addresses allow
template <typename E> inline int row_access(int W, const void* a, const void* b) {
    const uintptr_t bits = (uintptr_t)W * sizeof(E) | reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | 16;
    return (int)(bits & (~bits + 1));          // lowest set bit: 16, 8, 4 or 2 (1 is not a tensor of E)
}

}  // namespace rnnt
