// Rows of logits held by a group of lanes, in chunks of 8 elements: what the streaming kernels of hat.hip and tdt.hip both
// stand on.  A form that only one unit uses (HAT's register form) stays in that unit.
//   device: the load and the store of a chunk at every storage type and access width, and the running (max, log-sum)
//           pass over the first `end` elements of a row of pitch W;
//   host:   the choice of the access width (row_access), of the lanes per row and the workgroups (row_group, row_grid),
//           the dispatch of a launch over (lanes per row, access) (row_dispatch) and over the storage type (row_typed).
//
// The row is cut into chunks of 8 elements, chunk c is held by lane c mod G of the row's group, and that does not depend
// on the access: a chunk is one 16-byte access (two for fp32) where the row pitch W * sizeof(E) and the tensors'
// addresses are multiples of 16; otherwise accesses of 8, 4 or 2 bytes, the widest that pitch and addresses allow
// (W = 50 in fp32: 8 bytes).  bf16 / fp16 elements become floats at the load, so a half-precision row gives the bits of
// its fp32 upcast.
#pragma once
#include <type_traits>

#include "streaming.h"
#include "../../include/warp_rnnt_amd.h"

// Every product and sum below is rounded on its own: no fused multiply-add is formed (hat.hip has the reasons).  The
// pragma stands here, in front of the first function, because the including units' own one sits behind their includes
// and does not reach a function defined in this header -- row_stats' `s * exp(..)` and the `s += ..` behind it would be
// contracted, and the bits would move.  It stays in force to the end of the translation unit, the includer's code included.
#pragma clang fp contract(off)

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

// (max, log sum) of the elements [0, end) of the row at xr, whose pitch is W >= end, over the lanes of its group: lane
// `lane` of G runs over its chunks in ascending order with a running maximum and sum; an element with masked(idx), one
// past W and a logit of -inf enter the maximum as -inf and the sum as +0
template <typename E, int G, int ACC, bool NT, typename Masked>
__device__ __forceinline__ void row_stats(const E* __restrict__ xr, int lane, int end, int W, Masked masked, float& m,
                                          float& ls) {
    float ml = ROW_NEG_INF, s = 0.0f;
    for (int e0 = lane * ROW_CHUNK; e0 < end; e0 += G * ROW_CHUNK) {
        float z[ROW_CHUNK];
        row_load8<E, ACC, NT>(xr, e0, W, z);
        float mn = ml;
#pragma unroll
        for (int i = 0; i < ROW_CHUNK; ++i) {
            if (masked(e0 + i)) z[i] = ROW_NEG_INF;
            mn = fmaxf(mn, z[i]);
        }
        if (mn > ROW_NEG_INF) {               // (a lane that has seen nothing but -inf keeps s = 0)
            s = s * row_exp(ml - mn);         // exp(0) = 1 exactly where the maximum stays; 0 * exp(-inf) = 0 at the start
#pragma unroll
            for (int i = 0; i < ROW_CHUNK; ++i) s += row_exp(z[i] - mn);
            ml = mn;
        }
    }
    m = group_max<G>(ml);
    ls = logf(group_sum<G>(s * row_exp(ml - m)));
}

// ---------------------------------------------------------------------------------------------------------
// The launch side
// ---------------------------------------------------------------------------------------------------------
constexpr int ROW_THREADS = 256;         // a workgroup: ROW_THREADS / G rows

// Lanes per row, a function of the row's length alone: the smallest group with W <= 16 G, a wave beyond
inline int row_group(int W) { return W <= 16 * 16 ? 16 : W <= 16 * 32 ? 32 : 64; }
inline unsigned row_grid(size_t rows, int G) {
    const size_t per = ROW_THREADS / G;
    return (unsigned)((rows + per - 1) / per);             // rows < 2^32 (the C ABI's dims_ok): at most 2^28 workgroups
}

// The widest access of row_load8 / row_store8 that the row pitch and the addresses allow
template <typename E> inline int row_access(int W, const void* a, const void* b) {
    const uintptr_t bits = (uintptr_t)W * sizeof(E) | reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | 16;
    return (int)(bits & (~bits + 1));          // lowest set bit: 16, 8, 4 or 2 (1 is not a tensor of E)
}

// launch(G, ACC) with the call's lanes per row and access as compile-time constants (std::integral_constant); an access
// that E does not have (2 bytes in fp32; anything else) is hipErrorInvalidValue
template <typename E, typename Launch> hipError_t row_dispatch(int G, int acc, Launch launch) {
    const auto groups = [&](auto ACC) {
        switch (G) {
            case 16: launch(std::integral_constant<int, 16>{}, ACC); break;
            case 32: launch(std::integral_constant<int, 32>{}, ACC); break;
            default: launch(std::integral_constant<int, 64>{}, ACC); break;
        }
    };
    switch (acc) {
        case 16: groups(std::integral_constant<int, 16>{}); break;
        case 8: groups(std::integral_constant<int, 8>{}); break;
        case 4: groups(std::integral_constant<int, 4>{}); break;
        case 2:
            if constexpr (sizeof(E) == 2) {
                groups(std::integral_constant<int, 2>{});
                break;
            }
            return hipErrorInvalidValue;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// call(in, out) with the two pointers as const E* and E*, E the storage type of `dtype`
template <typename Call> hipError_t row_typed(int dtype, const void* in, void* out, Call call) {
    switch (dtype) {
        case RNNT_DTYPE_F32: return call(static_cast<const float*>(in), static_cast<float*>(out));
        case RNNT_DTYPE_BF16: return call(static_cast<const __bf16*>(in), static_cast<__bf16*>(out));
        case RNNT_DTYPE_F16: return call(static_cast<const _Float16*>(in), static_cast<_Float16*>(out));
    }
    return hipErrorInvalidValue;
}

}  // namespace rnnt
