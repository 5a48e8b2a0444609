// The unit of work of the fused joint kernels (joint.hip, tdt_joint.hip; DESIGN.md sections 3.9 and 3.16): one wave and
// sixteen lattice cells whose activations h = act(f+g) it stages in its own slice of LDS (16 rows of H elements of E, the
// MFMA operand type).  The waves of a workgroup are independent (no barrier); they share W through the caches.  Two
// products, both on the 16x16 MFMA forms:
//   z   = W h^T                 (A = W rows, B = h rows: one 16-byte K-slice per lane and step, mma_k)
//   2nd = dz W  or  dz^T h       (the A operand is dz straight out of the first product's accumulator registers: lane l
//                                 holds rows 4(l>>4)+r of column l&15, which is one K-slot group of the next MFMA; the
//                                 B operand is gathered in the same K order, b_slot)
// For fp32 inputs the f32 MFMA (16x16x4f32, exact f32 products); bf16 / fp16 use 16x16x32 with fp32 accumulation.
// Everything here has internal linkage: each unit that includes it gets its own copy of the two small kernels at the end.
#pragma once
#include <type_traits>

#include "../../include/warp_rnnt_amd.h"
#include "common.h"
#include "kernels.h"
#include "philox.h"

namespace rnnt {

namespace {

typedef float jf4 __attribute__((ext_vector_type(4)));
template <typename E> struct JFrag;
template <> struct JFrag<float> { typedef float type __attribute__((ext_vector_type(4))); };
template <> struct JFrag<__bf16> { typedef __bf16 type __attribute__((ext_vector_type(8))); };
template <> struct JFrag<_Float16> { typedef _Float16 type __attribute__((ext_vector_type(8))); };
template <typename E> using jfrag_t = typename JFrag<E>::type;     // one lane's 16 bytes of a K-slice
template <typename E> constexpr int EPF = 16 / (int)sizeof(E);      // elements per fragment: 4 (f32) or 8 (half)
template <typename E> constexpr int KSTEP = 4 * EPF<E>;             // K per step: 16 (f32) or 32 (half)
// Rows of a second product per MFMA step: the f32 form takes one 16-row accumulator block (four MFMAs), the half forms
// two (one MFMA over 32 K slots).
template <typename E> constexpr int ZB = EPF<E> / 4;
template <typename E> constexpr int CG = 16 * ZB<E>;   // cells per group of the weight kernels: 16 (f32), 32 (half)
constexpr int JWAVES = 4;          // waves per workgroup at most (each an independent unit of work)
constexpr int LDS_PER_WG = 81920;  // two workgroups per CU at the largest rows (fp32, H = 1024: one wave each)
constexpr int WT_PITCH = 32;       // W^T of the backward is (H, Vp), Vp = V rounded up to this, zero-padded
constexpr int HC_W = 256;          // columns of dW one unit of the weight kernel accumulates (16 x 4 registers)
constexpr int FG_MAXB = 64;        // H / 16 at H = 1024

template <typename E> __device__ __forceinline__ jf4 mma_k(jfrag_t<E> a, jfrag_t<E> b, jf4 c) {
    if constexpr (std::is_same_v<E, float>) {
        c = __builtin_amdgcn_mfma_f32_16x16x4f32(a[0], b[0], c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_16x16x4f32(a[1], b[1], c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_16x16x4f32(a[2], b[2], c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_16x16x4f32(a[3], b[3], c, 0, 0, 0);
    } else if constexpr (std::is_same_v<E, __bf16>) {
        c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
    } else {
        c = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
    }
    return c;
}
// K slot of fragment element j for lane group q in a second product: element j of the A operand is register (j&3) of
// accumulator block (j>>2), i.e. row 16(j>>2) + 4q + (j&3) of the first product
__device__ __forceinline__ int b_slot(int j, int q) { return 16 * (j >> 2) + 4 * q + (j & 3); }
template <typename E> __device__ __forceinline__ jfrag_t<E> pack_acc(const jf4* z) {
    jfrag_t<E> a;
#pragma unroll
    for (int j = 0; j < EPF<E>; ++j) a[j] = (E)z[j >> 2][j & 3];
    return a;
}

template <int ACT> __device__ __forceinline__ float act_fwd(float x) {
    return ACT == RNNT_ACT_TANH ? tanhf(x) : fmaxf(x, 0.0f);
}
// derivative from the activation's OUTPUT (what autograd's tanh / relu backward use): 1 - y^2, [y > 0]
template <int ACT> __device__ __forceinline__ float act_bwd(float y) {
    return ACT == RNNT_ACT_TANH ? 1.0f - y * y : (y > 0.0f ? 1.0f : 0.0f);
}

struct JointArgs {
    const void* f;        // (N,T,H) E
    const void* g;        // (N,U,H) E
    const void* w;        // (V,H) E
    const void* wt;       // (H,Vp) E, W transposed and zero-padded (backward only)
    const float* bias;    // (V,) or nullptr
    const int* labels;    // (N,U-1)
    const int* xn;
    const int* yn;
    const float2* g2;     // diagonal-major gradient pairs (backward)
    const float* scale;   // (N,) upstream gradient or nullptr (backward)
    float2* pairs;        // diagonal-major log-prob pairs (forward)
    float2* lse;          // (N,T,U) per cell: (max of the logits, log of the sum of exp(z - max)) -- see k_joint_fwd
    int N, T, U, H, V, Vp, blank, wpg;
};

// Dropout between the activation and the projection (include/warp_rnnt_amd_joint_dropout.h): the
// staged operand becomes m * scale * act(f+g), m from philox.h.  DROP is a template parameter of the three kernels; the
// DROP = false instantiations take JointArgs and are the code without dropout.
struct JointDropArgs : JointArgs {
    const unsigned long long* seed;   // one device word, read when the kernel runs (a graph replays with its contents then)
    uint32_t thr;                     // keep iff word < thr
    float scale, keep;                // 1 / (1 - p) and 1 - p
};
template <bool DROP> using jargs_t = std::conditional_t<DROP, JointDropArgs, JointArgs>;

// o[0..3] *= scale for elements 4 k4 ... 4 k4 + 3 of cell (n,t,u); returns the four keep bits (bit j: element j)
__device__ __forceinline__ unsigned drop4(const JointDropArgs& a, unsigned long long seed, int n, int t, int u, int k4,
                                          float* o) {
    const Philox4 r = dropout_words(seed, n, t, u, k4);
    unsigned m = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        o[j] *= a.scale;
        m |= (unsigned)(r.w[j] < a.thr) << j;
    }
    return m;
}

// How k_joint_bwd_fg's act' step gets its mask.  It cannot be read off h~ == 0: a kept element may hold an exact zero
// (tanh at f + g = 0) and has derivative scale there.  The staged value carries it in the sign of zero instead: a DROPPED
// element is staged as -0.0, a kept one never is (a kept value that rounds to a zero of either sign is staged as +0.0).
// To the matrix products -0.0 is a zero like the other -- accumulators start at +0.0, and +0.0 + -0.0 = +0.0 -- so z
// and dW are what a plane of +0.0 gives, bit for bit; the act' step tests the one bit pattern.  Against a bit plane in
// LDS beside hs (16 H / 8 bytes per wave: DESIGN.md section 3.11 has the comparison, built and measured) this costs no
// LDS, no further LDS reads in the innermost loop, and four registers in a kernel that holds 256 without dropout (the
// plane's reads took it to 512 and 1 KB of scratch per lane).
template <typename E> __device__ __forceinline__ E drop_stage(float v, bool keep) {
    const E e = (E)v;
    return keep ? (e == (E)0.0f ? (E)0.0f : e) : (E)(-0.0f);
}
template <typename E> __device__ __forceinline__ bool dropped(E h) { return __float_as_uint((float)h) == 0x80000000u; }

// LDS row pitch of the staged activations: H elements + 16 bytes (the 16 rows of a fragment read then start on
// different banks)
template <typename E> __device__ __forceinline__ int hs_pitch(int H) { return H + EPF<E>; }

// Stage h = act(f[n,t(c)] + g[n,u(c)]) of the wave's 16 cells (fp32 arithmetic, rounded once to E); dead cells get zeros.
// DROP: m * scale * act(...), the product in fp32, rounded once; dropped elements as -0.0 (drop_stage).
template <typename E, int ACT, bool DROP, typename CellOf>
__device__ __forceinline__ void stage_h(const jargs_t<DROP>& a, int n, E* hs, CellOf cell_of, int Tn, int Un, int lane,
                                        unsigned long long seed = 0) {
    const E* f = static_cast<const E*>(a.f);
    const E* g = static_cast<const E*>(a.g);
    const int H = a.H, P = hs_pitch<E>(H), H4 = H >> 2;
    for (int i = lane; i < 16 * H4; i += WAVE) {
        const int c = i / H4, k = (i - c * H4) * 4;
        int t, u;
        cell_of(c, t, u);
        float o[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        [[maybe_unused]] unsigned m = 15u;   // (dead cells: plain zeros)
        if (t < Tn && u < Un) {
            const E* fp = f + ((size_t)n * a.T + t) * H + k;
            const E* gp = g + ((size_t)n * a.U + u) * H + k;
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = act_fwd<ACT>((float)fp[j] + (float)gp[j]);
            if constexpr (DROP) m = drop4(a, seed, n, t, u, k >> 2, o);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if constexpr (DROP)
                hs[c * P + k + j] = drop_stage<E>(o[j], (m >> j) & 1u);
            else
                hs[c * P + k + j] = (E)o[j];
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// One 16x16 block of z: rows v0 + 4q + r, column = cell l&15 (wt == false: A = W rows, B = h rows), or rows = cells,
// column v0 + (l&15) (swap == true: A = h rows, B = W rows).  W rows >= V read as zeros.
template <typename E, bool SWAP>
__device__ __forceinline__ jf4 z_block(const JointArgs& a, const E* hs, int hrow0, int v0, int lane) {
    const E* W = static_cast<const E*>(a.w);
    const int H = a.H, P = hs_pitch<E>(H), q = lane >> 4, r = lane & 15;
    const int v = v0 + r;
    const bool vin = v < a.V;
    const jfrag_t<E>* wrow = reinterpret_cast<const jfrag_t<E>*>(W + (size_t)(vin ? v : 0) * H) + q;
    const jfrag_t<E>* hrow = reinterpret_cast<const jfrag_t<E>*>(hs + (hrow0 + r) * P) + q;
    jf4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
    const jfrag_t<E> zero = {};
    for (int k = 0; k < H / KSTEP<E>; ++k) {
        const jfrag_t<E> wv = vin ? wrow[4 * k] : zero;
        const jfrag_t<E> hv = hrow[4 * k];
        acc = SWAP ? mma_k<E>(hv, wv, acc) : mma_k<E>(wv, hv, acc);
    }
    return acc;
}

// The softmax probability of a logit z of a cell whose forward stored (mall, log sc): exp((z - mall) - log sc).  z - mall is
// formed first and alone: mall + log sc in one float would round at ulp(mall).  z = -inf gives exactly 0.
__device__ __forceinline__ float cell_prob(float z, float mall, float logsc) { return expf((z - mall) - logsc); }

__global__ void k_joint_reduce_w(const float* __restrict__ dw_part, const float* __restrict__ db_part, int splits, int V,
                                 int Vp, int H, float* dweight, float* dbias) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long vh = (long)V * H;
    if (dweight && i < vh) {
        float x = 0.0f;
        for (int s = 0; s < splits; ++s) x += dw_part[(size_t)s * Vp * H + i];
        dweight[i] = x;
    }
    if (dbias && i < V) {
        float x = 0.0f;
        for (int s = 0; s < splits; ++s) x += db_part[(size_t)s * Vp + i];
        dbias[i] = x;
    }
}

template <typename E>
__global__ void k_joint_transpose_w(const E* __restrict__ w, E* __restrict__ wt, int V, int Vp, int H) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;   // over (H, Vp)
    if (i >= (long)H * Vp) return;
    const int k = (int)(i / Vp), v = (int)(i - (long)k * Vp);
    wt[i] = v < V ? w[(size_t)v * H + k] : (E)0.0f;
}

template <typename E> int waves_per_group(int rows, int H) {
    const int bytes = rows * (H + EPF<E>) * (int)sizeof(E);
    const int w = LDS_PER_WG / bytes;
    return w < 1 ? 1 : (w > JWAVES ? JWAVES : w);
}

inline unsigned blocks_for(long items, int wpg) { return (unsigned)((items + wpg - 1) / wpg); }

template <bool DROP> jargs_t<DROP> drop_args(const JointArgs& a, float p, const uint64_t* seed) {
    if constexpr (DROP)
        return JointDropArgs{a, reinterpret_cast<const unsigned long long*>(seed), dropout_threshold(p), dropout_scale(p),
                             (float)(1.0 - (double)p)};
    else
        return a;
}

}  // namespace

}  // namespace rnnt
