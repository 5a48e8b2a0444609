// The forward log-softmax kernels over the vocabulary axis -- plain, fused with the gather of the (blank, label)
// log-prob pair per lattice cell, and fused into d/d logits -- as templates over the storage type E of the logits;
// lsm_f32.hip, lsm_bf16.hip and lsm_f16.hip instantiate them.  These are the HBM-bound part of the op (the dense
// (N,T,U,V) tensor is 25x..5000x larger than everything the lattice kernels touch).
//
// Reference counterparts:
//   log-softmax  : caller side, pytorch_binding/benchmark.py:65,70 (F.log_softmax)
//   gather       : warp_rnnt/__init__.py:118-128 (torch.full int64 index + slice-assign +
//                  torch.gather; 16 B of index per cell) and core_compact.cu:403-436
//   The fused form reads the logits once and never materialises log-probs; it writes the diagonal-major workspace (common.h).
#pragma once
#include <cstdlib>
#include <type_traits>

#include "lsm_plan.h"
#include "streaming.h"

namespace rnnt {

static_assert(LSM_WAVE == WAVE, "lsm_plan.h plans for this wave");

// The exponent of every element is exp2(fma(x, LOG2E, mb)) with mb = -mx * LOG2E ROUNDED to fp32.  That rounding, up to
// |mx| * 1.44 * 2^-24, is common to the whole row: the sum comes out as s = true sum * 2^-lo, and left in log(s) it moves
// every log-prob of the row by about |mx| * 6e-8 (2.7e-3 at mx = 60000) -- a log-softmax that is not invariant to a shift
// of its row.  lo = fma(-mx, LOG2E, -mb) is the residual of the rounded product EXACTLY, so the row's log-sum is
// log(s) + lo * ln 2: one fma per row, nothing per element.  `log_s` is log(s) however the body forms it.
// Every (mx, ls) pair a kernel hands on carries this ls.  The fused backward never forms mx + ls (rounded at ulp(mx)): it
// writes -e_j * (gs / s) with the forward's e_j = exp2(fma(x_j, LOG2E, mb)) -- the residual cancels between e_j and s.
__device__ __forceinline__ float lsm_log_sum(float log_s, float mx, float mb) {
    return __builtin_fmaf(__builtin_fmaf(-mx, LOG2E, -mb), LN2, log_s);
}

// The row -> cell map of the fused log-softmax kernels is a policy, passed by value and chosen by a template parameter.
// chunk(first, last) is called by every wave of a kernel, wave-uniformly, before at() is asked for rows in [first, last];
// pair() and scale() read the backward's gradient pair and upstream scale of a mapped row, put() stores the gather's pair.
//   DenseMap: the (N,T,U,V) tensor, map_cell -- what the dense kernels have always done.
struct DenseMap {
    static constexpr bool COMPACT = false;
    const int* labels;
    int T, U;
    __device__ __forceinline__ void chunk(int64_t, int64_t) {}
    __device__ __forceinline__ CellMap at(size_t cell, int V, int blank) const {
        return map_cell(cell, labels, T, U, V, blank);
    }
    template <class B> __device__ __forceinline__ float2 pair(const B& bw, const CellMap m) const { return bw.g2[m.sk]; }
    template <class B> __device__ __forceinline__ float scale(const B& bw, const CellMap m) const {
        return bw.scale ? bw.scale[m.n] : 1.0f;
    }
    __device__ __forceinline__ void put(float* out, const CellMap m, float2 p) const {
        reinterpret_cast<float2*>(out)[m.sk] = p;
    }
};

// The owner of packed row c -- the first n with offs[n+1] > c, N when there is none -- searched by a whole wave: its lanes
// probe 64 evenly spaced utterances at once and the first that already ends past c narrows the range 64-fold, so N <= 64
// costs one round of loads and N <= 4096 two (a binary search costs log2 N dependent loads, ~0.5 us each from L2).
// Lanes 0-31 search for `first`, lanes 32-63 for `last`, 32 probes per round each.  For offsets that are not
// non-decreasing the search still ends on one utterance of [0, N]; CompactMap::at checks the row against its range.
__device__ __forceinline__ void compact_owner_range(const int64_t* __restrict__ offs, int N, int64_t first, int64_t last,
                                                    int& n0, int& n1) {
    const int lane = threadIdx.x & (WAVE - 1), half = lane >> 5, j = lane & 31;
    const int64_t c = half ? last : first;
    int lo = 0, hi = N;                                // answer in [lo, hi]; hi = N stands for "no utterance"
    for (;;) {
        const bool more = lo < hi;
        const uint64_t act = __ballot(more);
        if (act == 0) break;
        const int step = (hi - lo + 31) >> 5;
        const int m = lo + j * step;
        const bool p = more && (m >= hi || offs[m + 1] > c);
        const uint64_t b = __ballot(p);
        const unsigned mine = (unsigned)(b >> (32 * half));   // this half's probes
        if (more) {
            if (mine) {
                const int f = __builtin_ctz(mine);
                hi = min(hi, lo + f * step);
                lo = f ? lo + (f - 1) * step + 1 : lo;
            } else {
                lo = lo + 31 * step + 1;
            }
            lo = min(lo, hi);
        }
    }
    n0 = __shfl(lo, 0, WAVE);
    n1 = __shfl(lo, 32, WAVE);
}

//   CompactMap: ragged packed rows (kernels.h: PackedRows).  The pair slot in the forward is the skewed one of the compact
//   workspace, offs[n] + ((t+u) mod T_n)*U_n + u; in the backward the row-major (STU,2) pairs are read at the row itself.
//   at() finds the owner inside the chunk's [n0, n1] only; m.n = -1 marks a row that belongs to nobody.
template <bool SKEW>
struct CompactMap {
    static constexpr bool COMPACT = true;
    PackedRows r;
    int n0, n1;
    __device__ __forceinline__ void chunk(int64_t first, int64_t last) {
        compact_owner_range(r.offs, r.N, first, last, n0, n1);
        n1 = min(n1, r.N - 1);
    }
    __device__ __forceinline__ CellMap at(size_t cell, int V, int blank) const {
        CellMap m = {0, blank, -1};
        const int64_t c = (int64_t)cell;
        int n = n0, hi = n1;
        while (n < hi) {
            const int mid = (n + hi) >> 1;
            if (r.offs[mid + 1] > c) hi = mid; else n = mid + 1;
        }
        if (n >= r.N || c >= r.rows) return m;
        const int64_t o = r.offs[n], e = r.offs[n + 1];
        const int T = r.xn[n], U = r.yn[n] + 1;
        // the owner's range must be exactly its T_n*U_n rows inside the tensor, or none of them is mapped
        if (c < o || c >= e || o < 0 || e > r.rows || T < 1 || U < 1 || e - o != (int64_t)T * U) return m;
        const unsigned local = (unsigned)(c - o);      // (< T_n*U_n < 2^32)
        const unsigned t = local / (unsigned)U;
        const int u = (int)(local - t * (unsigned)U);
        int lab = blank;
        if (u < U - 1) {
            const int64_t li = (int64_t)r.loffs[n] + u;
            const int64_t lim = r.nlab >= 0 ? r.nlab : (int64_t)r.loffs[r.N];
            if (li < 0 || li >= lim) return m;
            lab = safe_label(r.ys[li], V, blank);
        }
        if (SKEW) {
            int d = (int)t + u;
            d = d >= T ? d % T : d;
            m.sk = (size_t)o + (size_t)d * U + u;
        } else {
            m.sk = cell;
        }
        m.label = lab;
        m.n = n;
        return m;
    }
    template <class B> __device__ __forceinline__ float2 pair(const B& bw, const CellMap& m) const {
        return m.n >= 0 ? bw.g2[m.sk] : make_float2(0.0f, 0.0f);
    }
    template <class B> __device__ __forceinline__ float scale(const B& bw, const CellMap& m) const {
        return (bw.scale && m.n >= 0) ? bw.scale[m.n] : 1.0f;
    }
    __device__ __forceinline__ void put(float* out, const CellMap& m, float2 p) const {
        if (m.n >= 0) reinterpret_cast<float2*>(out)[m.sk] = p;
    }
};

// ---------------------------------------------------------------------------
// Small vocabularies (V <= 1024): a workgroup stages R whole rows in LDS with
// 16-byte coalesced loads (ds_write_b128, rows kept at their natural stride V so
// the tile is a byte copy of the global chunk), L lanes cooperate on a row, and
// results leave with ds_read_b128 + 16-byte coalesced stores (or as one float2
// per row for the fused gather).  The first version of this kernel was
// VALU-bound, not HBM-bound (rocprofv3: 871 VALU instructions per wave, i.e.
// ~70 per element: libm expf, per-element index division for padded LDS rows,
// per-lane loop control); this one spends ~12.
//   exp(x - max) is evaluated as exp2(x*log2e - max*log2e) on the hardware
//   v_exp_f32 unit, log(sum) as v_log_f32 * ln2 (sum in [1,V]); both are within
//   ~2 ulp, the result is within 4e-6 of torch.log_softmax (tests).
// ---------------------------------------------------------------------------
// Cache policy of the LDS-staged kernel's 16-byte global loads and stores: non-temporal in the fused modes (gather:
// a read-only stream of the logits; backward: logits in, d/d logits out -- fused forward 0.472 -> 0.464 ms, fused
// training step 1.00 -> 0.975 ms at c4, profiles/r03_bwd_nt_ab.txt), plain for the log-softmax itself, where the
// hints measured nothing to worse in rounds 1-2 (HISTORY.md).
// Written-through stores (sc1 / sc1 nt; round 6, after the dense gather gained from them): nothing at c4 in any mode of this
// kernel, c3's row-per-workgroup kernel 0.658 -> 0.73-0.76 ms, the register kernel 480 -> 520-580 us -- they pay only where
// every store instruction covers whole 128-byte lines (profiles/r06_lsm_store_policy.txt).
#define RNNT_LSM_NT_MODE(MODE) ((MODE) != LSM_NORM)
#define RNNT_LSM_LOAD(p) rnnt_load4<RNNT_LSM_NT_MODE(MODE)>(p)
#define RNNT_LSM_STORE(p, v) rnnt_store4<RNNT_LSM_NT_MODE(MODE)>(p, v)

// Storage type E of the logits: float, or __bf16 / _Float16 (RNNT_DTYPE_BF16 / _F16; one unit each).  Half-precision
// logits are converted to fp32 as they are loaded -- everything behind the load is the fp32 code -- and d/d logits (LSM_BWD)
// are converted back ONCE, round to nearest even (the compiler's cast: v_cvt_pk_bf16_f32 / v_cvt_f16_f32), as they are
// stored.  The kernels move rows in vectors of four elements (16 bytes of fp32, 8 of half) and every alignment predicate of
// plan_lsm (lsm_plan.h) is stated in those vectors, so a V reaches the same kernel, the same lanes per row and the same reduction
// tree at every E: the bits of a half-precision row are those of its fp32 upcast.
template <typename E> struct LsmVec { typedef E type __attribute__((ext_vector_type(4))); };
template <typename E> using lsm_vec_t = typename LsmVec<E>::type;
template <int MODE, typename E> using LsmOut = std::conditional_t<MODE == LSM_BWD, E, float>;   // what `out` holds
template <bool NT, typename E, typename I> __device__ __forceinline__ float4 lsm_ld4(const E* base, I i) {
    if constexpr (std::is_same_v<E, float>) {
        return rnnt_load4<NT>(reinterpret_cast<const float4*>(base) + i);
    } else {
        const lsm_vec_t<E>* p = reinterpret_cast<const lsm_vec_t<E>*>(base) + i;
        lsm_vec_t<E> h;
        if constexpr (NT) h = __builtin_nontemporal_load(p); else h = *p;
        const rnnt_f4 v = __builtin_convertvector(h, rnnt_f4);
        return make_float4(v.x, v.y, v.z, v.w);
    }
}
template <bool NT, typename E, typename I> __device__ __forceinline__ void lsm_st4(E* base, I i, float4 v) {
    if constexpr (std::is_same_v<E, float>) {
        rnnt_store4<NT>(reinterpret_cast<float4*>(base) + i, v);
    } else {
        const rnnt_f4 w = {v.x, v.y, v.z, v.w};
        const lsm_vec_t<E> h = __builtin_convertvector(w, lsm_vec_t<E>);
        lsm_vec_t<E>* p = reinterpret_cast<lsm_vec_t<E>*>(base) + i;
        if constexpr (NT) __builtin_nontemporal_store(h, p); else *p = h;
    }
}
template <typename E> __device__ __forceinline__ float lsm_ld1(const E* p) { return (float)*p; }
template <typename E> __device__ __forceinline__ void lsm_st1(E* p, float v) { *p = (E)v; }

struct LsmBwd {
    const float2* g2;    // diagonal-major gathered gradients (RNNT_GRADS_GATHERED_DIAGONAL)
    const float* scale;  // (N,) upstream gradient per utterance, or nullptr
    int xcd;             // row-per-workgroup kernel: 1 = every XCD streams a contiguous eighth of the rows
    // The clamped backward kernels only (CLAMP below; > 0 there): d/d logits at unit upstream are limited to [-clamp, +clamp]
    // elementwise, behind the two one-hot additions and IN FRONT of the upstream scale.  It belongs with `scale`; it sits
    // here, in what was padding, so that no other member moves and the unclamped kernels read their arguments where they did.
    float clamp;
    // LSM_NORM only: the column plane.  col_out[row] receives the float that goes into out[row*V + col] -- the blank
    // log-prob of every lattice cell, which the dense gather behind this kernel then reads as a coalesced stream instead of
    // fetching a 128-byte line of the row for it (to_diagonal.hip).  nullptr: no plane.
    float* col_out;
    int col;
};

// The gradient clamp of the fused backward (torchaudio's and warp-transducer's `clamp`):
//     u[v]  = [v==blank] gB + [v==label] gL - softmax(z)[v] (gB+gL)        (unit upstream)
//     dz[v] = s_n * min(max(u[v], -c), +c)
// CLAMP is a compile-time constant of every kernel that includes a body: false in the kernels that have always been here
// (their code is what it was), true in the k_*_clamped twins, which exist for LSM_BWD only and which a call with c > 0
// launches under the SAME plan.  The clamped bodies keep the unclamped operation order -- e_j * (gs / s), the two
// additions, then the clamp, then * s_n -- with the pair left unscaled, so at s_n = 1 and a clamp nothing reaches they give
// the unclamped bits.
__device__ __forceinline__ float lsm_clamp(float u, float c) { return __builtin_amdgcn_fmed3f(u, -c, c); }
// clamp, then scale, for a result that is stored straight from the register (LARGE, GENERIC).  The product is pinned as an
// fp32 value: with fp16 logits the store's conversion otherwise takes the multiply with it (v_fma_mixlo_f16, which measured
// as ONE rounding of the exact product to fp16 -- results off the fp32 kernel's by an fp16 ulp at ties), and a half result
// is the fp32 result rounded once.  (An empty statement: no instruction.)
__device__ __forceinline__ float lsm_clamp_scale(float u, float c, float sc) {
    float d = lsm_clamp(u, c) * sc;
    asm("" : "+v"(d));
    return d;
}
// SMALL: the one-hot additions of the unclamped kernel are LDS fix-ups by lane 0 of the row, made behind the row pass --
// behind which a clamped row is already clamped and scaled.  The clamped kernel has lane 0 form the two entries whole
// instead: it reads the blank's and the label's LOGIT out of the tile in front of the row pass, repeats the owning lane's
// exp2 and product (the same instructions on the same operands: the same bits), adds gB and gL in the order of the fix-ups
// (a label that is the blank -- the last column of a lattice -- takes both), clamps, scales, and stores the two floats over
// the row's behind the row pass.  The product is rounded on its own, as the LDS round trip of the unclamped kernel rounds it.
__device__ __forceinline__ void lsm_hot_clamped(float xb, float xl, bool same, float mb, float gq, float gB, float gL,
                                                float c, float sc, float& hb, float& hl) {
#pragma clang fp contract(off)
    const float pb = -__builtin_amdgcn_exp2f(__builtin_fmaf(xb, LOG2E, mb)) * gq;
    const float pl = -__builtin_amdgcn_exp2f(__builtin_fmaf(xl, LOG2E, mb)) * gq;
    const float ub = pb + gB;
    const float ul = (same ? ub : pl) + gL;
    hb = lsm_clamp(ub, c) * sc;
    hl = lsm_clamp(ul, c) * sc;
}

// (SM_THREADS, SM_FLOATS and the rows per tile of each mode and storage type: lsm_plan.h)
template <typename E, int MODE> constexpr int sm_floats() { return lsm_tile_floats(MODE, (int)sizeof(E)); }

// WP ("wave private", L <= 16 and one pass per tile): every wave stages, normalises and stores its own
// WAVE/L consecutive rows (a multiple of 4, so its chunk is 16-byte aligned) and the workgroup never
// synchronises -- 32 independent streams per CU instead of 8 workgroups that each wait for their slowest wave.
__device__ __forceinline__ void wave_sync_lds() {
    // LDS operations of one wave retire in order; this only stops the compiler from moving them
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <typename E, int L, int MODE, bool WP>
__global__ void __launch_bounds__(SM_THREADS)
k_lsm_small(const E* x, LsmOut<MODE, E>* out, const int* __restrict__ labels,
            int64_t rows, int V, int R, int q, int T, int U, int blank, LsmBwd bw) {
    constexpr bool CLAMP = false;
    DenseMap map{labels, T, U};
#include "lsm_body_small.h"
}
template <typename E, int L, int MODE, bool WP>
__global__ void __launch_bounds__(SM_THREADS)
k_lsm_small_compact(const E* x, LsmOut<MODE, E>* out, PackedRows cr, int64_t rows, int V, int R, int q, int blank,
                    LsmBwd bw) {
    constexpr bool CLAMP = false;
    CompactMap<MODE == LSM_GATHER> map{cr, 0, 0};
#include "lsm_body_small.h"
}
// (the clamped twins: LSM_BWD only)
template <typename E, int L, int MODE, bool WP>
__global__ void __launch_bounds__(SM_THREADS)
k_lsm_small_clamped(const E* x, LsmOut<MODE, E>* out, const int* __restrict__ labels,
                    int64_t rows, int V, int R, int q, int T, int U, int blank, LsmBwd bw) {
    static_assert(MODE == LSM_BWD, "the clamp is the backward's");
    constexpr bool CLAMP = true;
    DenseMap map{labels, T, U};
#include "lsm_body_small.h"
}
template <typename E, int L, int MODE, bool WP>
__global__ void __launch_bounds__(SM_THREADS)
k_lsm_small_compact_clamped(const E* x, LsmOut<MODE, E>* out, PackedRows cr, int64_t rows, int V, int R, int q, int blank,
                            LsmBwd bw) {
    static_assert(MODE == LSM_BWD, "the clamp is the backward's");
    constexpr bool CLAMP = true;
    CompactMap<false> map{cr, 0, 0};
#include "lsm_body_small.h"
}

// ---------------------------------------------------------------------------
// Large vocabularies (1024 < V <= 16384, V % 4 == 0): one workgroup per row,
// the row lives in registers (up to 16 float4 per lane), one HBM read and one
// HBM write per element.
// ---------------------------------------------------------------------------
// Shape of the row-per-workgroup kernel: THREADS x NV float4 must cover a row.  The registers that hold
// the row set the residency (NV=16 x 256 threads: 84 VGPRs, 5 waves/SIMD; NV=8: 8 waves/SIMD).  The launcher
// picks 1.25-2.5 float4 per thread for the plain log-softmax and the smallest cover for the read-mostly fused modes
// (plan_lsm, lsm_plan.h).
// cache policy of the plain (LSM_NORM) row-per-workgroup stream: non-temporal loads and non-temporal stores.
// Both (round 3; round 1 had tried them on the LDS-staged small-V kernel only, where they do nothing): c5 (V=10000, in
// place, 288 GB of traffic) 57.4 -> 51.3 ms per step, c3 (V=5000) 0.708 -> 0.695 ms; loads alone are WORSE (c3 0.733),
// stores alone neutral (profiles/r03_lg_nt_ab.txt).  The same policy in the fused gather / backward modes: c3 fused forward
// 0.336 -> 0.325 ms, fused training step 1.051 -> 1.018 ms (profiles/r03_lg_fused_nt_ab.txt)
template <typename E, int MODE, int LG_THREADS, int LG_MAXVEC>
__global__ void __launch_bounds__(LG_THREADS)
k_lsm_large(const E* x, LsmOut<MODE, E>* out, const int* __restrict__ labels,
            int64_t rows, int V, int T, int U, int blank, LsmBwd bw) {
    constexpr bool CLAMP = false;
    DenseMap map{labels, T, U};
#include "lsm_body_large.h"
}
template <typename E, int MODE, int LG_THREADS, int LG_MAXVEC>
__global__ void __launch_bounds__(LG_THREADS)
k_lsm_large_compact(const E* x, LsmOut<MODE, E>* out, PackedRows cr, int64_t rows, int V, int blank, LsmBwd bw) {
    constexpr bool CLAMP = false;
    CompactMap<MODE == LSM_GATHER> map{cr, 0, 0};
#include "lsm_body_large.h"
}
template <typename E, int MODE, int LG_THREADS, int LG_MAXVEC>
__global__ void __launch_bounds__(LG_THREADS)
k_lsm_large_clamped(const E* x, LsmOut<MODE, E>* out, const int* __restrict__ labels,
                    int64_t rows, int V, int T, int U, int blank, LsmBwd bw) {
    static_assert(MODE == LSM_BWD, "the clamp is the backward's");
    constexpr bool CLAMP = true;
    DenseMap map{labels, T, U};
#include "lsm_body_large.h"
}
template <typename E, int MODE, int LG_THREADS, int LG_MAXVEC>
__global__ void __launch_bounds__(LG_THREADS)
k_lsm_large_compact_clamped(const E* x, LsmOut<MODE, E>* out, PackedRows cr, int64_t rows, int V, int blank, LsmBwd bw) {
    static_assert(MODE == LSM_BWD, "the clamp is the backward's");
    constexpr bool CLAMP = true;
    CompactMap<false> map{cr, 0, 0};
#include "lsm_body_large.h"
}

// ---------------------------------------------------------------------------
// Generic fallback (any V, any alignment): one wave per row, three passes.
// ---------------------------------------------------------------------------
template <typename E, int MODE>
__global__ void __launch_bounds__(256)
k_lsm_generic(const E* x, LsmOut<MODE, E>* out, const int* __restrict__ labels,
              int64_t rows, int V, int T, int U, int blank, LsmBwd bw) {
    constexpr bool CLAMP = false;
    DenseMap map{labels, T, U};
#include "lsm_body_generic.h"
}
template <typename E, int MODE>
__global__ void __launch_bounds__(256)
k_lsm_generic_compact(const E* x, LsmOut<MODE, E>* out, PackedRows cr, int64_t rows, int V, int blank, LsmBwd bw) {
    constexpr bool CLAMP = false;
    CompactMap<MODE == LSM_GATHER> map{cr, 0, 0};
#include "lsm_body_generic.h"
}
template <typename E, int MODE>
__global__ void __launch_bounds__(256)
k_lsm_generic_clamped(const E* x, LsmOut<MODE, E>* out, const int* __restrict__ labels,
                      int64_t rows, int V, int T, int U, int blank, LsmBwd bw) {
    static_assert(MODE == LSM_BWD, "the clamp is the backward's");
    constexpr bool CLAMP = true;
    DenseMap map{labels, T, U};
#include "lsm_body_generic.h"
}
template <typename E, int MODE>
__global__ void __launch_bounds__(256)
k_lsm_generic_compact_clamped(const E* x, LsmOut<MODE, E>* out, PackedRows cr, int64_t rows, int V, int blank, LsmBwd bw) {
    static_assert(MODE == LSM_BWD, "the clamp is the backward's");
    constexpr bool CLAMP = true;
    CompactMap<false> map{cr, 0, 0};
#include "lsm_body_generic.h"
}

// ---------------------------------------------------------------------------
// Small vocabularies, plain log-softmax, rows in REGISTERS (round 3).  KR whole rows (KR <= 4, KR*V a multiple of 4,
// KR*V/4 <= 32 float4) form a 16-byte aligned group; a wave holds one group in lanes 0.. of each 32-lane half, one
// float4 per lane (V = 50: two rows = 25 lanes of 32 busy, the 800 bytes of a wave's two groups contiguous), and
// reduces the row maxima and sums with DPP butterflies inside the half (quad_perm xor 1 / xor 2, row_ror 4 / 8) plus
// one ds_swizzle across its two DPP rows -- no LDS memory, no barrier, one float4 load and one store per lane and
// group, non-temporal both ways.  This is the shape of the fastest plain copy on the part, and it runs at that
// copy's rate: 462 us for the c4 tensor (6.24 TB/s read + write) where the LDS-staged kernel below takes 498
// (tools/ubench/lsm_regs.hip, profiles/r03_ubench_lsm_regs.txt; without the non-temporal hint 484).
// ---------------------------------------------------------------------------
template <int CTRL> __device__ __forceinline__ float lsm_dpp(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, false));
}
__device__ __forceinline__ float lsm_swz16(float v) {   // lane ^ 16 inside each 32-lane half
    return __builtin_bit_cast(float, __builtin_amdgcn_ds_swizzle(__builtin_bit_cast(int, v), 0x401F));
}
__device__ __forceinline__ float half_sum32(float v) {
    v += lsm_dpp<0xB1>(v); v += lsm_dpp<0x4E>(v); v += lsm_dpp<0x124>(v); v += lsm_dpp<0x128>(v);
    return v + lsm_swz16(v);
}
// The KR row maxima of a group in ONE hand-written statement (round 6).  fmaxf() on a DPP result compiles to three
// instructions per butterfly step -- v_mov_b32_dpp, a v_max x,x that quiets a possible signalling NaN, the v_max -- where
// one v_max_f32_dpp does the work; with two rows per group that is 48 of the kernel's 311 vector instructions per wave, and
// the kernel sits AT the vector-issue bound (311 x 900 k waves / (1024 SIMDs x 0.6 G instructions/s) = 456 us of its 462).
// The KR chains are interleaved, so a step's result is two wait states old when the next step reads it through DPP
// (KR = 1, 2: topped up with s_nop); the leading s_nop 1 covers the compiler's instruction that produced the inputs
// (_isa_check.py walks the generated ISA for exactly these).  v_max_f32 returns the other operand for a quiet NaN as
// fmaxf does; a signalling NaN makes the row's maximum NaN and with it the row, which it would be anyway.
// The results leave through a per-wave LDS strip in ADDRESS order (round 6).  A group's segment (V = 50: 400 bytes) starts
// and ends inside 64-byte granules, and what that costs is the STORES: a copy whose stores sit 16 or 32 bytes off the
// 64-byte grid loses 5-19 %, one whose loads do loses nothing (tools/ubench/copy_shape.hip).  Two ds_write_b128 + two
// ds_read_b128 per lane turn the wave's four segments into one store instruction of 1024 contiguous bytes and one of the
// rest, all whole granules: the V=50 micro-benchmark 465 -> 457-460 us, same bits (tools/ubench/lsm_store_policy.hip).
// In the step (bench.py, c4, interleaved processes, profiles/r06_lsm_regs_ab.txt): 0.7997 -> 0.7924 ms on one box, 0.8418 ->
// 0.8323 on another; and with the stores then also written through AND streaming (sc1 nt: whole granules that nothing
// else will add to -- the case in which write-through pays) 0.8323 -> 0.8267.  Blocks of four groups per
// half lose 20 us.
#define RNNT_DPPMAX(R, CTRL) "v_max_f32_dpp " R ", " R ", " R " " CTRL " row_mask:0xf bank_mask:0xf\n\t"
#define RNNT_DPPMAX_STEPS(BODY, GAP)                                                                     \
    "s_nop 1\n\t" BODY("quad_perm:[1,0,3,2]") GAP BODY("quad_perm:[2,3,0,1]") GAP BODY("row_ror:4") GAP BODY("row_ror:8")
template <int KR> __device__ __forceinline__ void half_max32_rows(float (&M)[KR]) {
    static_assert(KR >= 1 && KR <= 4, "one to four rows per group");
    float t0, t1, t2, t3;
    if constexpr (KR == 1) {
#define RNNT_B1(C) RNNT_DPPMAX("%0", C)
        asm volatile(RNNT_DPPMAX_STEPS(RNNT_B1, "s_nop 1\n\t")
                     "ds_swizzle_b32 %1, %0 offset:swizzle(SWAP,16)\n\ts_waitcnt lgkmcnt(0)\n\tv_max_f32 %0, %0, %1"
                     : "+v"(M[0]), "=&v"(t0));
#undef RNNT_B1
    } else if constexpr (KR == 2) {
#define RNNT_B2(C) RNNT_DPPMAX("%0", C) RNNT_DPPMAX("%1", C)
        asm volatile(RNNT_DPPMAX_STEPS(RNNT_B2, "s_nop 0\n\t")
                     "ds_swizzle_b32 %2, %0 offset:swizzle(SWAP,16)\n\tds_swizzle_b32 %3, %1 offset:swizzle(SWAP,16)\n\t"
                     "s_waitcnt lgkmcnt(0)\n\tv_max_f32 %0, %0, %2\n\tv_max_f32 %1, %1, %3"
                     : "+v"(M[0]), "+v"(M[1]), "=&v"(t0), "=&v"(t1));
#undef RNNT_B2
    } else if constexpr (KR == 3) {
#define RNNT_B3(C) RNNT_DPPMAX("%0", C) RNNT_DPPMAX("%1", C) RNNT_DPPMAX("%2", C)
        asm volatile(RNNT_DPPMAX_STEPS(RNNT_B3, "")
                     "ds_swizzle_b32 %3, %0 offset:swizzle(SWAP,16)\n\tds_swizzle_b32 %4, %1 offset:swizzle(SWAP,16)\n\t"
                     "ds_swizzle_b32 %5, %2 offset:swizzle(SWAP,16)\n\t"
                     "s_waitcnt lgkmcnt(0)\n\tv_max_f32 %0, %0, %3\n\tv_max_f32 %1, %1, %4\n\tv_max_f32 %2, %2, %5"
                     : "+v"(M[0]), "+v"(M[1]), "+v"(M[2]), "=&v"(t0), "=&v"(t1), "=&v"(t2));
#undef RNNT_B3
    } else {
#define RNNT_B4(C) RNNT_DPPMAX("%0", C) RNNT_DPPMAX("%1", C) RNNT_DPPMAX("%2", C) RNNT_DPPMAX("%3", C)
        asm volatile(RNNT_DPPMAX_STEPS(RNNT_B4, "")
                     "ds_swizzle_b32 %4, %0 offset:swizzle(SWAP,16)\n\tds_swizzle_b32 %5, %1 offset:swizzle(SWAP,16)\n\t"
                     "ds_swizzle_b32 %6, %2 offset:swizzle(SWAP,16)\n\tds_swizzle_b32 %7, %3 offset:swizzle(SWAP,16)\n\t"
                     "s_waitcnt lgkmcnt(0)\n\tv_max_f32 %0, %0, %4\n\tv_max_f32 %1, %1, %5\n\tv_max_f32 %2, %2, %6\n\t"
                     "v_max_f32 %3, %3, %7"
                     : "+v"(M[0]), "+v"(M[1]), "+v"(M[2]), "+v"(M[3]), "=&v"(t0), "=&v"(t1), "=&v"(t2), "=&v"(t3));
#undef RNNT_B4
    }
}
#undef RNNT_DPPMAX_STEPS
#undef RNNT_DPPMAX
// (RG_UN = 2 groups per half and wave, loads first: lsm_plan.h)

// NT: bit 0 = non-temporal loads, bit 1 = non-temporal stores (both: 462 us for the c4 tensor, neither: 484); the launch
// passes 3, and the stores leave through the strip written through and streaming
// PLANE: the column plane (LsmBwd::col_out) on top -- the wave's 4 * KR rows lie in its strip in address order, so lane l
// picks element `col` of row l out of the strip and the wave's slice of the plane leaves as one store of 4 * KR
// consecutive floats (a workgroup's four waves: 16 * KR consecutive floats, whole lines from KR = 2 on); plain stores, for L2
// to put the pieces together.  Three vector instructions, one LDS read and one store per wave on top of ~311.
template <typename E, int KR, int NT, bool PLANE>
__global__ void __launch_bounds__(256) k_lsm_regs(const E* __restrict__ x, float* __restrict__ out,
                                                  const int64_t ngroups, const int V, const int xcd,
                                                  float* __restrict__ col_out, const int col) {
    const int lane = threadIdx.x & 63, j = lane & 31, half = lane >> 5;
    const int g4 = (KR * V) >> 2;                  // float4 per group
    const bool act = j < g4;
    __shared__ rnnt_f4 strip[4][64 * RG_UN];        // per wave: its 2 * RG_UN groups of <= 32 float4 in address order
    const int wv = threadIdx.x >> 6;
    // xcd: the eight XCDs (blockIdx mod 8; the grid is a multiple of 8) each stream a contiguous eighth of the groups
    const unsigned wg = xcd ? (blockIdx.x & 7u) * (gridDim.x >> 3) + (blockIdx.x >> 3) : blockIdx.x;
    const int64_t w = (int64_t)wg * 4 + (threadIdx.x >> 6);
    const rnnt_f4* __restrict__ xin = reinterpret_cast<const rnnt_f4*>(x);
    rnnt_f4* __restrict__ xout = reinterpret_cast<rnnt_f4*>(out);
    // the lane's four elements: the first `ns` of them belong to row r0 of the group, the rest to row r0 + 1
    const int e0 = 4 * j;
    const int r0 = e0 / V;
    const int ns = min(4, (r0 + 1) * V - e0);
    rnnt_f4 v[RG_UN];
#pragma unroll
    for (int i = 0; i < RG_UN; ++i) {
        const int64_t g = (w * RG_UN + i) * 2 + half;
        const float ninf = -__builtin_inff();
        v[i] = rnnt_f4{ninf, ninf, ninf, ninf};
        if constexpr (std::is_same_v<E, float>) {
            if (act && g < ngroups) v[i] = (NT & 1) ? __builtin_nontemporal_load(xin + g * g4 + j) : xin[g * g4 + j];
        } else {
            if (act && g < ngroups) { const float4 t = lsm_ld4<(NT & 1) != 0>(x, g * g4 + j); v[i] = rnnt_f4{t.x, t.y, t.z, t.w}; }
        }
    }
#pragma unroll
    for (int i = 0; i < RG_UN; ++i) {
        const rnnt_f4 t = v[i];
        const float ninf = -__builtin_inff();
        // maxima of the lane's two parts, then of every row of the group over the half
        const float a0 = t.x, a1 = ns > 1 ? t.y : ninf, a2 = ns > 2 ? t.z : ninf, a3 = ns > 3 ? t.w : ninf;
        const float b1 = ns > 1 ? ninf : t.y, b2 = ns > 2 ? ninf : t.z, b3 = ns > 3 ? ninf : t.w;
        const float mf = fmaxf(fmaxf(a0, a1), fmaxf(a2, a3)), ms = fmaxf(b1, fmaxf(b2, b3));
        float M[KR];
#pragma unroll
        for (int r = 0; r < KR; ++r) M[r] = act ? (r0 == r ? mf : (r0 + 1 == r ? ms : ninf)) : ninf;
        half_max32_rows<KR>(M);
        float m_first = M[0], m_second = M[KR - 1];
#pragma unroll
        for (int r = 1; r < KR; ++r) m_first = r0 == r ? M[r] : m_first;
#pragma unroll
        for (int r = KR - 2; r >= 0; --r) m_second = r0 + 1 == r ? M[r] : m_second;
        // x - max first, for the exponent AND the result (the association of torch): the exponent exp2((x - max) * LOG2E)
        // costs what exp2(fma(x, LOG2E, -max * LOG2E)) does, and nothing of the row's maximum is left in the sum -- no
        // per-row correction (lsm_log_sum), which two rows per lane would pay for per lane here
        const float d0 = t.x - m_first, d1 = t.y - (ns > 1 ? m_first : m_second);
        const float d2 = t.z - (ns > 2 ? m_first : m_second), d3 = t.w - (ns > 3 ? m_first : m_second);
        const float e0x = __builtin_amdgcn_exp2f(d0 * LOG2E);
        const float e1x = __builtin_amdgcn_exp2f(d1 * LOG2E);
        const float e2x = __builtin_amdgcn_exp2f(d2 * LOG2E);
        const float e3x = __builtin_amdgcn_exp2f(d3 * LOG2E);
        const float sf = e0x + (ns > 1 ? e1x : 0.f) + (ns > 2 ? e2x : 0.f) + (ns > 3 ? e3x : 0.f);
        const float ss = (ns > 1 ? 0.f : e1x) + (ns > 2 ? 0.f : e2x) + (ns > 3 ? 0.f : e3x);
        // log-sum of every row; the result is (x - max) - log-sum, the association of the LDS-staged kernel (and of
        // torch): subtracting a rounded max + log-sum instead loses an ulp of |max| per element, which the lattice
        // amplifies to 1e-4 on the gradients at c2's size
        float Lg[KR];
#pragma unroll
        for (int r = 0; r < KR; ++r)
            Lg[r] = __builtin_amdgcn_logf(half_sum32(act ? (r0 == r ? sf : (r0 + 1 == r ? ss : 0.f)) : 0.f)) * LN2;
        float l_first = Lg[0], l_second = Lg[KR - 1];
#pragma unroll
        for (int r = 1; r < KR; ++r) l_first = r0 == r ? Lg[r] : l_first;
#pragma unroll
        for (int r = KR - 2; r >= 0; --r) l_second = r0 + 1 == r ? Lg[r] : l_second;
        const rnnt_f4 res = rnnt_f4{d0 - l_first, d1 - (ns > 1 ? l_first : l_second), d2 - (ns > 2 ? l_first : l_second),
                                  d3 - (ns > 3 ? l_first : l_second)};
        if (act) strip[wv][(2 * i + half) * g4 + j] = res;
    }
    // the wave's 2 * RG_UN groups are 64 * g4 contiguous bytes: out of the strip in address order, one store instruction of
    // 1024 bytes and one of the rest -- every instruction whole 64-byte granules (the strip is the wave's own: no barrier)
    wave_sync_lds();
    if constexpr (PLANE) {
        const int64_t wu = (int64_t)wg * 4 + __builtin_amdgcn_readfirstlane(wv);      // w, known to be wave-uniform
        const int64_t r0w = wu * (2 * RG_UN * KR);                                   // the wave's first row
        const int nr = (int)min((int64_t)(2 * RG_UN * KR), ngroups * KR - r0w);     // its rows inside the tensor (<= 0: none)
        const float* srow = reinterpret_cast<const float*>(strip[__builtin_amdgcn_readfirstlane(wv)]);
        if (lane < nr) col_out[r0w + lane] = srow[__mul24(lane, V) + col];      // (lane < 64, V <= 128)
    }
    const int64_t f0 = w * (2 * RG_UN) * g4, nf = ngroups * g4;
    const int nw = 2 * RG_UN * g4;                  // float4 of this wave (<= 64 * RG_UN)
#pragma unroll
    for (int k = 0; k < RG_UN; ++k) {
        const int f = k * 64 + lane;
        if (f < nw && f0 + f < nf) {
            const rnnt_f4 r = strip[wv][f];
            // written through and streaming (the s_nop: _isa_check.py, second rule)
            asm volatile("global_store_dwordx4 %0, %1, off sc1 nt\n\ts_nop 1" ::"v"(xout + f0 + f), "v"(r) : "memory");
        }
    }
}

// ---------------------------------------------------------------------------
// Rows in registers, L lanes per row (round 4; fused gather, V a multiple of 4).  Every row is 16-byte aligned, so
// its L lanes load Q4 float4 each straight from HBM (a row instruction reads L*16 contiguous bytes: whole 128-byte lines
// from L = 8 on), reduce with L-wide butterflies and never touch LDS; a wave carries UN passes of 64/L rows, all loads
// issued before the first use.  The LDS-staged kernel spends 333 VALU instructions per wave on the same work at V = 128
// (run-time column loops, two LDS reads per element; SQ counters: the vector ALUs 67 % busy at 4.7 TB/s,
// profiles/r04_lsm_rows_ab.txt), this one about 150.  Fused gather only: as the plain log-softmax it runs at the rate of
// the kernels that serve it now (V = 160 ... 600: 5.5-5.7 TB/s either way), so that mode is not instantiated.
//   One lane per row (all rows of the wave in one go: the index arithmetic of map_cell is paid once per
//   wave) fetches the row's blank and label logits again -- the wave has just read those lines -- and stores the pair.
// ---------------------------------------------------------------------------
// all-reduce over aligned groups of L lanes on DPP (quad permutes, then the mirrors: once every lane of a quad holds the
// quad's value, reversing 8 / 16 lanes swaps whole quads / halves), lane ^ 16 on ds_swizzle, lane ^ 32 on a permute
template <int L, bool MAX> __device__ __forceinline__ float lsm_group_reduce(float v) {
#define LSM_STEP(w) v = MAX ? fmaxf(v, (w)) : v + (w)
    if constexpr (L >= 2) LSM_STEP(lsm_dpp<0xB1>(v));
    if constexpr (L >= 4) LSM_STEP(lsm_dpp<0x4E>(v));
    if constexpr (L >= 8) LSM_STEP(lsm_dpp<0x141>(v));
    if constexpr (L >= 16) LSM_STEP(lsm_dpp<0x140>(v));
    if constexpr (L >= 32) LSM_STEP(lsm_swz16(v));
    if constexpr (L >= 64) LSM_STEP(__shfl_xor(v, 32, WAVE));
#undef LSM_STEP
    return v;
}

// passes per wave: two for the 8-lane rows (V <= 128: 16 rows = 8 KB per wave at V = 128), one above (V = 256 ... 1024:
// 299 / 998 us against 306 / 1057 with two, profiles/r04_lsm_rows_ab.txt)
template <int L> struct RowsShape {
    static constexpr int UN = L <= 8 ? 2 : 1;
    static constexpr int RW = WAVE / L;            // rows per pass
    static constexpr int RPW = RW * UN;            // rows per wave
};

// loads (all passes first), row maxima and log-sums of the rows at src[p] (one pointer per lane and pass: the lane's
// first float4 of its row)
template <typename E, int L, int Q, int MODE>
__device__ __forceinline__ void lsm_rows_stats(const E* const (&src)[RowsShape<L>::UN], bool last_ok,
                                               float (&mx)[RowsShape<L>::UN], float (&ls)[RowsShape<L>::UN]) {
    constexpr int UN = RowsShape<L>::UN, VEC = 4;
    const float ninf = -__builtin_inff();
    const unsigned last_off = last_ok ? (Q - 1) * L : 0;   // a last float4 past the row: re-read the first, made -inf
    float v[UN][Q][VEC];
#pragma unroll
    for (int p = 0; p < UN; ++p) {
#pragma unroll
        for (int i = 0; i < Q; ++i) {
            const unsigned off = i < Q - 1 ? i * L : last_off;
            const float4 t = lsm_ld4<RNNT_LSM_NT_MODE(MODE)>(src[p], off);
            v[p][i][0] = t.x; v[p][i][1] = t.y; v[p][i][2] = t.z; v[p][i][3] = t.w;
        }
    }
#pragma unroll
    for (int p = 0; p < UN; ++p)
#pragma unroll
        for (int e = 0; e < VEC; ++e)
            if (!last_ok) v[p][Q - 1][e] = ninf;
#pragma unroll
    for (int p = 0; p < UN; ++p) {
        float m = ninf;
#pragma unroll
        for (int i = 0; i < Q; ++i)
#pragma unroll
            for (int e = 0; e < VEC; ++e) m = fmaxf(m, v[p][i][e]);
        m = lsm_group_reduce<L, true>(m);
        const float mb = -m * LOG2E;
        float s = 0.0f;
#pragma unroll
        for (int i = 0; i < Q; ++i)
#pragma unroll
            for (int e = 0; e < VEC; ++e) s += __builtin_amdgcn_exp2f(__builtin_fmaf(v[p][i][e], LOG2E, mb));
        s = lsm_group_reduce<L, false>(s);
        mx[p] = m;
        ls[p] = lsm_log_sum(__builtin_amdgcn_logf(s) * LN2, m, mb);
    }
}

// lane l < RPW picks up the statistics of row l of the wave: first lane of group l % RW, pass l / RW
template <int L>
__device__ __forceinline__ void lsm_rows_stats_of_lane(int lane, const float (&mx)[RowsShape<L>::UN],
                                                       const float (&ls)[RowsShape<L>::UN], float& m, float& lg) {
    constexpr int UN = RowsShape<L>::UN, RW = RowsShape<L>::RW;
    const int srcl = (lane % RW) * L;
    m = 0.0f;
    lg = 0.0f;
#pragma unroll
    for (int p = 0; p < UN; ++p) {
        const float mp = __shfl(mx[p], srcl, WAVE), lp = __shfl(ls[p], srcl, WAVE);
        if (lane / RW == p) { m = mp; lg = lp; }
    }
}

// consecutive rows per wave
template <typename E, int L, int Q>
__global__ void __launch_bounds__(256)
k_lsm_rows(const E* x, float* out, const int* __restrict__ labels, int64_t rows, int V, int T, int U, int blank) {
    DenseMap map{labels, T, U};
#include "lsm_body_rows.h"
}
template <typename E, int L, int Q>
__global__ void __launch_bounds__(256)
k_lsm_rows_compact(const E* x, float* out, PackedRows cr, int64_t rows, int V, int blank) {
    CompactMap<true> map{cr, 0, 0};
#include "lsm_body_rows.h"
}

// Along the diagonals (rows that are one or two whole 128-byte lines: V = 32, 64; T >= 16): a wave takes the 16 cells
// (t' - k mod T, u0 + k), k = 0 ... 15 -- one run of 16 consecutive pairs of the diagonal-major plane, stored as one
// 128-byte piece -- instead of 16 consecutive rows, whose pairs land 8 bytes each in 16 different lines (counters: 32
// bytes written per pair; with the pairs stored linearly the kernel is 12-17 us of 145 faster at V = 128, N*T*U = 1.6 M).
// V = 32 / 64: forward 96.5 / 134 us against 102 / 144; from V = 96 on the scattered rows cost what the stores save (174
// vs 177, 199 vs 193: consecutive rows kept there).  No index division: grid = (T / 4 rounded up, column blocks of 16, N).
template <typename E, int Q>
__global__ void __launch_bounds__(256)
k_lsm_rows_diag(const E* x, float* out, const int* __restrict__ labels, int V, int T, int U, int blank) {
    constexpr int L = 8, VEC = 4, MODE = LSM_GATHER;
    constexpr int UN = RowsShape<L>::UN, RW = RowsShape<L>::RW, RPW = RowsShape<L>::RPW;
    static_assert(RPW == 16, "one run of 16 pairs per wave");
    const int lane = threadIdx.x & 63, h = lane % L, rr = lane / L;
    const int tp = (int)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (tp >= T) return;
    const int u0 = (int)blockIdx.y * RPW, n = (int)blockIdx.z;
    const bool last_ok = (h + (Q - 1) * L) * VEC < V;
    const size_t plane = (size_t)n * T;            // frames in front of this utterance
    // the pair of cell k = lane (lane < 16), requested first
    float xb = 0.0f, xl = 0.0f;
    const bool own = lane < RPW && u0 + lane < U;
    if (own) {
        const int u = u0 + lane;
        int t = tp - lane;
        t += t < 0 ? T : 0;
        const int lab = (u < U - 1) ? safe_label(labels[(size_t)n * (U - 1) + u], V, blank) : blank;
        const E* xr = x + ((plane + t) * U + u) * V;
        xb = lsm_ld1(xr + blank);
        xl = lsm_ld1(xr + lab);
    }
    const E* src[UN];
#pragma unroll
    for (int p = 0; p < UN; ++p) {
        const int k = p * RW + rr;
        const int u = min(u0 + k, U - 1);          // (columns past the plane re-read the last one and are dropped)
        int t = tp - k;
        t += t < 0 ? T : 0;
        src[p] = x + ((plane + t) * U + u) * V + h * VEC;
    }
    float mx[UN], ls[UN];
    lsm_rows_stats<E, L, Q, MODE>(src, last_ok, mx, ls);
    float m, lg;
    lsm_rows_stats_of_lane<L>(lane, mx, ls, m, lg);
    int r = tp + u0;
    r = r >= T ? r % T : r;
    if (own) reinterpret_cast<float2*>(out)[(plane + r) * U + u0 + lane] = make_float2((xb - m) - lg, (xl - m) - lg);
}

// One launch of a fused log-softmax kernel family, dense or compact by the map policy; CLAMP (LSM_BWD only): the clamped
// twin of the same kernel, in the same launch shape.
template <typename E, int L, int MODE, bool WP, bool CLAMP, class Map>
static void launch_lsm_small(unsigned grid, size_t lds, hipStream_t stream, const E* x, LsmOut<MODE, E>* out,
                             const Map& map, int64_t rows, int V, int R, int q, int blank, LsmBwd bw) {
    if constexpr (CLAMP && Map::COMPACT)
        k_lsm_small_compact_clamped<E, L, MODE, WP><<<grid, SM_THREADS, lds, stream>>>(x, out, map.r, rows, V, R, q, blank,
                                                                                       bw);
    else if constexpr (CLAMP)
        k_lsm_small_clamped<E, L, MODE, WP><<<grid, SM_THREADS, lds, stream>>>(x, out, map.labels, rows, V, R, q, map.T,
                                                                               map.U, blank, bw);
    else if constexpr (Map::COMPACT)
        k_lsm_small_compact<E, L, MODE, WP><<<grid, SM_THREADS, lds, stream>>>(x, out, map.r, rows, V, R, q, blank, bw);
    else
        k_lsm_small<E, L, MODE, WP><<<grid, SM_THREADS, lds, stream>>>(x, out, map.labels, rows, V, R, q, map.T, map.U,
                                                                       blank, bw);
}
template <typename E, int MODE, int TH, int NV, bool CLAMP, class Map>
static void launch_lsm_large(unsigned grid, hipStream_t stream, const E* x, LsmOut<MODE, E>* out, const Map& map,
                             int64_t rows, int V, int blank, LsmBwd bw) {
    if constexpr (CLAMP && Map::COMPACT)
        k_lsm_large_compact_clamped<E, MODE, TH, NV><<<grid, TH, 0, stream>>>(x, out, map.r, rows, V, blank, bw);
    else if constexpr (CLAMP)
        k_lsm_large_clamped<E, MODE, TH, NV><<<grid, TH, 0, stream>>>(x, out, map.labels, rows, V, map.T, map.U, blank, bw);
    else if constexpr (Map::COMPACT)
        k_lsm_large_compact<E, MODE, TH, NV><<<grid, TH, 0, stream>>>(x, out, map.r, rows, V, blank, bw);
    else
        k_lsm_large<E, MODE, TH, NV><<<grid, TH, 0, stream>>>(x, out, map.labels, rows, V, map.T, map.U, blank, bw);
}
template <typename E, int MODE, bool CLAMP, class Map>
static void launch_lsm_generic(unsigned grid, hipStream_t stream, const E* x, LsmOut<MODE, E>* out, const Map& map,
                               int64_t rows, int V, int blank, LsmBwd bw) {
    if constexpr (CLAMP && Map::COMPACT)
        k_lsm_generic_compact_clamped<E, MODE><<<grid, 256, 0, stream>>>(x, out, map.r, rows, V, blank, bw);
    else if constexpr (CLAMP)
        k_lsm_generic_clamped<E, MODE><<<grid, 256, 0, stream>>>(x, out, map.labels, rows, V, map.T, map.U, blank, bw);
    else if constexpr (Map::COMPACT)
        k_lsm_generic_compact<E, MODE><<<grid, 256, 0, stream>>>(x, out, map.r, rows, V, blank, bw);
    else
        k_lsm_generic<E, MODE><<<grid, 256, 0, stream>>>(x, out, map.labels, rows, V, map.T, map.U, blank, bw);
}
template <typename E, int L, int Q, class Map>
static void launch_lsm_rows(unsigned grid, hipStream_t stream, const E* x, float* out, const Map& map, int64_t rows,
                            int V, int blank) {
    if constexpr (Map::COMPACT)
        k_lsm_rows_compact<E, L, Q><<<grid, 256, 0, stream>>>(x, out, map.r, rows, V, blank);
    else
        k_lsm_rows<E, L, Q><<<grid, 256, 0, stream>>>(x, out, map.labels, rows, V, map.T, map.U, blank);
}

// What the plan says, launched: a switch on the family and on its template selectors, nothing decided here.
// E: the storage type of x (and of out in LSM_BWD).  Map: the row -> cell policy (DenseMap, CompactMap).  CLAMP: the clamped
// twins of the plan's kernel (LSM_BWD, whose plans name SMALL, LARGE or GENERIC).
template <int MODE, typename E, bool CLAMP, class Map>
static hipError_t launch_lsm_plan(hipStream_t stream, const LsmPlan& p, const E* x, LsmOut<MODE, E>* out, const Map& map,
                                  int64_t rows, int V, int blank, LsmBwd bw) {
    bw.xcd = p.xcd;
#define LSM_LARGE(TH_, NV_) \
    if (p.TH == TH_ && p.NV == NV_) launch_lsm_large<E, MODE, TH_, NV_, CLAMP>(p.grid, stream, x, out, map, rows, V, blank, bw);
    switch (p.family) {
        case LsmFamily::REGS:
            if constexpr (MODE == LSM_NORM) {
                const int64_t ngroups = p.head_rows / p.KR;
#define LSM_REGS(KR_) \
    case KR_:                                                                                                    \
        if (bw.col_out)                                                                                          \
            k_lsm_regs<E, KR_, 3, true><<<p.grid, 256, 0, stream>>>(x, out, ngroups, V, p.xcd, bw.col_out, bw.col); \
        else                                                                                                     \
            k_lsm_regs<E, KR_, 3, false><<<p.grid, 256, 0, stream>>>(x, out, ngroups, V, p.xcd, nullptr, 0);     \
        break;
                switch (p.KR) { LSM_REGS(1) LSM_REGS(2) LSM_REGS(3) LSM_REGS(4) }
#undef LSM_REGS
            }
            break;
        case LsmFamily::LGR:
            if constexpr (MODE == LSM_NORM) {
                LSM_LARGE(64, 1) LSM_LARGE(64, 2) LSM_LARGE(64, 3) LSM_LARGE(128, 2)
                LSM_LARGE(128, 1) LSM_LARGE(192, 1) LSM_LARGE(256, 1)
            }
            break;
        case LsmFamily::ROWS:
            if constexpr (MODE == LSM_GATHER) {
#define LSM_ROWS(LL, QQ) \
    if (p.L == LL && p.Q == QQ) launch_lsm_rows<E, LL, QQ>(p.grid, stream, x, out, map, rows, V, blank);
#define LSM_ROWS_L(LL) LSM_ROWS(LL, 1) LSM_ROWS(LL, 2) LSM_ROWS(LL, 3) LSM_ROWS(LL, 4)
                LSM_ROWS_L(8) LSM_ROWS_L(16) LSM_ROWS_L(32) LSM_ROWS_L(64)
#undef LSM_ROWS_L
#undef LSM_ROWS
            }
            break;
        case LsmFamily::ROWS_DIAG:
            if constexpr (MODE == LSM_GATHER && !Map::COMPACT) {
                const dim3 grid(p.grid, p.grid_y, p.grid_z);
                if (p.Q == 1) k_lsm_rows_diag<E, 1><<<grid, 256, 0, stream>>>(x, out, map.labels, V, map.T, map.U, blank);
                else k_lsm_rows_diag<E, 2><<<grid, 256, 0, stream>>>(x, out, map.labels, V, map.T, map.U, blank);
            }
            break;
        case LsmFamily::SMALL:
#define LSM_SMALL(LL)                                                                                            \
    case LL:                                                                                                     \
        if (p.WP)                                                                                                \
            launch_lsm_small<E, LL, MODE, (LL <= 16), CLAMP>(p.grid, p.lds_bytes, stream, x, out, map, rows, V, p.R, p.q, blank, bw); \
        else                                                                                                     \
            launch_lsm_small<E, LL, MODE, false, CLAMP>(p.grid, p.lds_bytes, stream, x, out, map, rows, V, p.R, p.q, blank, bw);     \
        break;
            switch (p.L) {
                LSM_SMALL(1) LSM_SMALL(2) LSM_SMALL(4) LSM_SMALL(8) LSM_SMALL(16) LSM_SMALL(32)
                LSM_SMALL(64)
            }
#undef LSM_SMALL
            break;
        case LsmFamily::LARGE:
            if constexpr (MODE == LSM_NORM) {
                LSM_LARGE(512, 8) LSM_LARGE(768, 3) LSM_LARGE(896, 3) LSM_LARGE(1024, 3) LSM_LARGE(1024, 2)
                LSM_LARGE(768, 2) LSM_LARGE(512, 3) LSM_LARGE(256, 2) LSM_LARGE(384, 2) LSM_LARGE(512, 2)
            } else {
                LSM_LARGE(256, 4) LSM_LARGE(256, 8) LSM_LARGE(512, 8)
            }
            break;
        case LsmFamily::GENERIC:
            launch_lsm_generic<E, MODE, CLAMP>(p.grid, stream, x, out, map, rows, V, blank, bw);
            break;
    }
#undef LSM_LARGE
    return hipGetLastError();
}

// Facts, knobs, plan, launch.  The register kernel takes whole groups of rows; what is left over is planned and launched
// as a call of its own behind it (lsm_plan.h: never the register kernel again), with its slice of the plane.
template <int MODE, typename E, bool CLAMP = false, class Map>
static hipError_t dispatch_lsm_map(hipStream_t stream, const E* x, LsmOut<MODE, E>* out, Map map, int64_t rows, int V,
                                   int blank, LsmBwd bw) {
    if (rows <= 0) return hipSuccess;
    const bool aligned = (reinterpret_cast<uintptr_t>(x) % (4 * sizeof(E)) == 0) &&
                         (MODE == LSM_GATHER || reinterpret_cast<uintptr_t>(out) % (4 * sizeof(*out)) == 0);
    LsmFacts f{MODE, (int)sizeof(E), rows, V, aligned, Map::COMPACT, 1, 1, bw.col_out != nullptr};
    if constexpr (!Map::COMPACT) { f.T = map.T; f.U = map.U; }
    const LsmKnobs& knobs = lsm_knobs();
    const LsmPlan head = plan_lsm(f, knobs);
    static_assert(!CLAMP || MODE == LSM_BWD, "the clamp is the backward's");
    const hipError_t e = launch_lsm_plan<MODE, E, CLAMP>(stream, head, x, out, map, rows, V, blank, bw);
    if (head.family != LsmFamily::REGS || e != hipSuccess || head.head_rows == rows) return e;
    const int64_t done = head.head_rows;
    f.rows = rows - done;
    if (bw.col_out) bw.col_out += done;
    return launch_lsm_plan<MODE, E, CLAMP>(stream, plan_lsm(f, knobs), x + done * V, out + done * V, map, f.rows, V, blank, bw);
}

template <int MODE, typename E = float, bool CLAMP = false>
static hipError_t dispatch_lsm(hipStream_t stream, const E* x, LsmOut<MODE, E>* out, const int* labels,
                               int64_t rows, int V, int T, int U, int blank, LsmBwd bw) {
    return dispatch_lsm_map<MODE, E, CLAMP>(stream, x, out, DenseMap{labels, T, U}, rows, V, blank, bw);
}
// compact rows (kernels.h: PackedRows) in the two fused modes
template <int MODE, typename E, bool CLAMP = false>
static hipError_t dispatch_lsm_compact(hipStream_t stream, const E* x, LsmOut<MODE, E>* out, const PackedRows& cr,
                                       int V, int blank, LsmBwd bw) {
    static_assert(MODE != LSM_NORM, "the plain log-softmax has no map");
    return dispatch_lsm_map<MODE, E, CLAMP>(stream, x, out, CompactMap<MODE == LSM_GATHER>{cr, 0, 0}, cr.rows, V, blank, bw);
}

// The operations of kernels.h at one storage type: each lsm_<type>.hip instantiates them, and through them the kernels
// above, for its own E.  (Members defined outside the class: `extern template` does not hold back an inline member.)
template <typename E> struct LsmOps {
    static hipError_t log_softmax(hipStream_t stream, const E* x, float* out, int64_t rows, int V);
    static hipError_t log_softmax_plane(hipStream_t stream, const E* x, float* out, int64_t rows, int V, float* col_out,
                                        int col);
    static hipError_t gather(hipStream_t stream, const E* logits, const int* labels, float* ws2, int N, int T, int U, int V,
                             int blank);
    // clamp > 0: the clamped twins (LsmBwd::clamp); 0: the kernels that have always been here
    static hipError_t backward(hipStream_t stream, const E* logits, const int* labels, const float* g2_diagonal,
                               const float* scale, E* dlogits, int N, int T, int U, int V, int blank, float clamp);
    static hipError_t gather_compact(hipStream_t stream, const E* logits, float* ws2, const PackedRows& cr, int V, int blank);
    static hipError_t backward_compact(hipStream_t stream, const E* logits, const float* g2_rowmajor, const float* scale,
                                       E* dlogits, const PackedRows& cr, int V, int blank, float clamp);
};
template <typename E>
hipError_t LsmOps<E>::log_softmax(hipStream_t stream, const E* x, float* out, int64_t rows, int V) {
    return dispatch_lsm<LSM_NORM, E>(stream, x, out, nullptr, rows, V, 1, 1, 0, LsmBwd{nullptr, nullptr});
}
template <typename E>
hipError_t LsmOps<E>::log_softmax_plane(hipStream_t stream, const E* x, float* out, int64_t rows, int V, float* col_out,
                                        int col) {
    return dispatch_lsm<LSM_NORM, E>(stream, x, out, nullptr, rows, V, 1, 1, 0, LsmBwd{nullptr, nullptr, 0, 0.0f, col_out, col});
}
template <typename E>
hipError_t LsmOps<E>::gather(hipStream_t stream, const E* logits, const int* labels, float* ws2, int N, int T, int U, int V,
                             int blank) {
    return dispatch_lsm<LSM_GATHER, E>(stream, logits, ws2, labels, (int64_t)N * T * U, V, T, U, blank,
                                       LsmBwd{nullptr, nullptr});
}
template <typename E>
hipError_t LsmOps<E>::backward(hipStream_t stream, const E* logits, const int* labels, const float* g2_diagonal,
                               const float* scale, E* dlogits, int N, int T, int U, int V, int blank, float clamp) {
    const LsmBwd bw{reinterpret_cast<const float2*>(g2_diagonal), scale, 0, clamp};
    if (clamp > 0.0f)
        return dispatch_lsm<LSM_BWD, E, true>(stream, logits, dlogits, labels, (int64_t)N * T * U, V, T, U, blank, bw);
    return dispatch_lsm<LSM_BWD, E>(stream, logits, dlogits, labels, (int64_t)N * T * U, V, T, U, blank, bw);
}
template <typename E>
hipError_t LsmOps<E>::gather_compact(hipStream_t stream, const E* logits, float* ws2, const PackedRows& cr, int V,
                                     int blank) {
    return dispatch_lsm_compact<LSM_GATHER, E>(stream, logits, ws2, cr, V, blank, LsmBwd{nullptr, nullptr});
}
template <typename E>
hipError_t LsmOps<E>::backward_compact(hipStream_t stream, const E* logits, const float* g2_rowmajor, const float* scale,
                                       E* dlogits, const PackedRows& cr, int V, int blank, float clamp) {
    const LsmBwd bw{reinterpret_cast<const float2*>(g2_rowmajor), scale, 0, clamp};
    if (clamp > 0.0f) return dispatch_lsm_compact<LSM_BWD, E, true>(stream, logits, dlogits, cr, V, blank, bw);
    return dispatch_lsm_compact<LSM_BWD, E>(stream, logits, dlogits, cr, V, blank, bw);
}
extern template struct LsmOps<float>;
extern template struct LsmOps<__bf16>;
extern template struct LsmOps<_Float16>;

}  // namespace rnnt
