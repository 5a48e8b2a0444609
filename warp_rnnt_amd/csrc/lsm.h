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

// The row -> cell map of the fused log-softmax kernels is a policy, chosen by a template parameter.  A kernel builds its
// map with Map::make(head, tail) from two arguments of its own, which the launch takes from the host's map: head(), tail(blank).
// Head sits behind `out` and Tail behind V in every kernel's argument list -- where the labels or the packed rows, and T, U
// and the blank index, have always been: Tail ENDS with the blank, so that a map with nothing else to say (the compact one)
// adds no argument -- an empty struct would still take a slot, move `blank` and LsmBwd, and with them the scalar
// registers of the row-per-workgroup kernels, which have none to spare.  DenseMap's Head is the labels as
// `const int* __restrict__`: carried inside a by-value struct the qualifier is lost, and the dense fused kernels then
// fetch labels again that they already hold.
// chunk(first, last) is called by every wave of a kernel, wave-uniformly, before at() is asked for rows in [first, last];
// pair() and scale() read the backward's gradient pair and upstream scale of a mapped row, put() stores the gather's pair.
//   DenseMap: the (N,T,U,V) tensor, map_cell -- what the dense kernels have always done.
struct DenseMap {
    static constexpr bool COMPACT = false;
    using Head = const int* __restrict__;
    struct Tail { int T, U, blank; };
    const int* labels;
    int T, U;
    static __device__ __forceinline__ DenseMap make(Head labels, Tail s) { return {labels, s.T, s.U}; }
    Head head() const { return labels; }
    Tail tail(int blank) const { return {T, U, blank}; }
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
    using Head = PackedRows;
    struct Tail { int blank; };
    PackedRows r;
    int n0, n1;
    static __device__ __forceinline__ CompactMap make(const Head& r, Tail) { return {r, 0, 0}; }
    const Head& head() const { return r; }
    Tail tail(int blank) const { return {blank}; }
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
constexpr bool lsm_nt(int mode) { return mode != LSM_NORM; }

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
    // The CLAMP instantiations of the backward kernels only (below; > 0 there): d/d logits at unit upstream are limited to [-clamp, +clamp]
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
// CLAMP is a template parameter of the SMALL, LARGE and GENERIC kernels and of their bodies: false in the instantiations
// that have always been here (their code is what it was), true in those a call with c > 0 launches under the SAME plan,
// which exist for LSM_BWD only.  The clamped bodies keep the unclamped operation order -- e_j * (gs / s), the two
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

// The three per-element formulas of this kernel, written once for its two row forms (straight-line, and the run-time loops
// of q <= 8) and for the row-per-workgroup kernel.  `v` is the logit, mb = -max * LOG2E (rounded: lsm_log_sum), gq =
// (gB + gL) / s.  The row epilogues around them stay written out per form: folded into one callable they compile to one
// branch block and one v_mov less in three L = 1 kernels per unit, and this family changes by no instruction count.
__device__ __forceinline__ float lsm_norm_el(float v, float mx, float ls) { return (v - mx) - ls; }
__device__ __forceinline__ float lsm_bwd_el(float v, float mb, float gq) {
    return -__builtin_amdgcn_exp2f(__builtin_fmaf(v, LOG2E, mb)) * gq;      // -p_j (gB + gL), p_j = e_j / s
}
__device__ __forceinline__ float lsm_bwd_el_clamped(float v, float mb, float gq, float c, float sc) {
    return lsm_clamp(lsm_bwd_el(v, mb, gq), c) * sc;
}

template <typename E, int L, int MODE, bool WP, bool CLAMP, class Map>
__device__ __forceinline__ void lsm_small_body(const E* x, LsmOut<MODE, E>* out, Map map, int64_t rows, int V, int R, int q,
                                               int blank, LsmBwd bw) {
    constexpr bool GATHER = MODE == LSM_GATHER, NT = lsm_nt(MODE);
    extern __shared__ __attribute__((aligned(16))) float tile[];
    float2* stat = reinterpret_cast<float2*>(tile + (size_t)R * V);   // GATHER: (max, log-sum) per row
    const int tid = threadIdx.x;
    const int64_t row0 = (int64_t)stream_block() * R;
    if (row0 >= rows) return;
    const int nrows = (int)min((int64_t)R, rows - row0);
    map.chunk(row0, row0 + nrows - 1);
    const int nel = nrows * V;                      // floats in this chunk
    const E* src = x + row0 * V;                    // vector aligned: R % 4 == 0 (out may alias x)
    // wave-private view of the same tile: rows [wr0, wr0 + wn) of the chunk
    constexpr int RW = (WAVE / L) > 0 ? (WAVE / L) : 1;
    const int lane = tid & (WAVE - 1);
    const int wr0 = (tid >> 6) * RW;
    const int wn = min(max(nrows - wr0, 0), RW);
    const int wel = wn * V, wvec = wel >> 2;
    float* wtile = tile + wr0 * V;

    // ---- stage: the tile is a plain copy of the chunk ----
    const int nvec = nel >> 2;
    // fused backward: the gradient pair (and scale) of the row this thread works on first, requested before the tile
    [[maybe_unused]] CellMap pm = {0, 0, 0};
    [[maybe_unused]] float2 pg = make_float2(0.0f, 0.0f);
    [[maybe_unused]] float psc = 1.0f;
    if constexpr (MODE == LSM_BWD) {
        pm = map.at((size_t)(row0 + min(tid / L, nrows - 1)), V, blank);
        pg = map.pair(bw, pm);
        psc = map.scale(bw, pm);
    }
    // LOADS FIRST (round 5).  Written as `for (i ...) tile[i] = load(src + i)` the compiler emits load, s_waitcnt vmcnt(0),
    // ds_write per iteration: a wave had ONE 16-byte load per lane in flight at a time and paid the memory latency three
    // to four times per tile -- 1 KB per wave in flight, 32 KB per CU, which at ~1.5 us of loaded latency is the 5.2 TB/s
    // the fused gather ran at (read-only streams reach 7.0, tools/ubench/copy_rate.hip).  A tile is at most four passes
    // of the threads that stage it (SM_FLOATS, and V <= 16 L for the wave-private form): all of a lane's loads are
    // issued before the first of them is written to LDS -- unconditionally, at an index clamped into the tile, and so are
    // the LDS writes (lanes past the end rewrite the tile's last 16 bytes with the bytes that are there).  A predicate per
    // load comes out as a branch per load with a conservative wait at every join; predicates on the writes alone and the
    // compiler sinks the loads into them.
    constexpr int STAGE_UN = WP ? 4 : (sm_floats<E, MODE>() / 4 + SM_THREADS - 1) / SM_THREADS;   // (3200 floats, 256 threads: 4)
    if constexpr (WP) {
        const E* wsrc = src + (size_t)wr0 * V;
        for (int base = lane; base < wvec; base += STAGE_UN * WAVE) {
            float4 sv[STAGE_UN];
#pragma unroll
            for (int k = 0; k < STAGE_UN; ++k) sv[k] = lsm_ld4<NT>(wsrc, min(base + k * WAVE, wvec - 1));
#pragma unroll
            for (int k = 0; k < STAGE_UN; ++k)
                reinterpret_cast<float4*>(wtile)[min(base + k * WAVE, wvec - 1)] = sv[k];
        }
        for (int e = (wvec << 2) + lane; e < wel; e += WAVE) wtile[e] = lsm_ld1(wsrc + e);
        wave_sync_lds();
    } else {
        for (int base = tid; base < nvec; base += STAGE_UN * SM_THREADS) {
            float4 sv[STAGE_UN];
#pragma unroll
            for (int k = 0; k < STAGE_UN; ++k) sv[k] = lsm_ld4<NT>(src, min(base + k * SM_THREADS, nvec - 1));
#pragma unroll
            for (int k = 0; k < STAGE_UN; ++k)
                reinterpret_cast<float4*>(tile)[min(base + k * SM_THREADS, nvec - 1)] = sv[k];
        }
        for (int e = (nvec << 2) + tid; e < nel; e += SM_THREADS) tile[e] = lsm_ld1(src + e);   // last chunk only
        __syncthreads();
    }

    // ---- per-row max / sum(exp) / normalise: L lanes per row, lane h owns columns h, h+L, ... ----
    constexpr int RPP = SM_THREADS / L;             // rows per pass
    const int h = tid % L, rr = tid / L;
    const int ctail = h + (q - 1) * L;              // this lane's last column, may be >= V
    const bool tail_ok = ctail < V;
    // One row: the lane's q values are read ONCE into registers by a straight-line sequence (all LDS reads in flight
    // together), reduced, and -- in the modes that rewrite the row -- written back from the registers.  QC = q as a
    // compile-time constant (9 ... 16: what the launcher's choice of L gives for V > 16); the run-time loops of the first
    // version waited for every LDS read of the max pass on its own (~9 instructions and one LDS latency per element) and
    // read every element a second time for the sum.
    auto one_row = [&](auto QC, const int r) {
        constexpr int Q = decltype(QC)::value;
        float* row = tile + r * V;
        float v[Q];
#pragma unroll
        for (int i = 0; i < Q - 1; ++i) v[i] = row[h + i * L];
        v[Q - 1] = tail_ok ? row[ctail] : -__builtin_inff();
        float mx = v[0];
#pragma unroll
        for (int i = 1; i < Q; ++i) mx = fmaxf(mx, v[i]);
        mx = group_max<L>(mx);
        const float mb = -mx * LOG2E;
        float s = 0.0f;
#pragma unroll
        for (int i = 0; i < Q; ++i) s += __builtin_amdgcn_exp2f(__builtin_fmaf(v[i], LOG2E, mb));   // (exp2(-inf) = 0)
        s = group_sum<L>(s);
        const float ls = lsm_log_sum(__builtin_amdgcn_logf(s) * LN2, mx, mb);
        if constexpr (GATHER) {
            if (h == 0) stat[r] = make_float2(mx, ls);
        } else if constexpr (MODE == LSM_BWD) {
            const bool first = r == rr;                // (the row whose pair was requested up front)
            const CellMap m = first ? pm : map.at((size_t)(row0 + r), V, blank);
            const float sc = first ? psc : map.scale(bw, m);
            const float2 g = first ? pg : map.pair(bw, m);
            if constexpr (CLAMP) {
                // the clamp behind the sum and in front of the scale: the pair stays unscaled, every lane clamps and scales
                // what it writes, and lane 0 forms the two one-hot entries whole -- from the logits still in the tile --
                // and puts them over the row's behind the row pass (lsm_hot_clamped)
                const float gB = g.x, gL = g.y, gs = gB + gL;
                const float gq = gs * __builtin_amdgcn_rcpf(s);
                float hb = 0.0f, hl = 0.0f;
                if (h == 0) lsm_hot_clamped(row[blank], row[m.label], m.label == blank, mb, gq, gB, gL, bw.clamp, sc, hb, hl);
#pragma unroll
                for (int i = 0; i < Q - 1; ++i) row[h + i * L] = lsm_bwd_el_clamped(v[i], mb, gq, bw.clamp, sc);
                if (tail_ok) row[ctail] = lsm_bwd_el_clamped(v[Q - 1], mb, gq, bw.clamp, sc);
                if (h == 0) { row[blank] = hb; row[m.label] = hl; }
            } else {
                const float gB = g.x * sc, gL = g.y * sc, gs = gB + gL;
                const float gq = gs * __builtin_amdgcn_rcpf(s);      // p_j = e_j / s (lsm_log_sum)
#pragma unroll
                for (int i = 0; i < Q - 1; ++i) row[h + i * L] = lsm_bwd_el(v[i], mb, gq);
                if (tail_ok) row[ctail] = lsm_bwd_el(v[Q - 1], mb, gq);
                // the L lanes of a row sit in one wave and LDS operations of a wave retire in order
                if (h == 0) { row[blank] += gB; row[m.label] += gL; }
            }
        } else {
#pragma unroll
            for (int i = 0; i < Q - 1; ++i) row[h + i * L] = lsm_norm_el(v[i], mx, ls);
            if (tail_ok) row[ctail] = lsm_norm_el(v[Q - 1], mx, ls);
        }
    };
    auto all_rows = [&](auto QC) {
        for (int r = rr; r < nrows; r += RPP) one_row(QC, r);
    };
    switch (q) {
#define LSM_Q(QQ) case QQ: all_rows(std::integral_constant<int, QQ>{}); break;
        LSM_Q(9) LSM_Q(10) LSM_Q(11) LSM_Q(12) LSM_Q(13) LSM_Q(14) LSM_Q(15) LSM_Q(16)
#undef LSM_Q
        default:      // q <= 8 (V <= 16, or rows shorter than the lane cover): run-time loops
            for (int r = rr; r < nrows; r += RPP) {
                float* row = tile + r * V;
                float mx = -__builtin_inff();
                for (int i = 0, c = h; i < q - 1; ++i, c += L) mx = fmaxf(mx, row[c]);
                if (tail_ok) mx = fmaxf(mx, row[ctail]);
                mx = group_max<L>(mx);
                const float mb = -mx * LOG2E;
                float s = 0.0f;
                for (int i = 0, c = h; i < q - 1; ++i, c += L) s += __builtin_amdgcn_exp2f(__builtin_fmaf(row[c], LOG2E, mb));
                if (tail_ok) s += __builtin_amdgcn_exp2f(__builtin_fmaf(row[ctail], LOG2E, mb));
                s = group_sum<L>(s);
                const float ls = lsm_log_sum(__builtin_amdgcn_logf(s) * LN2, mx, mb);
                if constexpr (GATHER) {
                    if (h == 0) stat[r] = make_float2(mx, ls);
                } else if constexpr (MODE == LSM_BWD) {
                    const CellMap m = map.at((size_t)(row0 + r), V, blank);
                    const float sc = map.scale(bw, m);
                    const float2 g = map.pair(bw, m);
                    if constexpr (CLAMP) {       // (as in the straight-line form above)
                        const float gB = g.x, gL = g.y, gs = gB + gL;
                        const float gq = gs * __builtin_amdgcn_rcpf(s);
                        float hb = 0.0f, hl = 0.0f;
                        if (h == 0) lsm_hot_clamped(row[blank], row[m.label], m.label == blank, mb, gq, gB, gL, bw.clamp, sc, hb, hl);
                        for (int i = 0, c = h; i < q - 1; ++i, c += L) row[c] = lsm_bwd_el_clamped(row[c], mb, gq, bw.clamp, sc);
                        if (tail_ok) row[ctail] = lsm_bwd_el_clamped(row[ctail], mb, gq, bw.clamp, sc);
                        if (h == 0) { row[blank] = hb; row[m.label] = hl; }
                    } else {
                        const float gB = g.x * sc, gL = g.y * sc, gs = gB + gL;
                        const float gq = gs * __builtin_amdgcn_rcpf(s);      // p_j = e_j / s (lsm_log_sum)
                        for (int i = 0, c = h; i < q - 1; ++i, c += L) row[c] = lsm_bwd_el(row[c], mb, gq);
                        if (tail_ok) row[ctail] = lsm_bwd_el(row[ctail], mb, gq);
                        // the L lanes of a row sit in one wave and LDS operations of a wave retire in order
                        if (h == 0) { row[blank] += gB; row[m.label] += gL; }
                    }
                } else {
                    for (int i = 0, c = h; i < q - 1; ++i, c += L) row[c] = lsm_norm_el(row[c], mx, ls);
                    if (tail_ok) row[ctail] = lsm_norm_el(row[ctail], mx, ls);
                }
            }
    }
    if constexpr (GATHER && WP) {
        wave_sync_lds();
        for (int r = wr0 + lane; r < wr0 + wn; r += WAVE) {
            const CellMap m = map.at((size_t)(row0 + r), V, blank);
            const float2 st = stat[r];
            const float* row = tile + r * V;
            map.put(out, m, make_float2((row[blank] - st.x) - st.y, (row[m.label] - st.x) - st.y));
        }
    } else if constexpr (GATHER) {
        // one lane per row with all lanes busy (the per-row index arithmetic costs ~60 instructions;
        // doing it inside the L-lane row loop ran it with a quarter of the lanes)
        __syncthreads();
        for (int r = tid; r < nrows; r += SM_THREADS) {
            const CellMap m = map.at((size_t)(row0 + r), V, blank);
            const float2 st = stat[r];
            const float* row = tile + r * V;
            const float2 pr = make_float2((row[blank] - st.x) - st.y, (row[m.label] - st.x) - st.y);
            // (written through, sc1: +38 us at c4 -- scattered 8-byte stores need L2 to merge them.  Timing probes that sent
            // the pairs into a 64 KB region that stays in L2, or stored them in row-major order as coalesced 512-byte runs:
            // the gather's stores cost 40-55 us in any shape)
            map.put(out, m, pr);
        }
    } else if constexpr (WP) {
        wave_sync_lds();
        // the column plane (LsmBwd::col_out): the wave's rows are consecutive, so is its slice of the plane
        if constexpr (MODE == LSM_NORM) {
            if (bw.col_out)
                for (int r = lane; r < wn; r += WAVE) bw.col_out[row0 + wr0 + r] = wtile[r * V + bw.col];
        }
        LsmOut<MODE, E>* wdst = out + (row0 + wr0) * V;
        for (int i = lane; i < wvec; i += WAVE) lsm_st4<NT>(wdst, i, reinterpret_cast<const float4*>(wtile)[i]);
        for (int e = (wvec << 2) + lane; e < wel; e += WAVE) lsm_st1(wdst + e, wtile[e]);
    } else {
        __syncthreads();
        if constexpr (MODE == LSM_NORM) {      // the column plane: one contiguous run per workgroup
            if (bw.col_out)
                for (int r = tid; r < nrows; r += SM_THREADS) bw.col_out[row0 + r] = tile[r * V + bw.col];
        }
        LsmOut<MODE, E>* dst = out + row0 * V;
        for (int i = tid; i < nvec; i += SM_THREADS) lsm_st4<NT>(dst, i, reinterpret_cast<const float4*>(tile)[i]);
        for (int e = (nvec << 2) + tid; e < nel; e += SM_THREADS) lsm_st1(dst + e, tile[e]);
    }
}

// The kernels of the fused families are one template each over the map policy and CLAMP; the body is a function above its
// kernel, and takes LsmBwd by value as the kernel does (by reference the dense clamped kernels gain a branch per q).
template <typename E, int L, int MODE, bool WP, bool CLAMP, class Map>
__global__ void __launch_bounds__(SM_THREADS)
k_lsm_small(const E* x, LsmOut<MODE, E>* out, typename Map::Head head, int64_t rows, int V, int R, int q,
            typename Map::Tail tail, LsmBwd bw) {
    static_assert(!CLAMP || MODE == LSM_BWD, "the clamp is the backward's");
    lsm_small_body<E, L, MODE, WP, CLAMP>(x, out, Map::make(head, tail), rows, V, R, q, tail.blank, bw);
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
template <typename E, int MODE, int LG_THREADS, int LG_MAXVEC, bool CLAMP, class Map>
__device__ __forceinline__ void lsm_large_body(const E* x, LsmOut<MODE, E>* out, Map map, int64_t rows, int V, int blank,
                                               LsmBwd bw) {
    constexpr bool GATHER = MODE == LSM_GATHER;
    __shared__ float red[LG_THREADS / WAVE];
    // bw.xcd: every XCD (workgroups go to them by blockIdx mod 8; the grid is a multiple of 8) streams a contiguous
    // eighth of the rows instead of every eighth row -- see dispatch_lsm
    const size_t per_xcd = ((size_t)rows + 7) / 8;
    const size_t items = bw.xcd ? per_xcd * 8 : (size_t)rows;
    for (size_t it = blockIdx.x; it < items; it += gridDim.x) {
        const size_t row = bw.xcd ? (it & 7) * per_xcd + (it >> 3) : it;
        if (row >= (size_t)rows) continue;
        const E* src = x + row * V;
        const int nvec = V >> 2;
        // How a lane's LG_MAXVEC loads are issued (round 5).  As first written -- load and running maximum together under
        // `if (j < nvec)` -- every load sits in a branch of its own with an s_waitcnt vmcnt(0) behind it: LG_MAXVEC memory
        // round trips per row, one after the other.  Measured against two loads-first forms (tools/ab_kernels.py, three
        // interleaved rounds, profiles/r05_loads_first_ab.txt):
        //   * the read-mostly FUSED modes gain 5-7 % from all loads issued unconditionally at an index clamped into the row,
        //     what lies beyond the row replaced by -inf afterwards (c3: fused forward 317 -> 300 us, fused backward 739 -> 689);
        //   * the plain log-softmax -- a read and a write stream at the rate of a copy -- does not: V = 5000 629 -> 647 us,
        //     4096 596 -> 606, 2048 590 -> 594, nothing at 1000, 3000, 8192; only the three-pass covers of 768 threads and more
        //     gain (c5's V = 10000: 693 -> 674 clamped, -> 665 with the loads alone under their predicates and the maxima
        //     behind them), so those take the predicated form and everything else stays as it was.
        constexpr bool CLAMPED = MODE != LSM_NORM;      // (the load index, not the gradient)
        constexpr bool PREDICATED = MODE == LSM_NORM && LG_THREADS >= 768;
        float4 v[LG_MAXVEC];
        float mx = -__builtin_inff();
        if constexpr (CLAMPED || PREDICATED) {
#pragma unroll
            for (int i = 0; i < LG_MAXVEC; ++i) {
                const int j = (int)threadIdx.x + i * LG_THREADS;
                if constexpr (CLAMPED) {
                    v[i] = lsm_ld4<true>(src, min(j, nvec - 1));
                } else {
                    if (j < nvec) v[i] = lsm_ld4<true>(src, j);
                }
            }
        }
        // what the fused modes need besides the row, requested behind it instead of after the reductions
        [[maybe_unused]] CellMap m = {0, 0, 0};
        [[maybe_unused]] float2 side = make_float2(0.0f, 0.0f);      // GATHER: the row's (blank, label) logits; BWD: its gradient pair
        [[maybe_unused]] float sc = 1.0f;
        if constexpr (MODE != LSM_NORM) {
            map.chunk((int64_t)row, (int64_t)row);      // (compact rows: one search per row)
            m = map.at(row, V, blank);
            if constexpr (GATHER) {
                const E* xr = x + row * V;
                side = make_float2(lsm_ld1(xr + blank), lsm_ld1(xr + m.label));
            } else {
                side = map.pair(bw, m);
                sc = map.scale(bw, m);
            }
        }
#pragma unroll
        for (int i = 0; i < LG_MAXVEC; ++i) {
            const int j = (int)threadIdx.x + i * LG_THREADS;
            if constexpr (CLAMPED || PREDICATED) {
                if (j >= nvec) {
                    const float ninf = -__builtin_inff();
                    v[i] = make_float4(ninf, ninf, ninf, ninf);
                }
                mx = fmaxf(fmaxf(mx, fmaxf(v[i].x, v[i].y)), fmaxf(v[i].z, v[i].w));
            } else {
                if (j < nvec) {
                    v[i] = lsm_ld4<true>(src, j);
                    mx = fmaxf(fmaxf(mx, fmaxf(v[i].x, v[i].y)), fmaxf(v[i].z, v[i].w));
                }
            }
        }
        mx = block_reduce<LG_THREADS>(mx, true, red);
        const float mb = -mx * LOG2E;
        float s = 0.0f;
#pragma unroll
        for (int i = 0; i < LG_MAXVEC; ++i) {
            const int j = threadIdx.x + i * LG_THREADS;
            if (j < nvec)
                s += (__builtin_amdgcn_exp2f(__builtin_fmaf(v[i].x, LOG2E, mb)) + __builtin_amdgcn_exp2f(__builtin_fmaf(v[i].y, LOG2E, mb))) +
                     (__builtin_amdgcn_exp2f(__builtin_fmaf(v[i].z, LOG2E, mb)) + __builtin_amdgcn_exp2f(__builtin_fmaf(v[i].w, LOG2E, mb)));
        }
        s = block_reduce<LG_THREADS>(s, false, red);
        const float ls = lsm_log_sum(logf(s), mx, mb);
        if constexpr (GATHER) {
            if (threadIdx.x == 0) map.put(out, m, make_float2((side.x - mx) - ls, (side.y - mx) - ls));
        } else if constexpr (MODE == LSM_BWD) {
            const float2 g = side;
            // CLAMP: the pair stays unscaled -- the row is clamped behind the two additions and scaled behind the clamp
            const float gB = CLAMP ? g.x : g.x * sc, gL = CLAMP ? g.y : g.y * sc, gs = gB + gL;
            const float gq = gs / s;                                 // p_j = e_j / s (lsm_log_sum)
            LsmOut<MODE, E>* dst = out + row * V;
#pragma unroll
            for (int i = 0; i < LG_MAXVEC; ++i) {
                const int j = threadIdx.x + i * LG_THREADS;
                if (j < nvec) {
                    float o[4] = {v[i].x, v[i].y, v[i].z, v[i].w};
#pragma unroll
                    for (int cc = 0; cc < 4; ++cc) {
                        const int e = 4 * j + cc;
                        float d = lsm_bwd_el(o[cc], mb, gq);
                        d += (e == blank) ? gB : 0.0f;
                        d += (e == m.label) ? gL : 0.0f;
                        if constexpr (CLAMP) d = lsm_clamp_scale(d, bw.clamp, sc);
                        o[cc] = d;
                    }
                    lsm_st4<true>(dst, j, make_float4(o[0], o[1], o[2], o[3]));
                }
            }
        } else {
            float* dst = out + row * V;
#pragma unroll
            for (int i = 0; i < LG_MAXVEC; ++i) {
                const int j = threadIdx.x + i * LG_THREADS;
                if (j < nvec) {
                    const float4 r = make_float4(lsm_norm_el(v[i].x, mx, ls), lsm_norm_el(v[i].y, mx, ls),
                                                 lsm_norm_el(v[i].z, mx, ls), lsm_norm_el(v[i].w, mx, ls));
                    lsm_st4<true>(dst, j, r);
                    // the column plane (LsmBwd::col_out): the one lane that holds the column stores it (a row per workgroup:
                    // 4 bytes beside 4V)
                    if (bw.col_out && j == (bw.col >> 2)) {
                        const int c = bw.col & 3;
                        bw.col_out[row] = c == 0 ? r.x : (c == 1 ? r.y : (c == 2 ? r.z : r.w));
                    }
                }
            }
        }
    }
}
template <typename E, int MODE, int TH, int NV, bool CLAMP, class Map>
__global__ void __launch_bounds__(TH)
k_lsm_large(const E* x, LsmOut<MODE, E>* out, typename Map::Head head, int64_t rows, int V,
            typename Map::Tail tail, LsmBwd bw) {
    static_assert(!CLAMP || MODE == LSM_BWD, "the clamp is the backward's");
    lsm_large_body<E, MODE, TH, NV, CLAMP>(x, out, Map::make(head, tail), rows, V, tail.blank, bw);
}

// ---------------------------------------------------------------------------
// Generic fallback (any V, any alignment): one wave per row, three passes.
// ---------------------------------------------------------------------------
template <typename E, int MODE, bool CLAMP, class Map>
__device__ __forceinline__ void lsm_generic_body(const E* x, LsmOut<MODE, E>* out, Map map, int64_t rows, int V, int blank,
                                                 LsmBwd bw) {
    constexpr bool GATHER = MODE == LSM_GATHER;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int lane = threadIdx.x & 63;
    if constexpr (Map::COMPACT) map.chunk(row, row);
    const E* xr = x + row * V;
    float mx = -__builtin_inff();
    for (int c = lane; c < V; c += WAVE) mx = fmaxf(mx, lsm_ld1(xr + c));
    mx = group_max<WAVE>(mx);
    float s = 0.0f;
    for (int c = lane; c < V; c += WAVE) s += expf(lsm_ld1(xr + c) - mx);
    s = group_sum<WAVE>(s);
    const float ls = logf(s);
    if constexpr (GATHER) {
        if (lane == 0) {
            const CellMap m = map.at((size_t)row, V, blank);
            map.put(out, m, make_float2((lsm_ld1(xr + blank) - mx) - ls, (lsm_ld1(xr + m.label) - mx) - ls));
        }
    } else if constexpr (MODE == LSM_BWD) {
        const CellMap m = map.at((size_t)row, V, blank);
        const float sc = map.scale(bw, m);
        const float2 g = map.pair(bw, m);
        // CLAMP: the pair stays unscaled -- the row is clamped behind the two additions and scaled behind the clamp
        const float gB = CLAMP ? g.x : g.x * sc, gL = CLAMP ? g.y : g.y * sc, gs = gB + gL;
        LsmOut<MODE, E>* o = out + row * V;
        for (int c = lane; c < V; c += WAVE) {
            float d = -expf((lsm_ld1(xr + c) - mx) - ls) * gs;
            d += (c == blank) ? gB : 0.0f;
            d += (c == m.label) ? gL : 0.0f;
            if constexpr (CLAMP) d = lsm_clamp_scale(d, bw.clamp, sc);
            lsm_st1(o + c, d);
        }
    } else {
        float* o = out + row * V;
        for (int c = lane; c < V; c += WAVE) {
            const float r = (lsm_ld1(xr + c) - mx) - ls;
            o[c] = r;
            if (bw.col_out && c == bw.col) bw.col_out[row] = r;      // the column plane (LsmBwd::col_out)
        }
    }
}
template <typename E, int MODE, bool CLAMP, class Map>
__global__ void __launch_bounds__(256)
k_lsm_generic(const E* x, LsmOut<MODE, E>* out, typename Map::Head head, int64_t rows, int V,
              typename Map::Tail tail, LsmBwd bw) {
    static_assert(!CLAMP || MODE == LSM_BWD, "the clamp is the backward's");
    lsm_generic_body<E, MODE, CLAMP>(x, out, Map::make(head, tail), rows, V, tail.blank, bw);
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
            const float4 t = lsm_ld4<lsm_nt(MODE)>(src[p], off);
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
template <typename E, int L, int Q, class Map>
__device__ __forceinline__ void lsm_rows_body(const E* x, float* out, Map map, int64_t rows, int V, int blank) {
    constexpr int MODE = LSM_GATHER, VEC = 4;
    constexpr int UN = RowsShape<L>::UN, RW = RowsShape<L>::RW, RPW = RowsShape<L>::RPW;
    const int lane = threadIdx.x & 63, h = lane % L, rr = lane / L;
    // wave-uniform values kept in scalar registers (the 64-bit row arithmetic runs on the scalar unit)
    const int64_t row0 = ((int64_t)stream_block() * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6)) * RPW;
    if (row0 >= rows) return;
    const bool last_ok = (h + (Q - 1) * L) * VEC < V;   // the lane's last float4 is part of the row
    const bool whole = row0 + RPW <= rows;              // (uniform) every row of this wave exists
    if constexpr (Map::COMPACT) map.chunk(row0, min(row0 + RPW, rows) - 1);
    const E* const wave_src = x + row0 * V;
    const unsigned lane_off = (unsigned)rr * (unsigned)V + (unsigned)h * VEC;      // floats inside a pass
    // lane l < RPW owns the pair of row row0 + l.  Its two logits are requested FIRST, next to the row loads that bring
    // the same lines (asked for after the rows have streamed through, they are fetched a second time: forward 252 vs 216
    // us at V = 128, profiles/r04_lsm_rows_ab.txt)
    CellMap cm = {0, 0, 0};
    float xb = 0.0f, xl = 0.0f;
    const bool own = lane < RPW && row0 + lane < rows;
    if (own) {
        cm = map.at((size_t)(row0 + lane), V, blank);
        const E* xr = x + (row0 + lane) * V;
        xb = lsm_ld1(xr + blank);
        xl = lsm_ld1(xr + cm.label);
    }
    const E* src[UN];
#pragma unroll
    for (int p = 0; p < UN; ++p) {
        src[p] = wave_src + (size_t)(p * RW) * V + lane_off;
        // (rows past the end of the tensor -- last wave only -- re-read the last row and are dropped at the stores)
        if (!whole && row0 + p * RW + rr >= rows) src[p] = x + (rows - 1) * V + h * VEC;
    }
    float mx[UN], ls[UN];
    lsm_rows_stats<E, L, Q, MODE>(src, last_ok, mx, ls);
    float m, lg;
    lsm_rows_stats_of_lane<L>(lane, mx, ls, m, lg);
    if (own) map.put(out, cm, make_float2((xb - m) - lg, (xl - m) - lg));
}
template <typename E, int L, int Q, class Map>
__global__ void __launch_bounds__(256)
k_lsm_rows(const E* x, float* out, typename Map::Head head, int64_t rows, int V, typename Map::Tail tail) {
    lsm_rows_body<E, L, Q>(x, out, Map::make(head, tail), rows, V, tail.blank);
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

// What the plan says, launched: a switch on the family and on its template selectors, nothing decided here.
// E: the storage type of x (and of out in LSM_BWD).  Map: the row -> cell policy (DenseMap, CompactMap).  CLAMP: the clamped
// instantiation of the plan's kernel (LSM_BWD, whose plans name SMALL, LARGE or GENERIC), in the same launch shape.
template <int MODE, typename E, bool CLAMP, class Map>
static hipError_t launch_lsm_plan(hipStream_t stream, const LsmPlan& p, const E* x, LsmOut<MODE, E>* out, const Map& map,
                                  int64_t rows, int V, int blank, LsmBwd bw) {
    bw.xcd = p.xcd;
    const typename Map::Head head = map.head();
    const typename Map::Tail tail = map.tail(blank);
#define LSM_LARGE(TH_, NV_)         \
    if (p.TH == TH_ && p.NV == NV_) \
        k_lsm_large<E, MODE, TH_, NV_, CLAMP, Map><<<p.grid, TH_, 0, stream>>>(x, out, head, rows, V, tail, bw);
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
    if (p.L == LL && p.Q == QQ) k_lsm_rows<E, LL, QQ, Map><<<p.grid, 256, 0, stream>>>(x, out, head, rows, V, tail);
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
#define LSM_SMALL_WP(LL, WP_)                                                                                  \
    k_lsm_small<E, LL, MODE, WP_, CLAMP, Map><<<p.grid, SM_THREADS, p.lds_bytes, stream>>>(x, out, head, rows, V, p.R, p.q, \
                                                                                           tail, bw)
#define LSM_SMALL(LL)                          \
    case LL:                                   \
        if (p.WP) LSM_SMALL_WP(LL, (LL <= 16)); \
        else LSM_SMALL_WP(LL, false);          \
        break;
            switch (p.L) {
                LSM_SMALL(1) LSM_SMALL(2) LSM_SMALL(4) LSM_SMALL(8) LSM_SMALL(16) LSM_SMALL(32)
                LSM_SMALL(64)
            }
#undef LSM_SMALL
#undef LSM_SMALL_WP
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
            k_lsm_generic<E, MODE, CLAMP, Map><<<p.grid, 256, 0, stream>>>(x, out, head, rows, V, tail, bw);
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
    // clamp > 0: the CLAMP instantiations (LsmBwd::clamp); 0: the kernels that have always been here
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
