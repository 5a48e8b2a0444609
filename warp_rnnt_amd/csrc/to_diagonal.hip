// The dense layout turns around the lattice sweep: the gather of the (blank, label) log-prob pair per cell
// (reference: warp_rnnt/__init__.py:118-128) and the re-layout of row-major pairs into the diagonal-major float2
// workspace (common.h) that the sweep reads with coalesced row loads, and the way back.
#include <cstdlib>

#include "streaming.h"

namespace rnnt {

// ---------------------------------------------------------------------------
// To-diagonal kernels: dense log-probs (gather) or row-major pairs (re-layout) ->
// diagonal-major (blank,label) pairs.  A workgroup owns a 32x32 (t,u) tile of one
// utterance: it reads the tile with lanes along u (the contiguous axis of the
// source), parks it in LDS, and writes it back diagonal by diagonal, so that
// every store instruction covers contiguous runs of up to 32 pairs (256 B) of a
// diagonal-major row.  (One thread per cell writing its pair directly costs 4.6x
// write amplification: rocprofv3 WRITE_SIZE 268 MB for a 57.6 MB output.)
// ---------------------------------------------------------------------------
// Tiles are walked from the END of the tensor to its beginning: in the caller's step the kernel in front of this one
// is the log-softmax that has just written these log-probs front to back, and the last ~130-190 MB of what a
// streaming kernel wrote are still in the 256 MB Infinity Cache (tools/ubench/mall_probe.hip: 128 MB read back from
// the end of a freshly written 1.44 GB tensor in 22 us, from its beginning in 33-45 us).  Worth 8 us of the c4 step
// (0.4237 -> 0.4157 ms for the loss entry inside bench.py, three interleaved runs each); nothing on a tensor that
// was not just written (252 vs 249 us alone) -- which is how round 1 measured it and found no change.

// The dense gather's pair stores are written THROUGH (sc1) -- round 6: what its 58 MB of stores cost is dirty lines on their
// way out of L2 holding back the fills of the read stream; written through, nothing is left dirty: the kernel
// alone 252.0 -> 247.6 us (tools/ubench/gather_r06.hip), inside bench.py's c4 step 0.2215 -> 0.2182 ms (four interleaved
// pairs, profiles/r06_gather_sc1_ab.txt).  sc0 sc1 the same, nt / sc0 sc1 nt worse.
constexpr int TT = 32;   // frames per tile of k_to_diagonal (columns: TD)

// The preparation of the ring kernel that follows in the same call (kernels.h: RingPrep; lattice_wd.hip: k_prepare is the
// stand-alone form), carried out at the tail of a producer's workgroups: every workgroup zeroes its slice of the rings,
// the first one clears the flags and the queue head and takes the next value of the device's launch counter.  Everything
// is complete when the producer's launch is, i.e. before the ring kernel starts.
__device__ __forceinline__ void fold_ring_prepare(const RingPrep& p) {
    const size_t per = (p.ring_vec + gridDim.x - 1) / gridDim.x;
    const size_t lo = (size_t)blockIdx.x * per;
    const size_t hi = lo + per < p.ring_vec ? lo + per : p.ring_vec;
    const uint4 z = make_uint4(0, 0, 0, 0);
    for (size_t i = lo + threadIdx.x; i < hi; i += blockDim.x) p.rings[i] = z;
    if (blockIdx.x == 0) {
        for (int i = threadIdx.x; i < p.n_flags; i += blockDim.x) p.flags[i] = 0;
        if (threadIdx.x == 0) p.flags[p.n_flags] = (int)(atomicAdd(p.counter, 1u) + 1u);
    }
}

// PLANE (dense only): the blank log-prob of every cell comes from a contiguous (N,T,U) plane that the log-softmax in front
// wrote beside its rows (lsm.h: LsmBwd::col_out) -- a coalesced 4-byte load along u -- and only the label's dword is fetched
// from the row.  For rows longer than a line the two dwords touch 10.0 M of c4's 11.25 M lines, the label's alone 7.2 M
// (DESIGN.md 3.5): 0.36 GB of reads less for 28.8 MB more.  Same policy otherwise: non-temporal row loads, tiles from
// the end, pairs written through.
template <bool DENSE, int TTK, bool PLANE>
__global__ void __launch_bounds__(256)
k_to_diagonal(const float* __restrict__ src, const int* __restrict__ labels, float2* __restrict__ ws2,
              int T, int U, int V, int blank, int tiles_t, int tiles_u, const RingPrep prep,
              const float* __restrict__ blank_plane) {
    static_assert(DENSE || !PLANE, "the blank plane belongs to the dense gather");
    __shared__ float2 tile[TTK][TD];
    unsigned b = DENSE ? gridDim.x - 1 - blockIdx.x : blockIdx.x;
    const int tu = b % tiles_u; b /= tiles_u;
    const int tt = b % tiles_t;
    const int n = b / tiles_t;
    const int t0 = tt * TTK, u0 = tu * TD;
    const int ul = threadIdx.x & (TD - 1), tl0 = threadIdx.x >> 5;   // 8 rows of 32 lanes
    const int u = u0 + ul;
    const size_t nbase = (size_t)n * T * U;
    int lab = blank;
    if (DENSE && u < U - 1) lab = safe_label(labels[(size_t)n * (U - 1) + u], V, blank);
#pragma unroll
    for (int k = 0; k < TTK / 8; ++k) {
        const int tl = tl0 + 8 * k, t = t0 + tl;
        if (t < T && u < U) {
            const size_t cell = nbase + (size_t)t * U + u;
            if constexpr (DENSE) {
                // Two dwords of a 4V-byte row: the memory system fetches whole 128-byte lines (a one-dword-per-line
                // probe over the same tensor takes as long as reading all of it, tools/ubench/gather_variants.hip),
                // so this kernel streams ~1.4 lines per cell and none of them is touched again: non-temporal loads
                // (206 vs 227 us for the probe, 205-229 vs 227-255 us here, box to box).
                const float* p = src + cell * (size_t)V;
                if constexpr (PLANE)
                    tile[tl][ul] = make_float2(blank_plane[cell], __builtin_nontemporal_load(p + lab));
                else
                    tile[tl][ul] = make_float2(__builtin_nontemporal_load(p + blank), __builtin_nontemporal_load(p + lab));
            } else {
                tile[tl][ul] = reinterpret_cast<const float2*>(src)[cell];
            }
        }
    }
    __syncthreads();
    // diagonal d of the tile holds cells (tl = d - ul, ul): consecutive ul = consecutive pairs of
    // row (t0+u0+d) mod T of the diagonal-major plane
#pragma unroll
    for (int k = 0; k < (TTK + TD + 7) / 8; ++k) {
        const int d = tl0 + 8 * k;
        const int tl = d - ul;
        if (d < TTK + TD - 1 && tl >= 0 && tl < TTK) {
            const int t = t0 + tl;
            if (t < T && u < U) {
                int r = t + u;
                r = r >= T ? r % T : r;
                // written THROUGH (agent scope): nothing is left dirty in L2 for the read stream's fills to wait behind
                // (tools/ubench/gather_r06.hip: 247.6 vs 252.0 us alone)
                if constexpr (DENSE) {
                    asm volatile("global_store_dwordx2 %0, %1, off sc1" ::"v"(ws2 + nbase + (size_t)r * U + u), "v"(tile[tl][ul]) : "memory");
                } else {
                    ws2[nbase + (size_t)r * U + u] = tile[tl][ul];
                }
            }
        }
    }
    if (prep.flags) fold_ring_prepare(prep);
}

// Row-major (N,T,U,2) gather (what the reference's wrapper builds): one thread per cell.
__global__ void __launch_bounds__(256)
k_gather_rowmajor(const float* __restrict__ lp, const int* __restrict__ labels, float2* __restrict__ out2,
                  size_t cells, int T, int U, int V, int blank) {
    const size_t cell = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (cell >= cells) return;
    const CellMap m = map_cell(cell, labels, T, U, V, blank);
    const float* p = lp + cell * (size_t)V;
    out2[cell] = make_float2(p[blank], p[m.label]);
}

template <int TTK>
static hipError_t launch_to_diagonal_tt(hipStream_t stream, const float* src, const int* labels, float* ws2,
                                        int N, int T, int U, int V, int blank, bool dense, const RingPrep& prep,
                                        const float* blank_plane) {
    const int tiles_t = (T + TTK - 1) / TTK, tiles_u = (U + TD - 1) / TD;
    const size_t nblk = (size_t)N * tiles_t * tiles_u;
    if (nblk >= ((size_t)1 << 31)) return hipErrorInvalidValue;
    if (dense && blank_plane)
        k_to_diagonal<true, TTK, true><<<(unsigned)nblk, 256, 0, stream>>>(src, labels, reinterpret_cast<float2*>(ws2), T,
                                                                           U, V, blank, tiles_t, tiles_u, prep, blank_plane);
    else if (dense)
        k_to_diagonal<true, TTK, false><<<(unsigned)nblk, 256, 0, stream>>>(src, labels, reinterpret_cast<float2*>(ws2), T,
                                                                            U, V, blank, tiles_t, tiles_u, prep, nullptr);
    else
        k_to_diagonal<false, TTK, false><<<(unsigned)nblk, 256, 0, stream>>>(src, labels, reinterpret_cast<float2*>(ws2), T,
                                                                             U, 2, 0, tiles_t, tiles_u, prep, nullptr);
    return hipGetLastError();
}

static hipError_t launch_to_diagonal(hipStream_t stream, const float* src, const int* labels, float* ws2,
                                     int N, int T, int U, int V, int blank, bool dense, const RingPrep* prep_in,
                                     const float* blank_plane = nullptr) {
    const RingPrep prep = prep_in ? *prep_in : RingPrep{nullptr, 0, nullptr, nullptr, 0};
    if ((size_t)N * T * U == 0) return hipSuccess;
    // Small problems: 32-frame tiles do not even give every CU one workgroup (c2: 94 tiles for 256 CUs); 8-frame tiles --
    // one cell per thread -- quadruple the workgroups (RNNT_GATHER_SMALL_TILES=0 / 1 forces one or the other, for A/B runs)
    static const int force = ab_getenv("RNNT_GATHER_SMALL_TILES") ? atoi(ab_getenv("RNNT_GATHER_SMALL_TILES")) : -1;
    const size_t tiles32 = (size_t)N * ((T + TT - 1) / TT) * ((U + TD - 1) / TD);
    // (dense entry, us per call, 32- / 8-frame tiles: c2 28.1 / 27.4, N=32 35.1 / 33.2, N=64 46.2 / 45.2, N=128 67.1 / 68.1)
    const bool small_tiles = force >= 0 ? force != 0 : tiles32 < 512;
    if (small_tiles) return launch_to_diagonal_tt<8>(stream, src, labels, ws2, N, T, U, V, blank, dense, prep, blank_plane);
    return launch_to_diagonal_tt<TT>(stream, src, labels, ws2, N, T, U, V, blank, dense, prep, blank_plane);
}

// (Round 5 tried the dense gather as a coalesced STREAM for V <= 64, where the two dwords per row touch nearly every
//  128-byte line anyway: the LDS-staged log-softmax kernel without its arithmetic, pairs picked out of the staged tile.
//  Bit-identical, and slower: c4 274 us against 250 for k_to_diagonal in the same runs, loss path 0.403 vs 0.384 ms
//  -- a stream pays for all 1.44 GB, the scattered requests for the ~0.9 of the lines they touch.)
hipError_t launch_gather(hipStream_t stream, const float* log_probs, const int* labels, float* out2,
                         int N, int T, int U, int V, int blank, bool skewed, const RingPrep* prep,
                         const float* blank_plane) {
    const size_t cells = (size_t)N * T * U;
    if (cells == 0) return hipSuccess;
    if (skewed) return launch_to_diagonal(stream, log_probs, labels, out2, N, T, U, V, blank, true, prep, blank_plane);
    k_gather_rowmajor<<<(unsigned)((cells + 255) / 256), 256, 0, stream>>>(
        log_probs, labels, reinterpret_cast<float2*>(out2), cells, T, U, V, blank);
    return hipGetLastError();
}

hipError_t launch_reskew(hipStream_t stream, const float* lp2_rowmajor, float* ws2, int N, int T, int U,
                         const RingPrep* prep) {
    return launch_to_diagonal(stream, lp2_rowmajor, nullptr, ws2, N, T, U, 2, 0, false, prep);
}

// The way back: diagonal-major pairs -> row-major (N,T,U,2), the same 32x32 tiles walked the other way round (read by
// diagonals: consecutive lanes = consecutive pairs of a diagonal-major row; written by frames).  SPLIT: the two
// channels come from two float planes (the reference-named C entry points park the gradient pairs in the caller's
// alphas / betas buffers while the (N,T,U,2) output is still their staging area, api.hip).
template <bool SPLIT>
__global__ void __launch_bounds__(256)
k_from_diagonal(const float* __restrict__ a, const float* __restrict__ b, float2* __restrict__ out2, int T, int U,
                int tiles_t, int tiles_u) {
    __shared__ float2 tile[TT][TD + 1];
    unsigned blk = blockIdx.x;
    const int tu = blk % tiles_u; blk /= tiles_u;
    const int tt = blk % tiles_t;
    const int n = blk / tiles_t;
    const int t0 = tt * TT, u0 = tu * TD;
    const int ul = threadIdx.x & (TD - 1), tl0 = threadIdx.x >> 5;
    const int u = u0 + ul;
    const size_t nbase = (size_t)n * T * U;
    // LOADS FIRST (round 5: under their conditions the eight diagonals of a thread were eight memory round trips, one
    // after the other).  Every diagonal is loaded, at tile and lattice coordinates clamped into range -- a clamped slot
    // receives the value of the cell it stands for, so the LDS writes need no condition either.
    constexpr int ND = (TT + TD + 7) / 8;
    float2 pr[ND];
    int tls[ND];
    const int uc = min(u, U - 1);
#pragma unroll
    for (int k = 0; k < ND; ++k) {
        tls[k] = min(max(tl0 + 8 * k - ul, 0), TT - 1);
        const int t = min(t0 + tls[k], T - 1);
        int r = t + uc;
        r = r >= T ? r % T : r;
        const size_t at = nbase + (size_t)r * U + uc;
        pr[k] = SPLIT ? make_float2(a[at], b[at]) : reinterpret_cast<const float2*>(a)[at];
    }
#pragma unroll
    for (int k = 0; k < ND; ++k) tile[tls[k]][ul] = pr[k];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < TT / 8; ++k) {
        const int tl = tl0 + 8 * k, t = t0 + tl;
        if (t < T && u < U) out2[nbase + (size_t)t * U + u] = tile[tl][ul];
    }
}

hipError_t launch_unskew(hipStream_t stream, const float* a, const float* b, float* out2_rowmajor, int N, int T, int U) {
    if ((size_t)N * T * U == 0) return hipSuccess;
    const int tiles_t = (T + TT - 1) / TT, tiles_u = (U + TD - 1) / TD;
    const size_t nblk = (size_t)N * tiles_t * tiles_u;
    if (nblk >= ((size_t)1 << 31)) return hipErrorInvalidValue;
    if (b)
        k_from_diagonal<true><<<(unsigned)nblk, 256, 0, stream>>>(a, b, reinterpret_cast<float2*>(out2_rowmajor), T, U,
                                                                  tiles_t, tiles_u);
    else
        k_from_diagonal<false><<<(unsigned)nblk, 256, 0, stream>>>(a, nullptr, reinterpret_cast<float2*>(out2_rowmajor),
                                                                   T, U, tiles_t, tiles_u);
    return hipGetLastError();
}

// (blank, label) pairs -> two planes, same cell order (a plain stream: 8 bytes in, 2 x 4 out per cell)
__global__ void __launch_bounds__(256)
k_split_pairs(const float4* __restrict__ src, float2* __restrict__ a, float2* __restrict__ b, size_t n2, const float2* tail,
              float* ta, float* tb) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n2) {
        const float4 v = src[i];                  // two cells
        a[i] = make_float2(v.x, v.z);
        b[i] = make_float2(v.y, v.w);
    } else if (i == n2 && tail) {                 // an odd last cell
        const float2 v = *tail;
        *ta = v.x; *tb = v.y;
    }
}

hipError_t launch_split_pairs(hipStream_t stream, const float* pairs, float* a, float* b, size_t cells) {
    if (cells == 0) return hipSuccess;
    const size_t n2 = cells / 2;
    const bool odd = cells & 1;
    const bool al = (reinterpret_cast<uintptr_t>(pairs) % 16 == 0) && (reinterpret_cast<uintptr_t>(a) % 8 == 0) &&
                    (reinterpret_cast<uintptr_t>(b) % 8 == 0);
    if (!al) return hipErrorInvalidValue;
    k_split_pairs<<<(unsigned)((n2 + 1 + 255) / 256), 256, 0, stream>>>(
        reinterpret_cast<const float4*>(pairs), reinterpret_cast<float2*>(a), reinterpret_cast<float2*>(b), n2,
        odd ? reinterpret_cast<const float2*>(pairs) + (cells - 1) : nullptr, a + (cells - 1), b + (cells - 1));
    return hipGetLastError();
}

}  // namespace rnnt
