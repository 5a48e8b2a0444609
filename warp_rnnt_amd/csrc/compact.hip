// Helpers of the compact (ragged packed) layout: gathers, the 32-bit layout turns of the reference-named entry, offsets
// and launch bounds of a batch, zeroing behind a refused one.
#include <climits>
#include <cstdlib>
#include <algorithm>

#include "streaming.h"

namespace rnnt {

// ---------------------------------------------------------------------------
// Compact (ragged packed) layout, reference: core_compact.cu:403-436 (gather) and
// :456-484 (scatter backward).  log-probs are (STU, V) rows, utterance n owning
// rows [offs[n], offs[n+1]) as a (T_n, U_n) row-major block; labels are packed (sum yn,).
// The gather produces the diagonal-major pairs of each utterance's own (T_n,U_n) plane
// (same 32x32 tile scheme as k_to_diagonal) plus `loc`, the vocabulary index the label
// channel was taken from (blank on the last column), which the backward scatter needs.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_gather_compact(const float* __restrict__ xs, const int* __restrict__ ys, const int* __restrict__ xn,
                 const int* __restrict__ yn, const int64_t* __restrict__ offs,
                 const int* __restrict__ label_offs, float2* __restrict__ ws2, int64_t* __restrict__ loc,
                 int V, int blank, int tiles_t, int tiles_u, int N, int plain_order) {
    __shared__ float2 tile[TD][TD];
    // The grid covers the batch maxima, so a ragged batch has tiles that lie outside their utterance and return at once.
    // Workgroups go to the eight XCDs by blockIdx mod 8: with the tile column as the fastest index (tiles_u = 4 at U = 100)
    // two XCDs would get nothing but last-column tiles, nearly all of them dead.  The utterance is the fastest index
    // instead, skewed by the tile so that no XCD keeps the same utterances (N=32, T=500, U=100, V=128, lengths 50-100 %:
    // whole calls: N=64, T=500, U=100 173 -> 150 us, N=32, T=1000, U=100 194 -> 180, nothing at N=32, T=500, U=100; profiles/r04_compact_gather_order_ab.txt).
    unsigned b = blockIdx.x;
    int n, tt, tu;
    if (plain_order) {
        tu = b % tiles_u; b /= tiles_u;
        tt = b % tiles_t;
        n = b / tiles_t;
    } else {
        const unsigned rest = b / (unsigned)N;
        n = (int)((b % (unsigned)N + rest) % (unsigned)N);
        tu = rest % tiles_u;
        tt = rest / tiles_u;
    }
    const int T = xn[n], U = yn[n] + 1;
    const int t0 = tt * TD, u0 = tu * TD;
    if (t0 >= T || u0 >= U) return;                    // whole tile outside this utterance (uniform)
    const int ul = threadIdx.x & (TD - 1), tl0 = threadIdx.x >> 5;
    const int u = u0 + ul;
    const size_t nbase = (size_t)offs[n];
    int lab = blank;
    if (u < U - 1) lab = safe_label(ys[label_offs[n] + u], V, blank);
#pragma unroll
    for (int k = 0; k < TD / 8; ++k) {
        const int tl = tl0 + 8 * k, t = t0 + tl;
        if (t < T && u < U) {
            const size_t cell = nbase + (size_t)t * U + u;
            const float* p = xs + cell * (size_t)V;      // (non-temporal: see k_to_diagonal)
            tile[tl][ul] = make_float2(__builtin_nontemporal_load(p + blank), __builtin_nontemporal_load(p + lab));
            if (loc) loc[cell] = lab;
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < (2 * TD) / 8; ++k) {
        const int d = tl0 + 8 * k;
        const int tl = d - ul;
        if (d < 2 * TD - 1 && tl >= 0 && tl < TD) {
            const int t = t0 + tl;
            if (t < T && u < U) {
                int r = t + u;
                r = r >= T ? r % T : r;
                ws2[nbase + (size_t)r * U + u] = tile[tl][ul];
            }
        }
    }
}

// The same gather over the LIVE cells in their packed order: workgroup b takes cells [1024 b, 1024 b + 1024) of the
// (STU, V) tensor whatever utterances they belong to -- no tile outside its utterance, no partly filled tile, every
// workgroup the same amount of work (the tiled kernel above reaches 0.44-0.53 of the line rate on ragged batches of
// 0.1-0.4 GB because its grid covers the batch maxima: profiles/r04_shape_map.md).  Every lane reads its two dwords from
// a row of its own either way, so nothing is lost on the read side; the pairs leave as scattered 8-byte stores (the
// tiles write runs of up to 256 bytes), loc as one coalesced stream.
constexpr int GCL_CELLS = 4;       // cells per thread
__global__ void __launch_bounds__(256)
k_gather_compact_linear(const float* __restrict__ xs, const int* __restrict__ ys, const int* __restrict__ xn,
                        const int* __restrict__ yn, const int64_t* __restrict__ offs,
                        const int* __restrict__ label_offs, float2* __restrict__ ws2, int64_t* __restrict__ loc,
                        int V, int blank, int N, int64_t STU) {
    __shared__ int s_n0, s_n1;
    const int tid = threadIdx.x;
    const int64_t c0 = (int64_t)blockIdx.x * (256 * GCL_CELLS);
    // The utterances the chunk's first and last cell belong to: owner(c) = the first n with offs[n + 1] > c, by binary
    // search (two lanes, <= 17 steps over an array that sits in L2; the first version had every workgroup scan all N + 1
    // offsets).  Utterances without cells are never an owner; a refused batch -- every checked length 0 -- is dropped
    // cell by cell below.  offs must be non-decreasing for the result to mean anything; for a malformed array the search
    // still ends, on one well-defined utterance, and a cell outside that utterance's range is nobody's.
    if (tid < 2) {
        const int64_t c = tid == 0 ? c0 : min(c0 + 256 * GCL_CELLS, STU) - 1;
        int lo = 0, hi = N;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (offs[mid + 1] > c) hi = mid; else lo = mid + 1;
        }
        if (tid == 0) s_n0 = lo; else s_n1 = lo;
    }
    __syncthreads();
    const int n0 = s_n0, n1 = min(s_n1, N - 1);
    if (n0 >= N) return;
    float2 pair[GCL_CELLS];
    size_t dst[GCL_CELLS];
    int labs[GCL_CELLS];
    bool live[GCL_CELLS];
#pragma unroll
    for (int k = 0; k < GCL_CELLS; ++k) {
        const int64_t c = c0 + tid + 256 * k;
        live[k] = false;
        pair[k] = make_float2(0.0f, 0.0f);
        dst[k] = 0;
        labs[k] = blank;
        if (c >= STU) continue;
        int n = n0, hi = n1;                           // owner(c) within [n0, n1]: usually no step, or one
        while (n < hi) {
            const int mid = (n + hi) >> 1;
            if (offs[mid + 1] > c) hi = mid; else n = mid + 1;
        }
        if (c >= offs[n + 1] || c < offs[n]) continue;  // (malformed offsets: nobody's cell)
        const int T = xn[n], U = yn[n] + 1;
        if (T < 1 || U < 1) continue;
        const unsigned local = (unsigned)(c - offs[n]);
        const unsigned t = local / (unsigned)U;
        const int u = (int)(local - t * (unsigned)U);
        if ((int)t >= T) continue;
        if (u < U - 1) labs[k] = safe_label(ys[label_offs[n] + u], V, blank);
        const float* p = xs + (size_t)c * (size_t)V;
        pair[k] = make_float2(__builtin_nontemporal_load(p + blank), __builtin_nontemporal_load(p + labs[k]));
        int r = (int)t + u;
        r = r >= T ? r % T : r;
        dst[k] = (size_t)offs[n] + (size_t)r * U + u;
        live[k] = true;
    }
#pragma unroll
    for (int k = 0; k < GCL_CELLS; ++k) {
        if (!live[k]) continue;
        ws2[dst[k]] = pair[k];
        if (loc) loc[c0 + tid + 256 * k] = labs[k];
    }
}

hipError_t launch_gather_compact(hipStream_t stream, const float* xs, const int* ys, const int* xn,
                                 const int* yn, const int64_t* offs, const int* label_offs, float* ws2,
                                 int64_t* loc, int N, int Tmax, int Umax, int V, int blank, int64_t STU) {
    if (N <= 0 || Tmax <= 0 || Umax <= 0) return hipSuccess;
    // RNNT_COMPACT_GATHER=tiles|linear pins one of the two kernels (A/B runs)
    static const char* pin = ab_getenv("RNNT_COMPACT_GATHER");
    const bool want_linear = pin ? pin[0] == 'l' : true;
    if (want_linear && STU > 0 && N <= 4096) {
        const int64_t nblk = (STU + 256 * GCL_CELLS - 1) / (256 * GCL_CELLS);
        if (nblk < ((int64_t)1 << 31)) {
            k_gather_compact_linear<<<(unsigned)nblk, 256, 0, stream>>>(xs, ys, xn, yn, offs, label_offs,
                                                                        reinterpret_cast<float2*>(ws2), loc, V, blank,
                                                                        N, STU);
            return hipGetLastError();
        }
    }
    const int tiles_t = (Tmax + TD - 1) / TD, tiles_u = (Umax + TD - 1) / TD;
    const size_t nblk = (size_t)N * tiles_t * tiles_u;
    if (nblk >= ((size_t)1 << 31)) return hipErrorInvalidValue;
    static const bool plain_order = ab_getenv("RNNT_COMPACT_PLAIN_TILE_ORDER") != nullptr;      // A/B runs
    k_gather_compact<<<(unsigned)nblk, 256, 0, stream>>>(xs, ys, xn, yn, offs, label_offs,
                                                         reinterpret_cast<float2*>(ws2), loc, V, blank,
                                                         tiles_t, tiles_u, N, plain_order ? 1 : 0);
    return hipGetLastError();
}

// The reference's own compact gather (core_compact.cu:403-450, run_gather_for_compact): ROW-MAJOR packed pairs
// (STU,2) and loc (STU,), 32-bit exclusive offsets.  One thread per cell; serves the core.h shims of api.hip.
__global__ void __launch_bounds__(256)
k_gather_compact_rowmajor(const float* __restrict__ xs, const int* __restrict__ ys, const unsigned* __restrict__ xn,
                          const unsigned* __restrict__ yn, float2* __restrict__ out2, int64_t* __restrict__ loc,
                          const unsigned* __restrict__ mem_pref, const unsigned* __restrict__ label_pref, unsigned V,
                          unsigned blank) {
    const unsigned n = blockIdx.y;
    const unsigned Tn = xn[n], Un = yn[n] + 1;
    if ((int)Tn < 1 || (int)Un < 1) return;
    const unsigned c = blockIdx.x * 256u + threadIdx.x;
    if (c >= Tn * Un) return;
    const unsigned u = c % Un;
    const size_t index = (size_t)mem_pref[n] + c;
    const int l = (u == Un - 1) ? (int)blank : safe_label(ys[label_pref[n] + u], (int)V, (int)blank);
    const float* p = xs + index * (size_t)V;
    out2[index] = make_float2(p[blank], p[l]);
    loc[index] = l;
}

hipError_t launch_gather_compact_rowmajor(hipStream_t stream, const float* xs, const int* ys, const unsigned* xn,
                                          const unsigned* yn, float* gather_xs, int64_t* loc, const unsigned* mem_pref,
                                          const unsigned* label_pref, unsigned N, unsigned T, unsigned U, unsigned V,
                                          unsigned blank) {
    if (N == 0 || T == 0 || U == 0) return hipSuccess;
    const unsigned long long tiles = ((unsigned long long)T * U + 255ull) / 256ull;
    if (tiles >= (1ull << 31) || N > 65535u) return hipErrorInvalidValue;
    k_gather_compact_rowmajor<<<dim3((unsigned)tiles, N), 256, 0, stream>>>(
        xs, ys, xn, yn, reinterpret_cast<float2*>(gather_xs), loc, mem_pref, label_pref, V, blank);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------
// Layout turns of the staged form of run_warp_rnnt_compact (api.hip): the reference's compact tensors are ROW-MAJOR
// packed pairs with 32-bit exclusive prefixes (no total: the last utterance's size closes the batch), the tuned kernels
// want each utterance's own diagonal-major plane.  Same 32x32 LDS tiles as k_to_diagonal / k_from_diagonal, one grid over
// (utterance, tile) with the utterance as the fastest index (tiles outside their utterance return at once).
//   TO_DIAGONAL: src = row-major pairs -> dst = diagonal-major pairs
//   otherwise:   (sa, sb) = the two channels as diagonal-major float planes -> dst = row-major pairs
// ---------------------------------------------------------------------------------------------------------
template <bool TO_DIAGONAL>
__global__ void __launch_bounds__(256)
k_turn_compact32(const float2* __restrict__ src, const float* __restrict__ sa, const float* __restrict__ sb,
                 float2* __restrict__ dst, const unsigned* __restrict__ xn, const unsigned* __restrict__ yn,
                 const unsigned* __restrict__ mem_pref, int tiles_u, unsigned N) {
    __shared__ float2 tile[TD][TD + 1];
    const unsigned rest = blockIdx.x / N;
    const unsigned n = (blockIdx.x % N + rest) % N;
    const int tu = rest % tiles_u, tt = rest / tiles_u;
    const int T = (int)xn[n], U = (int)yn[n] + 1;
    const int t0 = tt * TD, u0 = tu * TD;
    if (T < 1 || U < 1 || t0 >= T || u0 >= U) return;          // (uniform)
    const int ul = threadIdx.x & (TD - 1), tl0 = threadIdx.x >> 5;
    const int u = u0 + ul;
    const size_t nbase = (size_t)mem_pref[n];
    // one pass by frames (lanes along u, row-major side), one by diagonals (diagonal-major side)
    auto by_frames = [&](auto&& f) {
#pragma unroll
        for (int k = 0; k < TD / 8; ++k) {
            const int tl = tl0 + 8 * k, t = t0 + tl;
            if (t < T && u < U) f(tl, nbase + (size_t)t * U + u);
        }
    };
    auto by_diagonals = [&](auto&& f) {
#pragma unroll
        for (int k = 0; k < (2 * TD) / 8; ++k) {
            const int d = tl0 + 8 * k, tl = d - ul;
            if (d < 2 * TD - 1 && tl >= 0 && tl < TD) {
                const int t = t0 + tl;
                if (t < T && u < U) {
                    int r = t + u;
                    r = r >= T ? r % T : r;
                    f(tl, nbase + (size_t)r * U + u);
                }
            }
        }
    };
    // The LOAD side of either direction is written out loads-first (round 5; see k_to_diagonal / k_from_diagonal: all of
    // a thread's loads issued before the first LDS write, at coordinates clamped into the tile and the utterance -- a
    // clamped slot receives the value of the cell it stands for); the store side keeps its conditions.
    const int uc = min(u, U - 1);
    if constexpr (TO_DIAGONAL) {
        constexpr int NK = TD / 8;
        float2 pr[NK];
#pragma unroll
        for (int k = 0; k < NK; ++k) pr[k] = src[nbase + (size_t)min(t0 + tl0 + 8 * k, T - 1) * U + uc];
#pragma unroll
        for (int k = 0; k < NK; ++k) tile[tl0 + 8 * k][ul] = pr[k];
        __syncthreads();
        by_diagonals([&](int tl, size_t at) { dst[at] = tile[tl][ul]; });
    } else {
        constexpr int ND = (2 * TD) / 8;
        float2 pr[ND];
        int tls[ND];
#pragma unroll
        for (int k = 0; k < ND; ++k) {
            tls[k] = min(max(tl0 + 8 * k - ul, 0), TD - 1);
            const int t = min(t0 + tls[k], T - 1);
            int r = t + uc;
            r = r >= T ? r % T : r;
            const size_t at = nbase + (size_t)r * U + uc;
            pr[k] = make_float2(sa[at], sb[at]);
        }
#pragma unroll
        for (int k = 0; k < ND; ++k) tile[tls[k]][ul] = pr[k];
        __syncthreads();
        by_frames([&](int tl, size_t at) { dst[at] = tile[tl][ul]; });
    }
}

static hipError_t launch_turn_compact32(hipStream_t stream, bool to_diagonal, const float* src, const float* sa,
                                        const float* sb, float* dst, const unsigned* xn, const unsigned* yn,
                                        const unsigned* mem_pref, unsigned N, unsigned Tmax, unsigned Umax) {
    if (N == 0 || Tmax == 0 || Umax == 0) return hipSuccess;
    const unsigned tiles_t = (Tmax + TD - 1) / TD, tiles_u = (Umax + TD - 1) / TD;
    const size_t nblk = (size_t)N * tiles_t * tiles_u;
    if (nblk >= ((size_t)1 << 31)) return hipErrorInvalidValue;
    if (to_diagonal)
        k_turn_compact32<true><<<(unsigned)nblk, 256, 0, stream>>>(reinterpret_cast<const float2*>(src), nullptr, nullptr,
                                                                   reinterpret_cast<float2*>(dst), xn, yn, mem_pref,
                                                                   (int)tiles_u, N);
    else
        k_turn_compact32<false><<<(unsigned)nblk, 256, 0, stream>>>(nullptr, sa, sb, reinterpret_cast<float2*>(dst), xn,
                                                                    yn, mem_pref, (int)tiles_u, N);
    return hipGetLastError();
}

hipError_t launch_reskew_compact32(hipStream_t stream, const float* pairs_rowmajor, float* pairs_diagonal,
                                   const unsigned* xn, const unsigned* yn, const unsigned* mem_pref, unsigned N,
                                   unsigned Tmax, unsigned Umax) {
    return launch_turn_compact32(stream, true, pairs_rowmajor, nullptr, nullptr, pairs_diagonal, xn, yn, mem_pref, N, Tmax,
                                 Umax);
}

hipError_t launch_unskew_compact32(hipStream_t stream, const float* a_diagonal, const float* b_diagonal,
                                   float* pairs_rowmajor, const unsigned* xn, const unsigned* yn, const unsigned* mem_pref,
                                   unsigned N, unsigned Tmax, unsigned Umax) {
    return launch_turn_compact32(stream, false, nullptr, a_diagonal, b_diagonal, pairs_rowmajor, xn, yn, mem_pref, N, Tmax,
                                 Umax);
}

// (blank, label) pairs -> two planes over the cells of a compact batch whose total only the device knows (the last
// prefix + the last utterance's size): the grid covers the bound, threads beyond the total return.
__global__ void __launch_bounds__(256)
k_split_pairs_compact32(const float2* __restrict__ src, float* __restrict__ a, float* __restrict__ b,
                        const unsigned* __restrict__ xn, const unsigned* __restrict__ yn,
                        const unsigned* __restrict__ mem_pref, unsigned N) {
    const int tl = (int)xn[N - 1], ul = (int)yn[N - 1] + 1;
    const size_t total = (size_t)mem_pref[N - 1] + ((tl >= 1 && ul >= 1) ? (size_t)tl * ul : 0);
    // two cells per thread where the pointers allow 16-byte loads (the caller checks), the odd last cell alone
    const size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 2;
    if (i + 1 < total) {
        const float4 v = *reinterpret_cast<const float4*>(src + i);
        *reinterpret_cast<float2*>(a + i) = make_float2(v.x, v.z);
        *reinterpret_cast<float2*>(b + i) = make_float2(v.y, v.w);
    } else if (i < total) {
        const float2 v = src[i];
        a[i] = v.x; b[i] = v.y;
    }
}

hipError_t launch_split_pairs_compact32(hipStream_t stream, const float* pairs, float* a, float* b, const unsigned* xn,
                                        const unsigned* yn, const unsigned* mem_pref, unsigned N, size_t cells_bound) {
    if (N == 0 || cells_bound == 0) return hipSuccess;
    const bool al = (reinterpret_cast<uintptr_t>(pairs) % 16 == 0) && (reinterpret_cast<uintptr_t>(a) % 8 == 0) &&
                    (reinterpret_cast<uintptr_t>(b) % 8 == 0);
    if (!al) return hipErrorInvalidValue;
    const size_t nblk = (cells_bound / 2 + 1 + 255) / 256;
    if (nblk >= ((size_t)1 << 31)) return hipErrorInvalidValue;
    k_split_pairs_compact32<<<(unsigned)nblk, 256, 0, stream>>>(reinterpret_cast<const float2*>(pairs), a, b, xn, yn,
                                                                mem_pref, N);
    return hipGetLastError();
}

// Prefix sums and launch bounds of a compact batch in ONE launch (the reference's binding does this
// with a chain of torch ops and four host synchronisations, binding.cpp:139-170):
//   cell_offsets[0..N] = exclusive sums of xn*(yn+1) (int64), label_offsets[0..N] = exclusive sums of yn,
//   stats = {sum cells, sum labels, max xn, max yn}.  One workgroup; N <= 65535.
constexpr int CP_THREADS = 1024;
__global__ void __launch_bounds__(CP_THREADS)
k_compact_offsets(const int* __restrict__ xn, const int* __restrict__ yn, int N, int64_t* __restrict__ cell_offs,
                  int* __restrict__ label_offs, int64_t* __restrict__ stats, const CompactBounds bounds) {
    __shared__ int64_t s_cells[CP_THREADS];
    __shared__ int s_labs[CP_THREADS];
    __shared__ int s_tmax[CP_THREADS / WAVE], s_umax[CP_THREADS / WAVE];
    const int tid = threadIdx.x;
    const int per = (N + CP_THREADS - 1) / CP_THREADS;
    const int lo = min(tid * per, N), hi = min(lo + per, N);
    int64_t c = 0;
    int l = 0, tmax = INT_MIN, umax = INT_MIN;
    for (int n = lo; n < hi; ++n) {
        const int x = xn[n], y = yn[n];
        c += (int64_t)x * (y + 1);
        l += y;
        tmax = max(tmax, x);
        umax = max(umax, y);
    }
    s_cells[tid] = c;
    s_labs[tid] = l;
    for (int o = 32; o > 0; o >>= 1) {
        tmax = max(tmax, __shfl_xor(tmax, o));
        umax = max(umax, __shfl_xor(umax, o));
    }
    if ((tid & (WAVE - 1)) == 0) { s_tmax[tid >> 6] = tmax; s_umax[tid >> 6] = umax; }
    __syncthreads();
    // inclusive scan over the 1024 per-thread totals: inside every wave on shuffles, then the sixteen wave totals by the
    // first wave -- two barriers (the first version's Hillis-Steele over shared memory took twenty)
    __shared__ int64_t s_wc[CP_THREADS / WAVE];
    __shared__ int s_wl[CP_THREADS / WAVE];
    const int lane = tid & (WAVE - 1), wv = tid >> 6;
    int64_t ic = c;
    int il = l;
    for (int o = 1; o < WAVE; o <<= 1) {
        const int64_t vc = __shfl_up(ic, o);
        const int vl = __shfl_up(il, o);
        if (lane >= o) { ic += vc; il += vl; }
    }
    if (lane == WAVE - 1) { s_wc[wv] = ic; s_wl[wv] = il; }
    __syncthreads();
    if (wv == 0) {
        int64_t wc = lane < CP_THREADS / WAVE ? s_wc[lane] : 0;
        int wl = lane < CP_THREADS / WAVE ? s_wl[lane] : 0;
        for (int o = 1; o < CP_THREADS / WAVE; o <<= 1) {
            const int64_t vc = __shfl_up(wc, o);
            const int vl = __shfl_up(wl, o);
            if (lane >= o) { wc += vc; wl += vl; }
        }
        if (lane < CP_THREADS / WAVE) { s_wc[lane] = wc; s_wl[lane] = wl; }   // inclusive totals of waves 0 ... lane
    }
    __syncthreads();
    if (wv > 0) { ic += s_wc[wv - 1]; il += s_wl[wv - 1]; }
    s_cells[tid] = ic;
    s_labs[tid] = il;
    __syncthreads();
    int64_t cbase = ic - c;     // exclusive
    int lbase = il - l;
    for (int n = lo; n < hi; ++n) {
        cell_offs[n] = cbase;
        label_offs[n] = lbase;
        cbase += (int64_t)xn[n] * (yn[n] + 1);
        lbase += yn[n];
    }
    if (tid == CP_THREADS - 1) {
        cell_offs[N] = s_cells[tid];
        label_offs[N] = s_labs[tid];
        int tm = s_tmax[0], um = s_umax[0];
        for (int i = 1; i < CP_THREADS / WAVE; ++i) { tm = max(tm, s_tmax[i]); um = max(um, s_umax[i]); }
        stats[0] = s_cells[tid];
        stats[1] = s_labs[tid];
        stats[2] = tm;
        stats[3] = um;
    }
    if (bounds.xn_checked) {
        // Caller-supplied launch bounds (no read-back of the maxima): what the host would have checked after its
        // synchronisation is checked here.  One length out of range, or totals that are not the tensors' sizes, make
        // every offset meaningless, so the whole batch is refused: lengths of 0 frames go to the kernels, which report
        // cost = NaN and touch nothing.
        __shared__ int s_bad;
        if (tid == 0) s_bad = 0;
        __syncthreads();
        bool bad = false;
        for (int n = lo; n < hi; ++n) {
            const int x = xn[n], y = yn[n];
            bad |= x < 1 || y < 0 || x > bounds.Tmax || y + 1 > bounds.Umax;
        }
        if (tid == CP_THREADS - 1) bad |= s_cells[tid] != bounds.STU || (int64_t)s_labs[tid] != bounds.n_labels;
        if (bad) atomicOr(&s_bad, 1);
        __syncthreads();
        const bool refuse = s_bad != 0;
        for (int n = lo; n < hi; ++n) bounds.xn_checked[n] = refuse ? 0 : xn[n];
        if (tid == 0) stats[4] = refuse ? 1 : 0;
    }
}

// behind a bounded compact call: a refused batch owns no cells the kernels could have written, so its (STU,2)
// gradients are zeroed here; returns at once otherwise (one flag read per thread)
__global__ void __launch_bounds__(256)
k_zero_if_refused(const int64_t* __restrict__ refused, float2* __restrict__ g2, size_t cells) {
    if (*refused == 0) return;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < cells; i += (size_t)gridDim.x * 256) g2[i] = make_float2(0.f, 0.f);
}

hipError_t launch_zero_if_refused(hipStream_t stream, const int64_t* refused, float* grads2, size_t cells) {
    if (!grads2 || cells == 0) return hipSuccess;
    const unsigned blocks = (unsigned)std::min<size_t>(1024, (cells + 255) / 256);
    k_zero_if_refused<<<blocks, 256, 0, stream>>>(refused, reinterpret_cast<float2*>(grads2), cells);
    return hipGetLastError();
}

hipError_t launch_compact_offsets(hipStream_t stream, const int* xn, const int* yn, int N, int64_t* cell_offs,
                                  int* label_offs, int64_t* stats, const CompactBounds* bounds) {
    const CompactBounds none{nullptr, 0, 0, 0, 0};
    k_compact_offsets<<<1, CP_THREADS, 0, stream>>>(xn, yn, N, cell_offs, label_offs, stats, bounds ? *bounds : none);
    return hipGetLastError();
}

}  // namespace rnnt
