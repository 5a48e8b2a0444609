// The band selection of the pruned recipe (k2 / icefall's get_rnnt_prune_ranges; warp_rnnt_amd.pruned.prune_ranges is the
// plain-torch definition): from the first pass's gradient pairs (N,T,U,2) -- minus the edge occupancies -- to the (N,T)
// int32 starts of every frame's band of S label positions (prune_ranges.h).  Two launches:
//
// k_prune_argmax   the memory-bound one.  A group of G = prune_group(U) lanes per frame, 256 / G frames per workgroup, so
//                  the N T frames fill the chip at any N.  The lanes read the row's float2 pairs coalesced and
//                  non-temporal (they are read once), form occ = -(gB + gL) and stage the row in the group's U floats of
//                  LDS; only the hi + S cells a window can touch are read, and a frame t >= T_n - 1 reads nothing.  Lane l
//                  then evaluates the windows that start at u0 = l, l + G, ..: S reads of consecutive LDS words across
//                  the lanes (no bank conflict), added left to right from u0 -- the order is a function of (S, u0) alone,
//                  whatever U, G, T and the place in the batch are.  It keeps (best, index) under `better`, the group
//                  reduces the pairs with xor shuffles under the same total order (larger sum, then lower index), a NaN
//                  occupancy travels as a ballot bit, never through a comparison.  The whole row is staged, not chunks
//                  with an S - 1 halo: S is bounded by U alone, so the halo is as large as the row, and one form serves
//                  every S.
// k_prune_scans    a wave per utterance walks the frames from the end in chunks of 512, eight consecutive frames per lane,
//                  with two carries: the suffix minimum and, on its result, the suffix maximum of m[t] - t (S-1) with the
//                  ramp added back.  Exact integer scans -- serial inside a lane, a shuffle tree over the lanes' totals;
//                  the next chunk's loads are issued before the current chunk's scans.  One read and one write of the
//                  (N,T) ints, in place.
// No atomics, no memset, no workspace: two runs give the same starts, and the pair can be captured into a graph.
#include "prune_ranges.h"

#include <climits>

namespace rnnt {
namespace {

constexpr int PR_THREADS = 256;
constexpr int PR_WAVE = 64;

typedef float pr_f2 __attribute__((ext_vector_type(2)));

// (sum, start) a beats (sum, start) b: the larger sum, of equal sums the lower start.  A NaN sum beats nothing and is beaten
// by nothing; it never becomes a `best`, which starts at (-inf, INT_MAX) -- below every window, a sum of -inf included.
__device__ __forceinline__ bool better(float wa, int ia, float wb, int ib) { return wa > wb || (wa == wb && ia < ib); }

// hi of utterance n: the last start a band may take
__device__ __forceinline__ int band_hi(int y, int U, int S) {
    const long long h = (long long)y + 1 - S;
    return h < 0 ? 0 : h > U - S ? U - S : (int)h;
}

template <int G>
__global__ void __launch_bounds__(PR_THREADS)
k_prune_argmax(const pr_f2* __restrict__ g2, long long pitch, const int* __restrict__ xn, const int* __restrict__ yn,
               int* __restrict__ raw, unsigned frames, int T, int U, int S) {
    extern __shared__ float pr_occ[];                  // (256 / G, U)
    const unsigned frame = blockIdx.x * (unsigned)(PR_THREADS / G) + threadIdx.x / G;
    if (frame >= frames) return;                       // (the whole group: no lane of it is asked for a shuffle below)
    const int lane = threadIdx.x % G;
    const unsigned n = frame / (unsigned)T;
    const int t = (int)(frame - n * (unsigned)T);
    const int hi = band_hi(yn[n], U, S);
    if ((long long)t >= (long long)xn[n] - 1) {        // the last live frame and everything behind it (any T_n)
        if (lane == 0) raw[frame] = hi;
        return;
    }
    float* occ = pr_occ + (threadIdx.x / G) * U;
    const pr_f2* row = g2 + (size_t)n * (size_t)pitch + (size_t)t * (size_t)U;
    const int need = hi + S;                           // <= U: the cells a window of this utterance can touch
    bool nan = false;
#pragma unroll 4
    for (int u = lane; u < need; u += G) {
        const pr_f2 g = __builtin_nontemporal_load(row + u);
        const float o = -(g.x + g.y);
        nan |= o != o;
        occ[u] = o;
    }
    // the group is part of one wave: its stores are ordered before its loads by a wave-level fence, no workgroup barrier
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

    float best = -__builtin_inff();
    int idx = INT_MAX;
    for (int u0 = lane; u0 <= hi; u0 += G) {
        float w = occ[u0];
        for (int s = 1; s < S; ++s) w += occ[u0 + s];
        if (better(w, u0, best, idx)) {
            best = w;
            idx = u0;
        }
    }
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) {
        const float wo = __shfl_xor(best, o, PR_WAVE);
        const int io = __shfl_xor(idx, o, PR_WAVE);
        if (better(wo, io, best, idx)) {
            best = wo;
            idx = io;
        }
    }
    // the NaN flags of the group's lanes: its G bits of the wave's ballot (lanes that left above are not in it)
    const unsigned long long flags = __ballot(nan);
    const unsigned long long mine = G == PR_WAVE ? ~0ull : ((1ull << (G % PR_WAVE)) - 1) << ((threadIdx.x % PR_WAVE) / G * G);
    if (lane == 0) raw[frame] = ((flags & mine) != 0 || idx > hi) ? hi : idx;
}

// suffix minimum / maximum over the wave: lane l ends with the extreme of lanes l .. 63 (a shuffle from beyond the wave
// hands back the lane's own value, which changes neither)
__device__ __forceinline__ int suffix_min(int v) {
#pragma unroll
    for (int o = 1; o < PR_WAVE; o <<= 1) v = min(v, __shfl_down(v, o, PR_WAVE));
    return v;
}
__device__ __forceinline__ int suffix_max(int v) {
#pragma unroll
    for (int o = 1; o < PR_WAVE; o <<= 1) v = max(v, __shfl_down(v, o, PR_WAVE));
    return v;
}

// A lane holds PR_RUN consecutive frames, the wave a chunk of 512: the scan inside a lane is a serial chain of PR_RUN VALU
// operations, and only the lanes' totals go through the shuffle tree -- two trees per 512 frames.  (A first form with one
// frame per lane, a chunk of 64, spent its time in the 24 dependent pairs of trees of T = 1500:
// profiles/prune_ranges_rate.txt.)
constexpr int PR_RUN = 8;
constexpr int PR_CHUNK = PR_WAVE * PR_RUN;

__global__ void __launch_bounds__(PR_WAVE) k_prune_scans(int* __restrict__ starts, int T, int S) {
    int* row = starts + (size_t)blockIdx.x * (size_t)T;
    const int lane = threadIdx.x;
    int carry_min = INT_MAX, carry_max = INT_MIN;
    int v[PR_RUN], vn[PR_RUN];
    int t0 = (T - 1) / PR_CHUNK * PR_CHUNK + lane * PR_RUN;     // lane 0's first frame is a frame in every chunk
#pragma unroll
    for (int j = 0; j < PR_RUN; ++j) v[j] = t0 + j < T ? row[t0 + j] : INT_MAX;
    for (; t0 >= 0; t0 -= PR_CHUNK) {
#pragma unroll
        for (int j = 0; j < PR_RUN; ++j)               // (the chunk in front, whole: in flight while this one is scanned)
            vn[j] = t0 >= PR_CHUNK ? row[t0 - PR_CHUNK + j] : 0;
        // m[t] = min(raw[t], m[t+1]): inside the lane, then the lanes behind it and the chunks behind the wave
#pragma unroll
        for (int j = PR_RUN - 2; j >= 0; --j) v[j] = min(v[j], v[j + 1]);
        int behind = __shfl_down(suffix_min(v[0]), 1, PR_WAVE);
        behind = min(lane == PR_WAVE - 1 ? INT_MAX : behind, carry_min);
#pragma unroll
        for (int j = 0; j < PR_RUN; ++j) v[j] = min(v[j], behind);
        carry_min = __shfl(v[0], 0, PR_WAVE);
        // start[t] = t (S-1) + max_{t' >= t} (m[t'] - t' (S-1)); the ramp < (T + 511) U: 32 bits (the launcher bounds T U)
#pragma unroll
        for (int j = 0; j < PR_RUN; ++j) v[j] = t0 + j < T ? v[j] - (t0 + j) * (S - 1) : INT_MIN;
#pragma unroll
        for (int j = PR_RUN - 2; j >= 0; --j) v[j] = max(v[j], v[j + 1]);
        behind = __shfl_down(suffix_max(v[0]), 1, PR_WAVE);
        behind = max(lane == PR_WAVE - 1 ? INT_MIN : behind, carry_max);
#pragma unroll
        for (int j = 0; j < PR_RUN; ++j) {
            v[j] = max(v[j], behind);
            if (t0 + j < T) row[t0 + j] = v[j] + (t0 + j) * (S - 1);
        }
        carry_max = __shfl(v[0], 0, PR_WAVE);
#pragma unroll
        for (int j = 0; j < PR_RUN; ++j) v[j] = vn[j];
    }
}

// Lanes per frame, a function of U alone: at most 8 cells per lane up to a wave, a wave walks a longer row in passes
inline int prune_group(int U) { return U <= 128 ? 16 : U <= 256 ? 32 : 64; }

}  // namespace

hipError_t launch_prune_ranges(hipStream_t stream, const float* pairs, long long pitch, const int* xn, const int* yn,
                               int* starts, int N, int T, int U, int S) {
    if (N < 0 || T < 1 || U < 1 || S < 2 || S > U || U > PRUNE_RANGES_MAX_U || pitch < (long long)T * U ||
        (long long)T * U >= 1ll << 29 || (long long)N * T >= 1ll << 31)
        return hipErrorInvalidValue;
    if (N == 0) return hipSuccess;
    const pr_f2* g2 = reinterpret_cast<const pr_f2*>(pairs);
    const unsigned frames = (unsigned)N * (unsigned)T;
    const int G = prune_group(U);
    const unsigned per = PR_THREADS / G, grid = (frames + per - 1) / per;
    const size_t lds = (size_t)per * U * sizeof(float);          // <= 64 KiB: per <= 4 where U > 256
    switch (G) {
        case 16: k_prune_argmax<16><<<grid, PR_THREADS, lds, stream>>>(g2, pitch, xn, yn, starts, frames, T, U, S); break;
        case 32: k_prune_argmax<32><<<grid, PR_THREADS, lds, stream>>>(g2, pitch, xn, yn, starts, frames, T, U, S); break;
        default: k_prune_argmax<64><<<grid, PR_THREADS, lds, stream>>>(g2, pitch, xn, yn, starts, frames, T, U, S); break;
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    k_prune_scans<<<(unsigned)N, PR_WAVE, 0, stream>>>(starts, T, S);
    return hipGetLastError();
}

}  // namespace rnnt
