// Best-path (Viterbi) alignments over the diagonal-major pair plane (include/warp_rnnt_amd_align.h): a max-plus sweep
// that records its decisions as ballot words, and the trace that reads the path back from them.
//
// The arithmetic is the header's and nothing else: per cell one fp32 add for each predecessor and one compare,
//     cb = v(t-1,u) + b(t-1,u),  cl = v(t,u-1) + l(t,u-1),  by_label = u > 0 and (t == 0 or cl > cb),  v = by_label ? cl : cb
// so a restatement in NumPy fp32 gives the same bits.
//
// Nothing here waits on memory: the column blocks of a wide lattice hand their boundary values over through LDS between
// workgroup barriers, the column stripes of a lattice wider than a workgroup through the workspace, behind a barrier of
// the one workgroup that writes and reads them.  A hand-over cannot be lost.
#include "align.h"
#include "common.h"

namespace rnnt {
namespace {

typedef unsigned long long u64;

constexpr int ALIGN_WAVES = 16;   // column blocks per stripe: the waves of one workgroup
constexpr int ALIGN_GROUP = 16;   // rows of pairs a wave has in flight while it works on the 16 before them
constexpr int ALIGN_GROUPS = WAVE / ALIGN_GROUP;
template <bool B> struct Flag { static constexpr bool value = B; };      // a compile-time switch as a lambda's argument

// One workgroup per utterance, lanes are lattice columns, one wave per block of 64 columns.  Step d takes a lane from
// its cell of diagonal d-1 to its cell of diagonal d: v + b and v + l from the pair of the cell it holds, the left
// neighbour's v + l by one DPP shift, compare, select.  The wave's 64 decisions of the step are one ballot word.
//
// The two structural edges cost nothing per step.  A lane that has not reached frame 0 of its column holds NaN, and the
// decision is taken as !(cl <= cb): at t == 0 cb is NaN + b, the comparison is unordered and the label edge is taken,
// whatever cl is (-inf included); for ordered operands it is cl > cb.  Column 0 is shifted -inf from its left: -inf <= cb
// holds for every cb there is.  (A NaN that meets a lane's first real value never survives: v becomes cl.)
//
// Steps come in chunks of 64.  Wave w works on chunk p - w in phase p, one chunk behind its left neighbour, and phases
// end at a workgroup barrier: what lane 63 of wave w-1 shifts out in the 64 steps of a chunk goes into mail[w-1], one
// float per step, and wave w picks the 64 of them up after the barrier, lane j holding step j's.  Two buffers by chunk
// parity: the writer is on chunk c+1 while the reader is on chunk c.  The ballot words of a chunk are staged in LDS the
// same way and leave in one store, lane j storing step j's.  Both LDS writes are issued by the whole wave, without a
// branch: the one lane whose value counts aims at the slot, the others at a sink that nobody reads (one for all waves:
// what ends up in it does not matter).
//
// A lattice of more than 16 column blocks runs as stripes of 16, one after the other in the same workgroup; the last
// wave of a stripe parks its boundary values in the workspace (`park`, two columns per utterance by stripe parity) and
// wave 0 of the next stripe reads them there.
//
// The v plane is never written: a lane holds its cell of the previous diagonal and nothing else.  Cells outside the
// utterance's (T_n, U_n + 1) window are computed like the others and never reach a cell inside it: values move right and
// down only.
__global__ __launch_bounds__(ALIGN_WAVES* WAVE) void k_align_sweep(const float2* __restrict__ pairs,
                                                                   const int* __restrict__ xn, const int* __restrict__ yn,
                                                                   u64* __restrict__ words, float* __restrict__ park,
                                                                   float* __restrict__ scores, int T, int U) {
    __shared__ float mail[ALIGN_WAVES][2][WAVE];
    __shared__ u64 staged[ALIGN_WAVES][WAVE];
    __shared__ float sink_out[2 * WAVE];      // lane l at step j: [l + j]; one sink for all waves, written and never read
    __shared__ u64 sink_word[2 * WAVE];
    const int n = blockIdx.x, lane = threadIdx.x & (WAVE - 1), waves = blockDim.x / WAVE;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);          // (wave-uniform, and known to be)
    const int Tn = xn[n], Un = yn[n];
    if (Tn < 1 || Tn > T || Un < 0 || Un >= U) return;        // (the whole workgroup; the trace writes its NaN and -1)
    const int D = Tn + Un;                    // steps 1 .. D: D-1 is the lattice's last diagonal, step D adds its blank
    const int chunks = (D + WAVE - 1) / WAVE;
    const int nblk = align_blocks(U);
    const int live = Un / WAVE + 1;           // column blocks that hold a column <= U_n
    const float2* plane = pairs + (size_t)n * T * U;
    u64* wn = words + (size_t)n * ((size_t)T + U - 1) * nblk;
    const size_t pitch = align_park_pitch(T, U);
    float* pk = park + (size_t)n * 2 * pitch;

    for (int s = 0; s * ALIGN_WAVES < live; ++s) {
        const int blk = s * ALIGN_WAVES + w;
        const int active = min(waves, live - s * ALIGN_WAVES);
        const int u = blk * WAVE + lane;
        const int uc = min(u, U - 1);         // (lanes past the last column read it again: they feed nobody to their left)
        const float* park_in = pk + (s & 1) * pitch;             // what stripe s-1 wrote
        float* park_out = pk + ((s & 1) ^ 1) * pitch;
        const bool works = w < active;
        float v = u == 0 ? 0.0f : __builtin_nanf("");            // v(0,0) = 0; nobody else is in its column yet
        int row = 0;                          // the next row of the plane to load: diagonal d sits in row d mod T
        float2 cur[ALIGN_GROUP];
        const auto load = [&](float2(&dst)[ALIGN_GROUP]) {
#pragma unroll
            for (int i = 0; i < ALIGN_GROUP; ++i) {
                dst[i] = plane[row * U + uc];
                row = row + 1 == T ? 0 : row + 1;
            }
        };
        if (works) load(cur);

        // chunk c of this wave: steps d0+1 .. d0+64 from the pairs of diagonals d0 .. d0+63.  is_last: the chunk that
        // holds step D, whose cb in the lane of column U_n is the score.
        const auto chunk = [&](auto is_last, const int c) {
            const int d0 = c * WAVE;
            float in = -__builtin_inff();     // lane j: what the column to the left of lane 0 shifts in at step j
            if (w > 0) in = mail[w - 1][c & 1][lane];
            else if (s > 0) in = park_in[d0 + lane];
            float* out = lane == WAVE - 1 ? &mail[w][c & 1][0] : &sink_out[lane];
            u64* word_out = lane == 0 ? &staged[w][0] : &sink_word[lane];
            const int last = D - d0 - 1;      // step D in this chunk's count
            float score = 0.0f;
#pragma unroll
            for (int g = 0; g < ALIGN_GROUPS; ++g) {
                float2 nxt[ALIGN_GROUP];
#pragma unroll
                for (int i = 0; i < ALIGN_GROUP; ++i) nxt[i] = cur[i];
                if (g + 1 < ALIGN_GROUPS || c + 1 < chunks) load(nxt);
#pragma unroll
                for (int i = 0; i < ALIGN_GROUP; ++i) {
                    const int j = g * ALIGN_GROUP + i;
                    const float cb = v + cur[i].x, own = v + cur[i].y;
                    const float cl = wave_shr1(readlane(in, j), own);
                    const bool by_label = !(cl <= cb);
                    v = by_label ? cl : cb;
                    out[j] = own;
                    word_out[j] = __builtin_amdgcn_ballot_w64(by_label);
                    if (decltype(is_last)::value) score = j == last ? cb : score;
                }
#pragma unroll
                for (int i = 0; i < ALIGN_GROUP; ++i) cur[i] = nxt[i];
            }
            // (each wave reads back what it wrote itself: the LDS accesses of one wave complete in order)
            const int d = d0 + 1 + lane;
            if (d < D) wn[(size_t)d * nblk + blk] = staged[w][lane];
            if (decltype(is_last)::value && u == Un) scores[n] = score;
            if (w + 1 == active && blk + 1 < live) park_out[d0 + lane] = mail[w][c & 1][lane];
        };

        for (int p = 0; p < chunks + active - 1; ++p) {
            const int c = p - w;
            if (works && c >= 0 && c < chunks) {
                if (c + 1 == chunks) chunk(Flag<true>{}, c);
                else chunk(Flag<false>{}, c);
            }
            __syncthreads();
        }
    }
}

__device__ __forceinline__ u64 readlane64(u64 v, int lane) {
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, lane);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), lane);
    return ((u64)hi << 32) | lo;
}

// One wave per utterance, from (T_n-1, U_n) down to column 0 in chunks of 64 diagonals.  Lane j holds the decision words
// of diagonal d - j for the two column blocks the path can be in during the chunk (it moves left by at most 64 columns):
// 128 columns from `base` on.  The 64 steps run from registers without a branch: two uniform readlanes each for the two
// words -- they do not depend on where the path is -- then select, shift, mask, r -= bit.  Steps past diagonal 1 read
// zero words and steps in column 0 find its bits clear, so every chunk runs all 64.  The chunk's 64 bits are kept in a
// scalar pair; afterwards lane j knows from them (a population count below its own bit) where the path was at its step
// and, if that was a label step, stores its frame.  The words of the next chunk are asked for before the steps of this
// one: for the three blocks the path can then need.
__global__ __launch_bounds__(WAVE) void k_align_trace(const u64* __restrict__ words, const int* __restrict__ xn,
                                                      const int* __restrict__ yn, float* __restrict__ scores,
                                                      int* __restrict__ emit_frames, int T, int U) {
    const int n = blockIdx.x, lane = threadIdx.x;
    const int Tn = xn[n], Un = yn[n];
    int* frames = emit_frames + (size_t)n * (U - 1);
    if (Tn < 1 || Tn > T || Un < 0 || Un >= U) {
        if (lane == 0) scores[n] = __builtin_nanf("");
        for (int u = lane; u < U - 1; u += WAVE) frames[u] = -1;
        return;
    }
    for (int u = Un + lane; u < U - 1; u += WAVE) frames[u] = -1;
    const int nblk = align_blocks(U);
    const u64* wn = words + (size_t)n * ((size_t)T + U - 1) * nblk;
    // the word of diagonal dd - lane and column block b, zero where there is none
    const auto word_of = [&](int dd, int b) -> u64 {
        const int dj = dd - lane;
        return dj >= 1 && b >= 0 ? wn[(size_t)dj * nblk + b] : 0;
    };
    int d = Tn - 1 + Un, u = Un;              // the path's cell: (d - u, u)
    int blk = u / WAVE;
    u64 here = word_of(d, blk), left = word_of(d, blk - 1);
    while (u > 0 && d > 0) {                  // (column 0 is all blank steps: nothing left to write)
        const u64 n0 = word_of(d - WAVE, blk), n1 = word_of(d - WAVE, blk - 1), n2 = word_of(d - WAVE, blk - 2);
        const int base = (blk - 1) * WAVE;
        int r = u - base;                     // 64 .. 127 now, never below 0: at most 64 steps to the left
        unsigned bits_lo = 0, bits_hi = 0;    // bit j: step j was a label step
#pragma unroll
        for (int j = 0; j < WAVE; ++j) {
            const u64 hi = readlane64(here, j), lo = readlane64(left, j);
            const unsigned bit = (unsigned)((r >= WAVE ? hi : lo) >> (r & (WAVE - 1))) & 1u;
            r -= (int)bit;
            if (j < 32) bits_lo |= bit << j;
            else bits_hi |= bit << (j - 32);
        }
        // lane j: the path's column when its step began, and the label step it may have been
        const int before = (int)__builtin_amdgcn_mbcnt_hi(bits_hi, __builtin_amdgcn_mbcnt_lo(bits_lo, 0));
        const int uj = u - before;
        const bool mine = ((lane < 32 ? bits_lo >> lane : bits_hi >> (lane - 32)) & 1u) != 0;
        if (mine && uj >= 1 && uj < U) frames[uj - 1] = d - lane - uj;
        u = base + r;
        d -= WAVE;
        const bool stayed = u / WAVE == blk;
        here = stayed ? n0 : n1;
        left = stayed ? n1 : n2;
        blk = u / WAVE;
    }
}

}  // namespace

hipError_t launch_align_sweep(hipStream_t stream, const float* pairs, const int* xn, const int* yn, u64* words,
                              float* park, float* scores, int N, int T, int U) {
    if (N == 0) return hipSuccess;
    const int waves = align_blocks(U) < ALIGN_WAVES ? align_blocks(U) : ALIGN_WAVES;
    k_align_sweep<<<N, waves * WAVE, 0, stream>>>(reinterpret_cast<const float2*>(pairs), xn, yn, words, park, scores, T, U);
    return hipGetLastError();
}

hipError_t launch_align_trace(hipStream_t stream, const u64* words, const int* xn, const int* yn, float* scores,
                              int* emit_frames, int N, int T, int U) {
    if (N == 0) return hipSuccess;
    k_align_trace<<<N, WAVE, 0, stream>>>(words, xn, yn, scores, emit_frames, T, U);
    return hipGetLastError();
}

}  // namespace rnnt
