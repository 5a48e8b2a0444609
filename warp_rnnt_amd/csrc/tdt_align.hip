// Best-path alignments over the token-and-duration (TDT) lattice (include/warp_rnnt_amd_tdt_align.h; tdt_align.h has the
// definition): a max-plus sweep over the (2+D)-channel plane that tdt.hip's producer fills, recording one
// decision byte per cell, and the trace that reads the path back from those bytes.
//
// The arithmetic is the definition's and nothing else: per incoming edge one fp32 add for its weight, one for
// v(source) + weight, one compare; no transcendental.  A restatement in NumPy fp32 on the same plane gives the same bits.
//
// The sweep is k_tdt_sweep's alpha side with the log-sum-exp replaced by the running maximum: one workgroup per
// utterance, lanes are lattice columns, the last max(durations)+2 diagonals of v in an LDS ring, one workgroup barrier
// per diagonal, the edge weights of the next diagonal asked for in front of that barrier.  The prefetched weights sit in
// two register sets used in turn, the loop unrolled by two, so no register copy waits for the loads at the end of a step.
// Nothing waits on memory, nothing passes between workgroups, no hand-written instructions; the trace is a second launch
// and the kernel boundary is the only hand-over.
#include "tdt_align.h"
#include "common.h"

// every sum below is rounded on its own
#pragma clang fp contract(off)

namespace rnnt {
namespace {

constexpr float TA_NEG_INF = -__builtin_inff();
typedef float TaTerms[TDT_MAX_D];

__host__ __device__ __forceinline__ int ta_mod(int a, int T) {
    const int r = a % T;
    return r < 0 ? r + T : r;
}

// blockIdx.x: the utterance.  Lane u is lattice column u; in step d it holds cell (d - u, u).  ring: (max duration + 2)
// rows of blockDim.x floats, diagonal d in row d mod (max duration + 2); a cell outside the utterance's window is -inf
// there.  The end of the lattice is cell (T_n, U_n) on diagonal T_n + U_n: blank edges only lead to it, its v is the score.
// An edge that the definition does not consider has the weight -inf: its candidate is -inf (v is never +inf), which is
// never strictly greater than the running best, so it cannot be chosen -- the loop has no branch on the edge's kind.
__global__ void __launch_bounds__(TDT_MAX_U)
k_tdt_align_sweep(const float* __restrict__ plane, const int* __restrict__ xn, const int* __restrict__ yn,
                  unsigned char* __restrict__ dec, float* __restrict__ scores, TdtDurations dur, size_t cells, int T, int U) {
    extern __shared__ float ring[];
    const int n = blockIdx.x, u = threadIdx.x, ncol = blockDim.x;
    const int Tn = xn[n], Un = yn[n];
    if (Tn < 1 || Tn > T || Un < 0 || Un >= U) {          // (the whole workgroup; the trace writes the rows of -1)
        if (u == 0) scores[n] = __builtin_nanf("");
        return;
    }
    const int D = dur.D;
    int longest = 0;
#pragma unroll
    for (int i = 0; i < TDT_MAX_D; ++i)
        if (i < D) longest = max(longest, dur.d[i]);
    const int R = longest + 2, last = Tn + Un;
    for (int r = 0; r < R; ++r) ring[r * ncol + u] = TA_NEG_INF;
    __syncthreads();
    const float* pB = plane + (size_t)n * T * U;
    const float* pL = pB + cells;
    const float* pD = pL + cells;             // channel i: pD + i * cells
    unsigned char* dn = dec + (size_t)n * ((size_t)T + U) * U;

    // rows of the plane that hold diagonals d - d_i (blank sources) and d - d_i - 1 (label sources) of the step asked for
    int rowB[TDT_MAX_D], rowL[TDT_MAX_D];
#pragma unroll
    for (int i = 0; i < TDT_MAX_D; ++i) {
        rowB[i] = ta_mod(-dur.d[i < D ? i : 0], T);
        rowL[i] = ta_mod(-dur.d[i < D ? i : 0] - 1, T);
    }
    const int ul = u > 0 ? u - 1 : 0;
    const auto fetch = [&](int d, TaTerms& wb, TaTerms& wl) {
        const int t = d - u;
        const bool cell = t >= 0 && t < Tn && u <= Un, end = t == Tn && u == Un;
#pragma unroll
        for (int i = 0; i < TDT_MAX_D; ++i) {
            wb[i] = wl[i] = TA_NEG_INF;
            if (i >= D) continue;
            const int di = dur.d[i];
            if ((cell || end) && di > 0 && t - di >= 0) {         // from (t - d_i, u)
                const int idx = rowB[i] * U + u;
                wb[i] = pB[idx] + pD[(size_t)i * cells + idx];
            }
            if (cell && u > 0 && t - di >= 0) {                   // from (t - d_i, u - 1)
                const int idx = rowL[i] * U + ul;
                wl[i] = pL[idx] + pD[(size_t)i * cells + idx];
            }
        }
    };
    int slot = 0;
    // step d with the weights (cb, cl); those of step d + 1 are asked for into (nb, nl) before anything waits
    const auto step = [&](int d, const TaTerms& cb, const TaTerms& cl, TaTerms& nb, TaTerms& nl) {
#pragma unroll
        for (int i = 0; i < TDT_MAX_D; ++i) {
            rowB[i] = rowB[i] + 1 == T ? 0 : rowB[i] + 1;
            rowL[i] = rowL[i] + 1 == T ? 0 : rowL[i] + 1;
        }
        if (d < last) fetch(d + 1, nb, nl);
        const int t = d - u;
        const bool cell = t >= 0 && t < Tn && u <= Un, end = t == Tn && u == Un;
        float best = TA_NEG_INF;
        int code = TDT_ALIGN_NO_EDGE;
#pragma unroll
        for (int i = 0; i < TDT_MAX_D; ++i) {
            if (i >= D) continue;
            int sb = slot - dur.d[i], sl = slot - dur.d[i] - 1;
            sb += sb < 0 ? R : 0;
            sl += sl < 0 ? R : 0;
            const float b = ring[sb * ncol + u] + cb[i];
            code = b > best ? 2 * i : code;
            best = b > best ? b : best;
            const float l = ring[sl * ncol + ul] + cl[i];
            code = l > best ? 2 * i + 1 : code;
            best = l > best ? l : best;
        }
        best = d == 0 && u == 0 ? 0.0f : best;
        best = cell || end ? best : TA_NEG_INF;
        ring[slot * ncol + u] = best;
        if (cell || end) dn[(size_t)d * U + u] = (unsigned char)code;
        if (end) scores[n] = best;
        slot = slot + 1 == R ? 0 : slot + 1;
        __syncthreads();
    };

    TaTerms ab, al, bb, bl;                   // the two register sets: one holds this step's weights, the other the next's
    fetch(0, ab, al);
    for (int d = 0; d <= last; d += 2) {      // (last is the workgroup's: every lane meets every barrier)
        step(d, ab, al, bb, bl);
        if (d + 1 <= last) step(d + 1, bb, bl, ab, al);
    }
}

// One wave per utterance.  The lanes write the -1 tails (both rows throughout for an utterance without a path); lane 0
// then walks the codes from the end cell (T_n, U_n): one dependent byte load per edge of the path.
__global__ void __launch_bounds__(WAVE)
k_tdt_align_trace(const unsigned char* __restrict__ dec, const int* __restrict__ xn, const int* __restrict__ yn,
                  const float* __restrict__ scores, int* __restrict__ emit_frames, int* __restrict__ emit_durations,
                  TdtDurations dur, int T, int U) {
    const int n = blockIdx.x, lane = threadIdx.x;
    const int Tn = xn[n], Un = yn[n];
    int* frames = emit_frames + (size_t)n * (U - 1);
    int* lengths = emit_durations + (size_t)n * (U - 1);
    const bool ok = Tn >= 1 && Tn <= T && Un >= 0 && Un < U;
    const bool path = ok && scores[n] > TA_NEG_INF;       // (false for the NaN of refused lengths too)
    for (int u = (path ? Un : 0) + lane; u < U - 1; u += WAVE) frames[u] = lengths[u] = -1;
    if (!path || lane != 0) return;
    const unsigned char* dn = dec + (size_t)n * ((size_t)T + U) * U;
    int t = Tn, u = Un;
    while (t + u > 0) {
        const int k = dn[(size_t)(t + u) * U + u];
        const int i = k >> 1, label = k & 1;
        int di = -1;
#pragma unroll
        for (int j = 0; j < TDT_MAX_D; ++j) di = j == i && j < dur.D ? dur.d[j] : di;
        // (a finite score implies a valid code on every cell of the path: what follows only keeps a walk inside its rows)
        if (di < 0 || di + label == 0) break;
        t -= di;
        u -= label;
        if (t < 0 || u < 0) break;
        if (label) {
            frames[u] = t;
            lengths[u] = di;
        }
    }
}

}  // namespace

hipError_t launch_tdt_align_sweep(hipStream_t stream, const float* plane, const int* xn, const int* yn, unsigned char* dec,
                                  float* scores, const TdtDurations& dur, int N, int T, int U) {
    if (U < 1 || U > TDT_MAX_U || dur.D < 1 || dur.D > TDT_MAX_D) return hipErrorInvalidValue;
    if (N == 0) return hipSuccess;
    int longest = 0;
    for (int i = 0; i < dur.D; ++i) {
        if (dur.d[i] < 0 || dur.d[i] > TDT_MAX_DURATION) return hipErrorInvalidValue;
        longest = dur.d[i] > longest ? dur.d[i] : longest;
    }
    const int ncol = (U + WAVE - 1) / WAVE * WAVE;
    const size_t lds = (size_t)(longest + 2) * ncol * sizeof(float);          // 40 KB at the most
    k_tdt_align_sweep<<<N, ncol, lds, stream>>>(plane, xn, yn, dec, scores, dur, (size_t)N * T * U, T, U);
    return hipGetLastError();
}

hipError_t launch_tdt_align_trace(hipStream_t stream, const unsigned char* dec, const int* xn, const int* yn,
                                  const float* scores, int* emit_frames, int* emit_durations, const TdtDurations& dur, int N,
                                  int T, int U) {
    if (U < 1 || dur.D < 1 || dur.D > TDT_MAX_D) return hipErrorInvalidValue;
    if (N == 0) return hipSuccess;
    k_tdt_align_trace<<<N, WAVE, 0, stream>>>(dec, xn, yn, scores, emit_frames, emit_durations, dur, T, U);
    return hipGetLastError();
}

}  // namespace rnnt
