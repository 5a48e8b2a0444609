// Best-path (Viterbi) forced alignment of the CTC lattice (include/warp_rnnt_amd_ctc_align.h has the recurrence, the tie
// rule and the layout of the decision words): the emissions of ctc.hip's k_ctc_emit, or
//
//   k_ctc_align_gather  log-probs taken as they are: a wave per row (n,t), the L_n + 1 columns the lattice uses gathered into
//                       the same (N,T,L+1) plane.  Rows t >= T_n are not touched.
//
// and then one launch,
//
//   k_ctc_align<K>      ONE WAVE per utterance, sequential in t, no barrier and no LDS on the chain.  Lane j owns the K
//                       consecutive label positions j K .. j K + K - 1, each a blank state and a label state, in 2 K
//                       registers (K = 1, 2, 4, 8, 16: 64 K >= L + 1).  A frame needs one value from outside the lane, the
//                       label state of lane j - 1's last position: one DPP wave_shr:1.  All blank states share one
//                       emission (column 0, a wave-uniform load); the lane's K label emissions are K consecutive floats.
//                       Emissions are fetched a block of D frames ahead into registers (D K = 32 label emissions per
//                       lane, 64 from K = 8 on; two register blocks taken in turn), so a frame's loads were issued D to
//                       2 D frames before its chain.  The 4 K decision bits
//                       of a lane and frame go out as one word, a row of 64 words per frame, coalesced.
//                       The walk back: blocks of 128 (64-bit words: 64) frames from the end; the block's decision rows are
//                       staged into LDS by all lanes (loads that do not depend on the path), lane 0 walks them in LDS and
//                       leaves the block's states there, then all lanes write frame_tokens coalesced and emit_frames where
//                       a frame enters a label state.  The staging reads what other lanes stored: a workgroup barrier
//                       (release / acquire at workgroup scope) stands between the sweep and the walk.
//
// Every value of the lattice is finite (CTC_FLOOR stands for log 0); max-plus has no difference to form at all.
#include "ctc_align.h"
#include "common.h"
#include "row_chunks.h"
#include "../../include/warp_rnnt_amd.h"

// every sum below is rounded on its own
#pragma clang fp contract(off)

namespace rnnt {
namespace {

constexpr int ALIGN_GATHER_THREADS = 256;

// ---------------------------------------------------------------------------------------------------------
// 1. emissions from log-probs
// ---------------------------------------------------------------------------------------------------------
template <typename E>
__global__ void __launch_bounds__(ALIGN_GATHER_THREADS)
k_ctc_align_gather(const E* __restrict__ lp, const int* __restrict__ labels, const int* __restrict__ xn,
                   const int* __restrict__ yn, float* __restrict__ em, unsigned rows, int T, int L, int V, int blank) {
    const int lane = threadIdx.x % WAVE;
    const unsigned row = blockIdx.x * (ALIGN_GATHER_THREADS / WAVE) + threadIdx.x / WAVE;
    if (row >= rows) return;
    const int n = (int)(row / (unsigned)T);
    const CtcLens lens = ctc_lens(xn, yn, n, T, L);
    if ((int)(row - (unsigned)n * T) >= lens.Tn) return;
    const E* xr = lp + (size_t)row * V;
    float* er = em + (size_t)row * (L + 1);
    const int* lab = labels + (size_t)n * L;
    for (int k = lane; k <= lens.Ln; k += WAVE) {
        const int v = k == 0 ? blank : safe_label(lab[k - 1], V, blank);
        er[k] = fmaxf((float)xr[v], CTC_FLOOR);
    }
}

// ---------------------------------------------------------------------------------------------------------
// 2. sweep and walk back
// ---------------------------------------------------------------------------------------------------------
template <int K> struct AlignWord { using type = unsigned; };
template <> struct AlignWord<16> { using type = unsigned long long; };

// The emissions of frames t0 .. t0 + D - 1 as the lane uses them: the blank's, and those of its label positions.  Every
// load is unconditional (a load under a condition is a branch of its own): a frame past the utterance reads row T_n - 1
// and is never used; a position past the labels reads column L_n, a cell the producer wrote, into a state that does not
// exist -- such a state holds some finite value, feeds only states above it, none of which exists, and is neither the end
// state nor on any walk back.  Nothing past row T_n - 1 or column L_n is read.
template <int K, int D>
__device__ __forceinline__ void align_fetch(const float* __restrict__ e0, int W, int col, int Ln, int t0, int Tn,
                                            float (&eb)[D], float (&el)[D][K]) {
#pragma unroll
    for (int d = 0; d < D; ++d) {
        const float* er = e0 + (size_t)min(t0 + d, Tn - 1) * W;
        eb[d] = er[0];
#pragma unroll
        for (int i = 0; i < K; ++i) el[d][i] = er[min(col + i, Ln)];
    }
}

// One frame: b[i], l[i] the blank and the label state of the lane's position i.  Returns the decision word: two bits per
// state, the blank's at 4 i, the label's at 4 i + 2.  The positions are taken from the top, so l[i - 1] is still frame
// t - 1's when position i reads it.
template <int K>
__device__ __forceinline__ typename AlignWord<K>::type align_step(float eb, const float (&el)[K], unsigned skip,
                                                                  float (&b)[K], float (&l)[K]) {
    using Word = typename AlignWord<K>::type;
    const float in = wave_shr1(CTC_FLOOR, l[K - 1]);        // lane j - 1's last label state; nothing in front of lane 0
    Word w = 0;
#pragma unroll
    for (int i = K - 1; i >= 0; --i) {
        const float below = i ? l[i - 1] : in;              // the label state of position j K + i - 1
        // the label state: stay, step from its blank, skip from the label below where the tokens differ
        const float stay = l[i], step = b[i], sk = skip >> i & 1u ? below : CTC_FLOOR;
        const unsigned dl = stay >= step && stay >= sk ? 0u : step >= sk ? 1u : 2u;
        const float ml = fmaxf(fmaxf(stay, step), sk);
        // the blank state: stay, or step from the label below
        const unsigned db = b[i] >= below ? 0u : 1u;
        const float mb = fmaxf(b[i], below);
        l[i] = fmaxf(el[i] + ml, CTC_FLOOR);
        b[i] = fmaxf(eb + mb, CTC_FLOOR);
        w |= (Word)(db | dl << 2) << (4 * i);
    }
    return w;
}

__device__ __forceinline__ void align_fill(int* __restrict__ p, int from, int to, int lane) {
    for (int i = from + lane; i < to; i += WAVE) p[i] = -1;
}

template <int K>
__global__ void __launch_bounds__(WAVE)
k_ctc_align(const float* __restrict__ em, const int* __restrict__ labels, const int* __restrict__ xn,
            const int* __restrict__ yn, typename AlignWord<K>::type* __restrict__ dec, float* __restrict__ scores,
            int* __restrict__ frame_tokens, int* __restrict__ emit_frames, int T, int L, int V, int blank) {
    using Word = typename AlignWord<K>::type;
    constexpr int D = (K >= 8 ? 64 : 32) / K;                                   // frames per fetched block
    constexpr int B = CTC_ALIGN_BLOCK_BYTES / (WAVE * (int)sizeof(Word));       // frames per block of the walk
    __shared__ Word rows[B * WAVE];
    __shared__ int path[B];
    __shared__ float fin[2 * WAVE * K];
    const int n = blockIdx.x, j = threadIdx.x;
    int* ft = frame_tokens + (size_t)n * T;
    int* ef = emit_frames + (size_t)n * L;
    const CtcLens lens = ctc_lens(xn, yn, n, T, L);
    if (!lens.ok) {                       // (the whole wave)
        align_fill(ft, 0, T, j);
        align_fill(ef, 0, L, j);
        if (j == 0) scores[n] = __builtin_nanf("");
        return;
    }
    const int Tn = lens.Tn, Ln = lens.Ln, W = L + 1, col = 1 + j * K;
    const int* lab = labels + (size_t)n * L;
    unsigned skip = 0;
#pragma unroll
    for (int i = 0; i < K; ++i) {
        const int p = j * K + i;
        if (p > 0 && p < Ln && safe_label(lab[p], V, blank) != safe_label(lab[p - 1], V, blank)) skip |= 1u << i;
    }
    const float* e0 = em + (size_t)n * T * W;
    dec += (size_t)n * T * WAVE;

    // ---- the sweep: frame 0, then blocks of D frames, the next block asked for in front of this block's chains ----
    float b[K], l[K];
#pragma unroll
    for (int i = 0; i < K; ++i) b[i] = l[i] = CTC_FLOOR;
    if (j == 0) {
        b[0] = e0[0];
        if (Ln > 0) l[0] = e0[1];
    }
    float eb[D], el[D][K], neb[D], nel[D][K];
    align_fetch<K, D>(e0, W, col, Ln, 1, Tn, eb, el);
    for (int t0 = 1; t0 < Tn; t0 += D) {
        align_fetch<K, D>(e0, W, col, Ln, t0 + D, Tn, neb, nel);
#pragma unroll
        for (int d = 0; d < D; ++d) {
            if (t0 + d < Tn) dec[(size_t)(t0 + d) * WAVE + j] = align_step<K>(eb[d], el[d], skip, b, l);
        }
#pragma unroll
        for (int d = 0; d < D; ++d) {
            eb[d] = neb[d];
#pragma unroll
            for (int i = 0; i < K; ++i) el[d][i] = nel[d][i];
        }
    }

    // ---- the end state ----
#pragma unroll
    for (int i = 0; i < K; ++i) {
        fin[2 * (j * K + i)] = b[i];
        fin[2 * (j * K + i) + 1] = l[i];
    }
    __syncthreads();                      // fin; and the decisions other lanes stored, ordered at workgroup scope
    const float vb = fin[2 * Ln], vl = Ln > 0 ? fin[2 * Ln - 1] : CTC_FLOOR;
    const int end = Ln == 0 || vb >= vl ? 2 * Ln : 2 * Ln - 1;
    const float score = end & 1 ? vl : vb;
    if (score <= 0.5f * CTC_FLOOR) {      // no path (the whole wave)
        align_fill(ft, 0, T, j);
        align_fill(ef, 0, L, j);
        if (j == 0) scores[n] = -__builtin_inff();
        return;
    }
    if (j == 0) scores[n] = score;
    align_fill(ft, Tn, T, j);
    align_fill(ef, Ln, L, j);

    // ---- the walk back, a block of B frames at a time ----
    int s = end;                          // (lane 0's is the path's)
    for (int t0 = (Tn - 1) / B * B; t0 >= 0; t0 -= B) {
        const int t1 = min(t0 + B, Tn);
#pragma unroll 8
        for (int t = max(t0, 1); t < t1; ++t) rows[(t - t0) * WAVE + j] = dec[(size_t)t * WAVE + j];
        __syncthreads();                  // the rows are in LDS
        if (j == 0) {
            for (int t = t1 - 1; t >= t0; --t) {
                int d = 1;                // frame 0: the path enters its state there
                if (t > 0) d = (int)(rows[(t - t0) * WAVE + s / (2 * K)] >> (2 * (s % (2 * K)))) & 3;
                path[t - t0] = s << 2 | d;
                s = max(s - d, 0);
            }
        }
        __syncthreads();                  // the block's states are in LDS
        for (int t = t0 + j; t < t1; t += WAVE) {
            const int c = path[t - t0], st = c >> 2;
            if (st & 1) {                 // (an odd state of 0 .. 2 L_n: position st / 2 < L_n)
                ft[t] = safe_label(lab[st >> 1], V, blank);
                if (c & 3) ef[st >> 1] = t;
            } else {
                ft[t] = blank;
            }
        }
        __syncthreads();                  // rows and path are free for the block below
    }
}

template <int K>
void align_launch(hipStream_t stream, const float* em, const int* labels, const int* xn, const int* yn, void* decisions,
                  float* scores, int* frame_tokens, int* emit_frames, int N, int T, int L, int V, int blank) {
    k_ctc_align<K><<<(unsigned)N, WAVE, 0, stream>>>(em, labels, xn, yn,
                                                     static_cast<typename AlignWord<K>::type*>(decisions), scores,
                                                     frame_tokens, emit_frames, T, L, V, blank);
}

}  // namespace

hipError_t launch_ctc_align_gather(hipStream_t stream, int dtype, const void* log_probs, const int* labels, const int* xn,
                                   const int* yn, float* em, int N, int T, int L, int V, int blank) {
    if (!ctc_shape_ok(N, T, L, V) || blank < 0 || blank >= V) return hipErrorInvalidValue;
    if (N == 0) return hipSuccess;
    const unsigned rows = (unsigned)N * T, per = ALIGN_GATHER_THREADS / WAVE;
    return row_typed(dtype, log_probs, nullptr, [&](auto* x, auto*) {
        k_ctc_align_gather<<<(rows + per - 1) / per, ALIGN_GATHER_THREADS, 0, stream>>>(x, labels, xn, yn, em, rows, T, L, V,
                                                                                      blank);
        return hipGetLastError();
    });
}

hipError_t launch_ctc_align_sweep(hipStream_t stream, const float* em, const int* labels, const int* xn, const int* yn,
                                  void* decisions, float* scores, int* frame_tokens, int* emit_frames, int N, int T, int L,
                                  int V, int blank) {
    if (!ctc_shape_ok(N, T, L, V) || blank < 0 || blank >= V) return hipErrorInvalidValue;
    if (N == 0) return hipSuccess;
    switch (ctc_align_k(L)) {
        case 1: align_launch<1>(stream, em, labels, xn, yn, decisions, scores, frame_tokens, emit_frames, N, T, L, V, blank); break;
        case 2: align_launch<2>(stream, em, labels, xn, yn, decisions, scores, frame_tokens, emit_frames, N, T, L, V, blank); break;
        case 4: align_launch<4>(stream, em, labels, xn, yn, decisions, scores, frame_tokens, emit_frames, N, T, L, V, blank); break;
        case 8: align_launch<8>(stream, em, labels, xn, yn, decisions, scores, frame_tokens, emit_frames, N, T, L, V, blank); break;
        case 16: align_launch<16>(stream, em, labels, xn, yn, decisions, scores, frame_tokens, emit_frames, N, T, L, V, blank); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace rnnt
