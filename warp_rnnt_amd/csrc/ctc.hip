// The CTC loss from logits (Graves et al. 2006; include/warp_rnnt_amd_ctc.h has the lattice and the order of every
// operation): four kernels.
//
//   k_ctc_emit         one pass over the logits on row_chunks.h's rows (G = 16, 32 or 64 lanes per row, chunks of 8): the
//                      row goes through LDS as floats while its running (max, log sum) is taken, and the L_n + 1 emissions
//                      of the row -- the blank's and one per label position -- are gathered from LDS, not from memory.
//                      Rows t >= T_n are not read.
//   k_ctc_sweep        one workgroup per (utterance, direction), sequential in t.  Lane l owns the state pair (the blank in
//                      front of label l, label l); lane L_n owns the final blank.  A step needs one value from outside the
//                      lane, the label state of lane l - 1: a DPP wave_shr:1 inside a wave, one LDS word per wave and one
//                      barrier per frame between waves (two words, taken in turn, so one barrier is enough); a lattice of
//                      up to 64 lanes runs without a barrier.  The skip predicate is one register; the emissions of frame
//                      t + 1 are asked for before frame t is computed.  beta is the same recursion on the utterance read
//                      backwards (frames and labels), so it needs lane l - 1 as well, and not two values of lane l + 1.
//   k_ctc_label_order  one workgroup per utterance: the label positions in a stable order by token, the first of every
//                      token marked.  A function of the labels alone.
//   k_ctc_grad         a row (n,t) per group of G lanes: the blank's occupancies added per lane in ascending l and joined
//                      by the xor butterfly; the positions' occupancies added per token by the lane that holds the token's
//                      first position, in the stored order, into a vector of V floats in LDS; then the row streams
//                      through, dlogits = dcost (softmax - occ), whole chunks stored.  No atomics, in LDS or in memory.
//                      Dead rows and utterances without a path are written as zeros and their logits are not read.
//
// Every value of the lattice is finite (CTC_FLOOR stands for log 0), so no difference of infinities is formed anywhere.
#include "ctc.h"
#include "row_chunks.h"
#include "../../include/warp_rnnt_amd.h"

// every product and sum below is rounded on its own (hat.hip has the reasons)
#pragma clang fp contract(off)

namespace rnnt {
namespace {

constexpr int CTC_LDS_FLOATS = 16384;    // a workgroup's LDS: rows of ceil8(V) floats, as many as fit (at least one)
constexpr int CTC_ORDER_THREADS = 256;

// M + log(exp(a-M) + exp(b-M) + exp(c-M)), the sum from the left; finite arguments (>= about 2 CTC_FLOOR) give a finite
// result: exp of a difference that large is +0, and three floors give the floor (log 3 is absorbed)
__device__ __forceinline__ float ctc_lse3(float a, float b, float c) {
    const float m = fmaxf(fmaxf(a, b), c);
    const float s = (row_exp(a - m) + row_exp(b - m)) + row_exp(c - m);
    return m + __builtin_amdgcn_logf(s) * LN2;
}

__device__ __forceinline__ void lds_store8(float* p, const float (&z)[ROW_CHUNK]) {
    reinterpret_cast<float4*>(p)[0] = make_float4(z[0], z[1], z[2], z[3]);
    reinterpret_cast<float4*>(p)[1] = make_float4(z[4], z[5], z[6], z[7]);
}

// ---------------------------------------------------------------------------------------------------------
// 1. emissions
// ---------------------------------------------------------------------------------------------------------
template <typename E, int G, int ACC>
__global__ void __launch_bounds__(ROW_THREADS)
k_ctc_emit(const E* __restrict__ x, const int* __restrict__ labels, const int* __restrict__ xn, const int* __restrict__ yn,
           float2* __restrict__ stats, float* __restrict__ em, unsigned rows, int T, int L, int V, int blank) {
    extern __shared__ __align__(16) float ctc_lds[];
    const int r = threadIdx.x / G, lane = threadIdx.x % G, Vp = (V + ROW_CHUNK - 1) & ~(ROW_CHUNK - 1);
    const unsigned row = blockIdx.x * (blockDim.x / G) + r;
    int n = 0, Ln = 0;
    bool live = false;
    if (row < rows) {
        n = (int)(row / (unsigned)T);
        const CtcLens lens = ctc_lens(xn, yn, n, T, L);
        live = (int)(row - (unsigned)n * T) < lens.Tn;
        Ln = lens.Ln;
    }
    float* zr = ctc_lds + r * Vp;
    const E* xr = x + (size_t)row * V;
    // row_stats' pass (row_chunks.h) with the chunk parked in LDS on its way; a row that is not live runs no chunk
    const int end = live ? V : 0;
    float ml = ROW_NEG_INF, s = 0.0f;
    for (int e0 = lane * ROW_CHUNK; e0 < end; e0 += G * ROW_CHUNK) {
        float z[ROW_CHUNK];
        row_load8<E, ACC, true>(xr, e0, V, z);
        lds_store8(zr + e0, z);
        float mn = ml;
#pragma unroll
        for (int i = 0; i < ROW_CHUNK; ++i) mn = fmaxf(mn, z[i]);
        if (mn > ROW_NEG_INF) {
            s = s * row_exp(ml - mn);
#pragma unroll
            for (int i = 0; i < ROW_CHUNK; ++i) s += row_exp(z[i] - mn);
            ml = mn;
        }
    }
    const float m = group_max<G>(ml);
    const float ls = logf(group_sum<G>(s * row_exp(ml - m)));
    __syncthreads();                      // the row is in LDS
    if (!live) return;
    if (lane == 0) stats[row] = make_float2(m, ls);
    float* er = em + (size_t)row * (L + 1);
    const int* lab = labels + (size_t)n * L;
    for (int k = lane; k <= Ln; k += G) {
        const int v = k == 0 ? blank : safe_label(lab[k - 1], V, blank);
        er[k] = fmaxf((zr[v] - m) - ls, CTC_FLOOR);
    }
}

// ---------------------------------------------------------------------------------------------------------
// 2. the sweeps: direction 0 is alpha, 1 is beta; grid (N, directions), 64 * ceil((L+1) / 64) lanes
// ---------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(CTC_MAX_L + 1)
k_ctc_sweep(const float* __restrict__ em, const int* __restrict__ labels, const int* __restrict__ xn,
            const int* __restrict__ yn, float* __restrict__ alpha, float* __restrict__ beta, float* __restrict__ ll,
            float* __restrict__ costs, int T, int L, int V, int blank, int first_direction) {
    __shared__ float edge[2][(CTC_MAX_L + 1) / WAVE];
    const int n = blockIdx.x, dir = first_direction + blockIdx.y, j = threadIdx.x, wave = j / WAVE;
    const bool many = blockDim.x > WAVE, wave_head = j % WAVE == 0 && wave > 0;
    const CtcLens lens = ctc_lens(xn, yn, n, T, L);
    if (!lens.ok) {                       // (the whole workgroup)
        if (dir == 0 && j == 0) ll[n] = costs[n] = __builtin_nanf("");
        return;
    }
    const int Tn = lens.Tn, Ln = lens.Ln;
    // the lane's blank and label as positions of the utterance: read backwards for beta
    const bool has_b = j <= Ln, has_l = j < Ln;
    const int bi = dir ? Ln - j : j, li = dir ? Ln - 1 - j : j;
    const int* lab = labels + (size_t)n * L;
    bool skip = false;
    if (has_l && j > 0) skip = safe_label(lab[li], V, blank) != safe_label(lab[dir ? li + 1 : li - 1], V, blank);
    float* plane = dir ? beta : alpha;
    const size_t W = (size_t)L + 1, row0 = (size_t)n * T;
    size_t row = row0 + (dir ? Tn - 1 : 0);
    float eb = has_b ? em[row * W] : CTC_FLOOR, el = has_l ? em[row * W + 1 + li] : CTC_FLOOR;
    float b = CTC_FLOOR, l = CTC_FLOOR;
    for (int s = 0; s < Tn; ++s) {
        // the next frame's emissions, asked for in front of this frame's chain
        size_t nrow = row;
        float neb = CTC_FLOOR, nel = CTC_FLOOR;
        if (s + 1 < Tn) {
            nrow = row0 + (dir ? Tn - 2 - s : s + 1);
            if (has_b) neb = em[nrow * W];
            if (has_l) nel = em[nrow * W + 1 + li];
        }
        if (s == 0) {
            b = j == 0 ? eb : CTC_FLOOR;
            l = j == 0 && has_l ? el : CTC_FLOOR;
        } else {
            float pl = wave_shr1(CTC_FLOOR, l);                      // lane j - 1's label state; nothing in front of lane 0
            if (many && wave_head) pl = edge[(s - 1) & 1][wave - 1];
            const float nb = fmaxf(eb + ctc_lse3(b, pl, CTC_FLOOR), CTC_FLOOR);
            const float nl = fmaxf(el + ctc_lse3(l, b, skip ? pl : CTC_FLOOR), CTC_FLOOR);
            b = has_b ? nb : CTC_FLOOR;
            l = has_l ? nl : CTC_FLOOR;
        }
        if (has_b) plane[(row * 2) * W + bi] = b;
        if (has_l) plane[(row * 2 + 1) * W + li] = l;
        if (many) {                       // (the words are taken in turn: a wave writes edge[s & 1] again only behind the
            if (j % WAVE == WAVE - 1) edge[s & 1][wave] = l;          //  barrier of step s + 1, which every reader of
            __syncthreads();                                         //  step s + 1 has passed)
        }
        eb = neb, el = nel, row = nrow;
    }
    if (dir == 0) {
        float pl = wave_shr1(CTC_FLOOR, l);
        if (many && wave_head) pl = edge[(Tn - 1) & 1][wave - 1];
        if (j == Ln) {
            const float v = ctc_lse3(b, pl, CTC_FLOOR);
            ll[n] = v;
            costs[n] = v <= 0.5f * CTC_FLOOR ? __builtin_inff() : -v;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------
// 3. the label positions in a stable order by token
// ---------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(CTC_ORDER_THREADS)
k_ctc_label_order(const int* __restrict__ labels, const int* __restrict__ xn, const int* __restrict__ yn,
                  int* __restrict__ order, int T, int L, int V, int blank) {
    __shared__ int tok[CTC_MAX_L + 1];
    const int n = blockIdx.x;
    const CtcLens lens = ctc_lens(xn, yn, n, T, L);
    const int Ln = lens.Ln;               // (0 where the lengths are refused: nothing is read or written)
    for (int i = threadIdx.x; i < Ln; i += CTC_ORDER_THREADS) tok[i] = safe_label(labels[(size_t)n * L + i], V, blank);
    __syncthreads();
    for (int i = threadIdx.x; i < Ln; i += CTC_ORDER_THREADS) {
        const int v = tok[i];
        int rank = 0, same_before = 0;
        for (int k = 0; k < Ln; ++k) {
            const int u = tok[k];
            rank += u < v;
            same_before += u == v && k < i;
        }
        order[(size_t)n * L + rank + same_before] = i | (same_before == 0 ? CTC_ORDER_HEAD : 0);
    }
}

// ---------------------------------------------------------------------------------------------------------
// 4. d/d logits
// ---------------------------------------------------------------------------------------------------------
template <typename E, int G, int ACC>
__global__ void __launch_bounds__(ROW_THREADS)
k_ctc_grad(const E* __restrict__ x, const int* __restrict__ labels, const int* __restrict__ xn, const int* __restrict__ yn,
           const float2* __restrict__ stats, const float* __restrict__ em, const float* __restrict__ alpha,
           const float* __restrict__ beta, const float* __restrict__ ll, const int* __restrict__ order,
           const float* __restrict__ dcosts, E* __restrict__ out, unsigned rows, int T, int L, int V, int blank) {
    extern __shared__ __align__(16) float ctc_lds[];
    const int r = threadIdx.x / G, lane = threadIdx.x % G, Vp = (V + ROW_CHUNK - 1) & ~(ROW_CHUNK - 1);
    const unsigned row = blockIdx.x * (blockDim.x / G) + r;
    int n = 0, Ln = 0;
    float llv = 0.0f;
    bool live = false;
    if (row < rows) {
        n = (int)(row / (unsigned)T);
        const CtcLens lens = ctc_lens(xn, yn, n, T, L);
        llv = ll[n];                      // (NaN where the lengths are refused, the floor where there is no path)
        live = (int)(row - (unsigned)n * T) < lens.Tn && llv > 0.5f * CTC_FLOOR;
        Ln = lens.Ln;
    }
    float* occ = ctc_lds + r * Vp;
    const size_t W = (size_t)L + 1;
    const float* er = em + (size_t)row * W;
    const float *aB = alpha + ((size_t)row * 2) * W, *aL = aB + W, *bB = beta + ((size_t)row * 2) * W, *bL = bB + W;
    const float zero8[ROW_CHUNK] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    float bsum = 0.0f;
    if (live) {
        for (int e0 = lane * ROW_CHUNK; e0 < Vp; e0 += G * ROW_CHUNK) lds_store8(occ + e0, zero8);
        const float eb = er[0];
        for (int k = lane; k <= Ln; k += G) bsum += row_exp(((aB[k] + bB[k]) - eb) - llv);
    }
    bsum = group_sum<G>(bsum);
    __syncthreads();                      // the vector is clear
    if (live) {
        const int* ord = order + (size_t)n * L;
        const int* lab = labels + (size_t)n * L;
        for (int k = lane; k < Ln; k += G) {
            int e = ord[k];
            if (!(e & CTC_ORDER_HEAD)) continue;
            const int head = min(e & (CTC_ORDER_HEAD - 1), L - 1);
            float sum = 0.0f;
            for (int kk = k;;) {
                const int pos = min(e & (CTC_ORDER_HEAD - 1), L - 1);
                sum += row_exp(((aL[pos] + bL[pos]) - er[1 + pos]) - llv);
                if (++kk >= Ln) break;
                e = ord[kk];
                if (e & CTC_ORDER_HEAD) break;
            }
            occ[safe_label(lab[head], V, blank)] = sum;             // (one head per token: no two lanes write one word)
        }
    }
    __syncthreads();                      // the vector is filled
    if (row >= rows) return;
    E* o = out + (size_t)row * V;
    if (!live) {
        for (int e0 = lane * ROW_CHUNK; e0 < V; e0 += G * ROW_CHUNK) row_store8<E, ACC>(o, e0, V, zero8);
        return;
    }
    const E* xr = x + (size_t)row * V;
    const float2 st = stats[row];
    const float dc = dcosts ? dcosts[n] : 1.0f;
    for (int e0 = lane * ROW_CHUNK; e0 < V; e0 += G * ROW_CHUNK) {
        float z[ROW_CHUNK], d[ROW_CHUNK];
        row_load8<E, ACC, true>(xr, e0, V, z);
#pragma unroll
        for (int i = 0; i < ROW_CHUNK; ++i) {
            const float taken = e0 + i == blank ? occ[e0 + i] + bsum : occ[e0 + i];
            d[i] = dc * (row_exp((z[i] - st.x) - st.y) - taken);
        }
        row_store8<E, ACC>(o, e0, V, d);
    }
}

// Rows per workgroup and its LDS: ROW_THREADS / G rows where they fit, fewer for a long row (V = 16384: one)
inline int ctc_rows_per_group(int G, int V) {
    const int Vp = (V + ROW_CHUNK - 1) & ~(ROW_CHUNK - 1), fit = CTC_LDS_FLOATS / Vp;
    return fit < ROW_THREADS / G ? fit : ROW_THREADS / G;
}

hipError_t ctc_sweep(hipStream_t stream, const int* labels, const int* xn, const int* yn, const CtcWorkspace& w,
                     float* costs, int N, int T, int L, int V, int blank, int direction) {
    const unsigned threads = (unsigned)((L + 1 + WAVE - 1) / WAVE * WAVE);
    k_ctc_sweep<<<dim3((unsigned)N, 1), threads, 0, stream>>>(w.E, labels, xn, yn, w.alpha, w.beta, w.ll, costs, T, L, V,
                                                             blank, direction);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_ctc_emit(hipStream_t stream, int dtype, const void* logits, const int* labels, const int* xn,
                           const int* yn, float2* stats, float* em, int N, int T, int L, int V, int blank) {
    if (!ctc_shape_ok(N, T, L, V) || blank < 0 || blank >= V) return hipErrorInvalidValue;
    if (N == 0) return hipSuccess;
    const unsigned rows = (unsigned)N * T;
    return row_typed(dtype, logits, nullptr, [&](auto* x, auto*) {
        using E = std::remove_cv_t<std::remove_pointer_t<decltype(x)>>;
        const int G = row_group(V), R = ctc_rows_per_group(G, V), Vp = (V + ROW_CHUNK - 1) & ~(ROW_CHUNK - 1);
        return row_dispatch<E>(G, row_access<E>(V, x, nullptr), [&](auto g, auto acc) {
            k_ctc_emit<E, decltype(g)::value, decltype(acc)::value>
                <<<(rows + R - 1) / R, R * G, (size_t)R * Vp * sizeof(float), stream>>>(x, labels, xn, yn, stats, em, rows,
                                                                                      T, L, V, blank);
        });
    });
}

hipError_t launch_ctc_forward(hipStream_t stream, int dtype, const void* logits, const int* labels, const int* xn,
                              const int* yn, const CtcWorkspace& w, float* costs, int N, int T, int L, int V, int blank) {
    if (!ctc_shape_ok(N, T, L, V) || blank < 0 || blank >= V) return hipErrorInvalidValue;
    if (N == 0) return hipSuccess;
    const hipError_t e = launch_ctc_emit(stream, dtype, logits, labels, xn, yn, w.stats, w.E, N, T, L, V, blank);
    if (e != hipSuccess) return e;
    return ctc_sweep(stream, labels, xn, yn, w, costs, N, T, L, V, blank, 0);
}

hipError_t launch_ctc_backward(hipStream_t stream, int dtype, const void* logits, const int* labels, const int* xn,
                               const int* yn, const CtcWorkspace& w, const float* dcosts, void* dlogits, int N, int T,
                               int L, int V, int blank) {
    if (!ctc_shape_ok(N, T, L, V) || blank < 0 || blank >= V) return hipErrorInvalidValue;
    if (N == 0) return hipSuccess;
    const hipError_t e = ctc_sweep(stream, labels, xn, yn, w, nullptr, N, T, L, V, blank, 1);
    if (e != hipSuccess) return e;
    k_ctc_label_order<<<(unsigned)N, CTC_ORDER_THREADS, 0, stream>>>(labels, xn, yn, w.order, T, L, V, blank);
    if (hipGetLastError() != hipSuccess) return hipErrorLaunchFailure;
    const unsigned rows = (unsigned)N * T;
    return row_typed(dtype, logits, dlogits, [&](auto* x, auto* dx) {
        using E = std::remove_cv_t<std::remove_pointer_t<decltype(x)>>;
        const int G = row_group(V), R = ctc_rows_per_group(G, V), Vp = (V + ROW_CHUNK - 1) & ~(ROW_CHUNK - 1);
        return row_dispatch<E>(G, row_access<E>(V, x, dx), [&](auto g, auto acc) {
            k_ctc_grad<E, decltype(g)::value, decltype(acc)::value>
                <<<(rows + R - 1) / R, R * G, (size_t)R * Vp * sizeof(float), stream>>>(
                    x, labels, xn, yn, w.stats, w.E, w.alpha, w.beta, w.ll, w.order, dcosts, dx, rows, T, L, V, blank);
        });
    });
}

}  // namespace rnnt
