// The multi-blank transducer loss, Xu et al. 2022 (include/warp_rnnt_amd_multiblank.h; multiblank.h): a
// producer, the two sweeps, the gradient kernel and the d/d logits kernel.  The lattice is neither the standard one nor
// TDT's: a blank edge jumps d frames, a label edge stays on its frame, one softmax per cell and no duration head.
//
// Per cell, logits z[0..V), sigma >= 0:   lp = log_softmax(z) - sigma.
// Edges out of (t,u), utterance of T_n frames and U_n labels, B blanks (blank_ids[i], d = blank_durations[i]):
//     blank i, weight lp[blank_ids[i]]:  to (t+d, u) if t+d < T_n;  to the end if t+d == T_n and u == U_n
//     label,   weight lp[labels[u]]:     to (t, u+1) if u < U_n
// alpha / beta are the log-sum-exp recurrences over these edges in pull form: the maximum of a cell's terms first, then
// one sum of exponentials with blanks i = 0..B-1 followed by the label, then one log.  costs = -ll, ll = alpha of the end.
// Edge occupancy: exp(alpha(t,u) + w + beta(dest) - ll), label edges times (1 + fastemit_lambda); per cell
//     G_l, G_blank[i],  S = G_l + sum_i G_blank[i]
//     dz[v] = go (p_v S - [v == label] G_l - sum_i [v == blank_ids[i]] G_blank[i])      p = softmax(z)
// rounded once to the logits' type; the label is subtracted first, then i ascending.
//
// The streaming kernels hold a row of V logits by a group of G lanes (16, 32 or 64, by the row's length alone): chunks of
// 8 elements, chunk c on lane c mod G, a running maximum and sum, the xor butterfly of streaming.h -- all of it
// row_chunks.h's, shared with hat.hip and tdt.hip, as are the launch side's lanes per row, workgroups and dispatch.  So a
// row's bits do not depend on the storage type, the access width or where the row lies.  -inf is a masked entry: +0 in
// the sum, and an exactly zero gradient.
//
// The sweeps: one workgroup per utterance and direction, lanes are lattice columns, one wave per 64 columns.  The last
// max(durations)+2 diagonals of alpha (beta) live in an LDS ring, and the waves meet at one workgroup barrier per
// diagonal.  The edge weights of the next diagonal are loaded into the second of two register sets, used in turn in a
// loop unrolled by two: the loads of diagonal d+1 stay in flight across the barrier of diagonal d and nothing is copied
// in front of it.  Nothing waits on memory, nothing passes between workgroups, no atomics, no assembly.
#include "multiblank.h"
#include "row_chunks.h"
#include "../../include/warp_rnnt_amd.h"

// every product and sum below is rounded on its own (hat.hip has the reasons; row_chunks.h sets the same for its own
// functions, which this line, behind the includes, does not reach)
#pragma clang fp contract(off)

namespace rnnt {
namespace {

__host__ __device__ __forceinline__ int mb_mod(int a, int T) {
    const int r = a % T;
    return r < 0 ? r + T : r;
}

// ---------------------------------------------------------------------------------------------------------
// The two streaming kernels
// ---------------------------------------------------------------------------------------------------------
template <typename E, int G, int ACC>
__global__ void __launch_bounds__(ROW_THREADS)
k_mb_plane(const E* __restrict__ x, const int* __restrict__ labels, float* __restrict__ plane, size_t rows, int T, int U,
           int V, MbBlanks bl, float sigma) {
    const size_t row = (size_t)blockIdx.x * (ROW_THREADS / G) + threadIdx.x / G;
    if (row >= rows) return;
    const int lane = threadIdx.x % G;
    const E* xr = x + row * (size_t)V;
    // (label and the 1 + B logits are asked for in front of the row: as in hat.hip)
    const CellMap c = map_cell(row, labels, T, U, V, bl.id[0]);
    const float zl = (float)xr[c.label];
    float zb[MB_MAX_B], m, ls;
#pragma unroll
    for (int i = 0; i < MB_MAX_B; ++i) zb[i] = i < bl.B ? (float)xr[bl.id[i]] : ROW_NEG_INF;
    row_stats<E, G, ACC, true>(xr, lane, V, V, [](int) { return false; }, m, ls);
    if (lane == 0) {
        plane[c.sk] = ((zl - m) - ls) - sigma;
#pragma unroll
        for (int i = 0; i < MB_MAX_B; ++i)
            if (i < bl.B) plane[(size_t)(1 + i) * rows + c.sk] = ((zb[i] - m) - ls) - sigma;
    }
}

template <typename E, int G, int ACC>
__global__ void __launch_bounds__(ROW_THREADS)
k_mb_backward(const E* __restrict__ x, const int* __restrict__ labels, const float* __restrict__ gplane,
              const float* __restrict__ scale, E* __restrict__ out, size_t rows, int T, int U, int V, MbBlanks bl) {
    const size_t row = (size_t)blockIdx.x * (ROW_THREADS / G) + threadIdx.x / G;
    if (row >= rows) return;
    const int lane = threadIdx.x % G;
    const E* xr = x + row * (size_t)V;
    const CellMap c = map_cell(row, labels, T, U, V, bl.id[0]);
    const float sc = scale ? scale[c.n] : 1.0f;
    const float Gl = gplane[c.sk];
    float Gb[MB_MAX_B], m, ls;
#pragma unroll
    for (int i = 0; i < MB_MAX_B; ++i) Gb[i] = i < bl.B ? gplane[(size_t)(1 + i) * rows + c.sk] : 0.0f;
    row_stats<E, G, ACC, false>(xr, lane, V, V, [](int) { return false; }, m, ls);    // (plain loads: the row is read again)
    float S = Gl;
#pragma unroll
    for (int i = 0; i < MB_MAX_B; ++i)
        if (i < bl.B) S += Gb[i];
    E* o = out + row * (size_t)V;
    for (int e0 = lane * ROW_CHUNK; e0 < V; e0 += G * ROW_CHUNK) {
        float z[ROW_CHUNK], d[ROW_CHUNK];
        row_load8<E, ACC, true>(xr, e0, V, z);
#pragma unroll
        for (int k = 0; k < ROW_CHUNK; ++k) d[k] = row_exp((z[k] - m) - ls) * S;      // (z = -inf past V and at masked logits: +0)
        // the chunks that hold the label or a blank: at most 1 + B of the row's; the label first, then i ascending
        if ((unsigned)(c.label - e0) < (unsigned)ROW_CHUNK) {
#pragma unroll
            for (int k = 0; k < ROW_CHUNK; ++k) d[k] = e0 + k == c.label ? d[k] - Gl : d[k];
        }
#pragma unroll
        for (int i = 0; i < MB_MAX_B; ++i) {
            if (i < bl.B && (unsigned)(bl.id[i] - e0) < (unsigned)ROW_CHUNK) {
#pragma unroll
                for (int k = 0; k < ROW_CHUNK; ++k) d[k] = e0 + k == bl.id[i] ? d[k] - Gb[i] : d[k];
            }
        }
#pragma unroll
        for (int k = 0; k < ROW_CHUNK; ++k) d[k] = sc * d[k];
        row_store8<E, ACC>(o, e0, V, d);
    }
}

// ---------------------------------------------------------------------------------------------------------
// The sweeps
// ---------------------------------------------------------------------------------------------------------
// The edge weights of one step: the B blank edges and the label edge; -inf where the lattice has no such edge
struct MbWeights {
    float b[MB_MAX_B];
    float l;
};

// log sum exp of the blank terms tb[i], i < B, and the label term tl: the maximum, one sum with the blanks in the order
// i = 0..B-1 followed by the label, one log; -inf where every term is
__device__ __forceinline__ float mb_lse(const float (&tb)[MB_MAX_B], float tl, int B) {
    float m = tl;
#pragma unroll
    for (int i = 0; i < MB_MAX_B; ++i)
        if (i < B) m = fmaxf(m, tb[i]);
    float s = 0.0f;
#pragma unroll
    for (int i = 0; i < MB_MAX_B; ++i)
        if (i < B) s += row_exp(tb[i] - m);
    s += row_exp(tl - m);
    return m > ROW_NEG_INF ? m + logf(s) : ROW_NEG_INF;
}

// blockIdx.x: the utterance; blockIdx.y: 0 the alpha sweep, 1 the beta sweep.  Lane u is lattice column u; in step d it
// holds cell (d - u, u).  ring: (max duration + 2) rows of blockDim.x floats, diagonal d in row d mod (max duration + 2);
// a cell outside the utterance's window is -inf there.  The end of the lattice is treated as cell (T_n, U_n) on diagonal
// T_n + U_n: blank edges only lead to it, its alpha is ll and its beta is 0.
__global__ void __launch_bounds__(MB_MAX_U)
k_mb_sweep(const float* __restrict__ plane, const int* __restrict__ xn, const int* __restrict__ yn,
           float* __restrict__ alphas, float* __restrict__ betas, float* __restrict__ ll, float* __restrict__ costs,
           MbBlanks bl, size_t cells, int T, int U) {
    extern __shared__ float ring[];
    const int n = blockIdx.x, u = threadIdx.x, ncol = blockDim.x;
    const bool backward = blockIdx.y != 0;
    const int Tn = xn[n], Un = yn[n];
    if (Tn < 1 || Tn > T || Un < 0 || Un >= U) {          // (the whole workgroup)
        if (!backward && u == 0) ll[n] = costs[n] = __builtin_nanf("");
        return;
    }
    const int B = bl.B;
    int longest = 1;
#pragma unroll
    for (int i = 0; i < MB_MAX_B; ++i)
        if (i < B) longest = max(longest, bl.d[i]);
    const int R = longest + 2, last = Tn + Un;
    for (int r = 0; r < R; ++r) ring[r * ncol + u] = ROW_NEG_INF;
    if (backward && u == Un) ring[(last % R) * ncol + u] = 0.0f;
    __syncthreads();
    const size_t base = (size_t)n * T * U;
    const float* pL = plane + base;
    const float* pB = pL + cells;             // blank i: pB + i * cells
    MbWeights wa, wb;                         // the two register sets: one holds this step's weights, the other the next's

    if (!backward) {
        // rows of the plane that hold diagonal d - d_i (blank sources) and d - 1 (the label source) of the step asked for
        int rowB[MB_MAX_B], rowL = mb_mod(-1, T);
#pragma unroll
        for (int i = 0; i < MB_MAX_B; ++i) rowB[i] = mb_mod(-bl.d[i < B ? i : 0], T);
        const int ul = u > 0 ? u - 1 : 0;
        const auto fetch = [&](int d, MbWeights& w) {
            const int t = d - u;
            const bool cell = t >= 0 && t < Tn && u <= Un, end = t == Tn && u == Un;
            w.l = ROW_NEG_INF;
            if (cell && u > 0) w.l = pL[rowL * U + ul];                              // from (t, u - 1)
#pragma unroll
            for (int i = 0; i < MB_MAX_B; ++i) {
                w.b[i] = ROW_NEG_INF;
                if (i < B && (cell || end) && t - bl.d[i] >= 0)                     // from (t - d_i, u)
                    w.b[i] = pB[(size_t)i * cells + (size_t)(rowB[i] * U + u)];
            }
        };
        int slot = 0, row = 0;
        // step d with the weights `cur`; those of step d + 1 are asked for into `next` before anything waits
        const auto step = [&](int d, const MbWeights& cur, MbWeights& next) {
#pragma unroll
            for (int i = 0; i < MB_MAX_B; ++i) rowB[i] = rowB[i] + 1 == T ? 0 : rowB[i] + 1;
            rowL = rowL + 1 == T ? 0 : rowL + 1;
            if (d < last) fetch(d + 1, next);
            const int t = d - u;
            const bool cell = t >= 0 && t < Tn && u <= Un, end = t == Tn && u == Un;
            float tb[MB_MAX_B];
#pragma unroll
            for (int i = 0; i < MB_MAX_B; ++i) {
                tb[i] = ROW_NEG_INF;
                if (i >= B) continue;
                int sb = slot - bl.d[i];
                sb += sb < 0 ? R : 0;
                tb[i] = ring[sb * ncol + u] + cur.b[i];
            }
            const int sl = slot == 0 ? R - 1 : slot - 1;
            const float tl = ring[sl * ncol + ul] + cur.l;
            float v = mb_lse(tb, tl, B);
            v = d == 0 && u == 0 ? 0.0f : v;
            v = cell || end ? v : ROW_NEG_INF;
            ring[slot * ncol + u] = v;
            if (cell) alphas[base + (size_t)row * U + u] = v;
            if (end) {
                ll[n] = v;
                costs[n] = -v;
            }
            slot = slot + 1 == R ? 0 : slot + 1;
            row = row + 1 == T ? 0 : row + 1;
            __syncthreads();
        };
        fetch(0, wa);
        for (int d = 0; d <= last; d += 2) {      // (last is the workgroup's: every lane meets every barrier)
            step(d, wa, wb);
            if (d + 1 <= last) step(d + 1, wb, wa);
        }
    } else {
        const int ur = u + 1 < ncol ? u + 1 : u;
        // the weights of the edges out of the lane's own cell (d - u, u), which sits in row `row` of the plane
        const auto fetch = [&](int d, int row, MbWeights& w) {
            const int t = d - u;
            const bool cell = t >= 0 && t < Tn && u <= Un;
            const int idx = row * U + u;
            w.l = ROW_NEG_INF;
            if (cell && u < Un) w.l = pL[idx];                                       // to (t, u + 1)
#pragma unroll
            for (int i = 0; i < MB_MAX_B; ++i) {
                w.b[i] = ROW_NEG_INF;
                if (i >= B) continue;
                const int di = bl.d[i];
                if (cell && (t + di < Tn || (t + di == Tn && u == Un)))              // to (t + d_i, u), or the end
                    w.b[i] = pB[(size_t)i * cells + (size_t)idx];
            }
        };
        int row = mb_mod(last - 1, T), slot = (last - 1) % R;
        const auto step = [&](int d, const MbWeights& cur, MbWeights& next) {
            const int prev = row == 0 ? T - 1 : row - 1;
            if (d > 0) fetch(d - 1, prev, next);
            const int t = d - u;
            const bool cell = t >= 0 && t < Tn && u <= Un;
            float tb[MB_MAX_B];
#pragma unroll
            for (int i = 0; i < MB_MAX_B; ++i) {
                tb[i] = ROW_NEG_INF;
                if (i >= B) continue;
                int sb = slot + bl.d[i];
                sb -= sb >= R ? R : 0;
                tb[i] = cur.b[i] + ring[sb * ncol + u];
            }
            const int sl = slot + 1 == R ? 0 : slot + 1;
            const float tl = cur.l + ring[sl * ncol + ur];
            const float v = cell ? mb_lse(tb, tl, B) : ROW_NEG_INF;
            ring[slot * ncol + u] = v;
            if (cell) betas[base + (size_t)row * U + u] = v;
            slot = slot == 0 ? R - 1 : slot - 1;
            row = prev;
            __syncthreads();
        };
        fetch(last - 1, row, wa);
        for (int d = last - 1; d >= 0; d -= 2) {
            step(d, wa, wb);
            if (d - 1 >= 0) step(d - 1, wb, wa);
        }
    }
}

// One thread per cell in diagonal-major order (blockIdx.y: the utterance): the 1 + B sums of the cell's edge occupancies
__global__ void __launch_bounds__(ROW_THREADS)
k_mb_grads(const float* __restrict__ plane, const float* __restrict__ alphas, const float* __restrict__ betas,
           const float* __restrict__ ll, const int* __restrict__ xn, const int* __restrict__ yn,
           float* __restrict__ gplane, MbBlanks bl, size_t cells, int T, int U, float label_scale) {
    const int n = blockIdx.y;
    const unsigned at = blockIdx.x * ROW_THREADS + threadIdx.x;
    if (at >= (unsigned)T * (unsigned)U) return;
    const int r = (int)(at / (unsigned)U), u = (int)(at - (unsigned)r * (unsigned)U);
    const int t = mb_mod(r - u, T);
    const int Tn = xn[n], Un = yn[n], B = bl.B;
    const size_t base = (size_t)n * T * U, sk = base + at;
    const bool ok = Tn >= 1 && Tn <= T && Un >= 0 && Un < U;
    float Gl = 0.0f, Gb[MB_MAX_B];
#pragma unroll
    for (int i = 0; i < MB_MAX_B; ++i) Gb[i] = 0.0f;
    if (ok && t < Tn && u <= Un) {
        const float a = alphas[sk], L = ll[n];
        if (u < Un)
            Gl = label_scale * expf(((a + plane[sk]) + betas[base + (size_t)mb_mod(r + 1, T) * U + u + 1]) - L);
#pragma unroll
        for (int i = 0; i < MB_MAX_B; ++i) {
            if (i >= B) continue;
            const int di = bl.d[i];
            if (t + di < Tn)
                Gb[i] = expf(((a + plane[(size_t)(1 + i) * cells + sk]) + betas[base + (size_t)mb_mod(r + di, T) * U + u]) - L);
            else if (t + di == Tn && u == Un)
                Gb[i] = expf((a + plane[(size_t)(1 + i) * cells + sk]) - L);
        }
    }
    gplane[sk] = Gl;
#pragma unroll
    for (int i = 0; i < MB_MAX_B; ++i)
        if (i < B) gplane[(size_t)(1 + i) * cells + sk] = Gb[i];
}

// ---------------------------------------------------------------------------------------------------------
// Launchers
// ---------------------------------------------------------------------------------------------------------
// The form of a streaming call is a function of the row's length V alone (row_group, row_grid)
template <typename E>
hipError_t mb_plane(hipStream_t stream, const E* x, const int* labels, float* plane, int N, int T, int U, int V,
                    const MbBlanks& bl, float sigma) {
    const size_t rows = (size_t)N * T * U;
    if (rows == 0) return hipSuccess;
    const int G = row_group(V);
    const unsigned grid = row_grid(rows, G);
    return row_dispatch<E>(G, row_access<E>(V, x, nullptr), [&](auto g, auto acc) {
        k_mb_plane<E, decltype(g)::value, decltype(acc)::value>
            <<<grid, ROW_THREADS, 0, stream>>>(x, labels, plane, rows, T, U, V, bl, sigma);
    });
}

template <typename E>
hipError_t mb_backward(hipStream_t stream, const E* x, const int* labels, const float* gplane, const float* scale, E* dx,
                       int N, int T, int U, int V, const MbBlanks& bl) {
    const size_t rows = (size_t)N * T * U;
    if (rows == 0) return hipSuccess;
    const int G = row_group(V);
    const unsigned grid = row_grid(rows, G);
    return row_dispatch<E>(G, row_access<E>(V, x, dx), [&](auto g, auto acc) {
        k_mb_backward<E, decltype(g)::value, decltype(acc)::value>
            <<<grid, ROW_THREADS, 0, stream>>>(x, labels, gplane, scale, dx, rows, T, U, V, bl);
    });
}

// what the kernels index with: B blanks whose ids lie in [0,V) and whose durations lie in [1,8]
inline bool mb_blanks_in_range(const MbBlanks& bl, int V) {
    if (bl.B < 1 || bl.B > MB_MAX_B || V < bl.B + 1) return false;
    for (int i = 0; i < bl.B; ++i)
        if (bl.id[i] < 0 || bl.id[i] >= V || bl.d[i] < 1 || bl.d[i] > MB_MAX_DURATION) return false;
    return true;
}

}  // namespace

hipError_t launch_mb_plane(hipStream_t stream, int dtype, const void* logits, const int* labels, float* plane, int N, int T,
                           int U, int V, const MbBlanks& blanks, float sigma) {
    if (!mb_blanks_in_range(blanks, V)) return hipErrorInvalidValue;
    return row_typed(dtype, logits, nullptr,
                     [&](auto* x, auto*) { return mb_plane(stream, x, labels, plane, N, T, U, V, blanks, sigma); });
}

hipError_t launch_mb_sweeps(hipStream_t stream, const float* plane, const int* xn, const int* yn, float* alphas,
                            float* betas, float* ll, float* costs, const MbBlanks& blanks, int N, int T, int U) {
    if (U < 1 || U > MB_MAX_U || blanks.B < 1 || blanks.B > MB_MAX_B) return hipErrorInvalidValue;
    if (N == 0) return hipSuccess;
    int longest = 1;
    for (int i = 0; i < blanks.B; ++i) {
        if (blanks.d[i] < 1 || blanks.d[i] > MB_MAX_DURATION) return hipErrorInvalidValue;
        longest = blanks.d[i] > longest ? blanks.d[i] : longest;
    }
    const int ncol = (U + WAVE - 1) / WAVE * WAVE;
    const size_t lds = (size_t)(longest + 2) * ncol * sizeof(float);          // 40 KB at the most
    k_mb_sweep<<<dim3(N, betas ? 2 : 1), ncol, lds, stream>>>(plane, xn, yn, alphas, betas, ll, costs, blanks,
                                                              (size_t)N * T * U, T, U);
    return hipGetLastError();
}

hipError_t launch_mb_grads(hipStream_t stream, const float* plane, const float* alphas, const float* betas, const float* ll,
                           const int* xn, const int* yn, float* gplane, const MbBlanks& blanks, int N, int T, int U,
                           float fastemit_lambda) {
    if (blanks.B < 1 || blanks.B > MB_MAX_B) return hipErrorInvalidValue;
    if (N == 0) return hipSuccess;
    const unsigned per = ((unsigned)T * (unsigned)U + ROW_THREADS - 1) / ROW_THREADS;
    k_mb_grads<<<dim3(per, N), ROW_THREADS, 0, stream>>>(plane, alphas, betas, ll, xn, yn, gplane, blanks, (size_t)N * T * U,
                                                         T, U, 1.0f + fastemit_lambda);
    return hipGetLastError();
}

hipError_t launch_mb_logits_backward(hipStream_t stream, int dtype, const void* logits, const int* labels,
                                     const float* gplane, const float* scale, void* dlogits, int N, int T, int U, int V,
                                     const MbBlanks& blanks) {
    if (!mb_blanks_in_range(blanks, V)) return hipErrorInvalidValue;
    return row_typed(dtype, logits, dlogits, [&](auto* x, auto* dx) {
        return mb_backward(stream, x, labels, gplane, scale, dx, N, T, U, V, blanks);
    });
}

}  // namespace rnnt
