// The token-and-duration transducer (TDT) loss, Xu et al. 2023 (include/warp_rnnt_amd_tdt.h; tdt.h): a
// producer, the two sweeps, the gradient kernel and the d/d logits kernel.  Nothing of the standard lattice serves here:
// a cell has up to 2D-1 incoming edges from up to max(durations)+1 earlier anti-diagonals.
//
// Per cell, logits z[0..V+D), sigma >= 0:   tok = log_softmax(z[:V]) - sigma,   dur = log_softmax(z[V:]).
// Edges out of (t,u), utterance of T_n frames and U_n labels, duration d = durations[i]:
//     blank, d > 0,  weight tok[blank] + dur[i]:        to (t+d, u) if t+d < T_n;  to the end if t+d == T_n and u == U_n
//     label, d >= 0, weight tok[labels[u]] + dur[i]:    to (t+d, u+1) if u < U_n and t+d < T_n
// alpha / beta are the log-sum-exp recurrences over these edges in pull form: the maximum of a cell's terms first, then
// one sum of exponentials in the order i = 0..D-1, blank before label, then one log.  costs = -ll, ll = alpha of the end.
// Edge occupancy: exp(alpha(t,u) + w + beta(dest) - ll), label edges times (1 + fastemit_lambda); per cell
//     G_b = sum_i blank_i,  G_l = sum_i label_i,  G_dur[i] = blank_i + label_i,  S = G_b + G_l
//     dz[v]   = go (p_v S - [v == blank] G_b - [v == label] G_l)      p = softmax(z[:V])
//     dz[V+i] = go (q_i S - G_dur[i])                                 q = softmax(z[V:])
// rounded once to the logits' type.
//
// The streaming kernels hold a row of V+D logits by a group of G lanes (16, 32 or 64, by the row's length alone): the row
// is cut into chunks of 8 elements, chunk c belongs to lane c mod G, a lane runs over its chunks in ascending order
// keeping a running maximum and sum of the TOKEN logits, the lanes are combined by the xor butterfly of streaming.h --
// all of it row_chunks.h's, shared with hat.hip, as are the launch side's lanes per row, workgroups and dispatch.  The D
// duration logits are read by every lane as single elements and reduced in the order i = 0..D-1.  So a row's bits do not
// depend on the storage type, the access width or where the row lies.  -inf is a masked entry: +0 in both sums, and an
// exactly zero gradient.
//
// The sweeps: one workgroup per utterance and direction, lanes are lattice columns, one wave per 64 columns.  The last
// max(durations)+2 diagonals of alpha (beta) live in an LDS ring -- the one being written and the max(durations)+1 that
// are read -- and the waves meet at one workgroup barrier per diagonal.  The edge weights of the next diagonal are asked
// for in front of that barrier.  Nothing waits on memory, nothing passes between workgroups, no atomics, no assembly.
#include "tdt.h"
#include "row_chunks.h"
#include "../../include/warp_rnnt_amd.h"

// every product and sum below is rounded on its own (hat.hip has the reasons; row_chunks.h sets the same for its own
// functions, which this line, behind the includes, does not reach)
#pragma clang fp contract(off)

namespace rnnt {
namespace {

__host__ __device__ __forceinline__ int tdt_mod(int a, int T) {
    const int r = a % T;
    return r < 0 ? r + T : r;
}

// ---------------------------------------------------------------------------------------------------------
// The two streaming kernels
// ---------------------------------------------------------------------------------------------------------
// (max, log sum) of the token logits z[0..V) of the row at xr, whose pitch is W = V + D: a chunk's duration logits masked
template <typename E, int G, int ACC, bool NT>
__device__ __forceinline__ void tdt_token_stats(const E* __restrict__ xr, int lane, int V, int W, float& m, float& ls) {
    row_stats<E, G, ACC, NT>(xr, lane, V, W, [V](int idx) { return idx >= V; }, m, ls);
}

// The D duration logits of the row, and their (max, log sum); every lane does this for itself
__device__ __forceinline__ void tdt_duration_stats(const float (&zd)[TDT_MAX_D], int D, float& m, float& ls) {
    m = ROW_NEG_INF;
#pragma unroll
    for (int i = 0; i < TDT_MAX_D; ++i)
        if (i < D) m = fmaxf(m, zd[i]);
    float s = 0.0f;
#pragma unroll
    for (int i = 0; i < TDT_MAX_D; ++i)
        if (i < D) s += row_exp(zd[i] - m);
    ls = logf(s);
}
template <typename E>
__device__ __forceinline__ void tdt_load_durations(const E* __restrict__ xr, int V, int D, float (&zd)[TDT_MAX_D]) {
#pragma unroll
    for (int i = 0; i < TDT_MAX_D; ++i) zd[i] = i < D ? (float)xr[V + i] : ROW_NEG_INF;
}

template <typename E, int G, int ACC>
__global__ void __launch_bounds__(ROW_THREADS)
k_tdt_plane(const E* __restrict__ x, const int* __restrict__ labels, float* __restrict__ plane, size_t rows, int T, int U,
            int V, int D, int blank, float sigma) {
    const size_t row = (size_t)blockIdx.x * (ROW_THREADS / G) + threadIdx.x / G;
    if (row >= rows) return;
    const int lane = threadIdx.x % G, W = V + D;
    const E* xr = x + row * (size_t)W;
    // (label, the two token logits and the duration logits are asked for in front of the row: as in hat.hip)
    const CellMap c = map_cell(row, labels, T, U, V, blank);
    const float zb = (float)xr[blank], zl = (float)xr[c.label];
    float zd[TDT_MAX_D], m, ls, md, lsd;
    tdt_load_durations(xr, V, D, zd);
    tdt_token_stats<E, G, ACC, true>(xr, lane, V, W, m, ls);
    tdt_duration_stats(zd, D, md, lsd);
    if (lane == 0) {
        plane[c.sk] = ((zb - m) - ls) - sigma;
        plane[rows + c.sk] = ((zl - m) - ls) - sigma;
#pragma unroll
        for (int i = 0; i < TDT_MAX_D; ++i)
            if (i < D) plane[(size_t)(2 + i) * rows + c.sk] = (zd[i] - md) - lsd;
    }
}

template <typename E, int G, int ACC>
__global__ void __launch_bounds__(ROW_THREADS)
k_tdt_backward(const E* __restrict__ x, const int* __restrict__ labels, const float* __restrict__ gplane,
               const float* __restrict__ scale, E* __restrict__ out, size_t rows, int T, int U, int V, int D, int blank) {
    const size_t row = (size_t)blockIdx.x * (ROW_THREADS / G) + threadIdx.x / G;
    if (row >= rows) return;
    const int lane = threadIdx.x % G, W = V + D;
    const E* xr = x + row * (size_t)W;
    const CellMap c = map_cell(row, labels, T, U, V, blank);
    const float sc = scale ? scale[c.n] : 1.0f;
    const float Gb = gplane[c.sk], Gl = gplane[rows + c.sk];
    float zd[TDT_MAX_D], dd[TDT_MAX_D], m, ls, md, lsd;
    tdt_load_durations(xr, V, D, zd);
#pragma unroll
    for (int i = 0; i < TDT_MAX_D; ++i) dd[i] = i < D ? gplane[(size_t)(2 + i) * rows + c.sk] : 0.0f;
    tdt_token_stats<E, G, ACC, false>(xr, lane, V, W, m, ls);       // (plain loads: the output pass reads the row again)
    tdt_duration_stats(zd, D, md, lsd);
    const float S = Gb + Gl;
#pragma unroll
    for (int i = 0; i < TDT_MAX_D; ++i) dd[i] = sc * (row_exp((zd[i] - md) - lsd) * S - dd[i]);     // dz[V+i]
    E* o = out + row * (size_t)W;
    for (int e0 = lane * ROW_CHUNK; e0 < W; e0 += G * ROW_CHUNK) {
        float z[ROW_CHUNK], d[ROW_CHUNK];
        row_load8<E, ACC, true>(xr, e0, W, z);
#pragma unroll
        for (int i = 0; i < ROW_CHUNK; ++i) {
            const int idx = e0 + i;
            float g = row_exp((z[i] - m) - ls) * S;                 // (z = -inf past W and at masked logits: +0)
            g = idx == blank ? g - Gb : g;
            g = idx == c.label ? g - Gl : g;
            d[i] = sc * g;
        }
        if (e0 + ROW_CHUNK > V) {             // the chunks that hold duration logits: the last one or two of the row
#pragma unroll
            for (int i = 0; i < ROW_CHUNK; ++i) {
#pragma unroll
                for (int k = 0; k < TDT_MAX_D; ++k) d[i] = e0 + i - V == k ? dd[k] : d[i];
            }
        }
        row_store8<E, ACC>(o, e0, W, d);
    }
}

// ---------------------------------------------------------------------------------------------------------
// The sweeps
// ---------------------------------------------------------------------------------------------------------
typedef float TdtTerms[TDT_MAX_D];

// log sum exp of the blank terms tb[i] and the label terms tl[i], i < D; -inf where every term is
__device__ __forceinline__ float tdt_lse(const TdtTerms& tb, const TdtTerms& tl, int D) {
    float m = ROW_NEG_INF;
#pragma unroll
    for (int i = 0; i < TDT_MAX_D; ++i)
        if (i < D) m = fmaxf(m, fmaxf(tb[i], tl[i]));
    float s = 0.0f;
#pragma unroll
    for (int i = 0; i < TDT_MAX_D; ++i)
        if (i < D) {
            s += row_exp(tb[i] - m);
            s += row_exp(tl[i] - m);
        }
    return m > ROW_NEG_INF ? m + logf(s) : ROW_NEG_INF;
}

// blockIdx.x: the utterance; blockIdx.y: 0 the alpha sweep, 1 the beta sweep.  Lane u is lattice column u; in step d it
// holds cell (d - u, u).  ring: (max duration + 2) rows of blockDim.x floats, diagonal d in row d mod (max duration + 2);
// a cell outside the utterance's window is -inf there.  The end of the lattice is treated as cell (T_n, U_n) on diagonal
// T_n + U_n: blank edges only lead to it, its alpha is ll and its beta is 0.
__global__ void __launch_bounds__(TDT_MAX_U)
k_tdt_sweep(const float* __restrict__ plane, const int* __restrict__ xn, const int* __restrict__ yn,
            float* __restrict__ alphas, float* __restrict__ betas, float* __restrict__ ll, float* __restrict__ costs,
            TdtDurations dur, size_t cells, int T, int U) {
    extern __shared__ float ring[];
    const int n = blockIdx.x, u = threadIdx.x, ncol = blockDim.x;
    const bool backward = blockIdx.y != 0;
    const int Tn = xn[n], Un = yn[n];
    if (Tn < 1 || Tn > T || Un < 0 || Un >= U) {          // (the whole workgroup)
        if (!backward && u == 0) ll[n] = costs[n] = __builtin_nanf("");
        return;
    }
    const int D = dur.D;
    int longest = 0;
#pragma unroll
    for (int i = 0; i < TDT_MAX_D; ++i)
        if (i < D) longest = max(longest, dur.d[i]);
    const int R = longest + 2, last = Tn + Un;
    for (int r = 0; r < R; ++r) ring[r * ncol + u] = ROW_NEG_INF;
    if (backward && u == Un) ring[(last % R) * ncol + u] = 0.0f;
    __syncthreads();
    const size_t base = (size_t)n * T * U;
    const float* pB = plane + base;
    const float* pL = pB + cells;
    const float* pD = pL + cells;             // channel i: pD + i * cells
    TdtTerms cb, cl, nb, nl, tb, tl;          // the edge weights of this step and of the next, the terms of this one

    if (!backward) {
        // rows of the plane that hold diagonals d - d_i (blank sources) and d - d_i - 1 (label sources) of the step asked for
        int rowB[TDT_MAX_D], rowL[TDT_MAX_D];
#pragma unroll
        for (int i = 0; i < TDT_MAX_D; ++i) {
            rowB[i] = tdt_mod(-dur.d[i < D ? i : 0], T);
            rowL[i] = tdt_mod(-dur.d[i < D ? i : 0] - 1, T);
        }
        const int ul = u > 0 ? u - 1 : 0;
        const auto fetch = [&](int d, TdtTerms& wb, TdtTerms& wl) {
            const int t = d - u;
            const bool cell = t >= 0 && t < Tn && u <= Un, end = t == Tn && u == Un;
#pragma unroll
            for (int i = 0; i < TDT_MAX_D; ++i) {
                wb[i] = wl[i] = ROW_NEG_INF;
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
        fetch(0, cb, cl);
        int slot = 0, row = 0;
        for (int d = 0; d <= last; ++d) {
#pragma unroll
            for (int i = 0; i < TDT_MAX_D; ++i) {
                rowB[i] = rowB[i] + 1 == T ? 0 : rowB[i] + 1;
                rowL[i] = rowL[i] + 1 == T ? 0 : rowL[i] + 1;
            }
            if (d < last) fetch(d + 1, nb, nl);
            const int t = d - u;
            const bool cell = t >= 0 && t < Tn && u <= Un, end = t == Tn && u == Un;
#pragma unroll
            for (int i = 0; i < TDT_MAX_D; ++i) {
                if (i >= D) continue;
                int sb = slot - dur.d[i], sl = slot - dur.d[i] - 1;
                sb += sb < 0 ? R : 0;
                sl += sl < 0 ? R : 0;
                tb[i] = ring[sb * ncol + u] + cb[i];
                tl[i] = ring[sl * ncol + ul] + cl[i];
            }
            float v = tdt_lse(tb, tl, D);
            v = d == 0 && u == 0 ? 0.0f : v;
            v = cell || end ? v : ROW_NEG_INF;
            ring[slot * ncol + u] = v;
            if (cell) alphas[base + (size_t)row * U + u] = v;
            if (end) {
                ll[n] = v;
                costs[n] = -v;
            }
#pragma unroll
            for (int i = 0; i < TDT_MAX_D; ++i) {
                cb[i] = nb[i];
                cl[i] = nl[i];
            }
            slot = slot + 1 == R ? 0 : slot + 1;
            row = row + 1 == T ? 0 : row + 1;
            __syncthreads();
        }
    } else {
        const int ur = u + 1 < ncol ? u + 1 : u;
        // the weights of the edges out of the lane's own cell (d - u, u), which sits in row `row` of the plane
        const auto fetch = [&](int d, int row, TdtTerms& wb, TdtTerms& wl) {
            const int t = d - u;
            const bool cell = t >= 0 && t < Tn && u <= Un;
#pragma unroll
            for (int i = 0; i < TDT_MAX_D; ++i) wb[i] = wl[i] = ROW_NEG_INF;
            if (!cell) return;
            const int idx = row * U + u;
            const float b = pB[idx], l = pL[idx];
#pragma unroll
            for (int i = 0; i < TDT_MAX_D; ++i) {
                if (i >= D) continue;
                const int di = dur.d[i];
                const float dv = pD[(size_t)i * cells + idx];
                if (di > 0 && (t + di < Tn || (t + di == Tn && u == Un))) wb[i] = b + dv;      // to (t + d_i, u), or the end
                if (u < Un && t + di < Tn) wl[i] = l + dv;                                     // to (t + d_i, u + 1)
            }
        };
        int row = tdt_mod(last - 1, T), slot = (last - 1) % R;
        fetch(last - 1, row, cb, cl);
        for (int d = last - 1; d >= 0; --d) {
            const int prev = row == 0 ? T - 1 : row - 1;
            if (d > 0) fetch(d - 1, prev, nb, nl);
            const int t = d - u;
            const bool cell = t >= 0 && t < Tn && u <= Un;
#pragma unroll
            for (int i = 0; i < TDT_MAX_D; ++i) {
                if (i >= D) continue;
                int sb = slot + dur.d[i], sl = slot + dur.d[i] + 1;
                sb -= sb >= R ? R : 0;
                sl -= sl >= R ? R : 0;
                tb[i] = cb[i] + ring[sb * ncol + u];
                tl[i] = cl[i] + ring[sl * ncol + ur];
            }
            const float v = cell ? tdt_lse(tb, tl, D) : ROW_NEG_INF;
            ring[slot * ncol + u] = v;
            if (cell) betas[base + (size_t)row * U + u] = v;
#pragma unroll
            for (int i = 0; i < TDT_MAX_D; ++i) {
                cb[i] = nb[i];
                cl[i] = nl[i];
            }
            slot = slot == 0 ? R - 1 : slot - 1;
            row = prev;
            __syncthreads();
        }
    }
}

// One thread per cell in diagonal-major order (blockIdx.y: the utterance): the 2 + D sums of the cell's edge occupancies
__global__ void __launch_bounds__(ROW_THREADS)
k_tdt_grads(const float* __restrict__ plane, const float* __restrict__ alphas, const float* __restrict__ betas,
            const float* __restrict__ ll, const int* __restrict__ xn, const int* __restrict__ yn,
            float* __restrict__ gplane, TdtDurations dur, size_t cells, int T, int U, float label_scale) {
    const int n = blockIdx.y;
    const unsigned at = blockIdx.x * ROW_THREADS + threadIdx.x;
    if (at >= (unsigned)T * (unsigned)U) return;
    const int r = (int)(at / (unsigned)U), u = (int)(at - (unsigned)r * (unsigned)U);
    const int t = tdt_mod(r - u, T);
    const int Tn = xn[n], Un = yn[n], D = dur.D;
    const size_t base = (size_t)n * T * U, sk = base + at;
    const bool ok = Tn >= 1 && Tn <= T && Un >= 0 && Un < U;
    float Gb = 0.0f, Gl = 0.0f, Gd[TDT_MAX_D];
#pragma unroll
    for (int i = 0; i < TDT_MAX_D; ++i) Gd[i] = 0.0f;
    if (ok && t < Tn && u <= Un) {
        const float a = alphas[sk], b = plane[sk], l = plane[cells + sk], L = ll[n];
#pragma unroll
        for (int i = 0; i < TDT_MAX_D; ++i) {
            if (i >= D) continue;
            const int di = dur.d[i];
            const float dv = plane[(size_t)(2 + i) * cells + sk];
            float gb = 0.0f, gl = 0.0f;
            if (di > 0 && t + di < Tn)
                gb = expf(((a + (b + dv)) + betas[base + (size_t)tdt_mod(r + di, T) * U + u]) - L);
            else if (di > 0 && t + di == Tn && u == Un)
                gb = expf((a + (b + dv)) - L);
            if (u < Un && t + di < Tn)
                gl = label_scale * expf(((a + (l + dv)) + betas[base + (size_t)tdt_mod(r + di + 1, T) * U + u + 1]) - L);
            Gb += gb;
            Gl += gl;
            Gd[i] = gb + gl;
        }
    }
    gplane[sk] = Gb;
    gplane[cells + sk] = Gl;
#pragma unroll
    for (int i = 0; i < TDT_MAX_D; ++i)
        if (i < D) gplane[(size_t)(2 + i) * cells + sk] = Gd[i];
}

// ---------------------------------------------------------------------------------------------------------
// Launchers
// ---------------------------------------------------------------------------------------------------------
// The form of a streaming call is a function of the row's length W = V + D alone (row_group, row_grid)
template <typename E>
hipError_t tdt_plane(hipStream_t stream, const E* x, const int* labels, float* plane, int N, int T, int U, int V, int D,
                     int blank, float sigma) {
    const size_t rows = (size_t)N * T * U;
    if (rows == 0) return hipSuccess;
    const int G = row_group(V + D);
    const unsigned grid = row_grid(rows, G);
    return row_dispatch<E>(G, row_access<E>(V + D, x, nullptr), [&](auto g, auto acc) {
        k_tdt_plane<E, decltype(g)::value, decltype(acc)::value>
            <<<grid, ROW_THREADS, 0, stream>>>(x, labels, plane, rows, T, U, V, D, blank, sigma);
    });
}

template <typename E>
hipError_t tdt_backward(hipStream_t stream, const E* x, const int* labels, const float* gplane, const float* scale, E* dx,
                        int N, int T, int U, int V, int D, int blank) {
    const size_t rows = (size_t)N * T * U;
    if (rows == 0) return hipSuccess;
    const int G = row_group(V + D);
    const unsigned grid = row_grid(rows, G);
    return row_dispatch<E>(G, row_access<E>(V + D, x, dx), [&](auto g, auto acc) {
        k_tdt_backward<E, decltype(g)::value, decltype(acc)::value>
            <<<grid, ROW_THREADS, 0, stream>>>(x, labels, gplane, scale, dx, rows, T, U, V, D, blank);
    });
}

inline bool tdt_rows_ok(int V, int D, int blank) { return V >= 2 && D >= 1 && D <= TDT_MAX_D && blank >= 0 && blank < V; }

}  // namespace

hipError_t launch_tdt_plane(hipStream_t stream, int dtype, const void* logits, const int* labels, float* plane, int N, int T,
                            int U, int V, int D, int blank, float sigma) {
    if (!tdt_rows_ok(V, D, blank)) return hipErrorInvalidValue;
    return row_typed(dtype, logits, nullptr,
                     [&](auto* x, auto*) { return tdt_plane(stream, x, labels, plane, N, T, U, V, D, blank, sigma); });
}

hipError_t launch_tdt_sweeps(hipStream_t stream, const float* plane, const int* xn, const int* yn, float* alphas,
                             float* betas, float* ll, float* costs, const TdtDurations& dur, int N, int T, int U) {
    if (U < 1 || U > TDT_MAX_U || dur.D < 1 || dur.D > TDT_MAX_D) return hipErrorInvalidValue;
    if (N == 0) return hipSuccess;
    int longest = 0;
    for (int i = 0; i < dur.D; ++i) longest = dur.d[i] > longest ? dur.d[i] : longest;
    if (longest > TDT_MAX_DURATION) return hipErrorInvalidValue;
    const int ncol = (U + WAVE - 1) / WAVE * WAVE;
    const size_t lds = (size_t)(longest + 2) * ncol * sizeof(float);          // 40 KB at the most
    k_tdt_sweep<<<dim3(N, betas ? 2 : 1), ncol, lds, stream>>>(plane, xn, yn, alphas, betas, ll, costs, dur,
                                                               (size_t)N * T * U, T, U);
    return hipGetLastError();
}

hipError_t launch_tdt_grads(hipStream_t stream, const float* plane, const float* alphas, const float* betas, const float* ll,
                            const int* xn, const int* yn, float* gplane, const TdtDurations& dur, int N, int T, int U,
                            float fastemit_lambda) {
    if (dur.D < 1 || dur.D > TDT_MAX_D) return hipErrorInvalidValue;
    if (N == 0) return hipSuccess;
    const unsigned per = ((unsigned)T * (unsigned)U + ROW_THREADS - 1) / ROW_THREADS;
    k_tdt_grads<<<dim3(per, N), ROW_THREADS, 0, stream>>>(plane, alphas, betas, ll, xn, yn, gplane, dur, (size_t)N * T * U, T,
                                                          U, 1.0f + fastemit_lambda);
    return hipGetLastError();
}

hipError_t launch_tdt_logits_backward(hipStream_t stream, int dtype, const void* logits, const int* labels,
                                      const float* gplane, const float* scale, void* dlogits, int N, int T, int U, int V,
                                      int D, int blank) {
    if (!tdt_rows_ok(V, D, blank)) return hipErrorInvalidValue;
    return row_typed(dtype, logits, dlogits, [&](auto* x, auto* dx) {
        return tdt_backward(stream, x, labels, gplane, scale, dx, N, T, U, V, D, blank);
    });
}

}  // namespace rnnt
