// The pruned transducer loss, Kuang et al. 2022 (k2 / icefall's rnnt_loss_pruned, "regular" topology): the two streaming
// kernels that stand where the fused log-softmax + gather and the fused d/d logits stand in the standard loss (pruned.h;
// DESIGN.md 3.17).  The lattice between them -- sweeps, costs, gradient pairs -- is the standard one over the (N,T,U)
// grid, with the cells outside the band switched off by a finite floor.
//
// Logits (N,T,S,V): row (n,t,s) is lattice cell (t, u = starts[n,t] + s).  Per row, z[0..V), b = blank, l = label of u:
//     m = max_v z_v,  ls = log sum_v exp(z_v - m),  pair = ((z_b - m) - ls, (z_l - m) - ls)
// and from the gradient pair (gB, gL) of the cell, p_v = exp((z_v - m) - ls):
//     dz_v = scale_n * (([v == b] gB + [v == l] gL) - p_v (gB + gL)),   rounded once to the logits' type.
//
// One form at every V: a group of G = row_group(V) lanes per row, chunk c of the row in lane c mod G, the running
// (max, log sum) pass of row_chunks.h; the backward reads its row a second time for the output pass (a row of V <= 1024 is
// at most 4 KB, two chunks per lane: from L1 / L2).  So a row's bits are a function of the row, V, the blank and the label
// (the backward: its pair and scale as well) -- not of the storage type, the access width, S, or where the row lies.
// Distinct s of a frame are distinct u: the rows of one call never meet in a cell.  No LDS, no atomics.
#include "pruned.h"
#include "row_chunks.h"
#include "../../include/warp_rnnt_amd.h"

// (as in hat.hip: every product and sum rounded on its own, the same bits at the three storage types)
#pragma clang fp contract(off)

namespace rnnt {
namespace {

// Where row `row` of (N,T,S) lies in the lattice.  live: u in [0,U) -- starts is device data nobody validated, and the sum
// is formed in 64 bits so that no start wraps into the grid
//
// TOPO_MODIFIED (pruned.h): the plane has T + 1 rows per utterance and is frame-major, cell (t,u) at ((n (T+1) + t) U + u) --
// the diagonal-major address of cell (t' = t - u, u) of the sheared lattice.  live: also t < xn[n], t >= u, u <= yn[n], the
// cells a path can reach -- row (t = T_n, u = U_n) of a padding frame has the address of the virtual terminal cell.
struct BandCell {
    size_t sk;      // float2 index into the diagonal-major plane
    int label;      // vocabulary index of the label channel (the blank in the last column and for a label outside [0,V))
    int n;
    int t;
    bool live;
};
template <int TOPO>
__device__ __forceinline__ BandCell band_cell(size_t row, const int* __restrict__ labels, const int* __restrict__ starts,
                                              const int* __restrict__ xn, const int* __restrict__ yn, int T, int U, int S,
                                              int V, int blank) {
    // N*T*S < 2^32 is checked by the C ABI, so 32-bit divisions are enough
    const unsigned r32 = (unsigned)row;
    const unsigned frame = r32 / (unsigned)S;          // n*T + t
    const int s = (int)(r32 - frame * (unsigned)S);
    const unsigned n = frame / (unsigned)T;
    const int t = (int)(frame - n * (unsigned)T);
    const long long u64 = (long long)starts[frame] + s;
    BandCell c;
    c.n = (int)n;
    c.t = t;
    c.live = u64 >= 0 && u64 < (long long)U;
    c.sk = 0;
    c.label = blank;
    if constexpr (TOPO == TOPO_MODIFIED) c.live = c.live && t < xn[n] && (long long)t >= u64 && u64 <= (long long)yn[n];
    if (c.live) {
        const int u = (int)u64;
        if constexpr (TOPO == TOPO_MODIFIED) {
            c.sk = ((size_t)n * (T + 1) + t) * (size_t)U + u;
        } else {
            int r = t + u;
            r = r >= T ? r % T : r;
            c.sk = ((size_t)n * T + r) * (size_t)U + u;
        }
        if (u < U - 1) c.label = safe_label(labels[(size_t)n * (U - 1) + u], V, blank);
    }
    return c;
}

// PEN: the label channel of frame t gets dp (0.5 (T_n - 1) - t) added, fp32: the bracket, one multiply, one add
template <typename E, int G, int ACC, int TOPO, bool PEN>
__global__ void __launch_bounds__(ROW_THREADS)
k_pruned_pairs(const E* __restrict__ x, const int* __restrict__ labels, const int* __restrict__ starts,
               const int* __restrict__ xn, const int* __restrict__ yn, float2* __restrict__ ws2, size_t rows, int T, int U,
               int S, int V, int blank, float dp) {
    const size_t row = (size_t)blockIdx.x * (ROW_THREADS / G) + threadIdx.x / G;
    if (row >= rows) return;
    const int lane = threadIdx.x % G;
    const BandCell c = band_cell<TOPO>(row, labels, starts, xn, yn, T, U, S, V, blank);
    if (!c.live) return;                               // (the whole group: no lane of it is asked for a shuffle below)
    const E* xr = x + row * (size_t)V;
    const float zb = (float)xr[blank], zl = (float)xr[c.label];
    float m, ls;
    row_stats<E, G, ACC, true>(xr, lane, V, V, [](int) { return false; }, m, ls);
    float lpl = (zl - m) - ls;
    if constexpr (PEN) lpl = lpl + dp * (0.5f * (float)(xn[c.n] - 1) - (float)c.t);
    if (lane == 0) ws2[c.sk] = make_float2((zb - m) - ls, lpl);
}

template <typename E, int G, int ACC, int TOPO>
__global__ void __launch_bounds__(ROW_THREADS)
k_pruned_backward(const E* __restrict__ x, const int* __restrict__ labels, const int* __restrict__ starts,
                  const int* __restrict__ xn, const int* __restrict__ yn, const float2* __restrict__ g2,
                  const float* __restrict__ scale, E* __restrict__ out, size_t rows, int T, int U, int S, int V, int blank) {
    const size_t row = (size_t)blockIdx.x * (ROW_THREADS / G) + threadIdx.x / G;
    if (row >= rows) return;
    const int lane = threadIdx.x % G;
    const BandCell c = band_cell<TOPO>(row, labels, starts, xn, yn, T, U, S, V, blank);
    const float sc = scale ? scale[c.n] : 1.0f;
    E* o = out + row * (size_t)V;
    // an utterance that is switched off is not looked at: its pairs may hold anything (a band without a path)
    float2 g = make_float2(0.0f, 0.0f);
    if (c.live && sc != 0.0f) g = g2[c.sk];
    if (g.x == 0.0f && g.y == 0.0f) {                  // outside the grid, switched off, outside the utterance's window
        const float zero[ROW_CHUNK] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        for (int e0 = lane * ROW_CHUNK; e0 < V; e0 += G * ROW_CHUNK) row_store8<E, ACC>(o, e0, V, zero);
        return;
    }
    const E* xr = x + row * (size_t)V;
    float m, ls;
    row_stats<E, G, ACC, false>(xr, lane, V, V, [](int) { return false; }, m, ls);   // (plain loads: the row is read again)
    const float gs = g.x + g.y;
    for (int e0 = lane * ROW_CHUNK; e0 < V; e0 += G * ROW_CHUNK) {
        float z[ROW_CHUNK], d[ROW_CHUNK];
        row_load8<E, ACC, true>(xr, e0, V, z);
#pragma unroll
        for (int i = 0; i < ROW_CHUNK; ++i) {
            const int idx = e0 + i;
            const float p = row_exp((z[i] - m) - ls);                  // (-inf past V and at a masked logit: p = +0)
            const float hit = (idx == blank ? g.x : 0.0f) + (idx == c.label ? g.y : 0.0f);
            d[i] = sc * (hit - p * gs);
        }
        row_store8<E, ACC>(o, e0, V, d);
    }
}

// The floor into both channels of every cell of the plane: two cells per lane, one 16-byte store; the odd cell of an odd
// plane by the lane behind the last pair.  (A kernel, not hipMemsetD32Async: with the memset in its place a captured step
// came back, on replay, with the costs of a plane that had not been filled -- tests/test_gpu_pruned.py replays one.)
__global__ void __launch_bounds__(ROW_THREADS) k_pruned_floor(float2* __restrict__ ws2, size_t cells) {
    const size_t i = (size_t)blockIdx.x * ROW_THREADS + threadIdx.x, pairs = cells / 2;
    if (i < pairs)
        reinterpret_cast<float4*>(ws2)[i] = make_float4(PRUNED_FLOOR, PRUNED_FLOOR, PRUNED_FLOOR, PRUNED_FLOOR);
    else if (i == pairs && (cells & 1))
        ws2[cells - 1] = make_float2(PRUNED_FLOOR, PRUNED_FLOOR);
}

// The modified plane's per-utterance words, a thread per utterance, behind the floor and the producer and in front of the
// sweeps (a kernel, not copies and memsets, for k_pruned_floor's reason): the sheared lattice's frame count
// xs[n] = T_n - U_n + 1 and its virtual terminal cell (t' = T_n - U_n, u = U_n), row T_n of the plane, whose blank is 0 -- the
// modified lattice has no terminal blank.  T_n < U_n holds no path: one frame, the terminal cell left at the floor, and
// the cost comes back >= 1e29.  Lengths the regular entries refuse (utt_lens) stay refused: xs[n] = 0.
__global__ void __launch_bounds__(ROW_THREADS)
k_modified_terminal(const int* __restrict__ xn, const int* __restrict__ yn, int* __restrict__ xs, float2* __restrict__ ws2,
                    int N, int T, int U) {
    const int n = blockIdx.x * ROW_THREADS + threadIdx.x;
    if (n >= N) return;
    const int x = xn[n], y = yn[n];
    const bool ok = x >= 1 && x <= T && y >= 0 && y < U;
    xs[n] = !ok ? 0 : x < y ? 1 : x - y + 1;
    if (ok && x >= y) ws2[((size_t)n * (T + 1) + x) * (size_t)U + y] = make_float2(0.0f, PRUNED_FLOOR);
}

// ... and behind the gradient kernel, for a reader that walks the plane by frames without the lengths: the terminal
// cell's gradient pair, (-1, 0) in row T_n, is no frame's
__global__ void __launch_bounds__(ROW_THREADS)
k_modified_clear_terminal(const int* __restrict__ xn, const int* __restrict__ yn, float2* __restrict__ g2, int N, int T,
                          int U) {
    const int n = blockIdx.x * ROW_THREADS + threadIdx.x;
    if (n >= N) return;
    const int x = xn[n], y = yn[n];
    if (x >= 1 && x <= T && y >= 0 && y < U && x >= y) g2[((size_t)n * (T + 1) + x) * (size_t)U + y] = make_float2(0.0f, 0.0f);
}

hipError_t pruned_floor(hipStream_t stream, float2* out, size_t cells) {
    // cells < 2^32 (the C ABI's dims_ok): at most 2^23 workgroups, one lane more than pairs for the odd cell
    k_pruned_floor<<<(unsigned)((cells / 2 + 1 + ROW_THREADS - 1) / ROW_THREADS), ROW_THREADS, 0, stream>>>(out, cells);
    return hipGetLastError();
}

template <typename E>
hipError_t pruned_pairs(hipStream_t stream, const E* x, const int* labels, const int* starts, const int* xn, const int* yn,
                        float* ws2, int N, int T, int U, int S, int V, int blank, int topology, float dp) {
    const bool modified = topology == TOPO_MODIFIED;
    const size_t rows = (size_t)N * T * S, cells = (size_t)N * (modified ? T + 1 : T) * U;
    if (rows == 0) return hipSuccess;
    float2* out = reinterpret_cast<float2*>(ws2);
    const hipError_t e = pruned_floor(stream, out, cells);
    if (e != hipSuccess) return e;
    const int G = row_group(V);
    const unsigned grid = row_grid(rows, G);
    return row_dispatch<E>(G, row_access<E>(V, x, nullptr), [&](auto g, auto acc) {
        constexpr int GG = decltype(g)::value, ACC = decltype(acc)::value;
        // (regular with dp == 0: the kernel as it was, no length is read)
        if (modified)
            k_pruned_pairs<E, GG, ACC, TOPO_MODIFIED, true><<<grid, ROW_THREADS, 0, stream>>>(x, labels, starts, xn, yn, out,
                                                                                             rows, T, U, S, V, blank, dp);
        else if (dp != 0.0f)
            k_pruned_pairs<E, GG, ACC, TOPO_REGULAR, true><<<grid, ROW_THREADS, 0, stream>>>(x, labels, starts, xn, yn, out,
                                                                                            rows, T, U, S, V, blank, dp);
        else
            k_pruned_pairs<E, GG, ACC, TOPO_REGULAR, false><<<grid, ROW_THREADS, 0, stream>>>(x, labels, starts, xn, yn, out,
                                                                                             rows, T, U, S, V, blank, dp);
    });
}

template <typename E>
hipError_t pruned_backward(hipStream_t stream, const E* x, const int* labels, const int* starts, const int* xn,
                           const int* yn, const float* g2_diagonal, const float* scale, E* dx, int N, int T, int U, int S,
                           int V, int blank, int topology) {
    const size_t rows = (size_t)N * T * S;
    if (rows == 0) return hipSuccess;
    const int G = row_group(V);
    const unsigned grid = row_grid(rows, G);
    const float2* g2 = reinterpret_cast<const float2*>(g2_diagonal);
    return row_dispatch<E>(G, row_access<E>(V, x, dx), [&](auto g, auto acc) {
        constexpr int GG = decltype(g)::value, ACC = decltype(acc)::value;
        if (topology == TOPO_MODIFIED)
            k_pruned_backward<E, GG, ACC, TOPO_MODIFIED><<<grid, ROW_THREADS, 0, stream>>>(x, labels, starts, xn, yn, g2, scale,
                                                                                          dx, rows, T, U, S, V, blank);
        else
            k_pruned_backward<E, GG, ACC, TOPO_REGULAR><<<grid, ROW_THREADS, 0, stream>>>(x, labels, starts, xn, yn, g2, scale,
                                                                                         dx, rows, T, U, S, V, blank);
    });
}

inline bool pruned_shape_ok(int N, int T, int U, int S, int V, int blank) {
    return N >= 0 && T >= 1 && U >= 1 && S >= 1 && S <= U && V >= 2 && blank >= 0 && blank < V &&
           (unsigned long long)N * T * S < (1ull << 32);
}

}  // namespace

inline bool topology_ok(int topology, const int* xn, const int* yn) {
    return topology == TOPO_REGULAR || (topology == TOPO_MODIFIED && xn && yn);
}

hipError_t launch_pruned_pairs(hipStream_t stream, int dtype, const void* logits, const int* labels, const int* starts,
                               const int* xn, const int* yn, float* ws2, int N, int T, int U, int S, int V, int blank,
                               int topology, float delay_penalty) {
    if (!pruned_shape_ok(N, T, U, S, V, blank) || !topology_ok(topology, xn, yn) || (delay_penalty != 0.0f && !xn))
        return hipErrorInvalidValue;
    return row_typed(dtype, logits, nullptr, [&](auto* x, auto*) {
        return pruned_pairs(stream, x, labels, starts, xn, yn, ws2, N, T, U, S, V, blank, topology, delay_penalty);
    });
}

hipError_t launch_pruned_floor(hipStream_t stream, float* ws2, size_t cells) {
    return cells ? pruned_floor(stream, reinterpret_cast<float2*>(ws2), cells) : hipSuccess;
}

hipError_t launch_modified_terminal(hipStream_t stream, const int* xn, const int* yn, int* xs, float* ws2, int N, int T,
                                    int U) {
    if (N <= 0) return hipSuccess;
    k_modified_terminal<<<(unsigned)((N + ROW_THREADS - 1) / ROW_THREADS), ROW_THREADS, 0, stream>>>(
        xn, yn, xs, reinterpret_cast<float2*>(ws2), N, T, U);
    return hipGetLastError();
}

hipError_t launch_modified_clear_terminal(hipStream_t stream, const int* xn, const int* yn, float* g2, int N, int T, int U) {
    if (N <= 0) return hipSuccess;
    k_modified_clear_terminal<<<(unsigned)((N + ROW_THREADS - 1) / ROW_THREADS), ROW_THREADS, 0, stream>>>(
        xn, yn, reinterpret_cast<float2*>(g2), N, T, U);
    return hipGetLastError();
}

hipError_t launch_pruned_logits_backward(hipStream_t stream, int dtype, const void* logits, const int* labels,
                                         const int* starts, const int* xn, const int* yn, const float* g2_diagonal,
                                         const float* scale, void* dlogits, int N, int T, int U, int S, int V, int blank,
                                         int topology) {
    if (!pruned_shape_ok(N, T, U, S, V, blank) || !topology_ok(topology, xn, yn)) return hipErrorInvalidValue;
    return row_typed(dtype, logits, dlogits, [&](auto* x, auto* dx) {
        return pruned_backward(stream, x, labels, starts, xn, yn, g2_diagonal, scale, dx, N, T, U, S, V, blank, topology);
    });
}

}  // namespace rnnt
