// The factorised-blank (HAT) loss on the pruned band -- k2's rnnt_loss_pruned(..., use_hat_loss=True), icefall's
// zipformer_hat: the two streaming kernels that stand where pruned.hip's stand in the pruned loss (pruned_hat.h; DESIGN.md
// 3.23).  Everything between them -- the floor, the sweeps over the (N,T,U) grid, the shear of the modified topology, the
// gradient pairs, the handling of a band without a path -- is the pruned loss's, unchanged.
//
// Logits (N,T,S,V): row (n,t,s) is lattice cell (t, u = starts[n,t] + s), band_cell of pruned.h.  Per row, z[0..V),
// b = blank, l = label of u, sp(x) = max(x,0) + log1p(exp(-|x|)) -- the pair and the chain rule of hat.h:
//     lpB = -sp(-z_b),   m = max_{v != b} z_v,  ls = log sum_{v != b} exp(z_v - m),   lpL = ((z_l - m) - ls) + (-sp(z_b))
//     (lpB again where the label channel is the blank's; the delay penalty added to the finished lpL)
//     u_b = gB (1 - sig) - gL sig,   u_v = gL ([v == l] - q_v),   dz = scale_n * u, rounded once to the logits' type.
//
// Two forms, chosen by V alone, hat.hip's and not pruned.hip's one:
//   rows of up to 1024 elements (REGS): G = row_group(V) lanes per row, chunks `lane` and `G + lane` of the row in 16
//   registers per lane; statistics and output pass from the registers -- the backward reads its row ONCE (k_pruned_backward
//   reads it twice);
//   longer rows: a wave per row, the running (max, log sum) pass of row_chunks.h, a second read for the output pass.
// The arithmetic of a row is hat.h's -- hat_small_stats, hat_wave_stats, hat_pair, hat_cell_grad, hat_dz, the functions
// hat.hip calls -- so a row's bits are a function of the row, V, the blank and the label (the backward: its pair and scale
// as well): with S = U and zero starts the call gives hat.hip's bits.  A dead row -- outside the grid, outside the modified
// window, the backward: switched off or with the pair (0,0) -- returns before any load of logits.  Distinct s of a frame are
// distinct u: the rows of a call never meet in a cell.  No LDS, no atomics, nothing between workgroups.
#include "pruned_hat.h"

#include "hat.h"
#include "pruned.h"
#include "row_chunks.h"
#include "../../include/warp_rnnt_amd.h"

// (as in hat.hip: every product and sum rounded on its own, the same bits at the three storage types)
#pragma clang fp contract(off)

namespace rnnt {
namespace {

// PEN: the label channel of frame t gets dp (0.5 (T_n - 1) - t) added, fp32: the bracket, one multiply, one add
template <typename E, int G, int ACC, int TOPO, bool PEN, bool REGS>
__global__ void __launch_bounds__(ROW_THREADS)
k_pruned_hat_pairs(const E* __restrict__ x, const int* __restrict__ labels, const int* __restrict__ starts,
                   const int* __restrict__ xn, const int* __restrict__ yn, float2* __restrict__ ws2, size_t rows, int T,
                   int U, int S, int V, int blank, float dp) {
    static_assert(REGS || G == WAVE, "the long form is a wave per row");
    const size_t row = (size_t)blockIdx.x * (ROW_THREADS / G) + threadIdx.x / G;
    if (row >= rows) return;
    const int lane = threadIdx.x % G;
    const BandCell c = band_cell<TOPO>(row, labels, starts, xn, yn, T, U, S, V, blank);
    if (!c.live) return;                               // (the whole group: no lane of it is asked for a shuffle below)
    const E* xr = x + row * (size_t)V;
    // (the two logits of the pair and the frame count of the penalty are asked for in front of the row, not behind its
    //  reduction: round trips that then overlap the row's)
    const float zb = (float)xr[blank], zl = (float)xr[c.label];
    float pen = 0.0f;
    if constexpr (PEN) pen = dp * (0.5f * (float)(xn[c.n] - 1) - (float)c.t);
    float m, ls;
    if constexpr (REGS) {
        float z[2][ROW_CHUNK];
        hat_small_stats<E, G, ACC>(xr, lane, V, blank, z, m, ls);
    } else {
        hat_wave_stats<E, ACC, true>(xr, lane, V, blank, m, ls);
    }
    float2 p = hat_pair(zb, zl, c.label, blank, m, ls);
    if constexpr (PEN) p.y = p.y + pen;
    if (lane == 0) ws2[c.sk] = p;
}

template <typename E, int G, int ACC, int TOPO, bool REGS>
__global__ void __launch_bounds__(ROW_THREADS)
k_pruned_hat_backward(const E* __restrict__ x, const int* __restrict__ labels, const int* __restrict__ starts,
                      const int* __restrict__ xn, const int* __restrict__ yn, const float2* __restrict__ g2,
                      const float* __restrict__ scale, E* __restrict__ out, size_t rows, int T, int U, int S, int V,
                      int blank) {
    static_assert(REGS || G == WAVE, "the long form is a wave per row");
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
    const float zb = (float)xr[blank];                 // (in front of the row: as in the pairs)
    float m, ls;
    if constexpr (REGS) {
        float z[2][ROW_CHUNK];
        hat_small_stats<E, G, ACC>(xr, lane, V, blank, z, m, ls);
        const HatCellGrad cg = hat_cell_grad(zb, g, sc, c.label);
        const int chunks = hat_small_chunks<G>(V);
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            if (k >= chunks) break;
            const int e0 = (k * G + lane) * ROW_CHUNK;
            float d[ROW_CHUNK];
#pragma unroll
            for (int i = 0; i < ROW_CHUNK; ++i) d[i] = hat_dz(cg, z[k][i], e0 + i, blank, m, ls);
            row_store8<E, ACC>(o, e0, V, d);
        }
    } else {
        hat_wave_stats<E, ACC, false>(xr, lane, V, blank, m, ls);      // (plain loads: the output pass reads the row again)
        const HatCellGrad cg = hat_cell_grad(zb, g, sc, c.label);
        for (int e0 = lane * ROW_CHUNK; e0 < V; e0 += WAVE * ROW_CHUNK) {
            float z[ROW_CHUNK], d[ROW_CHUNK];
            row_load8<E, ACC, true>(xr, e0, V, z);
#pragma unroll
            for (int i = 0; i < ROW_CHUNK; ++i) d[i] = hat_dz(cg, e0 + i == blank ? ROW_NEG_INF : z[i], e0 + i, blank, m, ls);
            row_store8<E, ACC>(o, e0, V, d);
        }
    }
}

// The launch of one form: the three (topology, penalty) kernels of pruned.hip -- the regular topology with dp == 0 reads no
// length
template <typename E, int G, int ACC, bool REGS>
void pairs_form(hipStream_t stream, unsigned grid, const E* x, const int* labels, const int* starts, const int* xn,
                const int* yn, float2* out, size_t rows, int T, int U, int S, int V, int blank, bool modified, float dp) {
    if (modified)
        k_pruned_hat_pairs<E, G, ACC, TOPO_MODIFIED, true, REGS><<<grid, ROW_THREADS, 0, stream>>>(
            x, labels, starts, xn, yn, out, rows, T, U, S, V, blank, dp);
    else if (dp != 0.0f)
        k_pruned_hat_pairs<E, G, ACC, TOPO_REGULAR, true, REGS><<<grid, ROW_THREADS, 0, stream>>>(
            x, labels, starts, xn, yn, out, rows, T, U, S, V, blank, dp);
    else
        k_pruned_hat_pairs<E, G, ACC, TOPO_REGULAR, false, REGS><<<grid, ROW_THREADS, 0, stream>>>(
            x, labels, starts, xn, yn, out, rows, T, U, S, V, blank, dp);
}

template <typename E, int G, int ACC, bool REGS>
void backward_form(hipStream_t stream, unsigned grid, const E* x, const int* labels, const int* starts, const int* xn,
                   const int* yn, const float2* g2, const float* scale, E* dx, size_t rows, int T, int U, int S, int V,
                   int blank, bool modified) {
    if (modified)
        k_pruned_hat_backward<E, G, ACC, TOPO_MODIFIED, REGS><<<grid, ROW_THREADS, 0, stream>>>(
            x, labels, starts, xn, yn, g2, scale, dx, rows, T, U, S, V, blank);
    else
        k_pruned_hat_backward<E, G, ACC, TOPO_REGULAR, REGS><<<grid, ROW_THREADS, 0, stream>>>(
            x, labels, starts, xn, yn, g2, scale, dx, rows, T, U, S, V, blank);
}

// The form of a call is a function of V alone: the register form with row_group(V) lanes per row up to HAT_SMALL_V, a
// wave per row beyond (where row_group(V) is 64: the same rows per workgroup)
template <typename E>
hipError_t pruned_hat_pairs(hipStream_t stream, const E* x, const int* labels, const int* starts, const int* xn,
                            const int* yn, float* ws2, int N, int T, int U, int S, int V, int blank, int topology, float dp) {
    const bool modified = topology == TOPO_MODIFIED;
    const size_t rows = (size_t)N * T * S, cells = (size_t)N * (modified ? T + 1 : T) * U;
    if (rows == 0) return hipSuccess;
    // (the floor by pruned.hip's kernel, not a memset: pruned.hip has the reason)
    const hipError_t e = launch_pruned_floor(stream, ws2, cells);
    if (e != hipSuccess) return e;
    const int G = row_group(V);
    const unsigned grid = row_grid(rows, G);
    float2* out = reinterpret_cast<float2*>(ws2);
    return row_dispatch<E>(G, row_access<E>(V, x, nullptr), [&](auto g, auto acc) {
        constexpr int GG = decltype(g)::value, ACC = decltype(acc)::value;
        if (V <= HAT_SMALL_V)
            pairs_form<E, GG, ACC, true>(stream, grid, x, labels, starts, xn, yn, out, rows, T, U, S, V, blank, modified, dp);
        else if constexpr (GG == WAVE)
            pairs_form<E, WAVE, ACC, false>(stream, grid, x, labels, starts, xn, yn, out, rows, T, U, S, V, blank, modified,
                                            dp);
    });
}

template <typename E>
hipError_t pruned_hat_backward(hipStream_t stream, const E* x, const int* labels, const int* starts, const int* xn,
                               const int* yn, const float* g2_diagonal, const float* scale, E* dx, int N, int T, int U,
                               int S, int V, int blank, int topology) {
    const size_t rows = (size_t)N * T * S;
    if (rows == 0) return hipSuccess;
    const int G = row_group(V);
    const unsigned grid = row_grid(rows, G);
    const float2* g2 = reinterpret_cast<const float2*>(g2_diagonal);
    const bool modified = topology == TOPO_MODIFIED;
    return row_dispatch<E>(G, row_access<E>(V, x, dx), [&](auto g, auto acc) {
        constexpr int GG = decltype(g)::value, ACC = decltype(acc)::value;
        if (V <= HAT_SMALL_V)
            backward_form<E, GG, ACC, true>(stream, grid, x, labels, starts, xn, yn, g2, scale, dx, rows, T, U, S, V, blank,
                                            modified);
        else if constexpr (GG == WAVE)
            backward_form<E, WAVE, ACC, false>(stream, grid, x, labels, starts, xn, yn, g2, scale, dx, rows, T, U, S, V,
                                               blank, modified);
    });
}

// what launch_pruned_pairs / launch_pruned_logits_backward take: a band inside the lattice, rows numbered in 32 bits, a
// known topology with the lengths it reads
inline bool band_args_ok(int N, int T, int U, int S, int V, int blank, int topology, const int* xn, const int* yn) {
    return N >= 0 && T >= 1 && U >= 1 && S >= 1 && S <= U && V >= 2 && blank >= 0 && blank < V &&
           (unsigned long long)N * T * S < (1ull << 32) &&
           (topology == TOPO_REGULAR || (topology == TOPO_MODIFIED && xn && yn));
}

}  // namespace

hipError_t launch_pruned_hat_pairs(hipStream_t stream, int dtype, const void* logits, const int* labels, const int* starts,
                                   const int* xn, const int* yn, float* ws2, int N, int T, int U, int S, int V, int blank,
                                   int topology, float delay_penalty) {
    if (!band_args_ok(N, T, U, S, V, blank, topology, xn, yn) || (delay_penalty != 0.0f && !xn)) return hipErrorInvalidValue;
    return row_typed(dtype, logits, nullptr, [&](auto* x, auto*) {
        return pruned_hat_pairs(stream, x, labels, starts, xn, yn, ws2, N, T, U, S, V, blank, topology, delay_penalty);
    });
}

hipError_t launch_pruned_hat_logits_backward(hipStream_t stream, int dtype, const void* logits, const int* labels,
                                             const int* starts, const int* xn, const int* yn, const float* g2_diagonal,
                                             const float* scale, void* dlogits, int N, int T, int U, int S, int V,
                                             int blank, int topology) {
    if (!band_args_ok(N, T, U, S, V, blank, topology, xn, yn)) return hipErrorInvalidValue;
    return row_typed(dtype, logits, dlogits, [&](auto* x, auto* dx) {
        return pruned_hat_backward(stream, x, labels, starts, xn, yn, g2_diagonal, scale, dx, N, T, U, S, V, blank, topology);
    });
}

}  // namespace rnnt
