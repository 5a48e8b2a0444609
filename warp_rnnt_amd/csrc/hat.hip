// The factorised-blank (HAT) transducer loss, Variani et al. 2020: the two streaming kernels that stand where the fused
// log-softmax + gather and the fused d/d logits stand in the standard loss (hat.h).  The lattice between
// them -- sweeps, costs, gradient pairs -- is the standard one.
//
// Per lattice cell, logits z[0..V), b = blank, sp(x) = max(x,0) + log1p(exp(-|x|)):
//     lpB   = -sp(-z_b)                       log sigmoid(z_b)
//     lnb   = -sp( z_b)                       log(1 - sigmoid(z_b))
//     m     = max_{v != b} z_v,  s = sum_{v != b} exp(z_v - m)
//     lp[v] = ((z_v - m) - log s) + lnb       v != b
// and from the gradient pair (gB, gL) of the cell, sig = sigmoid(z_b), q_v = exp((z_v - m) - log s):
//     u_b = gB (1 - sig) - gL sig,    u_v = gL ([v == label] - q_v),    dz = scale_n * u, rounded once to the logits' type.
// z_v - m is formed first and alone, so nothing but z_b moves under a shift of the non-blank logits.
//
// One map from the elements of a row to lanes and registers at every storage type and every access width: the row is
// cut into chunks of 8 elements, chunk c of a row is held by lane c mod G of the row's group, in ascending order of c; a
// lane adds its elements up in ascending order and the lanes are combined by the xor butterfly of streaming.h.  An element
// at or past V, the blank and a masked logit (-inf) all enter the maximum as -inf and the sum as +0.  So a row's bits are
// a function of the row, V, the blank and the label (the backward: its pair and scale as well) -- not of the storage type
// (bf16 / fp16 rows give the bits of their fp32 upcast), not of the access width, not of where the row lies.
//   rows of up to 1024 elements: a group of G = 16, 32 or 64 lanes per row (the smallest with V <= 16 G), the row read
//   once into 16 registers per lane, reduction and output pass from the registers;
//   longer rows: a wave per row, running maximum and sum in one pass, the backward reads the row a second time for its
//   output pass (20 KB at V = 5000: from L2).
// A chunk is one 16-byte access (two for fp32) where the row pitch V * sizeof(E) and the tensors' addresses are multiples
// of 16; otherwise accesses of 8, 4 or 2 bytes, the widest that pitch and addresses allow (V = 50 in fp32: 8 bytes).
// (row_chunks.h, shared with tdt.hip: the load and the store of a chunk, the running pass of the long form, and the launch
// side -- lanes per row, workgroups, the dispatch over access and storage type.  The register form is this unit's own.)
// No LDS, no atomics, nothing between workgroups.
#include "hat.h"
#include "row_chunks.h"
#include "../../include/warp_rnnt_amd.h"

// every product and sum below is rounded on its own: no fused multiply-add is formed, the same source gives the same bits
// at the three storage types, and a bf16 / fp16 result is the fp32 result rounded once (row_store8 has the one exception
// the compiler makes to that, and what stops it).  (row_chunks.h sets the same for its own functions, which this line,
// behind the includes, does not reach.)
#pragma clang fp contract(off)

namespace rnnt {
namespace {

constexpr int HAT_SMALL_V = 1024;        // rows up to here are held in registers: 2 chunks per lane, 64 lanes at the most

__device__ __forceinline__ float hat_softplus(float x) { return fmaxf(x, 0.0f) + log1pf(expf(-fabsf(x))); }

// What the forward stores for a cell: lpB, and lp[label] -- lpB again where the label channel is the blank's (the last
// column; a padded label), as the standard gather does
__device__ __forceinline__ float2 hat_pair(float zb, float zl, int label, int blank, float m, float ls) {
    const float lpB = -hat_softplus(-zb);
    const float lnb = -hat_softplus(zb);
    return make_float2(lpB, label == blank ? lpB : ((zl - m) - ls) + lnb);
}

// What the backward needs of a cell behind its row statistics
struct HatCellGrad {
    float ub;      // scale * u_b
    float gL, sc;
    int label;
};
__device__ __forceinline__ HatCellGrad hat_cell_grad(float zb, float2 g, float sc, int label) {
    const float e = expf(-fabsf(zb)), den = 1.0f + e;
    const float big = 1.0f / den, small = e / den;            // sigmoid(|z_b|), sigmoid(-|z_b|)
    const float sig = zb >= 0.0f ? big : small, nsig = zb >= 0.0f ? small : big;
    return {sc * (g.x * nsig - g.y * sig), g.y, sc, label};
}
__device__ __forceinline__ float hat_dz(const HatCellGrad& c, float z, int idx, int blank, float m, float ls) {
    const float q = row_exp((z - m) - ls);                    // (z = -inf at the blank, past V and at masked logits: q = +0)
    const float u = c.gL * ((idx == c.label ? 1.0f : 0.0f) - q);
    return idx == blank ? c.ub : c.sc * u;
}

// ---------------------------------------------------------------------------------------------------------
// Rows of up to 1024 elements: a group of G lanes per row, chunks `lane` and `G + lane` in 16 registers
// ---------------------------------------------------------------------------------------------------------
// (a row of up to 8 G elements has no second chunk in any lane: it is neither loaded nor worked on -- what it would add,
//  -inf to the maximum and +0 to the sum, changes no bit)
template <int G> __device__ __forceinline__ int hat_small_chunks(int V) { return V > G * ROW_CHUNK ? 2 : 1; }

template <typename E, int G, int ACC>
__device__ __forceinline__ void hat_small_stats(const E* __restrict__ xr, int lane, int V, int blank, float (&z)[2][ROW_CHUNK],
                                                float& m, float& ls) {
    const int chunks = hat_small_chunks<G>(V);
    row_load8<E, ACC, true>(xr, lane * ROW_CHUNK, V, z[0]);
    if (chunks > 1) row_load8<E, ACC, true>(xr, (G + lane) * ROW_CHUNK, V, z[1]);
    m = ROW_NEG_INF;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        if (k < chunks) {
#pragma unroll
            for (int i = 0; i < ROW_CHUNK; ++i) {
                if ((k * G + lane) * ROW_CHUNK + i == blank) z[k][i] = ROW_NEG_INF;
                m = fmaxf(m, z[k][i]);
            }
        }
    }
    m = group_max<G>(m);
    float s = 0.0f;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        if (k < chunks) {
#pragma unroll
            for (int i = 0; i < ROW_CHUNK; ++i) s += row_exp(z[k][i] - m);
        }
    }
    ls = logf(group_sum<G>(s));
}

template <typename E, int G, int ACC>
__global__ void __launch_bounds__(ROW_THREADS)
k_hat_gather_small(const E* __restrict__ x, const int* __restrict__ labels, float2* __restrict__ ws2, size_t rows, int T,
                   int U, int V, int blank) {
    const size_t row = (size_t)blockIdx.x * (ROW_THREADS / G) + threadIdx.x / G;
    if (row >= rows) return;
    const int lane = threadIdx.x % G;
    const E* xr = x + row * (size_t)V;
    // (the cell's label and its two logits are asked for in front of the row, not behind its reduction: three memory
    //  round trips that then overlap the row's)
    const CellMap c = map_cell(row, labels, T, U, V, blank);
    const float zb = (float)xr[blank], zl = (float)xr[c.label];
    float z[2][ROW_CHUNK], m, ls;
    hat_small_stats<E, G, ACC>(xr, lane, V, blank, z, m, ls);
    if (lane == 0) ws2[c.sk] = hat_pair(zb, zl, c.label, blank, m, ls);
}

template <typename E, int G, int ACC>
__global__ void __launch_bounds__(ROW_THREADS)
k_hat_backward_small(const E* __restrict__ x, const int* __restrict__ labels, const float2* __restrict__ g2,
                     const float* __restrict__ scale, E* __restrict__ out, size_t rows, int T, int U, int V, int blank) {
    const size_t row = (size_t)blockIdx.x * (ROW_THREADS / G) + threadIdx.x / G;
    if (row >= rows) return;
    const int lane = threadIdx.x % G;
    const E* xr = x + row * (size_t)V;
    const CellMap c = map_cell(row, labels, T, U, V, blank);          // (in front of the row: as in the gather)
    const float zb = (float)xr[blank], sc = scale ? scale[c.n] : 1.0f;
    const float2 g = g2[c.sk];
    float z[2][ROW_CHUNK], m, ls;
    hat_small_stats<E, G, ACC>(xr, lane, V, blank, z, m, ls);
    const HatCellGrad cg = hat_cell_grad(zb, g, sc, c.label);
    E* o = out + row * (size_t)V;
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
}

// ---------------------------------------------------------------------------------------------------------
// Longer rows: a wave per row, chunks lane, 64 + lane, ...; running maximum and sum per lane in one pass
// ---------------------------------------------------------------------------------------------------------
// (row_stats of row_chunks.h at G = 64 over the whole row, the blank masked)
template <typename E, int ACC, bool NT>
__device__ __forceinline__ void hat_wave_stats(const E* __restrict__ xr, int lane, int V, int blank, float& m, float& ls) {
    row_stats<E, WAVE, ACC, NT>(xr, lane, V, V, [blank](int idx) { return idx == blank; }, m, ls);
}

template <typename E, int ACC>
__global__ void __launch_bounds__(ROW_THREADS)
k_hat_gather_wave(const E* __restrict__ x, const int* __restrict__ labels, float2* __restrict__ ws2, size_t rows, int T,
                  int U, int V, int blank) {
    const size_t row = (size_t)blockIdx.x * (ROW_THREADS / WAVE) + threadIdx.x / WAVE;
    if (row >= rows) return;
    const int lane = threadIdx.x % WAVE;
    const E* xr = x + row * (size_t)V;
    const CellMap c = map_cell(row, labels, T, U, V, blank);
    const float zb = (float)xr[blank], zl = (float)xr[c.label];
    float m, ls;
    hat_wave_stats<E, ACC, true>(xr, lane, V, blank, m, ls);
    if (lane == 0) ws2[c.sk] = hat_pair(zb, zl, c.label, blank, m, ls);
}

template <typename E, int ACC>
__global__ void __launch_bounds__(ROW_THREADS)
k_hat_backward_wave(const E* __restrict__ x, const int* __restrict__ labels, const float2* __restrict__ g2,
                    const float* __restrict__ scale, E* __restrict__ out, size_t rows, int T, int U, int V, int blank) {
    const size_t row = (size_t)blockIdx.x * (ROW_THREADS / WAVE) + threadIdx.x / WAVE;
    if (row >= rows) return;
    const int lane = threadIdx.x % WAVE;
    const E* xr = x + row * (size_t)V;
    const CellMap c = map_cell(row, labels, T, U, V, blank);
    const float zb = (float)xr[blank], sc = scale ? scale[c.n] : 1.0f;
    const float2 g = g2[c.sk];
    float m, ls;
    hat_wave_stats<E, ACC, false>(xr, lane, V, blank, m, ls);      // (plain loads: the output pass reads the row again)
    const HatCellGrad cg = hat_cell_grad(zb, g, sc, c.label);
    E* o = out + row * (size_t)V;
    for (int e0 = lane * ROW_CHUNK; e0 < V; e0 += WAVE * ROW_CHUNK) {
        float z[ROW_CHUNK], d[ROW_CHUNK];
        row_load8<E, ACC, true>(xr, e0, V, z);
#pragma unroll
        for (int i = 0; i < ROW_CHUNK; ++i) d[i] = hat_dz(cg, e0 + i == blank ? ROW_NEG_INF : z[i], e0 + i, blank, m, ls);
        row_store8<E, ACC>(o, e0, V, d);
    }
}

// The form of a call is a function of V alone: the register form with row_group(V) lanes per row up to HAT_SMALL_V, a
// wave per row beyond (where row_group(V) is 64: the same rows per workgroup)
template <typename E>
hipError_t hat_gather(hipStream_t stream, const E* x, const int* labels, float* ws2, int N, int T, int U, int V, int blank) {
    const size_t rows = (size_t)N * T * U;
    if (rows == 0) return hipSuccess;
    const int G = row_group(V);
    const unsigned grid = row_grid(rows, G);
    float2* out = reinterpret_cast<float2*>(ws2);
    return row_dispatch<E>(G, row_access<E>(V, x, nullptr), [&](auto g, auto acc) {
        constexpr int GG = decltype(g)::value, ACC = decltype(acc)::value;
        if (V <= HAT_SMALL_V)
            k_hat_gather_small<E, GG, ACC><<<grid, ROW_THREADS, 0, stream>>>(x, labels, out, rows, T, U, V, blank);
        else
            k_hat_gather_wave<E, ACC><<<grid, ROW_THREADS, 0, stream>>>(x, labels, out, rows, T, U, V, blank);
    });
}

template <typename E>
hipError_t hat_backward(hipStream_t stream, const E* x, const int* labels, const float* g2_diagonal, const float* scale,
                        E* dx, int N, int T, int U, int V, int blank) {
    const size_t rows = (size_t)N * T * U;
    if (rows == 0) return hipSuccess;
    const int G = row_group(V);
    const unsigned grid = row_grid(rows, G);
    const float2* g2 = reinterpret_cast<const float2*>(g2_diagonal);
    return row_dispatch<E>(G, row_access<E>(V, x, dx), [&](auto g, auto acc) {
        constexpr int GG = decltype(g)::value, ACC = decltype(acc)::value;
        if (V <= HAT_SMALL_V)
            k_hat_backward_small<E, GG, ACC><<<grid, ROW_THREADS, 0, stream>>>(x, labels, g2, scale, dx, rows, T, U, V, blank);
        else
            k_hat_backward_wave<E, ACC><<<grid, ROW_THREADS, 0, stream>>>(x, labels, g2, scale, dx, rows, T, U, V, blank);
    });
}

}  // namespace

hipError_t launch_hat_gather_skewed(hipStream_t stream, int dtype, const void* logits, const int* labels, float* ws2,
                                    int N, int T, int U, int V, int blank) {
    if (V < 2 || blank < 0 || blank >= V) return hipErrorInvalidValue;
    return row_typed(dtype, logits, nullptr,
                     [&](auto* x, auto*) { return hat_gather(stream, x, labels, ws2, N, T, U, V, blank); });
}

hipError_t launch_hat_logits_backward(hipStream_t stream, int dtype, const void* logits, const int* labels,
                                      const float* g2_diagonal, const float* scale, void* dlogits, int N, int T, int U,
                                      int V, int blank) {
    if (V < 2 || blank < 0 || blank >= V) return hipErrorInvalidValue;
    return row_typed(dtype, logits, dlogits, [&](auto* x, auto* dx) {
        return hat_backward(stream, x, labels, g2_diagonal, scale, dx, N, T, U, V, blank);
    });
}

}  // namespace rnnt
