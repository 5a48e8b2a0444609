// The joint network fused into the pruned transducer loss (include/warp_rnnt_amd_pruned_joint.h):
// z[n,t,s,:] = W act(f[n,t] + g[n, starts[n,t] + s]) + b is formed tile by tile with MFMA and never stored; neither the
// (N,T,S,H) activations nor the (N,T,S,V) logits exist in memory.
//
// The band's rows (n,t,s) are contiguous, so this is a GEMM with M = N T S, K = H, N = V, a gather-and-activate prologue and
// a log-softmax / pick epilogue, and the unit of work is a workgroup tile, not joint_tile.h's wave of sixteen cells:
//   - a workgroup of four waves owns FT whole frames of ONE utterance -- FT S rows, walked in chunks of TR = 16 RG rows (one
//     chunk where S <= TR; a frame's rows never split across workgroups);
//   - it stages h = act(f + g) of a chunk ONCE in LDS, in the operand type E, pitch H + 16 bytes (hs_pitch);
//   - every 16-byte fragment of W (and of W^T in the backward) is fetched from memory once per chunk, by one lane, and
//     meets all RG row groups from registers.
// mma_k and the fragment types are joint_tile.h's.  No atomics: every output element has one writer and a fixed order.
#include "joint_tile.h"
#include "pruned.h"
#include "pruned_joint.h"

namespace rnnt {

namespace {

constexpr int PJ_THREADS = WAVE * JWAVES;
constexpr int PJ_VC = 64;            // V columns per pass of the backward: one 16-row block per wave
constexpr int PJ_HCW = 512;          // columns of dW one unit of the weight kernel accumulates (32 x 4 registers)
constexpr int PJ_LDS = 81920;        // two workgroups per CU

struct PJArgs {
    const void* f;        // (N,T,H) E
    const void* g;        // (N,U,H) E
    const void* w;        // (V,H) E
    const void* wt;       // (H,Vp) E (backward)
    const float* bias;    // (V,) or nullptr
    const int* labels;    // (N,U-1)
    const int* starts;    // (N,T)
    const int* xn;
    const int* yn;
    const float2* g2;     // diagonal-major gradient pairs (backward)
    const float* scale;   // (N,) upstream gradient or nullptr (backward)
    float2* pairs;        // diagonal-major log-prob pairs (forward)
    float2* stats;        // (N,T,S): (max, log sum) per row
    void* dpre;           // (N,T,S,H) E: d cost / d (f + g) per row (backward)
    int N, T, U, S, H, V, Vp, blank;
    int FT, chunks, tiles;   // frames per tile, chunks of TR rows per tile, tiles per utterance
};

// What the lanes need of the TR rows of a chunk, in LDS behind hs.  u < 0: the row is dead -- outside the (N,T,S) rows, the
// grid or the utterance's window; in the backward also a row whose utterance is switched off or whose pair gradient is
// (0,0): such a row is staged as zeros and gets dz = 0.
template <int TR> struct RowInfo {
    int u[TR], t[TR], lab[TR];
    float m[TR], ls[TR], gb[TR], gl[TR], sc[TR];
};

template <typename E, int RG> constexpr size_t pj_info_off(int H) { return (size_t)16 * RG * (H + EPF<E>) * sizeof(E); }
template <typename E, int RG> constexpr size_t pj_extra_off(int H) {
    return pj_info_off<E, RG>(H) + (sizeof(RowInfo<16 * RG>) + 15) / 16 * 16;
}

// Rows per chunk / 16: the largest of 4, 2, 1 whose h tile, dz tile and row info fit PJ_LDS
template <typename E> int pj_rg(int H) {
    if (sizeof(E) == 2) return H <= 512 ? 4 : 2;
    return H <= 128 ? 4 : H <= 512 ? 2 : 1;
}
// 16-column blocks of dh a wave of k_pj_bwd_h holds at most: H / 16 over four waves at the largest H of the row count
template <typename E, int RG> constexpr int pj_nbw() {
    return sizeof(E) == 2 ? (RG == 4 ? 8 : 16) : (RG == 4 ? 2 : RG == 2 ? 8 : 16);
}
inline void pj_geometry(PJArgs& a, int rg) {
    const int TR = 16 * rg;
    a.FT = a.S <= TR ? TR / a.S : 1;
    a.chunks = a.S <= TR ? 1 : (a.S + TR - 1) / TR;
    a.tiles = (a.T + a.FT - 1) / a.FT;
}

// Row c of chunk ch of the tile that starts at frame t0 of utterance n.  Returns whether the row is live.
template <int TR, bool BWD>
__device__ __forceinline__ bool pj_row_info(const PJArgs& a, RowInfo<TR>* ri, int n, int t0, int ch, const UttLens& len,
                                            int c) {
    const int tr = ch * TR + c, ft = tr / a.S, s = tr - ft * a.S, t = t0 + ft;
    int u = -1, lab = a.blank;
    float m = 0.0f, ls = 0.0f, gb = 0.0f, gl = 0.0f, sc = 0.0f;
    if (ft < a.FT && t < a.T && len.ok && t < len.Tn) {
        const long long u64 = (long long)a.starts[(size_t)n * a.T + t] + s;   // (64 bits: no start wraps into the grid)
        if (u64 >= 0 && u64 < (long long)len.Un) u = (int)u64;
    }
    if (u >= 0) {
        if (u < a.U - 1) lab = safe_label(a.labels[(size_t)n * (a.U - 1) + u], a.V, a.blank);
        if constexpr (BWD) {
            sc = a.scale ? a.scale[n] : 1.0f;
            float2 gp = make_float2(0.0f, 0.0f);
            if (sc != 0.0f) {                                  // (a switched-off utterance's pairs may hold anything)
                int d = t + u;
                d = d >= a.T ? d % a.T : d;
                gp = a.g2[((size_t)n * a.T + d) * a.U + u];
            }
            if (gp.x == 0.0f && gp.y == 0.0f) {
                u = -1;
            } else {
                const float2 st = a.stats[((size_t)n * a.T + t0) * a.S + tr];
                m = st.x; ls = st.y; gb = gp.x; gl = gp.y;
            }
        }
    }
    ri->u[c] = u; ri->t[c] = t; ri->lab[c] = lab;
    if constexpr (BWD) { ri->m[c] = m; ri->ls[c] = ls; ri->gb[c] = gb; ri->gl[c] = gl; ri->sc[c] = sc; }
    return u >= 0;
}

// h = act(f[n,t] + g[n,u]) of the chunk's TR rows, fp32 arithmetic, rounded once to E; dead rows are zeros
template <typename E, int ACT, int TR>
__device__ __forceinline__ void pj_stage(const PJArgs& a, const RowInfo<TR>* ri, int n, E* hs, int tid) {
    typedef E ev4 __attribute__((ext_vector_type(4)));
    const E* f = static_cast<const E*>(a.f);
    const E* g = static_cast<const E*>(a.g);
    const int H = a.H, P = hs_pitch<E>(H), H4 = H >> 2;
    for (int i = tid; i < TR * H4; i += PJ_THREADS) {
        const int c = i / H4, k = (i - c * H4) * 4, u = ri->u[c];
        ev4 o = {(E)0.0f, (E)0.0f, (E)0.0f, (E)0.0f};
        if (u >= 0) {
            const ev4 fv = *reinterpret_cast<const ev4*>(f + ((size_t)n * a.T + ri->t[c]) * H + k);
            const ev4 gv = *reinterpret_cast<const ev4*>(g + ((size_t)n * a.U + u) * H + k);
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = (E)act_fwd<ACT>((float)fv[j] + (float)gv[j]);
        }
        *reinterpret_cast<ev4*>(hs + c * P + k) = o;
    }
}

// z of the chunk for 16 rows of W: acc[j][i] = z[v0 + 4q + i][row 16 j + r] (SWAP: z[row 16 j + 4q + i][v0 + r]).  One
// fragment of W per K step from memory, RG fragments of h from LDS.  W rows >= V read as zeros.
template <typename E, int RG, bool SWAP>
__device__ __forceinline__ void pj_z(const PJArgs& a, const E* hs, int v0, int lane, jf4 (&acc)[RG]) {
    const E* W = static_cast<const E*>(a.w);
    const int H = a.H, P = hs_pitch<E>(H), q = lane >> 4, r = lane & 15;
    const int v = v0 + r;
    const bool vin = v < a.V;
    const jfrag_t<E>* wrow = reinterpret_cast<const jfrag_t<E>*>(W + (size_t)(vin ? v : 0) * H) + q;
    const jfrag_t<E> zero = {};
#pragma unroll
    for (int j = 0; j < RG; ++j) acc[j] = jf4{0.0f, 0.0f, 0.0f, 0.0f};
    for (int k = 0; k < H / KSTEP<E>; ++k) {
        const jfrag_t<E> wv = vin ? wrow[4 * k] : zero;
#pragma unroll
        for (int j = 0; j < RG; ++j) {
            const jfrag_t<E> hv = (reinterpret_cast<const jfrag_t<E>*>(hs + (16 * j + r) * P) + q)[4 * k];
            acc[j] = SWAP ? mma_k<E>(hv, wv, acc[j]) : mma_k<E>(wv, hv, acc[j]);
        }
    }
}

__device__ __forceinline__ float pj_dz(float z, int v, int blank, int lab, float m, float ls, float gb, float gl, float sc) {
    const float p = cell_prob(z, m, ls);
    return sc * (((v == blank ? gb : 0.0f) + (v == lab ? gl : 0.0f)) - p * (gb + gl));
}

// ---------------------------------------------------------------------------------------------------------------------
// Forward.  The waves split the 16-row blocks of W; each keeps an online (max, sum of exponentials) per row of the chunk
// and picks up z[blank] and z[label] as their block passes; the four lane groups merge by shuffles, the four waves through
// LDS in wave order.  The log-normaliser is never one float (joint.hip: k_joint_fwd has the reason).
// ---------------------------------------------------------------------------------------------------------------------
template <typename E, int ACT, int RG>
__global__ void __launch_bounds__(PJ_THREADS) k_pj_fwd(PJArgs a) {
    extern __shared__ __align__(16) unsigned char pj_lds[];
    constexpr int TR = 16 * RG;
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid >> 6, q = lane >> 4, r = lane & 15;
    E* hs = reinterpret_cast<E*>(pj_lds);
    RowInfo<TR>* ri = reinterpret_cast<RowInfo<TR>*>(pj_lds + pj_info_off<E, RG>(a.H));
    float4* mg = reinterpret_cast<float4*>(pj_lds + pj_extra_off<E, RG>(a.H));      // [JWAVES][TR]: (m, s, z_blank, z_label)
    const int n = blockIdx.x / a.tiles, t0 = (blockIdx.x - n * a.tiles) * a.FT;
    const UttLens len = utt_lens<false>(a.xn, a.yn, n, a.T, a.U);
    if (!len.ok || t0 >= len.Tn) return;
    for (int ch = 0; ch < a.chunks; ++ch) {
        __syncthreads();                                       // (the chunk before: its readers are done)
        bool live = false;
        if (tid < TR) live = pj_row_info<TR, false>(a, ri, n, t0, ch, len, tid);
        if (!__syncthreads_or(live)) continue;
        pj_stage<E, ACT, TR>(a, ri, n, hs, tid);
        __syncthreads();
        float m[RG], s[RG], zb[RG], zl[RG];
        int lab[RG];
#pragma unroll
        for (int j = 0; j < RG; ++j) {
            m[j] = -INFINITY; s[j] = 0.0f; zb[j] = 0.0f; zl[j] = 0.0f;
            lab[j] = ri->lab[16 * j + r];
        }
        const int nvb = (a.V + 15) >> 4;
        for (int vb = wave; vb < nvb; vb += JWAVES) {
            const int v0 = vb * 16;
            jf4 acc[RG];
            pj_z<E, RG, false>(a, hs, v0, lane, acc);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int v = v0 + 4 * q + i;
                if (v < a.V) {
                    const float bv = a.bias ? a.bias[v] : 0.0f;
#pragma unroll
                    for (int j = 0; j < RG; ++j) {
                        const float z = acc[j][i] + bv;
                        if (z > m[j]) { s[j] = s[j] * expf(m[j] - z) + 1.0f; m[j] = z; }
                        else if (z > -INFINITY) { s[j] += expf(z - m[j]); }
                        if (v == a.blank) zb[j] = z;
                        if (v == lab[j]) zl[j] = z;
                    }
                }
            }
        }
        // the four lane groups of a row: max, rescaled sums in a fixed order; z[blank] and z[label] were seen by one lane
#pragma unroll
        for (int j = 0; j < RG; ++j) {
            float mall = m[j];
            mall = fmaxf(mall, __shfl_xor(mall, 16, WAVE));
            mall = fmaxf(mall, __shfl_xor(mall, 32, WAVE));
            float sc = m[j] == -INFINITY ? 0.0f : s[j] * expf(m[j] - mall);
            sc += __shfl_xor(sc, 16, WAVE);
            sc += __shfl_xor(sc, 32, WAVE);
            float xb = zb[j], xl = zl[j];
            xb += __shfl_xor(xb, 16, WAVE);
            xb += __shfl_xor(xb, 32, WAVE);
            xl += __shfl_xor(xl, 16, WAVE);
            xl += __shfl_xor(xl, 32, WAVE);
            if (q == 0) mg[wave * TR + 16 * j + r] = make_float4(mall, sc, xb, xl);
        }
        __syncthreads();
        if (tid < TR && ri->u[tid] >= 0) {
            float mall = -INFINITY;
#pragma unroll
            for (int w = 0; w < JWAVES; ++w) mall = fmaxf(mall, mg[w * TR + tid].x);
            float sc = 0.0f, xb = 0.0f, xl = 0.0f;
#pragma unroll
            for (int w = 0; w < JWAVES; ++w) {
                const float4 p = mg[w * TR + tid];
                sc += p.x == -INFINITY ? 0.0f : p.y * expf(p.x - mall);
                xb += p.z;
                xl += p.w;
            }
            const float logsc = logf(sc);
            const int t = ri->t[tid], u = ri->u[tid];
            int d = t + u;
            d = d >= a.T ? d % a.T : d;
            a.pairs[((size_t)n * a.T + d) * a.U + u] = make_float2((xb - mall) - logsc, (xl - mall) - logsc);
            if (a.stats) a.stats[((size_t)n * a.T + t0) * a.S + ch * TR + tid] = make_float2(mall, logsc);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Backward to the activations.  The same tile.  Per pass of PJ_VC = 64 columns of V: each wave recomputes z of its 16-row
// block of W for all rows, forms dz, rounds it to E and puts it into the dz tile in LDS (rows = the chunk's rows); then
// the waves split the 16-column blocks of H: dh[rows][block] += dz W^T-fragment, A from the dz tile, B one 16-byte fragment
// of W^T per lane from memory, met by all RG row groups.  dpre = dh act'(h) replaces h in LDS element by element (each
// element is read and written by the same lane), goes to the (N,T,S,H) buffer in whole 16-byte words, and df[n,t] is its
// sum over the frame's S rows in ascending s, fp32, rounded once.
// ---------------------------------------------------------------------------------------------------------------------
template <typename E, int ACT, int RG>
__global__ void __launch_bounds__(PJ_THREADS) k_pj_bwd_h(PJArgs a, E* df) {
    extern __shared__ __align__(16) unsigned char pj_lds[];
    constexpr int TR = 16 * RG, NBW = pj_nbw<E, RG>(), DP = PJ_VC + EPF<E>;
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid >> 6, q = lane >> 4, r = lane & 15;
    const int H = a.H, P = hs_pitch<E>(H), nb = H >> 4, HV = H / EPF<E>;
    E* hs = reinterpret_cast<E*>(pj_lds);
    RowInfo<TR>* ri = reinterpret_cast<RowInfo<TR>*>(pj_lds + pj_info_off<E, RG>(H));
    E* dzs = reinterpret_cast<E*>(pj_lds + pj_extra_off<E, RG>(H));                 // [TR][DP]
    const E* WT = static_cast<const E*>(a.wt);
    const int n = blockIdx.x / a.tiles, t0 = (blockIdx.x - n * a.tiles) * a.FT;
    const UttLens len = utt_lens<false>(a.xn, a.yn, n, a.T, a.U);
    const int frames = min(a.FT, a.T - t0), grid_rows = frames * a.S;              // the tile's part of (N,T,S)
    const size_t row0 = ((size_t)n * a.T + t0) * a.S;
    E* dpre = static_cast<E*>(a.dpre);
    float dfacc[4] = {0.0f, 0.0f, 0.0f, 0.0f};                                      // (chunks > 1: one frame, H <= 1024)
    const jfrag_t<E> zero = {};
    for (int ch = 0; ch < a.chunks; ++ch) {
        __syncthreads();
        bool live = false;
        if (tid < TR) live = pj_row_info<TR, true>(a, ri, n, t0, ch, len, tid);
        const int rc = max(0, min(TR, grid_rows - ch * TR));                        // rows of the chunk inside (N,T,S)
        E* dp = dpre + (row0 + (size_t)ch * TR) * H;
        if (!__syncthreads_or(live)) {
            for (int i = tid; i < rc * HV; i += PJ_THREADS) reinterpret_cast<jfrag_t<E>*>(dp)[i] = zero;
            if (a.chunks == 1 && df)
                for (int i = tid; i < frames * H; i += PJ_THREADS) df[((size_t)n * a.T + t0) * H + i] = (E)0.0f;
            continue;
        }
        pj_stage<E, ACT, TR>(a, ri, n, hs, tid);
        __syncthreads();
        jf4 acc[RG][NBW];
#pragma unroll
        for (int j = 0; j < RG; ++j)
#pragma unroll
            for (int b = 0; b < NBW; ++b) acc[j][b] = jf4{0.0f, 0.0f, 0.0f, 0.0f};
        for (int vc0 = 0; vc0 < a.V; vc0 += PJ_VC) {
            const int v0 = vc0 + 16 * wave;
            jf4 z[RG];
            if (v0 < a.V) {
                pj_z<E, RG, false>(a, hs, v0, lane, z);
            } else {
#pragma unroll
                for (int j = 0; j < RG; ++j) z[j] = jf4{0.0f, 0.0f, 0.0f, 0.0f};
            }
            float bv[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) bv[i] = (a.bias && v0 + 4 * q + i < a.V) ? a.bias[v0 + 4 * q + i] : 0.0f;
#pragma unroll
            for (int j = 0; j < RG; ++j) {
                typedef E ev4 __attribute__((ext_vector_type(4)));
                const int row = 16 * j + r;
                const bool rl = ri->u[row] >= 0;
                const float m = ri->m[row], ls = ri->ls[row], gb = ri->gb[row], gl = ri->gl[row], sc = ri->sc[row];
                const int lab = ri->lab[row];
                ev4 o;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int v = v0 + 4 * q + i;
                    o[i] = (E)((rl && v < a.V) ? pj_dz(z[j][i] + bv[i], v, a.blank, lab, m, ls, gb, gl, sc) : 0.0f);
                }
                *reinterpret_cast<ev4*>(dzs + row * DP + 16 * wave + 4 * q) = o;
            }
            __syncthreads();
#pragma unroll
            for (int ks = 0; ks < PJ_VC / KSTEP<E>; ++ks) {
#pragma unroll
                for (int b = 0; b < NBW; ++b) {
                    const int cb = wave + JWAVES * b;
                    if (cb < nb) {
                        const jfrag_t<E> bw = *reinterpret_cast<const jfrag_t<E>*>(
                            WT + (size_t)(16 * cb + r) * a.Vp + vc0 + ks * KSTEP<E> + q * EPF<E>);
#pragma unroll
                        for (int j = 0; j < RG; ++j) {
                            const jfrag_t<E> adz = *reinterpret_cast<const jfrag_t<E>*>(
                                dzs + (16 * j + r) * DP + ks * KSTEP<E> + q * EPF<E>);
                            acc[j][b] = mma_k<E>(adz, bw, acc[j][b]);     // acc[j][b][i]: row 16 j + 4 q + i, column 16 cb + r
                        }
                    }
                }
            }
            __syncthreads();                                   // (the next pass rewrites the dz tile)
        }
#pragma unroll
        for (int j = 0; j < RG; ++j)
#pragma unroll
            for (int b = 0; b < NBW; ++b) {
                const int cb = wave + JWAVES * b;
                if (cb < nb) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        E* hp = hs + (16 * j + 4 * q + i) * P + 16 * cb + r;
                        *hp = (E)(acc[j][b][i] * act_bwd<ACT>((float)*hp));
                    }
                }
            }
        __syncthreads();
        for (int i = tid; i < rc * HV; i += PJ_THREADS) {
            const int c = i / HV, k = (i - c * HV) * EPF<E>;
            reinterpret_cast<jfrag_t<E>*>(dp)[i] = *reinterpret_cast<const jfrag_t<E>*>(hs + c * P + k);
        }
        if (a.chunks == 1) {
            if (df)
                for (int i = tid; i < frames * H; i += PJ_THREADS) {
                    const int ft = i / H, col = i - ft * H;
                    float x = 0.0f;
                    for (int s = 0; s < a.S; ++s) x += (float)hs[(ft * a.S + s) * P + col];
                    df[((size_t)n * a.T + t0) * H + i] = (E)x;
                }
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int col = tid + PJ_THREADS * k;
                if (col < H)
                    for (int c = 0; c < rc; ++c) dfacc[k] += (float)hs[c * P + col];
            }
        }
    }
    if (a.chunks > 1 && df) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int col = tid + PJ_THREADS * k;
            if (col < H) df[((size_t)n * a.T + t0) * H + col] = (E)dfacc[k];
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// dg[n,u] = sum over the frames t < T_n whose band holds u of dpre[n,t,u - starts[n,t]]: a lane per 16 bytes of a row of
// dg walks the frames in ascending t and tests membership per frame (any starts, monotone or not), fp32, rounded once.
// Rows behind yn[n] are zero.
// ---------------------------------------------------------------------------------------------------------------------
template <typename E>
__global__ void __launch_bounds__(PJ_THREADS)
k_pj_dg(const E* __restrict__ dpre, const int* __restrict__ starts, const int* __restrict__ xn, const int* __restrict__ yn,
        E* __restrict__ dg, int N, int T, int U, int S, int H) {
    const int HV = H / EPF<E>;
    const size_t item = (size_t)blockIdx.x * PJ_THREADS + threadIdx.x;
    const size_t row = item / HV;
    if (row >= (size_t)N * U) return;
    const int k = (int)(item - row * HV) * EPF<E>, n = (int)(row / U), u = (int)(row - (size_t)n * U);
    const UttLens len = utt_lens<false>(xn, yn, n, T, U);
    float acc[EPF<E>];
#pragma unroll
    for (int e = 0; e < EPF<E>; ++e) acc[e] = 0.0f;
    if (len.ok && u < len.Un) {
        for (int t = 0; t < len.Tn; ++t) {
            const long long s = (long long)u - (long long)starts[(size_t)n * T + t];
            if (s >= 0 && s < (long long)S) {
                const jfrag_t<E> v =
                    *reinterpret_cast<const jfrag_t<E>*>(dpre + (((size_t)n * T + t) * S + (size_t)s) * H + k);
#pragma unroll
                for (int e = 0; e < EPF<E>; ++e) acc[e] += (float)v[e];
            }
        }
    }
    jfrag_t<E> o;
#pragma unroll
    for (int e = 0; e < EPF<E>; ++e) o[e] = (E)acc[e];
    *reinterpret_cast<jfrag_t<E>*>(dg + row * H + k) = o;
}

// ---------------------------------------------------------------------------------------------------------------------
// Backward to W and b.  A workgroup owns 64 rows of W (16 per wave), a tile of PJ_HCW columns of H and a fixed range of row
// chunks (split-K over rows).  Per chunk: h staged once for the four waves; z with rows = the chunk's rows (one fragment
// of W per K step from memory), dz, dW_tile += dz^T h (MFMA: A = dz out of the accumulators, B = h gathered in the same
// slot order), db += sum dz.  One fp32 partial per split, reduced in split order by k_joint_reduce_w.
// ---------------------------------------------------------------------------------------------------------------------
template <typename E, int ACT, int RG>
__global__ void __launch_bounds__(PJ_THREADS) k_pj_bwd_w(PJArgs a, int splits, int per, float* dw_part, float* db_part) {
    extern __shared__ __align__(16) unsigned char pj_lds[];
    constexpr int TR = 16 * RG, NB = PJ_HCW / 16;
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid >> 6, q = lane >> 4, r = lane & 15;
    const int H = a.H, P = hs_pitch<E>(H), hts = (H + PJ_HCW - 1) / PJ_HCW;
    E* hs = reinterpret_cast<E*>(pj_lds);
    RowInfo<TR>* ri = reinterpret_cast<RowInfo<TR>*>(pj_lds + pj_info_off<E, RG>(H));
    const int sp = blockIdx.x % splits, ht = (blockIdx.x / splits) % hts, vg = blockIdx.x / (splits * hts);
    const int v0 = vg * PJ_VC + 16 * wave, h0 = ht * PJ_HCW, v = v0 + r;
    const float bv = (a.bias && v < a.V) ? a.bias[v] : 0.0f;
    jf4 acc[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) acc[b] = jf4{0.0f, 0.0f, 0.0f, 0.0f};
    float db = 0.0f;
    const long per_utt = (long)a.tiles * a.chunks, total = (long)a.N * per_utt;
    const long c_end = min(total, (long)(sp + 1) * per);
    for (long ci = (long)sp * per; ci < c_end; ++ci) {
        const int n = (int)(ci / per_utt), rem = (int)(ci - (long)n * per_utt);
        const int t0 = (rem / a.chunks) * a.FT, ch = rem % a.chunks;
        const UttLens len = utt_lens<false>(a.xn, a.yn, n, a.T, a.U);
        __syncthreads();
        bool live = false;
        if (tid < TR) live = pj_row_info<TR, true>(a, ri, n, t0, ch, len, tid);
        if (!__syncthreads_or(live)) continue;
        pj_stage<E, ACT, TR>(a, ri, n, hs, tid);
        __syncthreads();
        if (v0 >= a.V) continue;                               // (the whole wave; it still meets the barriers above)
        jf4 dz[RG];
        pj_z<E, RG, true>(a, hs, v0, lane, dz);
#pragma unroll
        for (int j = 0; j < RG; ++j)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int row = 16 * j + 4 * q + i;
                float x = 0.0f;
                if (ri->u[row] >= 0 && v < a.V)
                    x = pj_dz(dz[j][i] + bv, v, a.blank, ri->lab[row], ri->m[row], ri->ls[row], ri->gb[row], ri->gl[row],
                              ri->sc[row]);
                dz[j][i] = x;
                db += x;
            }
#pragma unroll
        for (int jj = 0; jj < RG / ZB<E>; ++jj) {
            const jfrag_t<E> adz = pack_acc<E>(dz + jj * ZB<E>);
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                if (h0 + 16 * b < H) {
                    const int k = h0 + 16 * b + r;
                    jfrag_t<E> bh;
#pragma unroll
                    for (int e = 0; e < EPF<E>; ++e) bh[e] = hs[(CG<E> * jj + b_slot(e, q)) * P + k];
                    acc[b] = mma_k<E>(adz, bh, acc[b]);
                }
            }
        }
    }
    // partial of split sp: rows v0 + 4q + i (below Vp: it is a multiple of PJ_VC), columns h0 + 16 b + r
    float* dp = dw_part + (size_t)sp * a.Vp * H;
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        if (h0 + 16 * b < H) {
#pragma unroll
            for (int i = 0; i < 4; ++i) dp[(size_t)(v0 + 4 * q + i) * H + h0 + 16 * b + r] = acc[b][i];
        }
    }
    if (ht == 0) {
        db += __shfl_xor(db, 16, WAVE);
        db += __shfl_xor(db, 32, WAVE);
        if (q == 0) db_part[(size_t)sp * a.Vp + v] = db;
    }
}

template <typename E, int RG> size_t pj_lds_bytes(int H, size_t extra) { return pj_extra_off<E, RG>(H) + extra; }

template <typename E, int ACT, int RG> hipError_t pj_fwd_rg(hipStream_t stream, PJArgs a) {
    pj_geometry(a, RG);
    const size_t lds = pj_lds_bytes<E, RG>(a.H, sizeof(float4) * JWAVES * 16 * RG);
    if (lds > (size_t)PJ_LDS) return hipErrorInvalidValue;
    k_pj_fwd<E, ACT, RG><<<(unsigned)((long)a.N * a.tiles), PJ_THREADS, lds, stream>>>(a);
    return hipGetLastError();
}

template <typename E, int ACT, int RG>
hipError_t pj_bwd_rg(hipStream_t stream, PJArgs a, void* wt, float* dw_part, float* db_part, int splits, void* df, void* dg,
                     float* dweight, float* dbias) {
    pj_geometry(a, RG);
    const size_t lds_h = pj_lds_bytes<E, RG>(a.H, (size_t)16 * RG * (PJ_VC + EPF<E>) * sizeof(E));
    const size_t lds_w = pj_lds_bytes<E, RG>(a.H, 0);
    if (lds_h > (size_t)PJ_LDS) return hipErrorInvalidValue;
    if (df || dg) {
        const long tw = (long)a.H * a.Vp;
        k_joint_transpose_w<E><<<(unsigned)((tw + 255) / 256), 256, 0, stream>>>(static_cast<const E*>(a.w),
                                                                                 static_cast<E*>(wt), a.V, a.Vp, a.H);
        a.wt = wt;
        k_pj_bwd_h<E, ACT, RG><<<(unsigned)((long)a.N * a.tiles), PJ_THREADS, lds_h, stream>>>(a, static_cast<E*>(df));
        if (dg) {
            const size_t items = (size_t)a.N * a.U * (a.H / EPF<E>);
            k_pj_dg<E><<<(unsigned)((items + PJ_THREADS - 1) / PJ_THREADS), PJ_THREADS, 0, stream>>>(
                static_cast<const E*>(a.dpre), a.starts, a.xn, a.yn, static_cast<E*>(dg), a.N, a.T, a.U, a.S, a.H);
        }
    }
    if (dweight || dbias) {
        const long total = (long)a.N * a.tiles * a.chunks;
        const int per = (int)((total + splits - 1) / splits);
        const long units = (long)(a.Vp / PJ_VC) * ((a.H + PJ_HCW - 1) / PJ_HCW) * splits;
        k_pj_bwd_w<E, ACT, RG><<<(unsigned)units, PJ_THREADS, lds_w, stream>>>(a, splits, per, dw_part, db_part);
        const long vh = (long)a.V * a.H;
        k_joint_reduce_w<<<(unsigned)((vh + 255) / 256), 256, 0, stream>>>(dw_part, db_part, splits, a.V, a.Vp, a.H,
                                                                           dweight, dbias);
    }
    return hipGetLastError();
}

// call(E, ACT, RG) with the element type, the activation and the row groups of a chunk as compile-time constants; the
// (type, RG) pairs are those pj_rg answers
template <typename Call> hipError_t pj_dispatch(int dtype, int act, int H, Call call) {
    const bool tanh_ = act == RNNT_ACT_TANH;
#define RNNT_PJ_RG(E, RGV)                                                                                              \
    return tanh_ ? call((E)0, std::integral_constant<int, RNNT_ACT_TANH>{}, std::integral_constant<int, RGV>{})         \
                 : call((E)0, std::integral_constant<int, RNNT_ACT_RELU>{}, std::integral_constant<int, RGV>{})
    switch (dtype) {
        case RNNT_DTYPE_F32:
            switch (pj_rg<float>(H)) {
                case 4: RNNT_PJ_RG(float, 4);
                case 2: RNNT_PJ_RG(float, 2);
                default: RNNT_PJ_RG(float, 1);
            }
        case RNNT_DTYPE_BF16:
            if (pj_rg<__bf16>(H) == 4) RNNT_PJ_RG(__bf16, 4);
            RNNT_PJ_RG(__bf16, 2);
        case RNNT_DTYPE_F16:
            if (pj_rg<_Float16>(H) == 4) RNNT_PJ_RG(_Float16, 4);
            RNNT_PJ_RG(_Float16, 2);
    }
#undef RNNT_PJ_RG
    return hipErrorInvalidValue;
}

inline bool pj_shape_ok(int N, int T, int U, int S, int H, int V, int blank) {
    return N >= 0 && T >= 1 && U >= 1 && S >= 1 && S <= U && H >= 32 && H <= 1024 && H % 32 == 0 && V >= 2 && blank >= 0 &&
           blank < V && (unsigned long long)N * T * S < (1ull << 32) && (unsigned long long)N * T < (1ull << 31);
}

}  // namespace

int pruned_joint_vpad(int V) { return (V + PJ_VC - 1) / PJ_VC * PJ_VC; }

// About 512 workgroups in all, at most 32 splits, and never so many that the partials outgrow a quarter of the bf16 logits
// the entry exists to avoid: splits Vp H 4 bytes against N T S V 2 bytes
int pruned_joint_w_splits(int dtype, int N, int T, int S, int H, int V) {
    PJArgs a{};
    a.T = T;
    a.S = S;
    pj_geometry(a, dtype == RNNT_DTYPE_F32 ? pj_rg<float>(H) : pj_rg<__bf16>(H));
    const long total = (long)N * a.tiles * a.chunks, rows = (long)N * T * S;
    const long units = (long)(pruned_joint_vpad(V) / PJ_VC) * ((H + PJ_HCW - 1) / PJ_HCW);
    long s = (512 + units - 1) / units;
    if (s > 32) s = 32;
    if (s > rows / (8L * H)) s = rows / (8L * H);
    if (s > total) s = total;
    return s < 1 ? 1 : (int)s;
}

hipError_t launch_pruned_joint_fwd(hipStream_t stream, int dtype, int act, const void* f, const void* g, const void* w,
                                   const float* bias, const int* labels, const int* starts, const int* xn, const int* yn,
                                   float* pairs, float* stats, int N, int T, int U, int S, int H, int V, int blank) {
    if (!pj_shape_ok(N, T, U, S, H, V, blank)) return hipErrorInvalidValue;
    if (N == 0) return hipSuccess;
    PJArgs a{f, g, w, nullptr, bias, labels, starts, xn, yn, nullptr, nullptr, reinterpret_cast<float2*>(pairs),
             reinterpret_cast<float2*>(stats), nullptr, N, T, U, S, H, V, pruned_joint_vpad(V), blank, 0, 0, 0};
    return pj_dispatch(dtype, act, H, [&](auto e, auto actc, auto rg) {
        return pj_fwd_rg<decltype(e), decltype(actc)::value, decltype(rg)::value>(stream, a);
    });
}

hipError_t launch_pruned_joint_bwd(hipStream_t stream, int dtype, int act, const void* f, const void* g, const void* w,
                                   const float* bias, const int* labels, const int* starts, const int* xn, const int* yn,
                                   const float* stats, const float* grads, const float* grad_costs, void* dpre, void* wt,
                                   float* dw_part, float* db_part, void* df, void* dg, float* dweight, float* dbias, int N,
                                   int T, int U, int S, int H, int V, int blank) {
    if (!pj_shape_ok(N, T, U, S, H, V, blank)) return hipErrorInvalidValue;
    if (N == 0) return hipSuccess;
    PJArgs a{f, g, w, nullptr, bias, labels, starts, xn, yn, reinterpret_cast<const float2*>(grads), grad_costs, nullptr,
             reinterpret_cast<float2*>(const_cast<float*>(stats)), dpre, N, T, U, S, H, V, pruned_joint_vpad(V), blank, 0,
             0, 0};
    const int splits = pruned_joint_w_splits(dtype, N, T, S, H, V);
    return pj_dispatch(dtype, act, H, [&](auto e, auto actc, auto rg) {
        return pj_bwd_rg<decltype(e), decltype(actc)::value, decltype(rg)::value>(stream, a, wt, dw_part, db_part, splits,
                                                                                 df, dg, dweight, dbias);
    });
}

}  // namespace rnnt
