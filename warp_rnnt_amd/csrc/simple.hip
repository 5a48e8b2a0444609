// The "simple" transducer loss: the smoothed first pass of the pruned recipe (k2 / icefall's rnnt_loss_smoothed, "regular"
// topology) over the trivial joiner am[n,t,:] + lm[n,u,:] (simple.h; include/warp_rnnt_amd_simple.h).  The
// lattice -- sweeps, costs, guard, gradient pairs -- is the standard one; what stands here is the producer in front of it
// and the backward behind it, and the hot part of both is a GEMM per utterance:
//
//     Z(t,u) - ma(t) - ml(u) = log sum_v exp(am[t,v] - ma(t)) exp(lm[u,v] - ml(u))                (T x U, K = V)
//     d am[t,v] -= c0 exp(am[t,v] - ma(t)) sum_u W(t,u) exp(lm[u,v] - ml(u))                       (T x V, K = U)
//     d lm[u,v] -= c0 exp(lm[u,v] - ml(u)) sum_t W(t,u) exp(am[t,v] - ma(t))                       (U x V, K = T)
//     W(t,u) = S(t,u) exp(-(Z(t,u) - ma(t) - ml(u))),  S = G(.,.,0) + G(.,.,1),  G = scale[n] * gradient pair
//
// One tile form for the three: a workgroup of four waves owns a 64 x 64 tile of the result, wave w the 32 x 32 quarter
// (w >> 1, w & 1) in the 16 accumulators of v_mfma_f32_32x32x2_f32 -- the exact fp32 MFMA: operands and products are
// fp32, so a cell's error is that of an fp32 dot product and does not grow along a path.  Per step of 32 along K the
// workgroup stages both operands through LDS, K-major ([k][row], pitch 98 floats: the staging writes of every form below
// fall into distinct banks or two per bank, the two k of a wave's read overlap in two banks); the lanes of a staging wave
// read whole 128-byte runs of a row; the exponentials are taken on the way in, so no exp(am), exp(lm) or W tensor exists
// in memory.
// Rows are read with row_chunks.h's chunk loads: -inf past V, whose exponential is +0, at every access width.
//
// Repeated labels: d am[t,v] += sum_u [v == y_u] G(t,u,1) is formed inside the K loop of the d am kernel -- the lane that
// owns column v adds G(t,u,1) of its 16 rows for every u of the step whose label is v, in ascending u.  No atomics
// anywhere: a result's bits are a function of the utterance (with c2 != 0: and of q).
#include "simple.h"
#include "pruned.h"
#include "row_chunks.h"

#include <cfloat>

// (as in hat.hip: every product and sum rounded on its own, the same bits at the three storage types)
#pragma clang fp contract(off)

namespace rnnt {
namespace {

constexpr int ST = 64;             // tile edge: rows and columns of a workgroup's result tile
constexpr int SK = 32;             // K per LDS stage
constexpr int SP = ST + 34;        // LDS pitch of a k-row, floats
constexpr int STHREADS = 256;      // four waves, a 2 x 2 arrangement of 32 x 32 quarters
typedef float f32x16 __attribute__((ext_vector_type(16)));

// row of accumulator r of lane `lane` inside the wave's 32 x 32 quarter (the column is lane & 31)
__device__ __forceinline__ int quarter_row(int r, int lane) { return (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5); }

// one element, converted as row_store8 converts (the median keeps a scalar fp16 cast from taking the multiply with it)
template <typename E> __device__ __forceinline__ void store_one(E* p, float v) {
    if constexpr (std::is_same_v<E, float>) *p = v;
    else *p = (E)__builtin_amdgcn_fmed3f(v, v, v);
}

// acc += A^T B over the staged step: a[k][wm + i] * b[k][wn + j]
__device__ __forceinline__ void mfma_stage(const float (*a)[SP], const float (*b)[SP], int wm, int wn, int lane,
                                           f32x16& acc) {
    const int i = lane & 31, kh = lane >> 5;
#pragma unroll
    for (int k = 0; k < SK; k += 2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[k + kh][wm + i], b[k + kh][wn + i], acc, 0, 0, 0);
}

__device__ __forceinline__ int column_label(const int* __restrict__ labels, int n, int u, int U, int V, int blank) {
    return u < U - 1 ? safe_label(labels[(size_t)n * (U - 1) + u], V, blank) : blank;
}

// ---- row statistics (simple.h: sa, sl) ----
template <typename E, int G, int ACC, bool LM>
__global__ void __launch_bounds__(ROW_THREADS)
k_simple_stats(const E* __restrict__ x, const float* __restrict__ q, const int* __restrict__ labels,
               float4* __restrict__ out, size_t rows, int U, int V, int blank) {
    const size_t row = (size_t)blockIdx.x * (ROW_THREADS / G) + threadIdx.x / G;
    if (row >= rows) return;
    const int lane = threadIdx.x % G;
    const E* xr = x + row * (size_t)V;
    float m, ls;
    row_stats<E, G, ACC, false>(xr, lane, V, V, [](int) { return false; }, m, ls);
    float z = 0.0f, extra = 0.0f;
    if constexpr (LM) {
        z = m + ls;
        const unsigned n = (unsigned)(row / (size_t)U);
        const int u = (int)(row - (size_t)n * U);
        extra = (float)xr[column_label(labels, (int)n, u, U, V, blank)];
    } else if (q) {
        // the (max, log sum) pass of row_stats over am + q
        float ml = ROW_NEG_INF, s = 0.0f;
        for (int e0 = lane * ROW_CHUNK; e0 < V; e0 += G * ROW_CHUNK) {
            float a[ROW_CHUNK], b[ROW_CHUNK];
            row_load8<E, ACC, false>(xr, e0, V, a);
            row_load8<float, 4, false>(q, e0, V, b);
            float mn = ml;
#pragma unroll
            for (int i = 0; i < ROW_CHUNK; ++i) {
                a[i] = a[i] + b[i];
                mn = fmaxf(mn, a[i]);
            }
            if (mn > ROW_NEG_INF) {
                s = s * row_exp(ml - mn);
#pragma unroll
                for (int i = 0; i < ROW_CHUNK; ++i) s += row_exp(a[i] - mn);
                ml = mn;
            }
        }
        const float mq = group_max<G>(ml);
        z = mq + logf(group_sum<G>(s * row_exp(ml - mq)));
    }
    if (lane == 0) out[row] = make_float4(m, z, (float)xr[blank], extra);
}

// ---- the producer: Z and the two pair channels of every cell ----
// TOPO_MODIFIED (pruned.h): the pair goes to the frame-major plane of T + 1 rows, and only from the cells a path can reach
// (t < xn[n], t >= u, u <= yn[n]; the rest of that plane is the floor, filled in front of this kernel); znorm as ever.
// PEN: the label channel of frame t gets dp (0.5 (T_n - 1) - t) added, fp32: the bracket, one multiply, one add.
template <typename E, int ACC, int TOPO, bool PEN>
__global__ void __launch_bounds__(STHREADS)
k_simple_pairs(const E* __restrict__ am, const E* __restrict__ lm, const float* __restrict__ q,
               const int* __restrict__ labels, const int* __restrict__ xn, const int* __restrict__ yn,
               const float4* __restrict__ sa, const float4* __restrict__ sl, float2* __restrict__ ws2,
               float* __restrict__ znorm, int T, int U, int V, int blank, SimpleScales c, float dp) {
    __shared__ float As[SK][SP], Bs[SK][SP];
    const int n = blockIdx.z, t0 = blockIdx.y * ST, u0 = blockIdx.x * ST;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
    // staging: thread (row lr, chunk kc) brings 8 consecutive v of am row t0 + lr and of lm row u0 + lr; the four chunks of
    // a row in neighbouring lanes
    const int lr = tid >> 2, kc = tid & 3;
    const bool ra = t0 + lr < T, rb = u0 + lr < U;
    const size_t rowa = (size_t)n * T + (ra ? t0 + lr : 0), rowb = (size_t)n * U + (rb ? u0 + lr : 0);
    const E* ar = am + rowa * (size_t)V;
    const E* br = lm + rowb * (size_t)V;
    const float ma = sa[rowa].x, ml = sl[rowb].x;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
    for (int k0 = 0; k0 < V; k0 += SK) {
        float a[ROW_CHUNK], b[ROW_CHUNK];
        row_load8<E, ACC, false>(ar, k0 + kc * ROW_CHUNK, V, a);
        row_load8<E, ACC, false>(br, k0 + kc * ROW_CHUNK, V, b);
#pragma unroll
        for (int i = 0; i < ROW_CHUNK; ++i) {
            As[kc * ROW_CHUNK + i][lr] = ra ? row_exp(a[i] - ma) : 0.0f;      // (-inf past V: +0)
            Bs[kc * ROW_CHUNK + i][lr] = rb ? row_exp(b[i] - ml) : 0.0f;
        }
        __syncthreads();
        mfma_stage(As, Bs, wm, wn, lane, acc);
        __syncthreads();
    }
    const int u = u0 + wn + (lane & 31);
    if (u >= U) return;
    const float4 su = sl[(size_t)n * U + u];
    const int lab = column_label(labels, n, u, U, V, blank);
    const float qb = q ? q[blank] : 0.0f, ql = q ? q[lab] : 0.0f;
    const float onlyB = c.c1 * (su.z - su.y), onlyL = c.c1 * (su.w - su.y);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int t = t0 + wm + quarter_row(r, lane);
        if (t >= T) continue;
        const size_t row = (size_t)n * T + t;
        const float4 s = sa[row];
        const float lz = logf(fmaxf(acc[r], FLT_MIN));
        const float z = (lz + s.x) + su.x;
        const float al = (float)am[row * (size_t)V + lab];
        const float pb = (c.c0 * ((s.z + su.z) - z) + onlyB) + c.c2 * ((s.z + qb) - s.y);
        float pl = (c.c0 * ((al + su.w) - z) + onlyL) + c.c2 * ((al + ql) - s.y);
        if constexpr (PEN) pl = pl + dp * (0.5f * (float)(xn[n] - 1) - (float)t);
        if constexpr (TOPO == TOPO_MODIFIED) {
            if (t < xn[n] && t >= u && u <= yn[n]) ws2[((size_t)n * (T + 1) + t) * (size_t)U + u] = make_float2(pb, pl);
        } else {
            int d = t + u;
            d = d >= T ? d % T : d;
            ws2[((size_t)n * T + d) * (size_t)U + u] = make_float2(pb, pl);
        }
        if (znorm) znorm[row * (size_t)U + u] = lz;
    }
}

// ---- the backward's row sums (simple.h: ra, rl) ----
// a wave per frame: lanes over u, then the wave's sum.  TP: frames per utterance of g2 (T; the modified plane: T + 1)
__global__ void __launch_bounds__(STHREADS)
k_simple_frame_sums(const float2* __restrict__ g2, const float* __restrict__ scale, float2* __restrict__ ra, int T, int U,
                    int TP) {
    const int n = blockIdx.y, t = blockIdx.x * (STHREADS / WAVE) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (t >= T) return;
    const float sc = scale ? scale[n] : 1.0f;
    const float2* g = g2 + ((size_t)n * TP + t) * (size_t)U;
    float s = 0.0f, b = 0.0f;
    if (sc != 0.0f)
        for (int u = lane; u < U; u += WAVE) {
            const float2 v = g[u];
            const float g0 = sc * v.x, g1 = sc * v.y;
            s += g0 + g1;
            b += g0;
        }
    s = group_sum<WAVE>(s);
    b = group_sum<WAVE>(b);
    if (lane == 0) ra[(size_t)n * T + t] = make_float2(s, b);
}

// 64 columns per workgroup: wave w sums the frames t = w mod 4, the four partial sums are added in the order of the waves
__global__ void __launch_bounds__(STHREADS)
k_simple_column_sums(const float2* __restrict__ g2, const float* __restrict__ scale, float4* __restrict__ rl, int T,
                     int U, int TP) {
    __shared__ float part[STHREADS / WAVE][3][WAVE];
    const int n = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6, u = blockIdx.x * WAVE + lane;
    const float sc = scale ? scale[n] : 1.0f;
    float s = 0.0f, b = 0.0f, l = 0.0f;
    if (u < U && sc != 0.0f)
        for (int t = wave; t < T; t += STHREADS / WAVE) {
            const float2 v = g2[((size_t)n * TP + t) * (size_t)U + u];
            const float g0 = sc * v.x, g1 = sc * v.y;
            s += g0 + g1;
            b += g0;
            l += g1;
        }
    part[wave][0][lane] = s;
    part[wave][1][lane] = b;
    part[wave][2][lane] = l;
    __syncthreads();
    if (wave == 0 && u < U) {
        float o[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) o[k] = ((part[0][k][lane] + part[1][k][lane]) + part[2][k][lane]) + part[3][k][lane];
        rl[(size_t)n * U + u] = make_float4(o[0], o[1], o[2], 0.0f);
    }
}

// ---- the backward's two GEMMs ----
// LM = false: d am.  Rows m = t, K = u; A[k][m] = W(t,u), B[k][v] = exp(lm[u,v] - ml(u)); the label one-hot in the loop.
// LM = true:  d lm.  Rows m = u, K = t; A[k][m] = W(t,u), B[k][v] = exp(am[t,v] - ma(t)); the staging threads sum S, G(.,.,0)
//             and G(.,.,1) of their column over the frames they bring (thread (u, chunk c): the t with (t mod 32) / 8 == c, in
//             ascending order), the four chunks are added in their order.
template <typename E, int ACC, bool LM>
__global__ void __launch_bounds__(STHREADS)
k_simple_backward(const E* __restrict__ am, const E* __restrict__ lm, const float* __restrict__ q,
                  const int* __restrict__ labels, const int* __restrict__ xn, const int* __restrict__ yn,
                  const float2* __restrict__ g2, const float* __restrict__ znorm, const float* __restrict__ scale,
                  const float4* __restrict__ sa, const float4* __restrict__ sl, const float2* __restrict__ ra,
                  E* __restrict__ out, int T, int U, int V, int blank, SimpleScales c, int TP) {
    __shared__ float As[SK][SP], Bs[SK][SP];
    __shared__ float Gs[LM ? 1 : SK][SP];
    __shared__ float sums[LM ? 4 : 1][3][ST];
    __shared__ int labs[SK];
    const int n = blockIdx.z, m0 = blockIdx.y * ST, v0 = blockIdx.x * ST;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
    const int M = LM ? U : T, K = LM ? T : U;
    const E* own = (LM ? lm : am) + (size_t)n * M * (size_t)V;      // the rows of the result
    const E* other = (LM ? am : lm) + (size_t)n * K * (size_t)V;    // the rows along K
    const float4* sown = (LM ? sl : sa) + (size_t)n * M;
    const float4* sother = (LM ? sa : sl) + (size_t)n * K;
    E* o = out + (size_t)n * M * (size_t)V;
    const UttLens len = utt_lens<false>(xn, yn, n, T, U);
    const int live = LM ? len.Un : len.Tn;                          // rows m < live are inside the window
    const float sc = scale ? scale[n] : 1.0f;
    const int v = v0 + wn + (lane & 31);

    if (sc == 0.0f || !len.ok || m0 >= live) {                      // (the whole workgroup) exactly zero rows
        if (v < V)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = m0 + wm + quarter_row(r, lane);
                if (m < M) store_one<E>(o + (size_t)m * V + v, 0.0f);
            }
        return;
    }

    // staging A, both along u in neighbouring lanes.  d lm: thread (lr, kc): row m0 + lr, the 8 k of chunk kc; d am: thread
    // (tid & 31, tid >> 5): k = tid & 31, the 8 rows (tid >> 5) + 8 i.  B: thread (kb, vc): row k0 + kb, 8 consecutive v.
    const int lr = tid & 63, kc = tid >> 6, kb = tid >> 3, vc = tid & 7;
    float cs = 0.0f, cb = 0.0f, cl = 0.0f;
    f32x16 acc;
    float hot[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f, hot[r] = 0.0f;
    for (int k0 = 0; k0 < K; k0 += SK) {
#pragma unroll
        for (int i = 0; i < ROW_CHUNK; ++i) {
            const int k = LM ? kc * ROW_CHUNK + i : tid & 31, m = LM ? lr : (tid >> 5) + 8 * i;
            const int t = LM ? k0 + k : m0 + m, u = LM ? m0 + m : k0 + k;
            float w = 0.0f, g1 = 0.0f;
            if (t < T && u < U) {
                const size_t cell = ((size_t)n * T + t) * (size_t)U + u;
                const float2 g = g2[((size_t)n * TP + t) * (size_t)U + u];
                const float a = sc * g.x, b = sc * g.y;
                w = (a + b) * row_exp(-znorm[cell]);
                g1 = b;
                if constexpr (LM) {
                    cs += a + b;
                    cb += a;
                    cl += b;
                }
            }
            As[k][m] = w;
            if constexpr (!LM) Gs[k][m] = g1;
        }
        {
            const int kr = k0 + kb;
            float z[ROW_CHUNK];
            float mx = 0.0f;
            if (kr < K) {
                row_load8<E, ACC, false>(other + (size_t)kr * V, v0 + vc * ROW_CHUNK, V, z);
                mx = sother[kr].x;
            }
#pragma unroll
            for (int i = 0; i < ROW_CHUNK; ++i) Bs[kb][vc * ROW_CHUNK + i] = kr < K ? row_exp(z[i] - mx) : 0.0f;
        }
        if constexpr (!LM)
            if (tid < SK) labs[tid] = k0 + tid < U ? column_label(labels, n, k0 + tid, U, V, blank) : -1;
        __syncthreads();
        mfma_stage(As, Bs, wm, wn, lane, acc);
        if constexpr (!LM) {
            // the u of this step whose label lies in the tile's 64 columns (the same in every wave), in ascending order
            const int mine = lane < SK ? labs[lane] : -1;
            unsigned long long in = __ballot(mine >= v0 && mine < v0 + ST);
            while (in) {
                const int k = __builtin_ctzll(in);
                in &= in - 1;
                if (labs[k] == v) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) hot[r] += Gs[k][wm + quarter_row(r, lane)];
                }
            }
        }
        __syncthreads();
    }
    if constexpr (LM) {
        sums[kc][0][lr] = cs;
        sums[kc][1][lr] = cb;
        sums[kc][2][lr] = cl;
        __syncthreads();
        if (tid < 3 * ST) {
            const int j = tid / ST, c = tid % ST;
            sums[0][j][c] = ((sums[0][j][c] + sums[1][j][c]) + sums[2][j][c]) + sums[3][j][c];
        }
        __syncthreads();
    }

    if (v >= V) return;
    const float qv = (!LM && q) ? q[v] : 0.0f;
    const float keep = LM ? c.c0 + c.c1 : c.c0 + c.c2, only = LM ? c.c1 : c.c2;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int m = m0 + wm + quarter_row(r, lane);
        if (m >= M) continue;
        float d = 0.0f;
        if (m < live) {
            const float x = (float)own[(size_t)m * V + v];
            const float4 s = sown[m];
            const float e = row_exp(x - s.x);
            float h, p, sum;
            if constexpr (LM) {
                const int lab = column_label(labels, n, m, U, V, blank);
                h = (v == blank ? sums[0][1][m - m0] : 0.0f) + (v == lab ? sums[0][2][m - m0] : 0.0f);
                p = row_exp(x - s.y);
                sum = sums[0][0][m - m0];
            } else {
                const float2 rs = ra[(size_t)n * T + m];
                h = hot[r] + (v == blank ? rs.y : 0.0f);
                p = q ? row_exp((x + qv) - s.y) : 0.0f;
                sum = rs.x;
            }
            d = (keep * h - c.c0 * (e * acc[r])) - only * (p * sum);
        }
        store_one<E>(o + (size_t)m * V + v, d);
    }
}

// ---- d q: per utterance, c2 (sum_{t,u,c} [v == sym(u,c)] G(t,u,c) - sum_t PA(t,v) sum_u S(t,u)) ----
template <typename E>
__global__ void __launch_bounds__(STHREADS)
k_simple_dq(const E* __restrict__ am, const float* __restrict__ q, const int* __restrict__ labels,
            const float4* __restrict__ sa, const float2* __restrict__ ra, const float4* __restrict__ rl,
            float* __restrict__ dq, int T, int U, int V, int blank, float c2) {
    __shared__ float part[STHREADS / WAVE][WAVE];
    const int n = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6, v = blockIdx.x * WAVE + lane;
    float s = 0.0f;
    if (v < V) {
        const float qv = q[v];
        float hit = 0.0f, pa = 0.0f;
        for (int u = wave; u < U; u += STHREADS / WAVE) {
            const float4 cs = rl[(size_t)n * U + u];
            hit += (v == blank ? cs.y : 0.0f) + (v == column_label(labels, n, u, U, V, blank) ? cs.z : 0.0f);
        }
        for (int t = wave; t < T; t += STHREADS / WAVE) {
            const size_t row = (size_t)n * T + t;
            pa += row_exp(((float)am[row * (size_t)V + v] + qv) - sa[row].y) * ra[row].x;
        }
        s = hit - pa;
    }
    part[wave][lane] = s;
    __syncthreads();
    if (wave == 0 && v < V)
        dq[(size_t)n * V + v] = c2 * (((part[0][lane] + part[1][lane]) + part[2][lane]) + part[3][lane]);
}

// launch(ACC) with the access as a compile-time constant; an access E does not have is hipErrorInvalidValue
template <typename E, typename Launch> hipError_t access_dispatch(int acc, Launch launch) {
    switch (acc) {
        case 16: launch(std::integral_constant<int, 16>{}); break;
        case 8: launch(std::integral_constant<int, 8>{}); break;
        case 4: launch(std::integral_constant<int, 4>{}); break;
        case 2:
            if constexpr (sizeof(E) == 2) {
                launch(std::integral_constant<int, 2>{});
                break;
            }
            return hipErrorInvalidValue;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

inline bool simple_shape_ok(int N, int T, int U, int V, int blank) {
    return N >= 0 && N <= 65535 && T >= 1 && T <= SIMPLE_MAX_ROWS && U >= 1 && U <= SIMPLE_MAX_ROWS && V >= 2 && V <= (1 << 24) && blank >= 0 && blank < V &&
           (unsigned long long)N * T * U < (1ull << 32);
}
inline unsigned tiles(int n) { return (unsigned)((n + ST - 1) / ST); }

template <typename E>
hipError_t simple_stats(hipStream_t stream, const E* am, const E* lm, const float* q, const int* labels,
                        const SimpleStats& st, int N, int T, int U, int V, int blank) {
    const int G = row_group(V);
    const size_t rowsa = (size_t)N * T, rowsl = (size_t)N * U;
    hipError_t e = row_dispatch<E>(G, row_access<E>(V, am, nullptr), [&](auto g, auto acc) {
        constexpr int GG = decltype(g)::value, ACC = decltype(acc)::value;
        k_simple_stats<E, GG, ACC, false><<<row_grid(rowsa, G), ROW_THREADS, 0, stream>>>(
            am, q, labels, reinterpret_cast<float4*>(st.sa), rowsa, U, V, blank);
    });
    if (e != hipSuccess) return e;
    return row_dispatch<E>(G, row_access<E>(V, lm, nullptr), [&](auto g, auto acc) {
        constexpr int GG = decltype(g)::value, ACC = decltype(acc)::value;
        k_simple_stats<E, GG, ACC, true><<<row_grid(rowsl, G), ROW_THREADS, 0, stream>>>(
            lm, nullptr, labels, reinterpret_cast<float4*>(st.sl), rowsl, U, V, blank);
    });
}

template <typename E>
hipError_t simple_pairs(hipStream_t stream, const E* am, const E* lm, const float* q, const int* labels,
                        const int* xn, const int* yn, const SimpleStats& st, float* ws2, float* znorm, int N, int T, int U,
                        int V, int blank, SimpleScales c, int topology, float dp) {
    if (N == 0) return hipSuccess;
    hipError_t e = simple_stats(stream, am, lm, q, labels, st, N, T, U, V, blank);
    if (e != hipSuccess) return e;
    const bool modified = topology == TOPO_MODIFIED;
    // (the regular form writes every cell of its plane; the modified one the cells on a path over the floor)
    if (modified && (e = launch_pruned_floor(stream, ws2, (size_t)N * (T + 1) * U)) != hipSuccess) return e;
    const dim3 grid(tiles(U), tiles(T), (unsigned)N);
    const float4* sa = reinterpret_cast<const float4*>(st.sa);
    const float4* sl = reinterpret_cast<const float4*>(st.sl);
    float2* out = reinterpret_cast<float2*>(ws2);
    return access_dispatch<E>(row_access<E>(V, am, lm), [&](auto acc) {
        constexpr int ACC = decltype(acc)::value;
        // (regular with dp == 0: the kernel as it was, no length is read)
        if (modified)
            k_simple_pairs<E, ACC, TOPO_MODIFIED, true><<<grid, STHREADS, 0, stream>>>(am, lm, q, labels, xn, yn, sa, sl, out,
                                                                                      znorm, T, U, V, blank, c, dp);
        else if (dp != 0.0f)
            k_simple_pairs<E, ACC, TOPO_REGULAR, true><<<grid, STHREADS, 0, stream>>>(am, lm, q, labels, xn, yn, sa, sl, out,
                                                                                     znorm, T, U, V, blank, c, dp);
        else
            k_simple_pairs<E, ACC, TOPO_REGULAR, false><<<grid, STHREADS, 0, stream>>>(am, lm, q, labels, xn, yn, sa, sl, out,
                                                                                      znorm, T, U, V, blank, c, dp);
    });
}

template <typename E>
hipError_t simple_backward(hipStream_t stream, const E* am, const E* lm, const float* q, const int* labels, const int* xn,
                           const int* yn, const float* g2, const float* znorm, const float* scale, const SimpleStats& st,
                           E* dam, E* dlm, float* dq, int N, int T, int U, int V, int blank, SimpleScales c, int TP) {
    if (N == 0) return hipSuccess;
    hipError_t e = simple_stats(stream, am, lm, q, labels, st, N, T, U, V, blank);
    if (e != hipSuccess) return e;
    const float2* g = reinterpret_cast<const float2*>(g2);
    const float4* sa = reinterpret_cast<const float4*>(st.sa);
    const float4* sl = reinterpret_cast<const float4*>(st.sl);
    float2* ra = reinterpret_cast<float2*>(st.ra);
    float4* rl = reinterpret_cast<float4*>(st.rl);
    const bool wants_dq = dq && q && c.c2 != 0.0f;
    k_simple_frame_sums<<<dim3((unsigned)((T + 3) / 4), (unsigned)N), STHREADS, 0, stream>>>(g, scale, ra, T, U, TP);
    if (wants_dq)      // (d lm forms its column sums on the way: only d q reads these)
        k_simple_column_sums<<<dim3((unsigned)((U + WAVE - 1) / WAVE), (unsigned)N), STHREADS, 0, stream>>>(g, scale, rl, T,
                                                                                                          U, TP);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (dam) {
        const dim3 grid(tiles(V), tiles(T), (unsigned)N);
        e = access_dispatch<E>(row_access<E>(V, lm, nullptr), [&](auto acc) {
            k_simple_backward<E, decltype(acc)::value, false><<<grid, STHREADS, 0, stream>>>(
                am, lm, q, labels, xn, yn, g, znorm, scale, sa, sl, ra, dam, T, U, V, blank, c, TP);
        });
        if (e != hipSuccess) return e;
    }
    if (dlm) {
        const dim3 grid(tiles(V), tiles(U), (unsigned)N);
        e = access_dispatch<E>(row_access<E>(V, am, nullptr), [&](auto acc) {
            k_simple_backward<E, decltype(acc)::value, true><<<grid, STHREADS, 0, stream>>>(
                am, lm, q, labels, xn, yn, g, znorm, scale, sa, sl, ra, dlm, T, U, V, blank, c, TP);
        });
        if (e != hipSuccess) return e;
    }
    if (wants_dq) {
        k_simple_dq<E><<<dim3((unsigned)((V + WAVE - 1) / WAVE), (unsigned)N), STHREADS, 0, stream>>>(
            am, q, labels, sa, ra, rl, dq, T, U, V, blank, c.c2);
        e = hipGetLastError();
    }
    return e;
}

}  // namespace

hipError_t launch_simple_pairs(hipStream_t stream, int dtype, const void* am, const void* lm, const float* q,
                               const int* labels, const int* xn, const int* yn, const SimpleStats& st, float* ws2,
                               float* znorm, int N, int T, int U, int V, int blank, SimpleScales c, int topology,
                               float delay_penalty) {
    if (!simple_shape_ok(N, T, U, V, blank) || (c.c2 != 0.0f && !q)) return hipErrorInvalidValue;
    if ((topology != TOPO_REGULAR && topology != TOPO_MODIFIED) || ((topology == TOPO_MODIFIED || delay_penalty != 0.0f) && (!xn || !yn)))
        return hipErrorInvalidValue;
    return row_typed(dtype, am, nullptr, [&](auto* a, auto*) {
        using E = std::remove_const_t<std::remove_pointer_t<decltype(a)>>;
        return simple_pairs<E>(stream, a, static_cast<const E*>(lm), q, labels, xn, yn, st, ws2, znorm, N, T, U, V, blank, c,
                               topology, delay_penalty);
    });
}

hipError_t launch_simple_backward(hipStream_t stream, int dtype, const void* am, const void* lm, const float* q,
                                  const int* labels, const int* xn, const int* yn, const float* g2, const float* znorm,
                                  const float* scale, const SimpleStats& st, void* dam, void* dlm, float* dq, int N, int T,
                                  int U, int V, int blank, SimpleScales c, int g2_frames) {
    if (!simple_shape_ok(N, T, U, V, blank) || (c.c2 != 0.0f && !q) || g2_frames < T) return hipErrorInvalidValue;
    return row_typed(dtype, am, dam, [&](auto* a, auto* da) {
        using E = std::remove_const_t<std::remove_pointer_t<decltype(a)>>;
        return simple_backward<E>(stream, a, static_cast<const E*>(lm), q, labels, xn, yn, g2, znorm, scale, st, da,
                                  static_cast<E*>(dlm), dq, N, T, U, V, blank, c, g2_frames);
    });
}

}  // namespace rnnt
