// The pruned joiner's hidden activations (pruned_hidden.h): h[n,t,s,:] = act(f[n,t,:] + g[n, clamp(
// starts[n,t] + s, 0, U-1), :]) and its backward to f and g -- what stands between the band selection and the vendor
// GEMM of the output projection.  Everything moves in 16-byte chunks of the H axis: 4 floats or 8 halves, HV = H / that
// per row.
//
// k_ph_fwd     frame-major.  A group of G = 2^lg lanes owns a frame (G: the power of two that covers HV, 256 at most),
//              a workgroup 256 / G frames, so the N T frames fill the chip at any H.  Lane l holds chunks l, l + G, .. --
//              at most four -- of the frame's f row in registers across the S rows; the g rows come through L2 (the bands
//              of neighbouring frames overlap); the sum and the activation are fp32, uncontracted; h leaves in 16-byte
//              stores, written once.  A frame that is not live stores zeros and reads nothing, its start included.
// k_ph_df      the same split: p = dh * act'(h) in fp32, summed over s in registers, df written once, zeros for a frame
//              that is not live.  One read of dh and h.
// k_ph_table   a workgroup per utterance.  It first asks whether the live starts ever decrease (one pass, a workgroup-wide
//              or).  If not, the frames whose band holds column u are one range: with bottom(t) = clamp(start), top(t) =
//              clamp(start + S - 1), both non-decreasing, lo(u) is the first t with top(t) >= u and hi(u) the first with
//              bottom(t) > u -- two binary searches per (n,u).  Otherwise every column gets [0, T_n).
// k_ph_dg      label-major.  A lane owns 16 bytes of dg[n,u,:] and walks [lo, hi) in ascending t; per frame the rows
//              s with clamp(start + s) == u are one run -- a single s inside the lattice, every s at or below 0 for u = 0,
//              every s at or above U - 1 for u = U - 1 -- found from the start itself, so the walk is right for ANY starts
//              and the table only shortens it.  The lanes of a wave read the same start (one broadcast load) and
//              consecutive chunks of the same rows.  The second read of dh and h; every row is read by one owner.
// No atomics, no memset, no (N,T,S,H) scratch; sums are serial per lane, ascending t then s: two runs give the same bits.
#include "pruned_hidden.h"

#include "../../include/warp_rnnt_amd.h"

#pragma clang fp contract(off)

namespace rnnt {
namespace {

constexpr int PH_THREADS = 256;
constexpr int PH_MAXC = 4;          // chunks of a row per lane at most: PRUNED_HIDDEN_MAX_H floats / (4 * PH_THREADS)

template <typename E> struct PhFrag;
template <> struct PhFrag<float> { typedef float type __attribute__((ext_vector_type(4))); };
template <> struct PhFrag<__bf16> { typedef __bf16 type __attribute__((ext_vector_type(8))); };
template <> struct PhFrag<_Float16> { typedef _Float16 type __attribute__((ext_vector_type(8))); };
template <typename E> using ph_frag = typename PhFrag<E>::type;
template <typename E> constexpr int PH_EPF = 16 / (int)sizeof(E);

template <int ACT> __device__ __forceinline__ float ph_act(float x) {
    return ACT == RNNT_ACT_TANH ? tanhf(x) : fmaxf(x, 0.0f);
}
// the derivative from the activation's rounded OUTPUT, as autograd's tanh / relu backward take it
template <int ACT> __device__ __forceinline__ float ph_dact(float y) {
    return ACT == RNNT_ACT_TANH ? 1.0f - y * y : (y > 0.0f ? 1.0f : 0.0f);
}
__device__ __forceinline__ long long ph_clamp(long long u, int U) { return u < 0 ? 0 : u > U - 1 ? U - 1 : u; }
// the live frames of utterance n: [0, ph_live(..))
__device__ __forceinline__ int ph_live(const int* xn, int n, int T) {
    if (!xn) return T;
    const int x = xn[n];
    return x < 0 ? 0 : x > T ? T : x;
}

template <typename E, int ACT>
__global__ void __launch_bounds__(PH_THREADS)
k_ph_fwd(const E* __restrict__ f, const E* __restrict__ g, const int* __restrict__ starts, const int* __restrict__ xn,
         E* __restrict__ h, unsigned frames, int T, int U, int S, int H, int lg) {
    constexpr int EPF = PH_EPF<E>;
    const unsigned frame = blockIdx.x * (unsigned)(PH_THREADS >> lg) + (threadIdx.x >> lg);
    if (frame >= frames) return;
    const int lane = threadIdx.x & ((1 << lg) - 1), HV = H / EPF;
    const unsigned n = frame / (unsigned)T;
    const int t = (int)(frame - n * (unsigned)T);
    E* hrow = h + (size_t)frame * S * H;
    if (t >= ph_live(xn, (int)n, T)) {
        const ph_frag<E> zero = {};
        for (int s = 0; s < S; ++s, hrow += H)
#pragma unroll
            for (int j = 0; j < PH_MAXC; ++j) {
                const int c = lane + (j << lg);
                if (c < HV) *reinterpret_cast<ph_frag<E>*>(hrow + c * EPF) = zero;
            }
        return;
    }
    ph_frag<E> fr[PH_MAXC];
#pragma unroll
    for (int j = 0; j < PH_MAXC; ++j) {
        const int c = lane + (j << lg);
        if (c < HV) fr[j] = *reinterpret_cast<const ph_frag<E>*>(f + (size_t)frame * H + c * EPF);
    }
    const long long st = starts[frame];
    const E* gn = g + (size_t)n * U * H;
#pragma unroll 2
    for (int s = 0; s < S; ++s, hrow += H) {
        const E* grow = gn + (size_t)ph_clamp(st + s, U) * H;
#pragma unroll
        for (int j = 0; j < PH_MAXC; ++j) {
            const int c = lane + (j << lg);
            if (c < HV) {
                const ph_frag<E> gv = *reinterpret_cast<const ph_frag<E>*>(grow + c * EPF);
                ph_frag<E> o;
#pragma unroll
                for (int e = 0; e < EPF; ++e) o[e] = (E)ph_act<ACT>((float)fr[j][e] + (float)gv[e]);
                *reinterpret_cast<ph_frag<E>*>(hrow + c * EPF) = o;
            }
        }
    }
}

template <typename E, int ACT>
__global__ void __launch_bounds__(PH_THREADS)
k_ph_df(const E* __restrict__ dh, const E* __restrict__ h, const int* __restrict__ xn, E* __restrict__ df,
        unsigned frames, int T, int S, int H, int lg) {
    constexpr int EPF = PH_EPF<E>;
    const unsigned frame = blockIdx.x * (unsigned)(PH_THREADS >> lg) + (threadIdx.x >> lg);
    if (frame >= frames) return;
    const int lane = threadIdx.x & ((1 << lg) - 1), HV = H / EPF;
    const unsigned n = frame / (unsigned)T;
    const int t = (int)(frame - n * (unsigned)T);
    float acc[PH_MAXC][EPF];
#pragma unroll
    for (int j = 0; j < PH_MAXC; ++j)
#pragma unroll
        for (int e = 0; e < EPF; ++e) acc[j][e] = 0.0f;
    if (t < ph_live(xn, (int)n, T)) {
        const size_t row0 = (size_t)frame * S * H;
#pragma unroll 2
        for (int s = 0; s < S; ++s) {
#pragma unroll
            for (int j = 0; j < PH_MAXC; ++j) {
                const int c = lane + (j << lg);
                if (c < HV) {
                    const size_t at = row0 + (size_t)s * H + c * EPF;
                    const ph_frag<E> d = *reinterpret_cast<const ph_frag<E>*>(dh + at);
                    const ph_frag<E> y = *reinterpret_cast<const ph_frag<E>*>(h + at);
#pragma unroll
                    for (int e = 0; e < EPF; ++e) acc[j][e] += (float)d[e] * ph_dact<ACT>((float)y[e]);
                }
            }
        }
    }
#pragma unroll
    for (int j = 0; j < PH_MAXC; ++j) {
        const int c = lane + (j << lg);
        if (c < HV) {
            ph_frag<E> o;
#pragma unroll
            for (int e = 0; e < EPF; ++e) o[e] = (E)acc[j][e];
            *reinterpret_cast<ph_frag<E>*>(df + (size_t)frame * H + c * EPF) = o;
        }
    }
}

// the first t in [0, Tn) at which pred(start[t]) holds, Tn if none; pred is false, then true, along non-decreasing starts
template <typename P> __device__ __forceinline__ int ph_first(const int* __restrict__ row, int Tn, P pred) {
    int lo = 0, hi = Tn;
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (pred((long long)row[mid])) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

__global__ void __launch_bounds__(PH_THREADS)
k_ph_table(const int* __restrict__ starts, const int* __restrict__ xn, int2* __restrict__ table, int T, int U, int S) {
    const int n = blockIdx.x, Tn = ph_live(xn, n, T);
    const int* row = starts + (size_t)n * T;
    int falls = 0;
    for (int t = 1 + threadIdx.x; t < Tn; t += PH_THREADS) falls |= row[t] < row[t - 1];
    falls = __syncthreads_or(falls);
    for (int u = threadIdx.x; u < U; u += PH_THREADS) {
        int2 r = make_int2(0, Tn);
        if (!falls) {
            r.x = ph_first(row, Tn, [=](long long st) { return ph_clamp(st + S - 1, U) >= u; });
            r.y = ph_first(row, Tn, [=](long long st) { return ph_clamp(st, U) > u; });
        }
        table[(size_t)n * U + u] = r;
    }
}

template <typename E, int ACT>
__global__ void __launch_bounds__(PH_THREADS)
k_ph_dg(const E* __restrict__ dh, const E* __restrict__ h, const int* __restrict__ starts, const int2* __restrict__ table,
        E* __restrict__ dg, size_t items, int T, int U, int S, int H) {
    constexpr int EPF = PH_EPF<E>;
    const size_t item = (size_t)blockIdx.x * PH_THREADS + threadIdx.x;
    if (item >= items) return;
    const int HV = H / EPF;
    const size_t row = item / HV;                           // n * U + u
    const int c = (int)(item - row * HV);
    const size_t n = row / U;
    const int u = (int)(row - n * U);
    const int2 range = table[row];
    float acc[EPF];
#pragma unroll
    for (int e = 0; e < EPF; ++e) acc[e] = 0.0f;
    for (int t = range.x; t < range.y; ++t) {
        const size_t frame = n * T + t;
        const long long a = (long long)u - (long long)starts[frame];     // the s with start + s == u
        const long long first = u == 0 ? 0 : (a < 0 ? 0 : a);
        const long long last = u == U - 1 ? S - 1 : (a > S - 1 ? S - 1 : a);
        for (long long s = first; s <= last; ++s) {
            const size_t at = (frame * S + (size_t)s) * H + c * EPF;
            const ph_frag<E> d = *reinterpret_cast<const ph_frag<E>*>(dh + at);
            const ph_frag<E> y = *reinterpret_cast<const ph_frag<E>*>(h + at);
#pragma unroll
            for (int e = 0; e < EPF; ++e) acc[e] += (float)d[e] * ph_dact<ACT>((float)y[e]);
        }
    }
    ph_frag<E> o;
#pragma unroll
    for (int e = 0; e < EPF; ++e) o[e] = (E)acc[e];
    *reinterpret_cast<ph_frag<E>*>(dg + row * H + c * EPF) = o;
}

// log2 of the lanes that own a frame: the power of two that covers the row's chunks, PH_THREADS at most
inline int frame_lanes_log2(int HV) {
    int lg = 0;
    while ((1 << lg) < HV && (1 << lg) < PH_THREADS) ++lg;
    return lg;
}

template <typename E, int ACT>
hipError_t ph_fwd(hipStream_t stream, const void* f, const void* g, const int* starts, const int* xn, void* h, int N, int T,
                  int U, int S, int H) {
    const unsigned frames = (unsigned)N * (unsigned)T;
    const int lg = frame_lanes_log2(H / PH_EPF<E>);
    const unsigned per = PH_THREADS >> lg;
    k_ph_fwd<E, ACT><<<(frames + per - 1) / per, PH_THREADS, 0, stream>>>(
        static_cast<const E*>(f), static_cast<const E*>(g), starts, xn, static_cast<E*>(h), frames, T, U, S, H, lg);
    return hipGetLastError();
}

template <typename E, int ACT>
hipError_t ph_bwd(hipStream_t stream, const void* dh, const void* h, const int* starts, const int* xn, int* table, void* df,
                  void* dg, int N, int T, int U, int S, int H) {
    if (df) {
        const unsigned frames = (unsigned)N * (unsigned)T;
        const int lg = frame_lanes_log2(H / PH_EPF<E>);
        const unsigned per = PH_THREADS >> lg;
        k_ph_df<E, ACT><<<(frames + per - 1) / per, PH_THREADS, 0, stream>>>(
            static_cast<const E*>(dh), static_cast<const E*>(h), xn, static_cast<E*>(df), frames, T, S, H, lg);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    if (dg) {
        int2* t2 = reinterpret_cast<int2*>(table);
        k_ph_table<<<(unsigned)N, PH_THREADS, 0, stream>>>(starts, xn, t2, T, U, S);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        const size_t items = (size_t)N * U * (H / PH_EPF<E>);
        k_ph_dg<E, ACT><<<(unsigned)((items + PH_THREADS - 1) / PH_THREADS), PH_THREADS, 0, stream>>>(
            static_cast<const E*>(dh), static_cast<const E*>(h), starts, t2, static_cast<E*>(dg), items, T, U, S, H);
        return hipGetLastError();
    }
    return hipSuccess;
}

// `call` instantiated for the element type and the activation: call(E{}, integral_constant<int, ACT>{})
#define PH_DISPATCH(dtype, act, CALL)                                                                                  \
    do {                                                                                                               \
        if ((act) != RNNT_ACT_TANH && (act) != RNNT_ACT_RELU) return hipErrorInvalidValue;                             \
        const bool tanh_ = (act) == RNNT_ACT_TANH;                                                                     \
        switch (dtype) {                                                                                               \
            case RNNT_DTYPE_F32: return tanh_ ? CALL(float, RNNT_ACT_TANH) : CALL(float, RNNT_ACT_RELU);               \
            case RNNT_DTYPE_BF16: return tanh_ ? CALL(__bf16, RNNT_ACT_TANH) : CALL(__bf16, RNNT_ACT_RELU);            \
            case RNNT_DTYPE_F16: return tanh_ ? CALL(_Float16, RNNT_ACT_TANH) : CALL(_Float16, RNNT_ACT_RELU);         \
            default: return hipErrorInvalidValue;                                                                      \
        }                                                                                                              \
    } while (0)

}  // namespace

hipError_t launch_pruned_hidden_fwd(hipStream_t stream, int dtype, int activation, const void* f, const void* g,
                                    const int* starts, const int* xn, void* h, int N, int T, int U, int S, int H) {
    if (!pruned_hidden_shape_ok(N, T, U, S, H)) return hipErrorInvalidValue;
    if (N == 0) return hipSuccess;
#define PH_FWD(E, ACT) ph_fwd<E, ACT>(stream, f, g, starts, xn, h, N, T, U, S, H)
    PH_DISPATCH(dtype, activation, PH_FWD);
#undef PH_FWD
}

hipError_t launch_pruned_hidden_bwd(hipStream_t stream, int dtype, int activation, const void* dh, const void* h,
                                    const int* starts, const int* xn, int* table, void* df, void* dg, int N, int T, int U,
                                    int S, int H) {
    if (!pruned_hidden_shape_ok(N, T, U, S, H) || (dg && !table)) return hipErrorInvalidValue;
    if (N == 0) return hipSuccess;
#define PH_BWD(E, ACT) ph_bwd<E, ACT>(stream, dh, h, starts, xn, table, df, dg, N, T, U, S, H)
    PH_DISPATCH(dtype, activation, PH_BWD);
#undef PH_BWD
}

}  // namespace rnnt
