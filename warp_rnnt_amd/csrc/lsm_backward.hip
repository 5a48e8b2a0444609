// Backward of the log-softmax over the vocabulary axis (fp32): the caller-side F.log_softmax of the reference's call
// chain (pytorch_binding/benchmark.py:65,70), differentiated.
#include <cstdlib>
#include <type_traits>

#include "lsm_plan.h"
#include "streaming.h"

namespace rnnt {

// ---------------------------------------------------------------------------
// cache policy of the log-softmax backward streams: non-temporal loads (dy, y) and non-temporal stores (dx).
// Both (round 3): the reference's call chain with the native log-softmax autograd function 1.96 -> 1.89 ms per training
// step at c4 (with the expand kernel's non-temporal stores on top: 1.84), profiles/r03_bwd_nt_ab.txt.

// Backward of log-softmax: dx = dy - exp(y) * sum_v(dy), y = the log-probabilities.
// Same three shapes as the forward kernels (LDS row tiles / one row per workgroup in
// registers / wave per row); 12V bytes per row element (read dy, read y, write dx).
// ---------------------------------------------------------------------------
// (SMB_THREADS, SMB_FLOATS: lsm_plan.h)
template <int L>
__global__ void __launch_bounds__(SMB_THREADS)
k_lsmbwd_small(const float* dy, const float* y, float* dx, int64_t rows, int V, int R, int q) {
    extern __shared__ __attribute__((aligned(16))) float tile[];
    float* tdy = tile;
    float* ty = tile + (size_t)R * V;
    const int tid = threadIdx.x;
    const int64_t row0 = (int64_t)stream_block() * R;
    if (row0 >= rows) return;
    const int nrows = (int)min((int64_t)R, rows - row0);
    const int nel = nrows * V, nvec = nel >> 2;
    const float* sdy = dy + row0 * V;
    const float* sy = y + row0 * V;
    for (int i = tid; i < nvec; i += SMB_THREADS) {
        reinterpret_cast<float4*>(tdy)[i] = rnnt_load4<true>(reinterpret_cast<const float4*>(sdy) + i);
        reinterpret_cast<float4*>(ty)[i] = rnnt_load4<true>(reinterpret_cast<const float4*>(sy) + i);
    }
    for (int e = (nvec << 2) + tid; e < nel; e += SMB_THREADS) { tdy[e] = sdy[e]; ty[e] = sy[e]; }
    __syncthreads();
    constexpr int RPP = SMB_THREADS / L;
    const int h = tid % L, rr = tid / L;
    const int ctail = h + (q - 1) * L;
    const bool tail_ok = ctail < V;
    // (q = 9 ... 16 as a compile-time constant: both rows read once into registers by straight-line code, as k_lsm_small)
    auto all_rows = [&](auto QC) {
        constexpr int Q = decltype(QC)::value;
        for (int r = rr; r < nrows; r += RPP) {
            float* rdy = tdy + r * V;
            const float* ry = ty + r * V;
            float g[Q], yv[Q];
#pragma unroll
            for (int i = 0; i < Q - 1; ++i) { g[i] = rdy[h + i * L]; yv[i] = ry[h + i * L]; }
            g[Q - 1] = tail_ok ? rdy[ctail] : 0.0f;
            yv[Q - 1] = tail_ok ? ry[ctail] : 0.0f;
            float s = 0.0f;
#pragma unroll
            for (int i = 0; i < Q; ++i) s += g[i];
            s = group_sum<L>(s);
#pragma unroll
            for (int i = 0; i < Q - 1; ++i)
                rdy[h + i * L] = __builtin_fmaf(-__builtin_amdgcn_exp2f(yv[i] * LOG2E), s, g[i]);
            if (tail_ok) rdy[ctail] = __builtin_fmaf(-__builtin_amdgcn_exp2f(yv[Q - 1] * LOG2E), s, g[Q - 1]);
        }
    };
    switch (q) {
#define LSMB_Q(QQ) case QQ: all_rows(std::integral_constant<int, QQ>{}); break;
        LSMB_Q(9) LSMB_Q(10) LSMB_Q(11) LSMB_Q(12) LSMB_Q(13) LSMB_Q(14) LSMB_Q(15) LSMB_Q(16)
#undef LSMB_Q
        default:
    for (int r = rr; r < nrows; r += RPP) {
        float* rdy = tdy + r * V;
        const float* ry = ty + r * V;
        float s = 0.0f;
        for (int i = 0, c = h; i < q - 1; ++i, c += L) s += rdy[c];
        if (tail_ok) s += rdy[ctail];
        s = group_sum<L>(s);
        for (int i = 0, c = h; i < q - 1; ++i, c += L)
            rdy[c] = __builtin_fmaf(-__builtin_amdgcn_exp2f(ry[c] * LOG2E), s, rdy[c]);
        if (tail_ok) rdy[ctail] = __builtin_fmaf(-__builtin_amdgcn_exp2f(ry[ctail] * LOG2E), s, rdy[ctail]);
    }
    }
    __syncthreads();
    float* dst = dx + row0 * V;
    for (int i = tid; i < nvec; i += SMB_THREADS)
        rnnt_store4<true>(reinterpret_cast<float4*>(dst) + i, reinterpret_cast<const float4*>(tdy)[i]);
    for (int e = (nvec << 2) + tid; e < nel; e += SMB_THREADS) dst[e] = tdy[e];
}

template <int LG_THREADS, int LG_MAXVEC>
__global__ void __launch_bounds__(LG_THREADS)
k_lsmbwd_large(const float* dy, const float* y, float* dx, int64_t rows, int V, int xcd) {
    __shared__ float red[LG_THREADS / WAVE];
    const int nvec = V >> 2;
    const size_t per_xcd = ((size_t)rows + 7) / 8;       // (xcd: as k_lsm_large)
    const size_t items = xcd ? per_xcd * 8 : (size_t)rows;
    for (size_t it = blockIdx.x; it < items; it += gridDim.x) {
        const size_t row = xcd ? (it & 7) * per_xcd + (it >> 3) : it;
        if (row >= (size_t)rows) continue;
        const float4* sdy = reinterpret_cast<const float4*>(dy + row * V);
        const float4* sy = reinterpret_cast<const float4*>(y + row * V);
        float4 g[LG_MAXVEC];
        float s = 0.0f;
#pragma unroll
        for (int i = 0; i < LG_MAXVEC; ++i) {
            const int j = threadIdx.x + i * LG_THREADS;
            if (j < nvec) { g[i] = rnnt_load4<true>(sdy + j); s += (g[i].x + g[i].y) + (g[i].z + g[i].w); }
        }
        s = block_reduce<LG_THREADS>(s, false, red);
        float4* dst = reinterpret_cast<float4*>(dx + row * V);
#pragma unroll
        for (int i = 0; i < LG_MAXVEC; ++i) {
            const int j = threadIdx.x + i * LG_THREADS;
            if (j < nvec) {
                const float4 p = rnnt_load4<true>(sy + j);
                rnnt_store4<true>(dst + j, make_float4(__builtin_fmaf(-__builtin_amdgcn_exp2f(p.x * LOG2E), s, g[i].x),
                                                      __builtin_fmaf(-__builtin_amdgcn_exp2f(p.y * LOG2E), s, g[i].y),
                                                      __builtin_fmaf(-__builtin_amdgcn_exp2f(p.z * LOG2E), s, g[i].z),
                                                      __builtin_fmaf(-__builtin_amdgcn_exp2f(p.w * LOG2E), s, g[i].w)));
            }
        }
    }
}

__global__ void __launch_bounds__(256)
k_lsmbwd_generic(const float* dy, const float* y, float* dx, int64_t rows, int V) {
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int lane = threadIdx.x & 63;
    const float* g = dy + row * V;
    const float* p = y + row * V;
    float s = 0.0f;
    for (int c = lane; c < V; c += WAVE) s += g[c];
    s = group_sum<WAVE>(s);
    float* o = dx + row * V;
    for (int c = lane; c < V; c += WAVE) o[c] = g[c] - expf(p[c]) * s;
}

// plan_lsm_backward (lsm_plan.h) decides; this launches what it says
hipError_t launch_log_softmax_backward(hipStream_t stream, const float* dy, const float* y, float* dx,
                                       int64_t rows, int V) {
    if (rows <= 0) return hipSuccess;
    const bool aligned = reinterpret_cast<uintptr_t>(dy) % 16 == 0 && reinterpret_cast<uintptr_t>(y) % 16 == 0 &&
                         reinterpret_cast<uintptr_t>(dx) % 16 == 0;
    const LsmPlan p = plan_lsm_backward(rows, V, aligned, lsm_knobs());
    switch (p.family) {
        case LsmFamily::SMALL:
#define LSMB_SMALL(LL) \
    case LL: k_lsmbwd_small<LL><<<p.grid, SMB_THREADS, p.lds_bytes, stream>>>(dy, y, dx, rows, V, p.R, p.q); break;
            switch (p.L) { LSMB_SMALL(1) LSMB_SMALL(2) LSMB_SMALL(4) LSMB_SMALL(8) LSMB_SMALL(16) LSMB_SMALL(32) LSMB_SMALL(64) }
#undef LSMB_SMALL
            break;
        case LsmFamily::LARGE:
#define LGB(TH_, NV_) \
    if (p.TH == TH_ && p.NV == NV_) k_lsmbwd_large<TH_, NV_><<<p.grid, TH_, 0, stream>>>(dy, y, dx, rows, V, p.xcd);
            LGB(256, 4) LGB(256, 8) LGB(512, 8)
            LGB(256, 2) LGB(384, 2) LGB(512, 2) LGB(640, 2) LGB(768, 2) LGB(896, 2) LGB(1024, 2)
            LGB(768, 3) LGB(896, 3) LGB(1024, 3)
#undef LGB
            break;
        default:
            k_lsmbwd_generic<<<p.grid, 256, 0, stream>>>(dy, y, dx, rows, V);
            break;
    }
    return hipGetLastError();
}

}  // namespace rnnt
