// Launch interface of the CTC loss from logits (ctc.hip) for the C ABI of include/warp_rnnt_amd_ctc.h: the pieces of the
// workspace and the two halves of a call.
#pragma once
#include <hip/hip_runtime.h>

namespace rnnt {

constexpr int CTC_MAX_L = 1023;          // a lane per label position and one for the final blank: a workgroup of 1024
constexpr int CTC_MIN_V = 2;
constexpr int CTC_MAX_V = 16384;         // a row as floats in LDS: 64 KiB
constexpr float CTC_FLOOR = -1e30f;      // what stands for log 0: finite, so no difference of infinities is ever formed

// The shapes the launchers take
inline bool ctc_shape_ok(int N, int T, int L, int V) {
    if (N < 0 || T < 1 || L < 1 || L > CTC_MAX_L || V < CTC_MIN_V || V > CTC_MAX_V) return false;
    return (long long)N * T * (L + 1) < 1ll << 31;
}

// The lengths of utterance n as the kernels use them; outside 1 <= xn <= T, 0 <= yn <= L nothing of it is read
struct CtcLens {
    int Tn, Ln;
    bool ok;
};
__device__ __forceinline__ CtcLens ctc_lens(const int* __restrict__ xn, const int* __restrict__ yn, int n, int T, int L) {
    const int x = xn[n], y = yn[n];
    CtcLens l;
    l.ok = x >= 1 && x <= T && y >= 0 && y <= L;
    l.Tn = l.ok ? x : 0;
    l.Ln = l.ok ? y : 0;
    return l;
}

// The workspace, carved by the C entry.  stats: (m, ls) per row; E: (N,T,L+1); alpha, beta: (N,T,2,L+1), channel 0 the
// blank in front of label l (l = L_n: the final blank), channel 1 label l; ll: the log-likelihoods (CTC_FLOOR or below:
// no path; NaN: lengths out of range); order: (N,L), position | CTC_ORDER_HEAD on the first position of a token
struct CtcWorkspace {
    float2* stats;
    float* E;
    float* alpha;
    float* beta;
    float* ll;
    int* order;
};
constexpr int CTC_ORDER_HEAD = 1 << 16;

// The emissions alone (k_ctc_emit): stats (N,T) and E (N,T,L+1), rows t >= T_n untouched.  What launch_ctc_forward runs
// first, and what the best-path alignment (ctc_align.hip) runs on logits: the same bits
hipError_t launch_ctc_emit(hipStream_t stream, int dtype, const void* logits, const int* labels, const int* xn,
                           const int* yn, float2* stats, float* E, int N, int T, int L, int V, int blank);

// Emissions, then the alpha sweep: stats, E, alpha, ll and costs (N,)
hipError_t launch_ctc_forward(hipStream_t stream, int dtype, const void* logits, const int* labels, const int* xn,
                              const int* yn, const CtcWorkspace& w, float* costs, int N, int T, int L, int V, int blank);

// The beta sweep and the label order, then d/d logits (N,T,V) of the dtype from what launch_ctc_forward left in w;
// dcosts (N,) or nullptr for ones
hipError_t launch_ctc_backward(hipStream_t stream, int dtype, const void* logits, const int* labels, const int* xn,
                               const int* yn, const CtcWorkspace& w, const float* dcosts, void* dlogits, int N, int T,
                               int L, int V, int blank);

}  // namespace rnnt
