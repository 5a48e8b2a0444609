// Launch interface of the token-and-duration transducer (TDT) kernels (tdt.hip) for the C ABI of
// include/warp_rnnt_amd_tdt.h, and what host and device share: the bounds of a duration set and its check.
#pragma once
#include <hip/hip_runtime.h>

namespace rnnt {

constexpr int TDT_MAX_DURATION = 8;                       // durations are distinct integers in [0, 8] ...
constexpr int TDT_MAX_D = TDT_MAX_DURATION + 1;           // ... so there are nine of them at the most
constexpr int TDT_MAX_U = 1024;                           // lattice columns: the lanes of one workgroup

// A duration set as a kernel argument (by value: nothing of it lives in device memory, so a captured call keeps it)
struct TdtDurations {
    int D;
    int d[TDT_MAX_D];
};

// D distinct integers in [0, 8], in any order, 1 among them (a step of one frame: every lattice then has a path)
inline bool tdt_durations_ok(const int* durations, int D) {
    if (!durations || D < 1 || D > TDT_MAX_D) return false;
    unsigned seen = 0;
    for (int i = 0; i < D; ++i) {
        if (durations[i] < 0 || durations[i] > TDT_MAX_DURATION || (seen >> durations[i] & 1u)) return false;
        seen |= 1u << durations[i];
    }
    return (seen >> 1 & 1u) != 0;
}
inline TdtDurations tdt_durations(const int* durations, int D) {
    TdtDurations t{};
    t.D = D;
    for (int i = 0; i < D; ++i) t.d[i] = durations[i];
    return t;
}

// Every plane below is fp32 and holds `cells` = N*T*U values per channel, channel c at plane + c * cells, a cell at the
// diagonal-major address of common.h: sk(n,t,u) = (n*T + (t+u) mod T)*U + u.
//   plane:  2 + D channels -- tok[blank], tok[label], dur[0..D) -- of EVERY cell of the (N,T,U) grid (tok = log_softmax of
//           the V token logits - sigma, dur = log_softmax of the D duration logits; the label of the last column and of a
//           padded label is the blank);
//   alphas, betas: one channel, written inside each utterance's (T_n, U_n + 1) window only;
//   gplane: 2 + D channels -- G_b, G_l, G_dur[0..D) -- of every cell, zero outside the windows.
// Logits (N,T,U,V+D) of RNNT_DTYPE_* (hipErrorInvalidValue for another dtype), fp32 arithmetic from the load on.
hipError_t launch_tdt_plane(hipStream_t stream, int dtype, const void* logits, const int* labels, float* plane, int N, int T,
                            int U, int V, int D, int blank, float sigma);
// alpha sweep (ll[n], costs[n] = -ll[n]; NaN for an utterance whose lengths are out of range) and, betas != nullptr, the
// beta sweep beside it: one workgroup per utterance and direction.  U <= TDT_MAX_U.
hipError_t launch_tdt_sweeps(hipStream_t stream, const float* plane, const int* xn, const int* yn, float* alphas,
                             float* betas, float* ll, float* costs, const TdtDurations& dur, int N, int T, int U);
hipError_t launch_tdt_grads(hipStream_t stream, const float* plane, const float* alphas, const float* betas, const float* ll,
                            const int* xn, const int* yn, float* gplane, const TdtDurations& dur, int N, int T, int U,
                            float fastemit_lambda);
// d/d logits (N,T,U,V+D) in the logits' type from gplane, scaled by scale[n] (nullptr: 1); every element written
hipError_t launch_tdt_logits_backward(hipStream_t stream, int dtype, const void* logits, const int* labels,
                                      const float* gplane, const float* scale, void* dlogits, int N, int T, int U, int V,
                                      int D, int blank);

}  // namespace rnnt
