// Launch interface of the multi-blank transducer kernels (multiblank.hip) for the C ABI of
// include/warp_rnnt_amd_multiblank.h, and what host and device share: the bounds of a blank set and its checks.
#pragma once
#include <hip/hip_runtime.h>

namespace rnnt {

constexpr int MB_MAX_DURATION = 8;                        // durations are distinct integers in [1, 8] ...
constexpr int MB_MAX_B = MB_MAX_DURATION;                 // ... so there are eight blanks at the most
constexpr int MB_MAX_U = 1024;                            // lattice columns: the lanes of one workgroup

// A blank set as a kernel argument (by value: nothing of it lives in device memory, so a captured call keeps it)
struct MbBlanks {
    int B;
    int id[MB_MAX_B];
    int d[MB_MAX_B];
};

// B distinct vocabulary indices, 1 <= B <= 8, with room for a label beside them
inline bool mb_ids_ok(const int* ids, int B, int V) {
    if (!ids || B < 1 || B > MB_MAX_B || V < B + 1) return false;
    for (int i = 0; i < B; ++i) {
        if (ids[i] < 0 || ids[i] >= V) return false;
        for (int k = 0; k < i; ++k)
            if (ids[k] == ids[i]) return false;
    }
    return true;
}
// B distinct integers in [1, 8], in any order, 1 among them (the standard blank: every lattice then has a path)
inline bool mb_durations_ok(const int* durations, int B) {
    if (!durations || B < 1 || B > MB_MAX_B) return false;
    unsigned seen = 0;
    for (int i = 0; i < B; ++i) {
        if (durations[i] < 1 || durations[i] > MB_MAX_DURATION || (seen >> durations[i] & 1u)) return false;
        seen |= 1u << durations[i];
    }
    return (seen >> 1 & 1u) != 0;
}
// (durations == nullptr: the backward, which does not need them)
inline MbBlanks mb_blanks(const int* ids, const int* durations, int B) {
    MbBlanks b{};
    b.B = B;
    for (int i = 0; i < B; ++i) {
        b.id[i] = ids[i];
        b.d[i] = durations ? durations[i] : 1;
    }
    return b;
}

// Every plane below is fp32 and holds `cells` = N*T*U values per channel, channel c at plane + c * cells, a cell at the
// diagonal-major address of common.h: sk(n,t,u) = (n*T + (t+u) mod T)*U + u.
//   plane:  1 + B channels -- lp[label], lp[blank_ids[0..B)] -- of EVERY cell of the (N,T,U) grid (lp = log_softmax of the
//           V logits - sigma; the label of the last column and of a padded label is blank_ids[0]);
//   alphas, betas: one channel, written inside each utterance's (T_n, U_n + 1) window only;
//   gplane: 1 + B channels -- G_l, G_blank[0..B) -- of every cell, zero outside the windows.
// Logits (N,T,U,V) of RNNT_DTYPE_* (hipErrorInvalidValue for another dtype), fp32 arithmetic from the load on.
hipError_t launch_mb_plane(hipStream_t stream, int dtype, const void* logits, const int* labels, float* plane, int N, int T,
                           int U, int V, const MbBlanks& blanks, float sigma);
// alpha sweep (ll[n], costs[n] = -ll[n]; NaN for an utterance whose lengths are out of range) and, betas != nullptr, the
// beta sweep beside it: one workgroup per utterance and direction.  U <= MB_MAX_U.
hipError_t launch_mb_sweeps(hipStream_t stream, const float* plane, const int* xn, const int* yn, float* alphas,
                            float* betas, float* ll, float* costs, const MbBlanks& blanks, int N, int T, int U);
hipError_t launch_mb_grads(hipStream_t stream, const float* plane, const float* alphas, const float* betas, const float* ll,
                           const int* xn, const int* yn, float* gplane, const MbBlanks& blanks, int N, int T, int U,
                           float fastemit_lambda);
// d/d logits (N,T,U,V) in the logits' type from gplane, scaled by scale[n] (nullptr: 1); every element written
hipError_t launch_mb_logits_backward(hipStream_t stream, int dtype, const void* logits, const int* labels,
                                     const float* gplane, const float* scale, void* dlogits, int N, int T, int U, int V,
                                     const MbBlanks& blanks);

}  // namespace rnnt
