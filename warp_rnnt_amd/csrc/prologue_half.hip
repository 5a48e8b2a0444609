// The fused log-softmax kernels of prologue.hip for bf16 and fp16 logits: the same templates, instantiated with the
// storage type E = __bf16 / _Float16, in a translation unit of their own so that the build compiles them next to the
// fp32 ones.  The conversion to fp32 happens at the load (d/d logits: back to E once, at the store); the lane mapping,
// the reduction tree and the routing of dispatch_lsm are the fp32 ones, so every result is bit-equal to the fp32 path
// on the upcast logits (d/d logits: that result rounded to E).  The included kernels hold inline asm (k_lsm_regs' row
// maxima), so the build walks this object's ISA for wait-state hazards as it does prologue.hip's (_build.HAZARD_CHECKED).
#define RNNT_PROLOGUE_LSM_ONLY
#include "prologue.hip"
#include "../../include/warp_rnnt_amd.h"

namespace rnnt {

// The typed launchers of kernels.h: RNNT_DTYPE_F32 forwards to prologue.hip's launcher, the two half types dispatch here.
hipError_t launch_log_softmax_typed(hipStream_t stream, int dtype, const void* x, float* out, int64_t rows, int V) {
    const LsmBwd none{nullptr, nullptr};
    switch (dtype) {
        case RNNT_DTYPE_F32:
            return launch_log_softmax(stream, static_cast<const float*>(x), out, rows, V);
        case RNNT_DTYPE_BF16:
            return dispatch_lsm<LSM_NORM, __bf16>(stream, static_cast<const __bf16*>(x), out, nullptr, rows, V, 1, 1, 0, none);
        case RNNT_DTYPE_F16:
            return dispatch_lsm<LSM_NORM, _Float16>(stream, static_cast<const _Float16*>(x), out, nullptr, rows, V, 1, 1, 0,
                                                    none);
    }
    return hipErrorInvalidValue;
}

hipError_t launch_log_softmax_gather_skewed_typed(hipStream_t stream, int dtype, const void* logits, const int* labels,
                                                  float* ws2, int N, int T, int U, int V, int blank) {
    const int64_t rows = (int64_t)N * T * U;
    const LsmBwd none{nullptr, nullptr};
    switch (dtype) {
        case RNNT_DTYPE_F32:
            return launch_log_softmax_gather_skewed(stream, static_cast<const float*>(logits), labels, ws2, N, T, U, V, blank);
        case RNNT_DTYPE_BF16:
            return dispatch_lsm<LSM_GATHER, __bf16>(stream, static_cast<const __bf16*>(logits), ws2, labels, rows, V, T, U,
                                                    blank, none);
        case RNNT_DTYPE_F16:
            return dispatch_lsm<LSM_GATHER, _Float16>(stream, static_cast<const _Float16*>(logits), ws2, labels, rows, V, T,
                                                      U, blank, none);
    }
    return hipErrorInvalidValue;
}

hipError_t launch_logits_backward_typed(hipStream_t stream, int dtype, const void* logits, const int* labels,
                                        const float* g2_diagonal, const float* scale, void* dlogits, int N, int T,
                                        int U, int V, int blank) {
    const int64_t rows = (int64_t)N * T * U;
    const LsmBwd bw{reinterpret_cast<const float2*>(g2_diagonal), scale};
    switch (dtype) {
        case RNNT_DTYPE_F32:
            return launch_logits_backward(stream, static_cast<const float*>(logits), labels, g2_diagonal, scale,
                                          static_cast<float*>(dlogits), N, T, U, V, blank);
        case RNNT_DTYPE_BF16:
            return dispatch_lsm<LSM_BWD, __bf16>(stream, static_cast<const __bf16*>(logits), static_cast<__bf16*>(dlogits),
                                                 labels, rows, V, T, U, blank, bw);
        case RNNT_DTYPE_F16:
            return dispatch_lsm<LSM_BWD, _Float16>(stream, static_cast<const _Float16*>(logits),
                                                   static_cast<_Float16*>(dlogits), labels, rows, V, T, U, blank, bw);
    }
    return hipErrorInvalidValue;
}

// compact (ragged packed) rows: the fused modes with CompactMap (prologue.hip)
hipError_t launch_lsm_gather_compact_typed(hipStream_t stream, int dtype, const void* logits, float* ws2,
                                           const PackedRows& cr, int V, int blank) {
    const LsmBwd none{nullptr, nullptr};
    switch (dtype) {
        case RNNT_DTYPE_F32:
            return launch_lsm_gather_compact(stream, static_cast<const float*>(logits), ws2, cr, V, blank);
        case RNNT_DTYPE_BF16:
            return dispatch_lsm_compact<LSM_GATHER, __bf16>(stream, static_cast<const __bf16*>(logits), ws2, cr, V, blank,
                                                            none);
        case RNNT_DTYPE_F16:
            return dispatch_lsm_compact<LSM_GATHER, _Float16>(stream, static_cast<const _Float16*>(logits), ws2, cr, V,
                                                              blank, none);
    }
    return hipErrorInvalidValue;
}

hipError_t launch_logits_backward_compact_typed(hipStream_t stream, int dtype, const void* logits, const float* g2_rowmajor,
                                                const float* scale, void* dlogits, const PackedRows& cr, int V, int blank) {
    const LsmBwd bw{reinterpret_cast<const float2*>(g2_rowmajor), scale};
    switch (dtype) {
        case RNNT_DTYPE_F32:
            return launch_logits_backward_compact(stream, static_cast<const float*>(logits), g2_rowmajor, scale,
                                                  static_cast<float*>(dlogits), cr, V, blank);
        case RNNT_DTYPE_BF16:
            return dispatch_lsm_compact<LSM_BWD, __bf16>(stream, static_cast<const __bf16*>(logits),
                                                         static_cast<__bf16*>(dlogits), cr, V, blank, bw);
        case RNNT_DTYPE_F16:
            return dispatch_lsm_compact<LSM_BWD, _Float16>(stream, static_cast<const _Float16*>(logits),
                                                           static_cast<_Float16*>(dlogits), cr, V, blank, bw);
    }
    return hipErrorInvalidValue;
}

}  // namespace rnnt
