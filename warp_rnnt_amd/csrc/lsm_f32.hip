// The forward log-softmax kernels of lsm.h for fp32 logits, and the family's launchers (kernels.h).
#include "lsm.h"
#include "../../include/warp_rnnt_amd.h"

namespace rnnt {

template struct LsmOps<float>;
// RNNT_DTYPE_* -> the storage type E, written once: f receives a null E* to take the type from.
template <class F> static hipError_t with_logits_type(int dtype, F&& f) {
    switch (dtype) {
        case RNNT_DTYPE_F32: return f(static_cast<float*>(nullptr));
        case RNNT_DTYPE_BF16: return f(static_cast<__bf16*>(nullptr));
        case RNNT_DTYPE_F16: return f(static_cast<_Float16*>(nullptr));
    }
    return hipErrorInvalidValue;
}

hipError_t launch_log_softmax(hipStream_t stream, int dtype, const void* x, float* out, int64_t rows, int V) {
    return with_logits_type(dtype, [&](auto* e) {
        using E = std::remove_pointer_t<decltype(e)>;
        return LsmOps<E>::log_softmax(stream, static_cast<const E*>(x), out, rows, V);
    });
}

hipError_t launch_log_softmax_plane(hipStream_t stream, int dtype, const void* x, float* out, float* col_out, int64_t rows,
                                    int V, int col) {
    return with_logits_type(dtype, [&](auto* e) {
        using E = std::remove_pointer_t<decltype(e)>;
        return LsmOps<E>::log_softmax_plane(stream, static_cast<const E*>(x), out, rows, V, col_out, col);
    });
}

hipError_t launch_log_softmax_gather_skewed(hipStream_t stream, int dtype, const void* logits, const int* labels,
                                            float* ws2, int N, int T, int U, int V, int blank) {
    return with_logits_type(dtype, [&](auto* e) {
        using E = std::remove_pointer_t<decltype(e)>;
        return LsmOps<E>::gather(stream, static_cast<const E*>(logits), labels, ws2, N, T, U, V, blank);
    });
}

hipError_t launch_logits_backward(hipStream_t stream, int dtype, const void* logits, const int* labels,
                                  const float* g2_diagonal, const float* scale, void* dlogits, int N, int T, int U, int V,
                                  int blank) {
    return with_logits_type(dtype, [&](auto* e) {
        using E = std::remove_pointer_t<decltype(e)>;
        return LsmOps<E>::backward(stream, static_cast<const E*>(logits), labels, g2_diagonal, scale,
                                   static_cast<E*>(dlogits), N, T, U, V, blank);
    });
}

hipError_t launch_lsm_gather_compact(hipStream_t stream, int dtype, const void* logits, float* ws2, const PackedRows& cr,
                                     int V, int blank) {
    return with_logits_type(dtype, [&](auto* e) {
        using E = std::remove_pointer_t<decltype(e)>;
        return LsmOps<E>::gather_compact(stream, static_cast<const E*>(logits), ws2, cr, V, blank);
    });
}

hipError_t launch_logits_backward_compact(hipStream_t stream, int dtype, const void* logits, const float* g2_rowmajor,
                                          const float* scale, void* dlogits, const PackedRows& cr, int V, int blank) {
    return with_logits_type(dtype, [&](auto* e) {
        using E = std::remove_pointer_t<decltype(e)>;
        return LsmOps<E>::backward_compact(stream, static_cast<const E*>(logits), g2_rowmajor, scale,
                                           static_cast<E*>(dlogits), cr, V, blank);
    });
}

}  // namespace rnnt
