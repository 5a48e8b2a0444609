// The forward log-softmax kernels of lsm.h for fp32 logits, and the family's launchers (kernels.h).
#include <climits>

#include "lsm.h"
#include "../../include/warp_rnnt_amd.h"

namespace rnnt {

template struct LsmOps<float>;

// The knobs of the log-softmax family and of its backward, read from the environment once per process -- here and nowhere
// else, and only in the A/B build (common.h: ab_getenv): the shipped library keeps the defaults.
const LsmKnobs& lsm_knobs() {
    static const LsmKnobs knobs = [] {
        LsmKnobs k;
        const auto set = [](const char* name) { return ab_getenv(name) != nullptr; };
        const auto number = [](const char* name, int unset) { const char* v = ab_getenv(name); return v ? atoi(v) : unset; };
        k.no_regs = set("RNNT_LSM_NO_REGS");
        k.regs_xcd = number("RNNT_LSM_REGS_XCD", k.regs_xcd);
        k.no_lgr = set("RNNT_LSM_NO_LGR");
        k.no_rows = set("RNNT_LSM_NO_ROWS");
        k.no_diag = set("RNNT_LSM_NO_DIAG");
        k.rows_any = set("RNNT_LSM_ROWS_ANY");
        k.no_wp = set("RNNT_LSM_NO_WP");
        k.wp_fused = set("RNNT_LSM_WP_FUSED");
        k.lg_xcd = number("RNNT_LG_XCD", k.lg_xcd);
        k.lg_xcd_fused = number("RNNT_LG_XCD_FUSED", k.lg_xcd_fused);
        k.bwd_xcd = number("RNNT_LSMBWD_XCD", k.bwd_xcd);
        k.bwd_smallest_cover = set("RNNT_LSMBWD_SMALLEST_COVER");
        return k;
    }();
    return knobs;
}

int debug_lsm_plan(int mode, int dtype, int64_t rows, int V, int T, int U, int compact, int aligned, int plane, int* out,
                   int n_out) {
    if (mode < LSM_NORM || mode > LSM_BWD + 1 || dtype < RNNT_DTYPE_F32 || dtype > RNNT_DTYPE_F16 || rows < 0 || V < 1)
        return -1;
    const LsmKnobs& knobs = lsm_knobs();
    LsmFacts f{mode, dtype == RNNT_DTYPE_F32 ? 4 : 2, rows, V, aligned != 0, compact != 0, T, U, plane != 0};
    const LsmPlan p = mode > LSM_BWD ? plan_lsm_backward(rows, V, aligned != 0, knobs) : plan_lsm(f, knobs);
    int tail = -1;
    if (p.family == LsmFamily::REGS && p.head_rows < rows) {
        f.rows = rows - p.head_rows;
        tail = (int)plan_lsm(f, knobs).family;
    }
    const int fields[16] = {(int)p.family, p.KR, p.L, p.Q, p.WP, p.TH, p.NV, (int)p.grid, (int)p.grid_y, (int)p.grid_z,
                            (int)p.lds_bytes, p.R, p.q, p.xcd, p.head_rows > INT_MAX ? INT_MAX : (int)p.head_rows, tail};
    for (int i = 0; out && i < n_out && i < 16; ++i) out[i] = fields[i];
    return (int)p.family;
}
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
                                  int blank, float clamp) {
    return with_logits_type(dtype, [&](auto* e) {
        using E = std::remove_pointer_t<decltype(e)>;
        return LsmOps<E>::backward(stream, static_cast<const E*>(logits), labels, g2_diagonal, scale,
                                   static_cast<E*>(dlogits), N, T, U, V, blank, clamp);
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
                                          const float* scale, void* dlogits, const PackedRows& cr, int V, int blank,
                                          float clamp) {
    return with_logits_type(dtype, [&](auto* e) {
        using E = std::remove_pointer_t<decltype(e)>;
        return LsmOps<E>::backward_compact(stream, static_cast<const E*>(logits), g2_rowmajor, scale,
                                           static_cast<E*>(dlogits), cr, V, blank, clamp);
    });
}

}  // namespace rnnt
