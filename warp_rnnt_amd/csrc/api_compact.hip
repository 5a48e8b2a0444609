// C ABI of libwarp_rnnt_amd.so (declared in include/warp_rnnt_amd.h), the native compact (ragged packed) family: replaces
// run_gather_for_compact + run_warp_rnnt_compact + run_scatter_grad_for_compact (core.h:41-60, core_compact.cu:360-500)
// with the conventions of the rest of this ABI (status codes, caller's stream, no exit(), no host synchronisation).
#include "../../include/warp_rnnt_amd_clamp.h"

#include "api_common.h"

using namespace rnnt;

namespace {

// The loss layout for STU cells and sweeps within the launch bounds, ALIGN bytes of padding behind it
Workspace compact_layout(Carver& c, int N, int64_t STU, int Tmax, int Umax) {
    const Workspace w = loss_layout(c, (size_t)STU, N, Tmax > 0 ? Tmax : 1, Umax > 0 ? Umax : 1);
    c.take<char>(ALIGN);
    return w;
}

// What the bounded entries keep behind it
struct BoundedExtra {
    int64_t* cell_offsets;   // (N+1,)
    int64_t* stats;          // (5,): the four of rnnt_amd_compact_offsets + "refused"
    int* label_offsets;      // (N+1,)
    int* xn_checked;         // (N,)
};
BoundedExtra bounded_layout(Carver& c, int N) {
    BoundedExtra e;
    e.cell_offsets = c.take<int64_t>((size_t)N + 1);
    e.stats = c.take<int64_t>(5);
    e.label_offsets = c.take<int>((size_t)N + 1);
    e.xn_checked = c.take<int>((size_t)N);
    return e;
}

// What step 1 of a compact loss call reads: fp32 log-probs (STU,V) -- the gather also writes each row's label index to
// loc -- or logits of `dtype`, through the fused log-softmax + gather over the packed rows (lsm.h: CompactMap).
struct CompactInput {
    bool logits;
    int dtype;
    const void* rows;
    int64_t* loc;
};

// The compact loss behind its entry's checks, on its carved workspace: step 1 by the kind of input, steps 2 and 3 with
// the cell offsets.  n_labels: what ys holds (< 0: label_offsets[N] labels, the kernels read no further).
rnntStatus_t compact_core(rnntStream_t stream, const Workspace& w, const CompactInput& in, const int* ys, int64_t n_labels,
                          const int* xn, const int* yn, const int64_t* cell_offsets, const int* label_offsets,
                          float* costs, float* grads2, int N, int64_t STU, int Tmax, int Umax, int V, int blank,
                          float fastemit_lambda) {
    // (rnnt_amd_loss_compact_bounded looks at the vocabulary only here, behind its offsets: N == 0 and STU == 0 come first)
    if (!vocab_ok(V, blank)) return RNNT_STATUS_INVALID_ARGUMENT;
    hipError_t e;
    if (in.logits) {
        const PackedRows cr{cell_offsets, label_offsets, xn, yn, ys, n_labels, STU, N};
        e = launch_lsm_gather_compact(stream, in.dtype, in.rows, w.ws2, cr, V, blank);
    } else {
        e = launch_gather_compact(stream, static_cast<const float*>(in.rows), ys, xn, yn, cell_offsets, label_offsets, w.ws2,
                                  in.loc, N, Tmax, Umax, V, blank, STU);
    }
    if (e != hipSuccess) return RNNT_STATUS_PROLOGUE_FAILED;
    return sweeps_and_pair_grads(stream, w, xn, yn, costs, grads2 ? grads2 : w.ws2, grads2 ? WRITE_ROWMAJOR2 : WRITE_SKEWED2,
                                 N, Tmax, Umax, cell_offsets, fastemit_lambda);
}

// The same with the launch bounds supplied by the caller: the offsets are computed here, on the device, and what the
// host would have checked after reading the maxima back is checked there too (compact.hip: k_compact_offsets) -- no
// host synchronisation anywhere, so the call can be captured into a HIP graph.  A batch whose lengths do not fit the
// bounds, or whose totals are not STU / n_labels, gets NaN costs and zero gradients.
rnntStatus_t compact_bounded(rnntStream_t stream, void* workspace, const CompactInput& in, const int* ys, int64_t n_labels,
                             const int* xn, const int* yn, float* costs, float* grads2, int N, int64_t STU, int Tmax,
                             int Umax, int V, int blank, float fastemit_lambda) {
    if (!compact_dims_ok(N, STU, Tmax, Umax) || !workspace_ok(workspace) || Tmax < 1 || Umax < 1 || n_labels < 0)
        return RNNT_STATUS_INVALID_ARGUMENT;
    if (N == 0) return RNNT_STATUS_SUCCESS;
    if (STU == 0) {
        // utterances but no cells: no length >= 1 frame can add up to that, so the batch is one this entry always
        // refuses -- and the kernels behind it return before they write anything.  Say so the way a refusal does.
        return fill_nan(costs, (size_t)N, stream) == hipSuccess ? RNNT_STATUS_SUCCESS : RNNT_STATUS_COSTS_FAILED;
    }
    Carver c(workspace);
    const Workspace w = compact_layout(c, N, STU, Tmax, Umax);
    const BoundedExtra e = bounded_layout(c, N);
    const CompactBounds b{e.xn_checked, STU, n_labels, Tmax, Umax};
    if (launch_compact_offsets(stream, xn, yn, N, e.cell_offsets, e.label_offsets, e.stats, &b) != hipSuccess)
        return RNNT_STATUS_PROLOGUE_FAILED;
    const rnntStatus_t st = compact_core(stream, w, in, ys, n_labels, e.xn_checked, yn, e.cell_offsets, e.label_offsets, costs,
                                         grads2, N, STU, Tmax, Umax, V, blank, fastemit_lambda);
    if (st != RNNT_STATUS_SUCCESS) return st;
    if (launch_zero_if_refused(stream, e.stats + 4, grads2, (size_t)STU) != hipSuccess) return RNNT_STATUS_EXPAND_FAILED;
    return RNNT_STATUS_SUCCESS;
}

rnntStatus_t compact_logits_backward(rnntStream_t stream, int dtype, const void* logits, const int* ys, int64_t n_labels,
                                     const int* xn, const int* yn, const int64_t* cell_offsets, const int* label_offsets,
                                     const float* grads2, const float* grad_costs, void* dlogits, int N, int64_t STU,
                                     int V, int blank, float clamp) {
    if (!dtype_ok(dtype) || !compact_dims_ok(N, STU, 1, 1) || !vocab_ok(V, blank) || n_labels < 0)
        return RNNT_STATUS_INVALID_ARGUMENT;
    if (n_labels > 0 && !ys) return RNNT_STATUS_INVALID_ARGUMENT;
    if (STU == 0) return RNNT_STATUS_SUCCESS;
    const PackedRows cr{cell_offsets, label_offsets, xn, yn, ys, n_labels, STU, N};
    if (launch_logits_backward_compact(stream, dtype, logits, grads2, grad_costs, dlogits, cr, V, blank, clamp) !=
        hipSuccess)
        return RNNT_STATUS_EXPAND_FAILED;
    return RNNT_STATUS_SUCCESS;
}

}  // namespace

extern "C" {

size_t rnnt_amd_workspace_size_compact(int N, int64_t STU, int Tmax, int Umax) {
    if (!compact_dims_ok(N, STU, Tmax, Umax)) return 0;
    Carver c(nullptr);
    compact_layout(c, N, STU, Tmax, Umax);
    return c.off;
}

size_t rnnt_amd_workspace_size_compact_bounded(int N, int64_t STU, int Tmax, int Umax) {
    if (!compact_dims_ok(N, STU, Tmax, Umax)) return 0;
    Carver c(nullptr);
    compact_layout(c, N, STU, Tmax, Umax);
    bounded_layout(c, N);
    return c.off;
}

// Device-side preparation of a compact batch (offsets + launch bounds), one launch.
rnntStatus_t rnnt_amd_compact_offsets(rnntStream_t stream, const int* xn, const int* yn, int N,
                                      int64_t* cell_offsets, int* label_offsets, int64_t* stats) {
    if (N < 0 || N > 65535 || !cell_offsets || !label_offsets || !stats) return RNNT_STATUS_INVALID_ARGUMENT;
    if (N > 0 && (!xn || !yn)) return RNNT_STATUS_INVALID_ARGUMENT;
    if (launch_compact_offsets(stream, xn, yn, N, cell_offsets, label_offsets, stats) != hipSuccess)
        return RNNT_STATUS_PROLOGUE_FAILED;
    return RNNT_STATUS_SUCCESS;
}

rnntStatus_t rnnt_amd_loss_compact(rnntStream_t stream, void* workspace, const float* xs, const int* ys,
                                   const int* xn, const int* yn, const int64_t* cell_offsets,
                                   const int* label_offsets, float* costs, float* grads2, int64_t* loc,
                                   int N, int64_t STU, int Tmax, int Umax, int V, int blank,
                                   float fastemit_lambda) {
    if (!compact_dims_ok(N, STU, Tmax, Umax) || !workspace_ok(workspace) || !vocab_ok(V, blank))
        return RNNT_STATUS_INVALID_ARGUMENT;
    if (N == 0 || STU == 0) return RNNT_STATUS_SUCCESS;
    Carver c(workspace);
    return compact_core(stream, compact_layout(c, N, STU, Tmax, Umax), CompactInput{false, RNNT_DTYPE_F32, xs, loc}, ys, -1,
                        xn, yn, cell_offsets, label_offsets, costs, grads2, N, STU, Tmax, Umax, V, blank, fastemit_lambda);
}

rnntStatus_t rnnt_amd_loss_compact_bounded(rnntStream_t stream, void* workspace, const float* xs, const int* ys,
                                           int64_t n_labels, const int* xn, const int* yn, float* costs, float* grads2,
                                           int64_t* loc, int N, int64_t STU, int Tmax, int Umax, int V, int blank,
                                           float fastemit_lambda) {
    return compact_bounded(stream, workspace, CompactInput{false, RNNT_DTYPE_F32, xs, loc}, ys, n_labels, xn, yn, costs,
                           grads2, N, STU, Tmax, Umax, V, blank, fastemit_lambda);
}

// The compact layout with LOGITS (fp32 / bf16 / fp16) in place of log-probs: the fused log-softmax + gather replaces the
// gather, everything behind it is rnnt_amd_loss_compact's.
rnntStatus_t rnnt_amd_loss_compact_logits(rnntStream_t stream, void* workspace, int dtype, const void* logits,
                                          const int* ys, const int* xn, const int* yn, const int64_t* cell_offsets,
                                          const int* label_offsets, float* costs, float* grads2, int N, int64_t STU,
                                          int Tmax, int Umax, int V, int blank, float fastemit_lambda) {
    if (!dtype_ok(dtype) || !compact_dims_ok(N, STU, Tmax, Umax) || !vocab_ok(V, blank) || !workspace_ok(workspace))
        return RNNT_STATUS_INVALID_ARGUMENT;
    if (labels_missing(Umax, ys)) return RNNT_STATUS_INVALID_ARGUMENT;
    if (N == 0 || STU == 0) return RNNT_STATUS_SUCCESS;
    Carver c(workspace);
    return compact_core(stream, compact_layout(c, N, STU, Tmax, Umax), CompactInput{true, dtype, logits, nullptr}, ys, -1,
                        xn, yn, cell_offsets, label_offsets, costs, grads2, N, STU, Tmax, Umax, V, blank, fastemit_lambda);
}

rnntStatus_t rnnt_amd_loss_compact_logits_bounded(rnntStream_t stream, void* workspace, int dtype, const void* logits,
                                                  const int* ys, int64_t n_labels, const int* xn, const int* yn,
                                                  float* costs, float* grads2, int N, int64_t STU, int Tmax, int Umax,
                                                  int V, int blank, float fastemit_lambda) {
    if (!dtype_ok(dtype) || !vocab_ok(V, blank) || (n_labels > 0 && !ys)) return RNNT_STATUS_INVALID_ARGUMENT;
    return compact_bounded(stream, workspace, CompactInput{true, dtype, logits, nullptr}, ys, n_labels, xn, yn, costs,
                           grads2, N, STU, Tmax, Umax, V, blank, fastemit_lambda);
}

rnntStatus_t rnnt_amd_compact_logits_backward(rnntStream_t stream, int dtype, const void* logits, const int* ys,
                                              int64_t n_labels, const int* xn, const int* yn,
                                              const int64_t* cell_offsets, const int* label_offsets,
                                              const float* grads2, const float* grad_costs, void* dlogits, int N,
                                              int64_t STU, int V, int blank) {
    return compact_logits_backward(stream, dtype, logits, ys, n_labels, xn, yn, cell_offsets, label_offsets, grads2,
                                   grad_costs, dlogits, N, STU, V, blank, 0.0f);
}

// include/warp_rnnt_amd_clamp.h: the same with the gradient clamp of the fused backward -- d/d logits at unit upstream
// limited to [-clamp, +clamp] elementwise, then scaled by grad_costs.  clamp == 0 IS the entry above.
rnntStatus_t rnnt_amd_compact_logits_backward_clamped(rnntStream_t stream, int dtype, const void* logits, const int* ys,
                                                      int64_t n_labels, const int* xn, const int* yn,
                                                      const int64_t* cell_offsets, const int* label_offsets,
                                                      const float* grads2, const float* grad_costs, void* dlogits,
                                                      int N, int64_t STU, int V, int blank, float clamp) {
    if (!clamp_ok(clamp)) return RNNT_STATUS_INVALID_ARGUMENT;
    return compact_logits_backward(stream, dtype, logits, ys, n_labels, xn, yn, cell_offsets, label_offsets, grads2,
                                   grad_costs, dlogits, N, STU, V, blank, clamp);
}

// Replaces run_scatter_grad_for_compact (core.h:56-60, core_compact.cu:456-500): dense (STU,V)
// gradient rows, fully written.  cum_lens = inclusive prefix sums of xn*(yn+1) (int32, as the
// reference's RNNTLossCompact.forward builds them, __init__.py:38).
rnntStatus_t rnnt_amd_compact_scatter_grads(rnntStream_t stream, const float* grad_costs,
                                            const float* grads2, const int64_t* loc, const int* cum_lens,
                                            float* dense_grads, int64_t STU, int N, int V, int blank) {
    if (N < 0 || STU < 0 || !vocab_ok(V, blank)) return RNNT_STATUS_INVALID_ARGUMENT;
    if (launch_scatter_compact(stream, grad_costs, grads2, loc, cum_lens, dense_grads, STU, N, V, blank) !=
        hipSuccess)
        return RNNT_STATUS_EXPAND_FAILED;
    return RNNT_STATUS_SUCCESS;
}

}  // extern "C"
