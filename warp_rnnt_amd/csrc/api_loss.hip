// C ABI of libwarp_rnnt_amd.so (declared in include/warp_rnnt_amd.h), the native padded family: version and diagnostics,
// workspace sizes, the loss and the two steps every loss entry is made of, expand, the logits backward, log-softmax, gather.
// Host-side orchestration only: argument checks, workspace carving, launches.
#include "../../include/warp_rnnt_amd_align.h"
#include "../../include/warp_rnnt_amd_clamp.h"

#include <cstdlib>

#include "api_common.h"
#include "hat.h"

using namespace rnnt;

namespace {

// Dense gradients: up to this many lattice cells the gradient kernel and the expansion run as ONE launch whose row writer
// reads alpha / beta / pairs itself (scattered reads of planes that sit in L2 / the Infinity Cache); above, two streaming
// launches.  One launch / two (tools/dense_rate.py, profiles/r04_grads_dense_ab.txt; us per call of the dense entry):
// T=150, U=40, V=28: N=16 28.2 / 30.7, N=32 35.0 / 37.6, N=64 46.2 / 48.2, N=128 67.0 / 68.7, N=256 114 / 113;
// T=500, U=100, V=50: N=4 ... 32 (0.2 M ... 1.6 M cells) equal within 0.5 us.  RNNT_DENSE_ONE_LAUNCH_CELLS overrides
// (0: never), for A/B runs.
inline size_t dense_in_one_launch_cells() {
    static const size_t v = ab_getenv("RNNT_DENSE_ONE_LAUNCH_CELLS") ? (size_t)atoll(ab_getenv("RNNT_DENSE_ONE_LAUNCH_CELLS"))
                                                                  : ((size_t)1 << 20);
    return v;
}

// rnnt_amd_workspace_mismatch_offset / rnnt_amd_debug_redo_offset: where a plane of the loss layout starts
size_t loss_layout_offset(int N, int T, int U, int* Workspace::*plane) {
    if (!dims_ok(N, T, U)) return 0;
    Carver c(reinterpret_cast<void*>(ALIGN));   // any non-null base: only the offset is wanted
    return reinterpret_cast<uintptr_t>(loss_layout(c, N, T, U).*plane) - ALIGN;
}

}  // namespace

hipError_t rnnt::fill_pair_plane(hipStream_t stream, const PairSource& src, const int* labels, float* ws2, int N, int T,
                                 int U, int V, int blank, LatticeArgs* la) {
    RingPrep prep{nullptr, 0, nullptr, nullptr, 0};
    const bool log_probs = src.kind == RNNT_IN_LOG_PROBS_DENSE || src.kind == RNNT_IN_LOG_PROBS_GATHERED;
    // where the sweeps are going to run on the ring kernel, let this launch prepare its flags and rings on the way
    if (la && log_probs) la->prepared = lattice_ring_prep(stream, *la, N, LOAD_SKEWED, &prep) ? 1 : 0;
    const RingPrep* carried = la ? &prep : nullptr;
    switch (src.kind) {
        case RNNT_IN_LOG_PROBS_DENSE:
            return launch_gather(stream, static_cast<const float*>(src.input), labels, ws2, N, T, U, V, blank, true, carried,
                                 src.blank_plane);
        case RNNT_IN_LOG_PROBS_GATHERED:
            return launch_reskew(stream, static_cast<const float*>(src.input), ws2, N, T, U, carried);
        case RNNT_IN_LOGITS_DENSE:
            return launch_log_softmax_gather_skewed(stream, src.dtype, src.input, labels, ws2, N, T, U, V, blank);
        case RNNT_ALIGN_IN_HAT_LOGITS:
            return launch_hat_gather_skewed(stream, src.dtype, src.input, labels, ws2, N, T, U, V, blank);
        default:
            return hipErrorInvalidValue;
    }
}

rnntStatus_t rnnt::sweeps_and_pair_grads(rnntStream_t stream, const Workspace& w, const int* xn, const int* yn,
                                         float* costs, float* gout, int writer, int N, int T, int U, const int64_t* offs,
                                         float fastemit_lambda, int prepared) {
    LatticeArgs la = sweep_args(w, xn, yn, N, T, U, offs);
    la.prepared = prepared;
    if (launch_lattice(stream, la, N, LOAD_SKEWED) != hipSuccess) return RNNT_STATUS_WARP_FAILED;
    if (!gout) return RNNT_STATUS_SUCCESS;
    GradArgs ga{w.ws2, nullptr, xn, yn, w.alphas, w.betas, w.ll, gout, costs, w.mismatch,
                T, U, 2, 0, fastemit_lambda, offs};
    if (launch_grads(stream, ga, N, LOAD_SKEWED, writer) != hipSuccess) return RNNT_STATUS_GRADS_BLANK_FAILED;
    return RNNT_STATUS_SUCCESS;
}

// rnnt_amd_loss with the element type of the input (RNNT_DTYPE_*: anything but fp32 for RNNT_IN_LOGITS_DENSE only);
// blank_plane (RNNT_IN_LOG_PROBS_DENSE only, or nullptr): the blank column of the log-probs as a plane of its own
static rnntStatus_t loss_of_type(rnntStream_t stream, void* workspace, int input_kind, int dtype, const void* input,
                                 const int* labels, const int* xn, const int* yn, float* costs, float* grads,
                                 int grads_kind, int N, int T, int U, int V, int blank, float fastemit_lambda,
                                 const float* blank_plane = nullptr) {
    if (!dtype_ok(dtype) || (dtype != RNNT_DTYPE_F32 && input_kind != RNNT_IN_LOGITS_DENSE))
        return RNNT_STATUS_INVALID_ARGUMENT;
    if (!dims_ok(N, T, U) || !workspace_ok(workspace)) return RNNT_STATUS_INVALID_ARGUMENT;
    if (input_kind != RNNT_IN_LOG_PROBS_GATHERED && (!vocab_ok(V, blank) || labels_missing(U, labels)))
        return RNNT_STATUS_INVALID_ARGUMENT;
    if (grads_kind == RNNT_GRADS_DENSE && input_kind != RNNT_IN_LOG_PROBS_DENSE)
        return RNNT_STATUS_INVALID_ARGUMENT;
    if (grads_kind < RNNT_GRADS_GATHERED || grads_kind > RNNT_GRADS_NONE)
        return RNNT_STATUS_INVALID_ARGUMENT;
    if (grads_kind != RNNT_GRADS_NONE && !grads) return RNNT_STATUS_INVALID_ARGUMENT;
    if (N == 0) return RNNT_STATUS_SUCCESS;
    // (the kinds of this entry: fill_pair_plane knows one more)
    if (input_kind < RNNT_IN_LOG_PROBS_DENSE || input_kind > RNNT_IN_LOGITS_DENSE) return RNNT_STATUS_INVALID_ARGUMENT;

    Carver c(workspace);
    const Workspace w = loss_layout(c, N, T, U);

    // 1. bring the (blank,label) log-prob pairs into the diagonal-major workspace
    LatticeArgs la = sweep_args(w, xn, yn, N, T, U, nullptr);
    if (fill_pair_plane(stream, PairSource{input_kind, dtype, input, blank_plane}, labels, w.ws2, N, T, U, V, blank, &la) !=
        hipSuccess)
        return RNNT_STATUS_PROLOGUE_FAILED;

    // 2. alpha / beta sweeps, 3. gradients + costs (+ guard).  For a dense result the pairs are produced in place in the
    //    workspace and expanded to full rows (zeros included) in one coalesced pass.
    float* gout = grads;
    int writer = WRITE_SKEWED2;
    // (row-major pairs for the caller: produced in place in the workspace like the others, then turned through LDS
    //  tiles -- 33 + 30 us at N=16, T=1500, U=300 against 92 for row-major writes from the diagonal-major thread order)
    const bool unskew_gathered = grads_kind == RNNT_GRADS_GATHERED && (size_t)N * T * U >= STAGED_FROM_CELLS;
    if (grads_kind == RNNT_GRADS_GATHERED && !unskew_gathered) writer = WRITE_ROWMAJOR2;   // (launch-bound sizes: direct)
    else if (grads_kind != RNNT_GRADS_GATHERED_DIAGONAL) gout = w.ws2;
    // launch-bound sizes: the gradient kernel and the expansion as one launch (c2 in bench.py: 0.0371 -> 0.0348 ms per
    // step); the row writer reads its cells' values from the planes itself
    const bool dense_in_one = grads_kind == RNNT_GRADS_DENSE && (size_t)N * T * U <= dense_in_one_launch_cells();
    const rnntStatus_t st = sweeps_and_pair_grads(stream, w, xn, yn, costs, dense_in_one ? nullptr : gout, writer, N, T, U,
                                                  nullptr, fastemit_lambda, la.prepared);
    if (st != RNNT_STATUS_SUCCESS) return st;
    if (dense_in_one) {
        GradArgs gd{w.ws2, labels, xn, yn, w.alphas, w.betas, w.ll, nullptr, costs, w.mismatch, T, U, V, blank,
                    fastemit_lambda};
        if (launch_grads_dense(stream, gd, grads, N) != hipSuccess) return RNNT_STATUS_GRADS_BLANK_FAILED;
        return RNNT_STATUS_SUCCESS;
    }
    if (grads_kind == RNNT_GRADS_DENSE) {
        if (launch_expand(stream, w.ws2, labels, xn, yn, nullptr, grads, N, T, U, V, blank, 1) != hipSuccess)
            return RNNT_STATUS_EXPAND_FAILED;
    }
    if (unskew_gathered) {
        if (launch_unskew(stream, w.ws2, nullptr, grads, N, T, U) != hipSuccess) return RNNT_STATUS_EXPAND_FAILED;
    }
    return RNNT_STATUS_SUCCESS;
}

// Diagnostics (bench.py: the gather kernel's own roofline entry): only step 1 of rnnt_amd_loss for dense log-probs, i.e.
// k_to_diagonal<true> into the workspace's pair plane -- with the blank column read from its plane where one is given
// (k_to_diagonal<true, ., true>): the two forms timed alone
static rnntStatus_t gather_only(rnntStream_t stream, void* workspace, const float* log_probs, const float* blank_plane,
                                const int* labels, int N, int T, int U, int V, int blank) {
    if (!dims_ok(N, T, U) || !workspace || !vocab_ok(V, blank)) return RNNT_STATUS_INVALID_ARGUMENT;
    if (labels_missing(U, labels)) return RNNT_STATUS_INVALID_ARGUMENT;
    Carver c(workspace);
    const PairSource src{RNNT_IN_LOG_PROBS_DENSE, RNNT_DTYPE_F32, log_probs, blank_plane};
    if (fill_pair_plane(stream, src, labels, loss_layout(c, N, T, U).ws2, N, T, U, V, blank, nullptr) != hipSuccess)
        return RNNT_STATUS_PROLOGUE_FAILED;
    return RNNT_STATUS_SUCCESS;
}

// Backward of the fused RNNT_IN_LOGITS_DENSE path: d(sum_n grad_costs[n]*cost[n]) / d(logits).
static rnntStatus_t logits_backward(rnntStream_t stream, int dtype, const void* logits, const int* labels,
                                    const float* grads_diagonal, const float* grad_costs, void* dlogits, int N, int T,
                                    int U, int V, int blank, float clamp) {
    if (!dtype_ok(dtype) || !dims_ok(N, T, U) || !vocab_ok(V, blank)) return RNNT_STATUS_INVALID_ARGUMENT;
    if (labels_missing(U, labels)) return RNNT_STATUS_INVALID_ARGUMENT;
    if (launch_logits_backward(stream, dtype, logits, labels, grads_diagonal, grad_costs, dlogits, N, T, U, V, blank,
                               clamp) != hipSuccess)
        return RNNT_STATUS_EXPAND_FAILED;
    return RNNT_STATUS_SUCCESS;
}

extern "C" {

int rnnt_amd_version(void) { return 110; }

int rnnt_amd_debug_set_lattice_kernel(int kernel) { return set_lattice_kernel_override(kernel); }

int rnnt_amd_debug_get_lattice_kernel(void) { return lattice_kernel_override(); }

int rnnt_amd_debug_last_lattice_kernel(void) { return last_lattice_kernel(); }

int rnnt_amd_debug_lattice_plan(int N, int T, int U, int loader, int resources, int cus, int pin, int folded) {
    return debug_lattice_plan(N, T, U, loader, resources, cus, pin, folded);
}

int rnnt_amd_debug_lsm_plan(int mode, int dtype, int64_t rows, int V, int T, int U, int compact, int aligned, int plane,
                            int* out, int n_out) {
    return debug_lsm_plan(mode, dtype, rows, V, T, U, compact, aligned, plane, out, n_out);
}

volatile unsigned* rnnt_amd_mismatch_flag(int device) { return mismatch_words(device, true); }

size_t rnnt_amd_workspace_size(int N, int T, int U) {
    if (!dims_ok(N, T, U)) return 0;
    Carver c(nullptr);
    loss_layout(c, N, T, U);
    return c.off;
}

size_t rnnt_amd_workspace_mismatch_offset(int N, int T, int U) { return loss_layout_offset(N, T, U, &Workspace::mismatch); }

size_t rnnt_amd_debug_redo_offset(int N, int T, int U) { return loss_layout_offset(N, T, U, &Workspace::redo); }

rnntStatus_t rnnt_amd_loss(rnntStream_t stream, void* workspace, int input_kind, const float* input,
                           const int* labels, const int* xn, const int* yn, float* costs, float* grads,
                           int grads_kind, int N, int T, int U, int V, int blank,
                           float fastemit_lambda) {
    return loss_of_type(stream, workspace, input_kind, RNNT_DTYPE_F32, input, labels, xn, yn, costs, grads, grads_kind, N, T,
                        U, V, blank, fastemit_lambda);
}

rnntStatus_t rnnt_amd_loss_blank_plane(rnntStream_t stream, void* workspace, const float* log_probs,
                                       const float* blank_plane, const int* labels, const int* xn, const int* yn,
                                       float* costs, float* grads, int grads_kind, int N, int T, int U, int V, int blank,
                                       float fastemit_lambda) {
    if (!blank_plane) return RNNT_STATUS_INVALID_ARGUMENT;
    return loss_of_type(stream, workspace, RNNT_IN_LOG_PROBS_DENSE, RNNT_DTYPE_F32, log_probs, labels, xn, yn, costs, grads,
                        grads_kind, N, T, U, V, blank, fastemit_lambda, blank_plane);
}

rnntStatus_t rnnt_amd_loss_logits(rnntStream_t stream, void* workspace, int dtype, const void* logits, const int* labels,
                                  const int* xn, const int* yn, float* costs, float* grads, int grads_kind, int N, int T,
                                  int U, int V, int blank, float fastemit_lambda) {
    return loss_of_type(stream, workspace, RNNT_IN_LOGITS_DENSE, dtype, logits, labels, xn, yn, costs, grads, grads_kind, N,
                        T, U, V, blank, fastemit_lambda);
}

// Diagnostics: run only the alpha/beta sweep on whatever the workspace holds (after a call to
// rnnt_amd_loss the (blank,label) pairs are still there unless grads were produced in place).
rnntStatus_t rnnt_amd_debug_lattice_only(rnntStream_t stream, void* workspace, const int* xn,
                                         const int* yn, int N, int T, int U) {
    if (!dims_ok(N, T, U) || !workspace) return RNNT_STATUS_INVALID_ARGUMENT;
    Carver c(workspace);
    return sweeps_and_pair_grads(stream, loss_layout(c, N, T, U), xn, yn, nullptr, nullptr, 0, N, T, U, nullptr, 0.f);
}

rnntStatus_t rnnt_amd_debug_gather_only(rnntStream_t stream, void* workspace, const float* log_probs,
                                        const int* labels, int N, int T, int U, int V, int blank) {
    return gather_only(stream, workspace, log_probs, nullptr, labels, N, T, U, V, blank);
}

rnntStatus_t rnnt_amd_debug_gather_only_blank_plane(rnntStream_t stream, void* workspace, const float* log_probs,
                                                    const float* blank_plane, const int* labels, int N, int T, int U,
                                                    int V, int blank) {
    if (!blank_plane) return RNNT_STATUS_INVALID_ARGUMENT;
    return gather_only(stream, workspace, log_probs, blank_plane, labels, N, T, U, V, blank);
}

rnntStatus_t rnnt_amd_expand_grads(rnntStream_t stream, const float* grads_diagonal, const int* labels,
                                   const int* xn, const int* yn, const float* grad_costs,
                                   float* dense_grads, int N, int T, int U, int V, int blank,
                                   int overwrite) {
    if (!dims_ok(N, T, U) || !vocab_ok(V, blank)) return RNNT_STATUS_INVALID_ARGUMENT;
    if ((int64_t)U * V >= (int64_t)1 << 31) return RNNT_STATUS_INVALID_ARGUMENT;
    if ((int64_t)N * T >= (int64_t)1 << 31) return RNNT_STATUS_INVALID_ARGUMENT;
    if (launch_expand(stream, grads_diagonal, labels, xn, yn, grad_costs, dense_grads, N, T, U, V, blank,
                      overwrite) != hipSuccess)
        return RNNT_STATUS_EXPAND_FAILED;
    return RNNT_STATUS_SUCCESS;
}

rnntStatus_t rnnt_amd_logits_backward_typed(rnntStream_t stream, int dtype, const void* logits, const int* labels,
                                            const float* grads_diagonal, const float* grad_costs, void* dlogits,
                                            int N, int T, int U, int V, int blank) {
    return logits_backward(stream, dtype, logits, labels, grads_diagonal, grad_costs, dlogits, N, T, U, V, blank, 0.0f);
}

// include/warp_rnnt_amd_clamp.h: the same with the gradient clamp.  clamp == 0 IS rnnt_amd_logits_backward_typed.
rnntStatus_t rnnt_amd_logits_backward_clamped(rnntStream_t stream, int dtype, const void* logits, const int* labels,
                                              const float* grads_diagonal, const float* grad_costs, void* dlogits,
                                              int N, int T, int U, int V, int blank, float clamp) {
    if (!clamp_ok(clamp)) return RNNT_STATUS_INVALID_ARGUMENT;
    return logits_backward(stream, dtype, logits, labels, grads_diagonal, grad_costs, dlogits, N, T, U, V, blank, clamp);
}

rnntStatus_t rnnt_amd_logits_backward(rnntStream_t stream, const float* logits, const int* labels,
                                      const float* grads_diagonal, const float* grad_costs, float* dlogits,
                                      int N, int T, int U, int V, int blank) {
    return rnnt_amd_logits_backward_typed(stream, RNNT_DTYPE_F32, logits, labels, grads_diagonal, grad_costs, dlogits, N, T,
                                          U, V, blank);
}

rnntStatus_t rnnt_amd_log_softmax_typed(rnntStream_t stream, int dtype, const void* x, float* out, int64_t rows, int V) {
    if (!dtype_ok(dtype) || rows < 0 || V < 1) return RNNT_STATUS_INVALID_ARGUMENT;
    if (launch_log_softmax(stream, dtype, x, out, rows, V) != hipSuccess) return RNNT_STATUS_PROLOGUE_FAILED;
    return RNNT_STATUS_SUCCESS;
}

rnntStatus_t rnnt_amd_log_softmax(rnntStream_t stream, const float* x, float* out, int64_t rows, int V) {
    return rnnt_amd_log_softmax_typed(stream, RNNT_DTYPE_F32, x, out, rows, V);
}

rnntStatus_t rnnt_amd_log_softmax_plane_typed(rnntStream_t stream, int dtype, const void* x, float* out, float* col_out,
                                              int64_t rows, int V, int col) {
    if (!dtype_ok(dtype) || rows < 0 || V < 1 || col < 0 || col >= V || !col_out) return RNNT_STATUS_INVALID_ARGUMENT;
    if (launch_log_softmax_plane(stream, dtype, x, out, col_out, rows, V, col) != hipSuccess)
        return RNNT_STATUS_PROLOGUE_FAILED;
    return RNNT_STATUS_SUCCESS;
}

rnntStatus_t rnnt_amd_log_softmax_plane(rnntStream_t stream, const float* x, float* out, float* col_out, int64_t rows,
                                        int V, int col) {
    return rnnt_amd_log_softmax_plane_typed(stream, RNNT_DTYPE_F32, x, out, col_out, rows, V, col);
}

rnntStatus_t rnnt_amd_log_softmax_backward(rnntStream_t stream, const float* grad_out, const float* out,
                                           float* grad_in, int64_t rows, int V) {
    if (rows < 0 || V < 1) return RNNT_STATUS_INVALID_ARGUMENT;
    if (launch_log_softmax_backward(stream, grad_out, out, grad_in, rows, V) != hipSuccess)
        return RNNT_STATUS_PROLOGUE_FAILED;
    return RNNT_STATUS_SUCCESS;
}

rnntStatus_t rnnt_amd_gather(rnntStream_t stream, const float* log_probs, const int* labels,
                             float* gathered, int N, int T, int U, int V, int blank) {
    if (!dims_ok(N, T, U) || !vocab_ok(V, blank)) return RNNT_STATUS_INVALID_ARGUMENT;
    if (launch_gather(stream, log_probs, labels, gathered, N, T, U, V, blank, false) != hipSuccess)
        return RNNT_STATUS_PROLOGUE_FAILED;
    return RNNT_STATUS_SUCCESS;
}

}  // extern "C"
