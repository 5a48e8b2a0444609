// C ABI of libwarp_rnnt_amd.so (declared in include/warp_rnnt_amd.h), the reference-named family: the five entry points
// of core.h under their names and argument lists, so that the reference's own binding.cpp links against this library
// whole.  Host-side orchestration only.
#include <cstdio>

#include "api_common.h"

using namespace rnnt;

namespace {
// The staged forms of run_warp_rnnt / run_warp_rnnt_gather behind their sweeps: gradient pairs in place of the log-prob
// pairs staged in `grads`, then parked as two planes in the caller's alphas / betas (dead by then)
rnntStatus_t grads_in_place_then_split(rnntStream_t stream, float* grads, const int* xn, const int* yn, float* alphas,
                                       float* betas, const float* ll, float* costs, int N, int T, int U,
                                       float fastemit_lambda) {
    GradArgs gs{grads, nullptr, xn, yn, alphas, betas, ll, grads, costs, nullptr, T, U, 2, 0, fastemit_lambda};
    if (launch_grads(stream, gs, N, LOAD_SKEWED, WRITE_SKEWED2) != hipSuccess) return RNNT_STATUS_GRADS_BLANK_FAILED;
    if (launch_split_pairs(stream, grads, alphas, betas, (size_t)N * T * U) != hipSuccess)
        return RNNT_STATUS_GRADS_LABEL_FAILED;
    return RNNT_STATUS_SUCCESS;
}

}  // namespace

extern "C" {

// The reference-named entry points (core.h:29-39) own no workspace: everything they need has to come out of the buffers
// the caller's binding allocates (binding.cpp:58-75) -- and does: the tuned kernels want the (blank,label) pairs in the
// diagonal-major layout, which is exactly one (N,T,U,2) plane, and `grads` is at least that large and not yet written.
// So the pairs are staged in `grads`, the sweeps run on them (alphas / betas are the caller's scratch already, in the
// diagonal-major layout since round 1), and the gradient kernel -- which reads the log-probs from the caller's input
// again -- overwrites the staging area with the result.  Until round 4 these entries ran the single-role kernel with
// per-lane row-major / dense loads: 0.50 / 2.67 ms at N=16, T=1500, U=300 (V=50), now 0.27 / 0.64
// (tools/cabi_probe.py, profiles/r04_cabi_probe.txt).
rnntStatus_t run_warp_rnnt(rnntStream_t stream, unsigned int* counts, float* alphas, float* betas,
                           const int* labels, const float* log_probs, float* grads, float* costs,
                           const int* xn, const int* yn, int N, int T, int U, int V, int blank,
                           float fastemit_lambda) {
    if (!dims_ok(N, T, U) || !vocab_ok(V, blank)) return RNNT_STATUS_INVALID_ARGUMENT;
    if (N == 0) return RNNT_STATUS_SUCCESS;
    float* ll = reinterpret_cast<float*>(counts);   // (N,2U) uint32 scratch: first N words reused
    const size_t cells = (size_t)N * T * U;
    const bool stage = V >= 2 && (U == 1 || labels) && (int64_t)U * V < ((int64_t)1 << 31) && cells >= STAGED_FROM_CELLS;
    if (stage) {
        // dense (N,T,U,V) grads, zeroed by the caller: its head is the staging area -- pairs, then (room permitting:
        // V >= 4 or so) the flags and hand-over rings of the distributed lattice kernel -- and is zeroed again before the
        // gradient kernel writes its two slots per cell
        char* base = reinterpret_cast<char*>(grads);
        const size_t avail = cells * (size_t)V * sizeof(float);
        size_t off = align_up(cells * 2 * sizeof(float));
        int* redo = nullptr;
        unsigned long long* mail = nullptr;
        const size_t flag_bytes = align_up(((size_t)N * 2 + 2) * sizeof(int)), ring_bytes = wd_mail_bytes(N, T, U);
        if (aligned(base, ALIGN) && off + flag_bytes + align_up(ring_bytes) <= avail) {
            redo = reinterpret_cast<int*>(base + off);
            off += flag_bytes;
            mail = reinterpret_cast<unsigned long long*>(base + off);
            off += align_up(ring_bytes);
        }
        LatticeArgs la{grads, nullptr, xn, yn, alphas, betas, ll, T, U, 2, 0, nullptr, redo, redo ? redo + 2 * N : nullptr, mail};
        RingPrep prep{nullptr, 0, nullptr, nullptr, 0};
        la.prepared = lattice_ring_prep(stream, la, N, LOAD_SKEWED, &prep) ? 1 : 0;
        if (launch_gather(stream, log_probs, labels, grads, N, T, U, V, blank, true, &prep) != hipSuccess)
            return RNNT_STATUS_WARP_FAILED;
        if (launch_lattice(stream, la, N, LOAD_SKEWED) != hipSuccess) return RNNT_STATUS_WARP_FAILED;
        // gradient pairs in place of the log-prob pairs (coalesced both ways), parked in the caller's alphas / betas --
        // dead by then -- and expanded from there into whole dense rows, zeros included: the staging area is
        // overwritten with the rest, and nothing depends on the caller's zero-fill any more (the slot writes of the
        // direct form below cost 0.8 ms at N=16, T=1500, U=300, V=50, this 0.37)
        if (split_aligned(grads, alphas, betas)) {
            const rnntStatus_t st = grads_in_place_then_split(stream, grads, xn, yn, alphas, betas, ll, costs, N, T, U,
                                                              fastemit_lambda);
            if (st != RNNT_STATUS_SUCCESS) return st;
            if (launch_expand_split(stream, alphas, betas, labels, xn, yn, grads, N, T, U, V, blank) != hipSuccess)
                return RNNT_STATUS_GRADS_LABEL_FAILED;
            return RNNT_STATUS_SUCCESS;
        }
        if (hipMemsetAsync(grads, 0, off < avail ? off : avail, stream) != hipSuccess) return RNNT_STATUS_WARP_FAILED;
    } else {
        LatticeArgs la{log_probs, labels, xn, yn, alphas, betas, ll, T, U, V, blank};
        if (launch_lattice(stream, la, N, LOAD_DENSE) != hipSuccess) return RNNT_STATUS_WARP_FAILED;
    }
    GradArgs ga{log_probs, labels, xn, yn, alphas, betas, ll, grads, costs, nullptr,
                T, U, V, blank, fastemit_lambda};
    if (launch_grads(stream, ga, N, LOAD_DENSE, WRITE_DENSE_SLOTS) != hipSuccess)
        return RNNT_STATUS_GRADS_BLANK_FAILED;
    return RNNT_STATUS_SUCCESS;
}

rnntStatus_t run_warp_rnnt_gather(rnntStream_t stream, unsigned int* counts, float* alphas,
                                  float* betas, const float* log_probs, float* grads, float* costs,
                                  const int* xn, const int* yn, int N, int T, int U,
                                  float fastemit_lambda) {
    if (!dims_ok(N, T, U)) return RNNT_STATUS_INVALID_ARGUMENT;
    if (N == 0) return RNNT_STATUS_SUCCESS;
    float* ll = reinterpret_cast<float*>(counts);
    const size_t cells = (size_t)N * T * U;
    if (cells >= STAGED_FROM_CELLS && split_aligned(grads, alphas, betas)) {
        // (N,T,U,2) grads = one pair plane: staging area first, result afterwards.  No room for hand-over rings here:
        // the sweeps run on the single-workgroup log-domain kernel.
        if (launch_reskew(stream, log_probs, grads, N, T, U) != hipSuccess) return RNNT_STATUS_WARP_FAILED;
        LatticeArgs la{grads, nullptr, xn, yn, alphas, betas, ll, T, U, 2, 0};
        if (launch_lattice(stream, la, N, LOAD_SKEWED) != hipSuccess) return RNNT_STATUS_WARP_FAILED;
        // gradient pairs in place of the log-prob pairs, parked in alphas / betas (dead by then), turned back into the
        // row-major layout through LDS tiles: three coalesced passes (33 + 35 + 30 us at N=16, T=1500, U=300) instead
        // of one whose row-major reads and writes are scattered over the diagonal-major thread order (158 us)
        const rnntStatus_t st = grads_in_place_then_split(stream, grads, xn, yn, alphas, betas, ll, costs, N, T, U,
                                                          fastemit_lambda);
        if (st != RNNT_STATUS_SUCCESS) return st;
        if (launch_unskew(stream, alphas, betas, grads, N, T, U) != hipSuccess) return RNNT_STATUS_GRADS_LABEL_FAILED;
        return RNNT_STATUS_SUCCESS;
    }
    LatticeArgs la{log_probs, nullptr, xn, yn, alphas, betas, ll, T, U, 2, 0};
    if (launch_lattice(stream, la, N, LOAD_ROWMAJOR2) != hipSuccess) return RNNT_STATUS_WARP_FAILED;
    GradArgs ga{log_probs, nullptr, xn, yn, alphas, betas, ll, grads, costs, nullptr,
                T, U, 2, 0, fastemit_lambda};
    if (launch_grads(stream, ga, N, LOAD_ROWMAJOR2, WRITE_ROWMAJOR2) != hipSuccess)
        return RNNT_STATUS_GRADS_BLANK_FAILED;
    return RNNT_STATUS_SUCCESS;
}

// ---------------------------------------------------------------------------------------------------------
// The reference's own compact entry points (core.h:41-60), same names and argument lists, so that its
// binding.cpp links against this library whole.  Kept conventions: void return, the NULL stream (its binding
// relies on stream 0: it launches nothing on a stream of its own, binding.cpp:170,197,241).  Changed: a failed
// launch does not exit(-1) the process (core.h:7-14) but is remembered per thread -- rnnt_amd_compact_last_status().
// ---------------------------------------------------------------------------------------------------------
static thread_local rnntStatus_t g_compact_status = RNNT_STATUS_SUCCESS;

// A void entry point has failed: remember the status for rnnt_amd_compact_last_status(), say so on stderr (the
// reference's CHECK_KERNEL_STAT prints and exits, core.h:7-14; its binding never looks at a status) and make the
// failure impossible to miss downstream: costs become NaN (best effort, NULL stream like everything here) instead
// of whatever torch.empty held, so a training loop that ignores the status stops on a NaN loss rather than
// learning from uninitialised memory.
// `err` is what the failed launcher returned (it has already taken the error off the runtime's per-thread slot, so
// asking hipGetLastError() here would report "no error").
static void compact_fail(rnntStatus_t st, const char* what, float* costs, unsigned int N, hipError_t err = hipSuccess) {
    g_compact_status = st;
    fprintf(stderr, "%s failed: rnnt status %d (%s)\n", what, (int)st,
            st == RNNT_STATUS_INVALID_ARGUMENT ? "invalid argument or unsupported size" : hipGetErrorString(err));
    if (costs && N) {
        const hipError_t m = fill_nan(costs, N, nullptr);
        if (m != hipSuccess)
            fprintf(stderr, "%s: costs could not be set to NaN either (%s)\n", what, hipGetErrorString(m));
    }
}

rnntStatus_t rnnt_amd_compact_last_status(void) {
    const rnntStatus_t s = g_compact_status;
    g_compact_status = RNNT_STATUS_SUCCESS;
    return s;
}

void run_gather_for_compact(const float* xs, const int* ys, const unsigned int* xn, const unsigned int* yn,
                            float* gather_xs, long* loc, const unsigned int* memPref,
                            const unsigned int* labelPref, unsigned int N, unsigned int T, unsigned int U,
                            unsigned int V, unsigned int blank) {
    static_assert(sizeof(long) == sizeof(int64_t), "loc is the reference's `long` (at::kLong)");
    if (V < 1 || blank >= V) { compact_fail(RNNT_STATUS_INVALID_ARGUMENT, "run_gather_for_compact", nullptr, 0); return; }
    const hipError_t e = launch_gather_compact_rowmajor(nullptr, xs, ys, xn, yn, gather_xs,
                                                        reinterpret_cast<int64_t*>(loc), memPref, labelPref, N, T, U, V,
                                                        blank);
    if (e != hipSuccess) compact_fail(RNNT_STATUS_PROLOGUE_FAILED, "run_gather_for_compact", nullptr, 0, e);
}

void run_warp_rnnt_compact(unsigned int* counts, float* alphas, float* betas, const float* log_probs, float* grads,
                           float* costs, const unsigned int* xn, const unsigned int* yn,
                           const unsigned int* memPref, const unsigned int* labelPref, unsigned int N,
                           unsigned int T, unsigned int U, float fastemit_lambda, bool required_grad) {
    (void)labelPref;
    if (N == 0) return;
    if (!dims_ok((int)N, T > 0 ? (int)T : 1, U > 0 ? (int)U : 1)) {
        compact_fail(RNNT_STATUS_INVALID_ARGUMENT, "run_warp_rnnt_compact", costs, N);
        return;
    }
    const int* ixn = reinterpret_cast<const int*>(xn);
    const int* iyn = reinterpret_cast<const int*>(yn);
    // counts (2*sum(yn) + 2N words, binding.cpp:187): the first N hold the alpha-side log-likelihoods
    float* ll = reinterpret_cast<float*>(counts);
    // Staged like the padded entry points (round 5; until then: the single-role kernel with per-lane row-major loads,
    // tools/cabi_probe.py): `grads` (STU,2) is the caller's and not yet written -- exactly one plane of pairs.  The
    // row-major pairs are turned into each utterance's diagonal-major plane there (LDS tiles), the sweeps run on the
    // tuned kernels that need nothing but planes (k_lattice_wd as a plain launch for U <= 64, k_lattice_wl, lattice_ws.hip),
    // the gradient pairs replace the log-prob pairs in place, are parked in alphas / betas (dead by then) and turned
    // back.  Five coalesced passes instead of two whose loads and stores are scattered over the diagonal-major thread
    // order.  Not for required_grad = false (alphas and grads alias betas there, binding.cpp:192-195) and not below
    // 2^20 cells of launch bound (launch-bound sizes keep the two-launch form).
    const bool staged = required_grad && (size_t)N * T * U >= STAGED_FROM_CELLS && split_aligned(grads, alphas, betas) &&
                        grads != betas && alphas != betas;
    // (the staged form's first launch -- nothing of the caller's has been overwritten yet -- may be refused where the direct
    //  form is not, e.g. on its 2^31-workgroup grid limit: then the direct form runs)
    hipError_t e_stage = staged ? launch_reskew_compact32(nullptr, log_probs, grads, xn, yn, memPref, N, T, U) : hipErrorNotSupported;
    if (staged && e_stage != hipSuccess) (void)hipGetLastError();
    if (staged && e_stage == hipSuccess) {
        hipError_t e;
        LatticeArgs ls{grads, nullptr, ixn, iyn, alphas, betas, ll, (int)T, (int)U, 2, 0};
        ls.offs32 = memPref;
        e = launch_lattice(nullptr, ls, (int)N, LOAD_SKEWED);
        if (e != hipSuccess) { compact_fail(RNNT_STATUS_WARP_FAILED, "run_warp_rnnt_compact", costs, N, e); return; }
        GradArgs gs{grads, nullptr, ixn, iyn, alphas, betas, ll, grads, costs, nullptr, (int)T, (int)U, 2, 0, fastemit_lambda};
        gs.offs32 = memPref;
        e = launch_grads(nullptr, gs, (int)N, LOAD_SKEWED, WRITE_SKEWED2);
        if (e != hipSuccess) { compact_fail(RNNT_STATUS_GRADS_BLANK_FAILED, "run_warp_rnnt_compact", costs, N, e); return; }
        e = launch_split_pairs_compact32(nullptr, grads, alphas, betas, xn, yn, memPref, N, (size_t)N * T * U);
        if (e == hipSuccess) e = launch_unskew_compact32(nullptr, alphas, betas, grads, xn, yn, memPref, N, T, U);
        if (e != hipSuccess) compact_fail(RNNT_STATUS_GRADS_LABEL_FAILED, "run_warp_rnnt_compact", costs, N, e);
        return;
    }
    LatticeArgs la{log_probs, nullptr, ixn, iyn, alphas, betas, ll, (int)T, (int)U, 2, 0};
    la.offs32 = memPref;
    la.beta_only = required_grad ? 0 : 1;
    hipError_t e = launch_lattice(nullptr, la, (int)N, LOAD_ROWMAJOR2);
    if (e != hipSuccess) {
        compact_fail(RNNT_STATUS_WARP_FAILED, "run_warp_rnnt_compact", costs, N, e);
        return;
    }
    if (!required_grad) {   // the reference's "beta only" inference mode: costs from beta[0,0], nothing else is touched
        e = launch_costs_from_betas(nullptr, betas, memPref, ixn, iyn, costs, (int)N);
        if (e != hipSuccess) compact_fail(RNNT_STATUS_COSTS_FAILED, "run_warp_rnnt_compact", costs, N, e);
        return;
    }
    GradArgs ga{log_probs, nullptr, ixn, iyn, alphas, betas, ll, grads, costs, nullptr, (int)T, (int)U, 2, 0,
                fastemit_lambda};
    ga.offs32 = memPref;
    e = launch_grads(nullptr, ga, (int)N, LOAD_ROWMAJOR2, WRITE_ROWMAJOR2);
    if (e != hipSuccess) compact_fail(RNNT_STATUS_GRADS_BLANK_FAILED, "run_warp_rnnt_compact", costs, N, e);
}

void run_scatter_grad_for_compact(const float* grad_cost, const float* gather_grad, const long* loc,
                                  const int* cum_lens, float* scatter_grad, unsigned int STU, unsigned int N,
                                  unsigned int V, unsigned int blank) {
    if (V < 1 || blank >= V) { compact_fail(RNNT_STATUS_INVALID_ARGUMENT, "run_scatter_grad_for_compact", nullptr, 0); return; }
    const hipError_t e = launch_scatter_compact(nullptr, grad_cost, gather_grad, reinterpret_cast<const int64_t*>(loc),
                                                cum_lens, scatter_grad, (int64_t)STU, (int)N, (int)V, (int)blank);
    if (e != hipSuccess) compact_fail(RNNT_STATUS_EXPAND_FAILED, "run_scatter_grad_for_compact", nullptr, 0, e);
}

}  // extern "C"
