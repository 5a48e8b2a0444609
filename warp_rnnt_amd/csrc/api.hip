// C ABI of libwarp_rnnt_amd.so (declared in include/warp_rnnt_amd.h).
// Host-side orchestration only: argument checks, workspace carving, launches.
#include "../../include/warp_rnnt_amd.h"
#include "../../include/warp_rnnt_amd_clamp.h"
#include "../../include/warp_rnnt_amd_joint_dropout.h"
#include "../../include/warp_rnnt_amd_hat.h"
#include "../../include/warp_rnnt_amd_align.h"

#include <cstdio>
#include <cstdlib>

#include "align.h"
#include "common.h"
#include "hat.h"
#include "kernels.h"
#include "philox.h"

using namespace rnnt;

namespace {

constexpr size_t ALIGN = 256;
// Lattices from this many cells on take the multi-pass forms (stage, sweep on the tuned kernels, turn the layout
// through LDS tiles); smaller ones are launch-bound and keep the single-kernel forms (tools/cabi_probe.py: N=16, T=150,
// U=40: 24 us in two launches against 35 in five; N=16, T=1500, U=300: 500 against 274)
constexpr size_t STAGED_FROM_CELLS = (size_t)1 << 20;
inline size_t align_up(size_t x) { return (x + ALIGN - 1) / ALIGN * ALIGN; }
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

struct Workspace {
    float* alphas;
    float* betas;
    float* ws2;      // diagonal-major (blank,label) pairs; later the gathered grads
    float* ll;
    int* mismatch;
    int* redo;       // (2N + 2,) redo flags of k_lattice_wd, its work-item counter, the launch counter's value
    unsigned long long* mail;   // boundary-column rings of k_lattice_wd (kernels.h)
};

// One layout for the padded and the compact form: `cells` lattice cells (N*T*U / STU), rings for sweeps of shape (T, U)
// (the compact form: its launch bounds), `pad` bytes behind everything (the compact form's ALIGN).
size_t carve(void* base, size_t cells, int N, int T, int U, size_t pad, Workspace* w) {
    size_t off = 0;
    char* p = static_cast<char*>(base);
    auto take = [&](size_t bytes) { size_t o = off; off += align_up(bytes); return p ? p + o : nullptr; };
    float* alphas = reinterpret_cast<float*>(take(cells * sizeof(float)));
    float* betas = reinterpret_cast<float*>(take(cells * sizeof(float)));
    float* ws2 = reinterpret_cast<float*>(take(cells * 2 * sizeof(float)));
    float* ll = reinterpret_cast<float*>(take((size_t)N * sizeof(float)));
    int* mismatch = reinterpret_cast<int*>(take((size_t)N * sizeof(int)));
    int* redo = reinterpret_cast<int*>(take(((size_t)N * 2 + 2) * sizeof(int)));   // flags, queue head, launch counter
    // (reserved by SHAPE, never by the current route: the size of a workspace must not depend on a setting)
    unsigned long long* mail = reinterpret_cast<unsigned long long*>(take(wd_mail_bytes(N, T, U)));
    if (w) *w = Workspace{alphas, betas, ws2, ll, mismatch, redo, mail};
    return off + pad;
}
size_t carve(void* base, int N, int T, int U, Workspace* w) { return carve(base, (size_t)N * T * U, N, T, U, 0, w); }

inline bool vocab_ok(int V, int blank) { return V >= 1 && blank >= 0 && blank < V; }
// the gradient clamp of the *_clamped entries: 0 = off, otherwise a finite positive bound
inline bool clamp_ok(float clamp) { return clamp >= 0.0f && clamp <= 3.402823466e+38f; }     // (false for a NaN)
inline bool dtype_ok(int dtype) { return dtype == RNNT_DTYPE_F32 || dtype == RNNT_DTYPE_BF16 || dtype == RNNT_DTYPE_F16; }
inline bool aligned(const void* p, size_t to) { return reinterpret_cast<uintptr_t>(p) % to == 0; }
inline bool workspace_ok(const void* workspace) { return workspace && aligned(workspace, ALIGN); }
// what launch_split_pairs / launch_unskew / launch_expand_split ask of a pair plane and the two planes it is parked in
inline bool split_aligned(const float* pairs, const float* a, const float* b) {
    return aligned(pairs, 16) && aligned(a, 8) && aligned(b, 8);
}
inline hipError_t fill_nan(float* costs, size_t N, hipStream_t stream) {
    return hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(costs), 0x7fc00000, N, stream);
}

bool dims_ok(int N, int T, int U) {
    if (N < 0 || T < 1 || U < 1) return false;
    if (N > 65535) return false;                               // gridDim.y of the gradient kernel
    if ((int64_t)T * U >= (int64_t)1 << 29) return false;      // per-utterance plane < 4 GiB of float2 (buffer descriptors)
    if ((int64_t)N * T * U >= (int64_t)1 << 32) return false;  // flat cell index is 32-bit
    return true;
}
bool compact_dims_ok(int N, int64_t STU, int Tmax, int Umax) {
    return dims_ok(N, Tmax > 0 ? Tmax : 1, Umax > 0 ? Umax : 1) && STU >= 0 && STU < ((int64_t)1 << 32);
}

LatticeArgs sweep_args(const Workspace& w, const int* xn, const int* yn, int N, int T, int U, const int64_t* offs) {
    return LatticeArgs{w.ws2, nullptr, xn, yn, w.alphas, w.betas, w.ll, T, U, 2, 0, offs, w.redo, w.redo + 2 * N, w.mail};
}

// Steps 2 and 3 of a loss call on a carved workspace whose pair plane is filled: the alpha / beta sweeps of shape (T, U),
// then costs, guard and the gradient pairs, written by `writer` into gout (nullptr: the sweeps only).  offs: the compact
// layout's cell offsets, nullptr for padded planes; prepared: LatticeArgs::prepared (the producer of the pairs carried
// the ring kernel's RingPrep).
rnntStatus_t sweeps_and_pair_grads(rnntStream_t stream, const Workspace& w, const int* xn, const int* yn, float* costs,
                                   float* gout, int writer, int N, int T, int U, const int64_t* offs,
                                   float fastemit_lambda, int prepared = 0) {
    LatticeArgs la = sweep_args(w, xn, yn, N, T, U, offs);
    la.prepared = prepared;
    if (launch_lattice(stream, la, N, LOAD_SKEWED) != hipSuccess) return RNNT_STATUS_WARP_FAILED;
    if (!gout) return RNNT_STATUS_SUCCESS;
    GradArgs ga{w.ws2, nullptr, xn, yn, w.alphas, w.betas, w.ll, gout, costs, w.mismatch,
                T, U, 2, 0, fastemit_lambda, offs};
    if (launch_grads(stream, ga, N, LOAD_SKEWED, writer) != hipSuccess) return RNNT_STATUS_GRADS_BLANK_FAILED;
    return RNNT_STATUS_SUCCESS;
}

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
    return carve(nullptr, N, T, U, nullptr);
}

size_t rnnt_amd_workspace_mismatch_offset(int N, int T, int U) {
    if (!dims_ok(N, T, U)) return 0;
    Workspace w;
    carve(reinterpret_cast<void*>(ALIGN), N, T, U, &w);   // any non-null base: only the offset is wanted
    return reinterpret_cast<uintptr_t>(w.mismatch) - ALIGN;
}

size_t rnnt_amd_debug_redo_offset(int N, int T, int U) {
    if (!dims_ok(N, T, U)) return 0;
    Workspace w;
    carve(reinterpret_cast<void*>(ALIGN), N, T, U, &w);
    return reinterpret_cast<uintptr_t>(w.redo) - ALIGN;
}

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

// rnnt_amd_loss with the element type of the input (RNNT_DTYPE_*: anything but fp32 for RNNT_IN_LOGITS_DENSE only);
// blank_plane (RNNT_IN_LOG_PROBS_DENSE only, or nullptr): the blank column of the log-probs as a plane of its own
static rnntStatus_t loss_of_type(rnntStream_t stream, void* workspace, int input_kind, int dtype, const void* input_any,
                                 const int* labels, const int* xn, const int* yn, float* costs, float* grads,
                                 int grads_kind, int N, int T, int U, int V, int blank, float fastemit_lambda,
                                 const float* blank_plane = nullptr) {
    if (!dtype_ok(dtype) || (dtype != RNNT_DTYPE_F32 && input_kind != RNNT_IN_LOGITS_DENSE))
        return RNNT_STATUS_INVALID_ARGUMENT;
    const float* input = static_cast<const float*>(input_any);      // (fp32 input kinds only)
    if (!dims_ok(N, T, U) || !workspace_ok(workspace)) return RNNT_STATUS_INVALID_ARGUMENT;
    if (input_kind != RNNT_IN_LOG_PROBS_GATHERED && (!vocab_ok(V, blank) || (U > 1 && !labels)))
        return RNNT_STATUS_INVALID_ARGUMENT;
    if (grads_kind == RNNT_GRADS_DENSE && input_kind != RNNT_IN_LOG_PROBS_DENSE)
        return RNNT_STATUS_INVALID_ARGUMENT;
    if (grads_kind < RNNT_GRADS_GATHERED || grads_kind > RNNT_GRADS_NONE)
        return RNNT_STATUS_INVALID_ARGUMENT;
    if (grads_kind != RNNT_GRADS_NONE && !grads) return RNNT_STATUS_INVALID_ARGUMENT;
    if (N == 0) return RNNT_STATUS_SUCCESS;

    Workspace w;
    carve(workspace, N, T, U, &w);

    // 1. bring the (blank,label) log-prob pairs into the diagonal-major workspace -- and, where the sweeps are going to run on
    //    the ring kernel, let that launch prepare its flags and rings on the way (kernels.h: RingPrep)
    LatticeArgs la = sweep_args(w, xn, yn, N, T, U, nullptr);
    RingPrep prep{nullptr, 0, nullptr, nullptr, 0};
    hipError_t e;
    switch (input_kind) {
        case RNNT_IN_LOG_PROBS_DENSE:
            la.prepared = lattice_ring_prep(stream, la, N, LOAD_SKEWED, &prep) ? 1 : 0;
            e = launch_gather(stream, input, labels, w.ws2, N, T, U, V, blank, true, &prep, blank_plane); break;
        case RNNT_IN_LOG_PROBS_GATHERED:
            la.prepared = lattice_ring_prep(stream, la, N, LOAD_SKEWED, &prep) ? 1 : 0;
            e = launch_reskew(stream, input, w.ws2, N, T, U, &prep); break;
        case RNNT_IN_LOGITS_DENSE:
            e = launch_log_softmax_gather_skewed(stream, dtype, input_any, labels, w.ws2, N, T, U, V, blank); break;
        default:
            return RNNT_STATUS_INVALID_ARGUMENT;
    }
    if (e != hipSuccess) return RNNT_STATUS_PROLOGUE_FAILED;

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
    Workspace w;
    carve(workspace, N, T, U, &w);
    return sweeps_and_pair_grads(stream, w, xn, yn, nullptr, nullptr, 0, N, T, U, nullptr, 0.f);
}

// Diagnostics (bench.py: the gather kernel's own roofline entry): only step 1 of rnnt_amd_loss for dense log-probs,
// i.e. k_to_diagonal<true> into the workspace's pair plane.
rnntStatus_t rnnt_amd_debug_gather_only(rnntStream_t stream, void* workspace, const float* log_probs,
                                        const int* labels, int N, int T, int U, int V, int blank) {
    if (!dims_ok(N, T, U) || !workspace || !vocab_ok(V, blank)) return RNNT_STATUS_INVALID_ARGUMENT;
    if (U > 1 && !labels) return RNNT_STATUS_INVALID_ARGUMENT;
    Workspace w;
    carve(workspace, N, T, U, &w);
    if (launch_gather(stream, log_probs, labels, w.ws2, N, T, U, V, blank, true) != hipSuccess)
        return RNNT_STATUS_PROLOGUE_FAILED;
    return RNNT_STATUS_SUCCESS;
}

// ... and the same step with the blank column read from its plane (k_to_diagonal<true, ., true>): the two forms timed alone
rnntStatus_t rnnt_amd_debug_gather_only_blank_plane(rnntStream_t stream, void* workspace, const float* log_probs,
                                                    const float* blank_plane, const int* labels, int N, int T, int U,
                                                    int V, int blank) {
    if (!dims_ok(N, T, U) || !workspace || !vocab_ok(V, blank) || !blank_plane) return RNNT_STATUS_INVALID_ARGUMENT;
    if (U > 1 && !labels) return RNNT_STATUS_INVALID_ARGUMENT;
    Workspace w;
    carve(workspace, N, T, U, &w);
    if (launch_gather(stream, log_probs, labels, w.ws2, N, T, U, V, blank, true, nullptr, blank_plane) != hipSuccess)
        return RNNT_STATUS_PROLOGUE_FAILED;
    return RNNT_STATUS_SUCCESS;
}

size_t rnnt_amd_workspace_size_compact(int N, int64_t STU, int Tmax, int Umax) {
    if (!compact_dims_ok(N, STU, Tmax, Umax)) return 0;
    return carve(nullptr, (size_t)STU, N, Tmax > 0 ? Tmax : 1, Umax > 0 ? Umax : 1, ALIGN, nullptr);
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

namespace {
// What step 1 of a compact loss call reads: fp32 log-probs (STU,V) -- the gather also writes each row's label index to
// loc -- or logits of `dtype`, through the fused log-softmax + gather over the packed rows (lsm.h: CompactMap).
struct CompactInput {
    bool logits;
    int dtype;
    const void* rows;
    int64_t* loc;
};

// The compact loss behind its entry's checks: step 1 by the kind of input, steps 2 and 3 with the cell offsets.
// n_labels: what ys holds (< 0: label_offsets[N] labels, the kernels read no further).
rnntStatus_t compact_core(rnntStream_t stream, void* workspace, const CompactInput& in, const int* ys, int64_t n_labels,
                          const int* xn, const int* yn, const int64_t* cell_offsets, const int* label_offsets,
                          float* costs, float* grads2, int N, int64_t STU, int Tmax, int Umax, int V, int blank,
                          float fastemit_lambda) {
    // (rnnt_amd_loss_compact_bounded looks at the vocabulary only here, behind its offsets: N == 0 and STU == 0 come first)
    if (!vocab_ok(V, blank)) return RNNT_STATUS_INVALID_ARGUMENT;
    Workspace w;
    carve(workspace, (size_t)STU, N, Tmax > 0 ? Tmax : 1, Umax > 0 ? Umax : 1, ALIGN, &w);
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
struct BoundedExtra {
    int64_t* cell_offsets;   // (N+1,)
    int64_t* stats;          // (5,): the four of rnnt_amd_compact_offsets + "refused"
    int* label_offsets;      // (N+1,)
    int* xn_checked;         // (N,)
};
size_t carve_bounded(char* base, size_t off, int N, BoundedExtra* e) {
    auto take = [&](size_t bytes) { size_t o = off; off += align_up(bytes); return base ? base + o : nullptr; };
    int64_t* co = reinterpret_cast<int64_t*>(take(((size_t)N + 1) * 8));
    int64_t* st = reinterpret_cast<int64_t*>(take(5 * 8));
    int* lo = reinterpret_cast<int*>(take(((size_t)N + 1) * 4));
    int* xc = reinterpret_cast<int*>(take((size_t)N * 4));
    if (e) *e = BoundedExtra{co, st, lo, xc};
    return off;
}
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
    BoundedExtra e;
    carve_bounded(static_cast<char*>(workspace), rnnt_amd_workspace_size_compact(N, STU, Tmax, Umax), N, &e);
    const CompactBounds b{e.xn_checked, STU, n_labels, Tmax, Umax};
    if (launch_compact_offsets(stream, xn, yn, N, e.cell_offsets, e.label_offsets, e.stats, &b) != hipSuccess)
        return RNNT_STATUS_PROLOGUE_FAILED;
    const rnntStatus_t st = compact_core(stream, workspace, in, ys, n_labels, e.xn_checked, yn, e.cell_offsets,
                                         e.label_offsets, costs, grads2, N, STU, Tmax, Umax, V, blank, fastemit_lambda);
    if (st != RNNT_STATUS_SUCCESS) return st;
    if (launch_zero_if_refused(stream, e.stats + 4, grads2, (size_t)STU) != hipSuccess) return RNNT_STATUS_EXPAND_FAILED;
    return RNNT_STATUS_SUCCESS;
}
}  // namespace

// Compact (ragged packed) layout: replaces run_gather_for_compact + run_warp_rnnt_compact
// (core.h:41-54, core_compact.cu:360-436) with the conventions of the rest of this ABI
// (status codes, caller's stream, no exit(), no host synchronisation).
rnntStatus_t rnnt_amd_loss_compact(rnntStream_t stream, void* workspace, const float* xs, const int* ys,
                                   const int* xn, const int* yn, const int64_t* cell_offsets,
                                   const int* label_offsets, float* costs, float* grads2, int64_t* loc,
                                   int N, int64_t STU, int Tmax, int Umax, int V, int blank,
                                   float fastemit_lambda) {
    if (!compact_dims_ok(N, STU, Tmax, Umax) || !workspace_ok(workspace) || !vocab_ok(V, blank))
        return RNNT_STATUS_INVALID_ARGUMENT;
    if (N == 0 || STU == 0) return RNNT_STATUS_SUCCESS;
    return compact_core(stream, workspace, CompactInput{false, RNNT_DTYPE_F32, xs, loc}, ys, -1, xn, yn, cell_offsets,
                        label_offsets, costs, grads2, N, STU, Tmax, Umax, V, blank, fastemit_lambda);
}

size_t rnnt_amd_workspace_size_compact_bounded(int N, int64_t STU, int Tmax, int Umax) {
    const size_t base = rnnt_amd_workspace_size_compact(N, STU, Tmax, Umax);
    if (base == 0) return 0;
    return carve_bounded(nullptr, base, N, nullptr);
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
    if (Umax > 1 && !ys) return RNNT_STATUS_INVALID_ARGUMENT;
    if (N == 0 || STU == 0) return RNNT_STATUS_SUCCESS;
    return compact_core(stream, workspace, CompactInput{true, dtype, logits, nullptr}, ys, -1, xn, yn, cell_offsets,
                        label_offsets, costs, grads2, N, STU, Tmax, Umax, V, blank, fastemit_lambda);
}

rnntStatus_t rnnt_amd_loss_compact_logits_bounded(rnntStream_t stream, void* workspace, int dtype, const void* logits,
                                                  const int* ys, int64_t n_labels, const int* xn, const int* yn,
                                                  float* costs, float* grads2, int N, int64_t STU, int Tmax, int Umax,
                                                  int V, int blank, float fastemit_lambda) {
    if (!dtype_ok(dtype) || !vocab_ok(V, blank) || (n_labels > 0 && !ys)) return RNNT_STATUS_INVALID_ARGUMENT;
    return compact_bounded(stream, workspace, CompactInput{true, dtype, logits, nullptr}, ys, n_labels, xn, yn, costs,
                           grads2, N, STU, Tmax, Umax, V, blank, fastemit_lambda);
}

namespace {
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

// Backward of the fused RNNT_IN_LOGITS_DENSE path: d(sum_n grad_costs[n]*cost[n]) / d(logits).
namespace {
rnntStatus_t logits_backward(rnntStream_t stream, int dtype, const void* logits, const int* labels,
                             const float* grads_diagonal, const float* grad_costs, void* dlogits, int N, int T, int U,
                             int V, int blank, float clamp) {
    if (!dtype_ok(dtype) || !dims_ok(N, T, U) || !vocab_ok(V, blank)) return RNNT_STATUS_INVALID_ARGUMENT;
    if (U > 1 && !labels) return RNNT_STATUS_INVALID_ARGUMENT;
    if (launch_logits_backward(stream, dtype, logits, labels, grads_diagonal, grad_costs, dlogits, N, T, U, V, blank,
                               clamp) != hipSuccess)
        return RNNT_STATUS_EXPAND_FAILED;
    return RNNT_STATUS_SUCCESS;
}
}  // namespace

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

// include/warp_rnnt_amd_hat.h: the factorised-blank (HAT) loss.  joint_loss's shape below: a producer of its own (hat.hip)
// fills the pair plane, the sweeps and the gradient pairs are the standard ones; the backward is one streaming launch.
rnntStatus_t rnnt_amd_hat_loss_logits(rnntStream_t stream, void* workspace, int dtype, const void* logits,
                                      const int* labels, const int* xn, const int* yn, float* costs, float* grads, int N,
                                      int T, int U, int V, int blank, float fastemit_lambda) {
    if (!dtype_ok(dtype) || !dims_ok(N, T, U) || V < 2 || !vocab_ok(V, blank)) return RNNT_STATUS_INVALID_ARGUMENT;
    if (!workspace_ok(workspace) || !logits || !xn || !yn || !costs || (U > 1 && !labels))
        return RNNT_STATUS_INVALID_ARGUMENT;
    if (N == 0) return RNNT_STATUS_SUCCESS;
    Workspace w;
    carve(workspace, N, T, U, &w);
    if (launch_hat_gather_skewed(stream, dtype, logits, labels, w.ws2, N, T, U, V, blank) != hipSuccess)
        return RNNT_STATUS_PROLOGUE_FAILED;
    return sweeps_and_pair_grads(stream, w, xn, yn, costs, grads ? grads : w.ws2, WRITE_SKEWED2, N, T, U, nullptr,
                                 fastemit_lambda);
}

rnntStatus_t rnnt_amd_hat_logits_backward(rnntStream_t stream, int dtype, const void* logits, const int* labels,
                                          const float* grads_diagonal, const float* grad_costs, void* dlogits, int N,
                                          int T, int U, int V, int blank) {
    if (!dtype_ok(dtype) || !dims_ok(N, T, U) || V < 2 || !vocab_ok(V, blank)) return RNNT_STATUS_INVALID_ARGUMENT;
    if (!logits || !grads_diagonal || !aligned(grads_diagonal, 8) || !dlogits || (U > 1 && !labels))
        return RNNT_STATUS_INVALID_ARGUMENT;
    if (N == 0) return RNNT_STATUS_SUCCESS;
    if (launch_hat_logits_backward(stream, dtype, logits, labels, grads_diagonal, grad_costs, dlogits, N, T, U, V, blank) !=
        hipSuccess)
        return RNNT_STATUS_EXPAND_FAILED;
    return RNNT_STATUS_SUCCESS;
}

// include/warp_rnnt_amd_align.h: best-path alignments.  A producer of the loss fills the pair plane -- and leaves it
// filled -- the max-plus sweep and the trace of align.hip take the place of the alpha / beta sweeps.  Workspace:
// rnnt_amd_workspace_size's carve, then the decision words, then the columns parked between column stripes.
namespace {
struct AlignWorkspace {
    unsigned long long* words;
    float* park;
};
size_t carve_align(void* base, int N, int T, int U, AlignWorkspace* aw) {
    size_t off = carve(base, N, T, U, nullptr);
    char* p = static_cast<char*>(base);
    auto take = [&](size_t bytes) { size_t o = off; off += align_up(bytes); return p ? p + o : nullptr; };
    unsigned long long* words = reinterpret_cast<unsigned long long*>(take(align_word_count(N, T, U) * 8));
    float* park = reinterpret_cast<float*>(take(align_park_count(N, T, U) * sizeof(float)));
    if (aw) *aw = AlignWorkspace{words, park};
    return off;
}
}  // namespace

size_t rnnt_amd_align_workspace_size(int N, int T, int U) {
    if (!dims_ok(N, T, U)) return 0;
    return carve_align(nullptr, N, T, U, nullptr);
}

rnntStatus_t rnnt_amd_align(rnntStream_t stream, void* workspace, int input_kind, int dtype, const void* input,
                            const int* labels, const int* xn, const int* yn, float* scores, int* emit_frames, int N, int T,
                            int U, int V, int blank) {
    const bool log_probs = input_kind == RNNT_IN_LOG_PROBS_DENSE || input_kind == RNNT_IN_LOG_PROBS_GATHERED;
    if (!log_probs && input_kind != RNNT_IN_LOGITS_DENSE && input_kind != RNNT_ALIGN_IN_HAT_LOGITS)
        return RNNT_STATUS_INVALID_ARGUMENT;
    if (!dtype_ok(dtype) || (log_probs && dtype != RNNT_DTYPE_F32)) return RNNT_STATUS_INVALID_ARGUMENT;
    if (!dims_ok(N, T, U) || !workspace_ok(workspace)) return RNNT_STATUS_INVALID_ARGUMENT;
    if (!input || !xn || !yn || !scores || (U > 1 && !emit_frames)) return RNNT_STATUS_INVALID_ARGUMENT;
    if (input_kind != RNNT_IN_LOG_PROBS_GATHERED &&
        (!vocab_ok(V, blank) || (input_kind == RNNT_ALIGN_IN_HAT_LOGITS && V < 2) || (U > 1 && !labels)))
        return RNNT_STATUS_INVALID_ARGUMENT;
    if (N == 0) return RNNT_STATUS_SUCCESS;

    Workspace w;
    carve(workspace, N, T, U, &w);
    AlignWorkspace aw;
    carve_align(workspace, N, T, U, &aw);
    hipError_t e;
    switch (input_kind) {
        case RNNT_IN_LOG_PROBS_DENSE:
            e = launch_gather(stream, static_cast<const float*>(input), labels, w.ws2, N, T, U, V, blank, true); break;
        case RNNT_IN_LOG_PROBS_GATHERED:
            e = launch_reskew(stream, static_cast<const float*>(input), w.ws2, N, T, U); break;
        case RNNT_IN_LOGITS_DENSE:
            e = launch_log_softmax_gather_skewed(stream, dtype, input, labels, w.ws2, N, T, U, V, blank); break;
        default:
            e = launch_hat_gather_skewed(stream, dtype, input, labels, w.ws2, N, T, U, V, blank); break;
    }
    if (e != hipSuccess) return RNNT_STATUS_PROLOGUE_FAILED;
    if (launch_align_sweep(stream, w.ws2, xn, yn, aw.words, aw.park, scores, N, T, U) != hipSuccess)
        return RNNT_STATUS_WARP_FAILED;
    if (launch_align_trace(stream, aw.words, xn, yn, scores, emit_frames, N, T, U) != hipSuccess)
        return RNNT_STATUS_WARP_FAILED;
    return RNNT_STATUS_SUCCESS;
}

// The joint network fused into the loss (joint.hip).  Workspace: rnnt_amd_workspace_size's carve, then W^T (H,Vp) for
// the backward, then the weight kernel's fp32 partials (splits x Vp x H and splits x Vp), splits sized for fp32 (the
// most a dtype takes).
namespace {
struct JointWorkspace {
    void* wt;
    float* dw_part;
    float* db_part;
};
size_t carve_joint(void* base, int N, int T, int U, int H, int V, JointWorkspace* jw) {
    size_t off = carve(base, N, T, U, nullptr);
    char* p = static_cast<char*>(base);
    auto take = [&](size_t bytes) { size_t o = off; off += align_up(bytes); return p ? p + o : nullptr; };
    const size_t vp = (size_t)joint_vpad(V), splits = (size_t)joint_w_splits(N, T, U, H, V, RNNT_DTYPE_F32);
    void* wt = take((size_t)H * vp * 4);
    float* dw = reinterpret_cast<float*>(take(splits * vp * H * 4));
    float* db = reinterpret_cast<float*>(take(splits * vp * 4));
    if (jw) *jw = JointWorkspace{wt, dw, db};
    return off;
}
bool joint_args_ok(int dtype, int activation, int N, int T, int U, int H, int V, int blank) {
    return dtype_ok(dtype) && (activation == RNNT_ACT_TANH || activation == RNNT_ACT_RELU) && dims_ok(N, T, U) &&
           H >= 32 && H <= 1024 && H % 32 == 0 && V >= 2 && V <= (1 << 24) && vocab_ok(V, blank);
}
// f, g and the weight are read in 16-byte words, the bias (optional) as floats
inline bool joint_inputs_aligned(const void* f, const void* g, const void* weight, const float* bias) {
    return aligned(f, 16) && aligned(g, 16) && aligned(weight, 16) && aligned(bias, 4);
}
}  // namespace

size_t rnnt_amd_joint_workspace_size(int N, int T, int U, int H, int V) {
    if (!joint_args_ok(RNNT_DTYPE_F32, RNNT_ACT_TANH, N, T, U, H, V, 0)) return 0;
    return carve_joint(nullptr, N, T, U, H, V, nullptr);
}

// p, seed: the dropout of include/warp_rnnt_amd_joint_dropout.h (p == 0: none, seed unread)
namespace {
rnntStatus_t joint_loss(rnntStream_t stream, void* workspace, int dtype, int activation, const void* f, const void* g,
                        const void* weight, const float* bias, const int* labels, const int* xn, const int* yn,
                        float* costs, float* lse, float* grads, int N, int T, int U, int H, int V, int blank,
                        float fastemit_lambda, float p, const uint64_t* seed) {
    if (!joint_args_ok(dtype, activation, N, T, U, H, V, blank)) return RNNT_STATUS_INVALID_ARGUMENT;
    if (!workspace_ok(workspace) || !f || !g || !weight || !xn || !yn || !costs || (U > 1 && !labels) || (grads && !lse))
        return RNNT_STATUS_INVALID_ARGUMENT;
    if (!joint_inputs_aligned(f, g, weight, bias) || !aligned(lse, 8)) return RNNT_STATUS_INVALID_ARGUMENT;
    if (N == 0) return RNNT_STATUS_SUCCESS;
    Workspace w;
    carve(workspace, N, T, U, &w);
    // 1. z tile by tile: the (blank,label) log-prob pairs into the pair plane (launch_log_softmax_gather_skewed's
    //    layout), (max, log sum) per cell
    if (launch_joint_fwd(stream, dtype, activation, f, g, weight, bias, labels, xn, yn, w.ws2, grads ? lse : nullptr, N,
                         T, U, H, V, blank, p, seed) != hipSuccess)
        return RNNT_STATUS_PROLOGUE_FAILED;
    // 2. + 3. as rnnt_amd_loss_logits(RNNT_GRADS_GATHERED_DIAGONAL or RNNT_GRADS_NONE)
    return sweeps_and_pair_grads(stream, w, xn, yn, costs, grads ? grads : w.ws2, WRITE_SKEWED2, N, T, U, nullptr,
                                 fastemit_lambda);
}

rnntStatus_t joint_backward(rnntStream_t stream, void* workspace, int dtype, int activation, const void* f,
                            const void* g, const void* weight, const float* bias, const int* labels, const int* xn,
                            const int* yn, const float* lse, const float* grads, const float* grad_costs, void* df,
                            void* dg, float* dweight, float* dbias, int N, int T, int U, int H, int V, int blank, float p,
                            const uint64_t* seed) {
    if (!joint_args_ok(dtype, activation, N, T, U, H, V, blank)) return RNNT_STATUS_INVALID_ARGUMENT;
    if (!workspace_ok(workspace) || !f || !g || !weight || !xn || !yn || !lse || !grads || (U > 1 && !labels))
        return RNNT_STATUS_INVALID_ARGUMENT;
    if (!joint_inputs_aligned(f, g, weight, bias) || !aligned(grads, 8) || !aligned(lse, 8))
        return RNNT_STATUS_INVALID_ARGUMENT;
    if (N == 0 || (!df && !dg && !dweight && !dbias)) return RNNT_STATUS_SUCCESS;
    JointWorkspace jw;
    carve_joint(workspace, N, T, U, H, V, &jw);
    if (launch_joint_bwd(stream, dtype, activation, f, g, weight, bias, labels, xn, yn, lse, grads, grad_costs, jw.wt,
                         jw.dw_part, jw.db_part, joint_w_splits(N, T, U, H, V, dtype), df, dg, dweight, dbias, N, T, U,
                         H, V, blank, p, seed) != hipSuccess)
        return RNNT_STATUS_EXPAND_FAILED;
    return RNNT_STATUS_SUCCESS;
}

// the dropout of the *_dropout entries: p in [0,1) (false for a NaN); p > 0 needs the device word
inline bool dropout_ok(float p, const uint64_t* seed) {
    return p >= 0.0f && p < 1.0f && (p == 0.0f || (seed && aligned(seed, 8)));
}
}  // namespace

rnntStatus_t rnnt_amd_joint_loss(rnntStream_t stream, void* workspace, int dtype, int activation, const void* f,
                                 const void* g, const void* weight, const float* bias, const int* labels, const int* xn,
                                 const int* yn, float* costs, float* lse, float* grads, int N, int T, int U, int H, int V,
                                 int blank, float fastemit_lambda) {
    return joint_loss(stream, workspace, dtype, activation, f, g, weight, bias, labels, xn, yn, costs, lse, grads, N, T, U,
                      H, V, blank, fastemit_lambda, 0.0f, nullptr);
}

rnntStatus_t rnnt_amd_joint_backward(rnntStream_t stream, void* workspace, int dtype, int activation, const void* f,
                                     const void* g, const void* weight, const float* bias, const int* labels,
                                     const int* xn, const int* yn, const float* lse, const float* grads,
                                     const float* grad_costs, void* df, void* dg, float* dweight, float* dbias, int N,
                                     int T, int U, int H, int V, int blank) {
    return joint_backward(stream, workspace, dtype, activation, f, g, weight, bias, labels, xn, yn, lse, grads, grad_costs,
                          df, dg, dweight, dbias, N, T, U, H, V, blank, 0.0f, nullptr);
}

// include/warp_rnnt_amd_joint_dropout.h: the same with dropout between the activation and the projection.  p == 0 IS the
// entry above (seed unread).
rnntStatus_t rnnt_amd_joint_loss_dropout(rnntStream_t stream, void* workspace, int dtype, int activation, const void* f,
                                         const void* g, const void* weight, const float* bias, const int* labels,
                                         const int* xn, const int* yn, float* costs, float* lse, float* grads, int N,
                                         int T, int U, int H, int V, int blank, float fastemit_lambda, float p,
                                         const uint64_t* seed) {
    if (!dropout_ok(p, seed)) return RNNT_STATUS_INVALID_ARGUMENT;
    return joint_loss(stream, workspace, dtype, activation, f, g, weight, bias, labels, xn, yn, costs, lse, grads, N, T, U,
                      H, V, blank, fastemit_lambda, p, p > 0.0f ? seed : nullptr);
}

rnntStatus_t rnnt_amd_joint_backward_dropout(rnntStream_t stream, void* workspace, int dtype, int activation,
                                             const void* f, const void* g, const void* weight, const float* bias,
                                             const int* labels, const int* xn, const int* yn, const float* lse,
                                             const float* grads, const float* grad_costs, void* df, void* dg,
                                             float* dweight, float* dbias, int N, int T, int U, int H, int V, int blank,
                                             float p, const uint64_t* seed) {
    if (!dropout_ok(p, seed)) return RNNT_STATUS_INVALID_ARGUMENT;
    return joint_backward(stream, workspace, dtype, activation, f, g, weight, bias, labels, xn, yn, lse, grads, grad_costs,
                          df, dg, dweight, dbias, N, T, U, H, V, blank, p, p > 0.0f ? seed : nullptr);
}

// The keep mask of those entries on the host (philox.h is one definition for both sides): no HIP call.
rnntStatus_t rnnt_amd_joint_dropout_mask_host(uint64_t seed, float p, int N, int T, int U, int H, unsigned char* keep) {
    if (!(p >= 0.0f && p < 1.0f) || N < 0 || T < 0 || U < 0 || H < 0 || !keep) return RNNT_STATUS_INVALID_ARGUMENT;
    const uint32_t thr = dropout_threshold(p);
    for (int n = 0; n < N; ++n)
        for (int t = 0; t < T; ++t)
            for (int u = 0; u < U; ++u) {
                unsigned char* row = keep + (((size_t)n * T + t) * U + u) * H;
                for (int k = 0; k < H; k += 4) {
                    const Philox4 r = dropout_words(seed, n, t, u, k >> 2);
                    for (int j = 0; j < 4 && k + j < H; ++j) row[k + j] = r.w[j] < thr;
                }
            }
    return RNNT_STATUS_SUCCESS;
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
