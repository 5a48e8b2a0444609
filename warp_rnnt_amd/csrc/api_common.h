// What the entry families of the C ABI share (api_loss.hip, api_compact.hip, api_reference.hip, api_fused.hip): argument
// predicates, the workspace carver and the loss layout, the two steps every loss is made of.  Host code only: no unit that
// holds a kernel includes this.
#pragma once
#include "../../include/warp_rnnt_amd.h"

#include "common.h"
#include "kernels.h"

#pragma GCC visibility push(hidden)     // the library's own: nothing of this in its dynamic symbol table
namespace rnnt {

constexpr size_t ALIGN = 256;
// Lattices from this many cells on take the multi-pass forms (stage, sweep on the tuned kernels, turn the layout
// through LDS tiles); smaller ones are launch-bound and keep the single-kernel forms (tools/cabi_probe.py: N=16, T=150,
// U=40: 24 us in two launches against 35 in five; N=16, T=1500, U=300: 500 against 274)
constexpr size_t STAGED_FROM_CELLS = (size_t)1 << 20;
inline size_t align_up(size_t x) { return (x + ALIGN - 1) / ALIGN * ALIGN; }

inline bool dims_ok(int N, int T, int U) {
    if (N < 0 || T < 1 || U < 1) return false;
    if (N > 65535) return false;                               // gridDim.y of the gradient kernel
    if ((int64_t)T * U >= (int64_t)1 << 29) return false;      // per-utterance plane < 4 GiB of float2 (buffer descriptors)
    if ((int64_t)N * T * U >= (int64_t)1 << 32) return false;  // flat cell index is 32-bit
    return true;
}
inline bool compact_dims_ok(int N, int64_t STU, int Tmax, int Umax) {
    return dims_ok(N, Tmax > 0 ? Tmax : 1, Umax > 0 ? Umax : 1) && STU >= 0 && STU < ((int64_t)1 << 32);
}
inline bool vocab_ok(int V, int blank) { return V >= 1 && blank >= 0 && blank < V; }
// the labels of a lattice with more than its blank column (U: the padded width, or the compact layout's bound)
inline bool labels_missing(int U, const int* labels) { return U > 1 && !labels; }
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

// Walks a workspace piece by piece, every piece on a multiple of ALIGN.  A null base only counts -- the size entries --
// and hands out null pointers.  A layout is a function of a carver and the shape; an entry that needs two of them runs
// one behind the other on the same carver.
struct Carver {
    char* base;
    size_t off = 0;
    explicit Carver(void* workspace) : base(static_cast<char*>(workspace)) {}
    template <typename T>
    T* take(size_t count) {
        const size_t o = off;
        off += align_up(count * sizeof(T));
        return base ? reinterpret_cast<T*>(base + o) : nullptr;
    }
};

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
// (the compact form: its launch bounds).
inline Workspace loss_layout(Carver& c, size_t cells, int N, int T, int U) {
    Workspace w;
    w.alphas = c.take<float>(cells);
    w.betas = c.take<float>(cells);
    w.ws2 = c.take<float>(cells * 2);
    w.ll = c.take<float>((size_t)N);
    w.mismatch = c.take<int>((size_t)N);
    w.redo = c.take<int>((size_t)N * 2 + 2);   // flags, queue head, launch counter
    // (reserved by SHAPE, never by the current route: the size of a workspace must not depend on a setting)
    w.mail = reinterpret_cast<unsigned long long*>(c.take<char>(wd_mail_bytes(N, T, U)));
    return w;
}
inline Workspace loss_layout(Carver& c, int N, int T, int U) { return loss_layout(c, (size_t)N * T * U, N, T, U); }

inline LatticeArgs sweep_args(const Workspace& w, const int* xn, const int* yn, int N, int T, int U, const int64_t* offs) {
    return LatticeArgs{w.ws2, nullptr, xn, yn, w.alphas, w.betas, w.ll, T, U, 2, 0, offs, w.redo, w.redo + 2 * N, w.mail};
}

// Step 1 of a loss call on padded planes (api_loss.hip): the (blank,label) log-prob pairs of `input` into the
// diagonal-major plane ws2.  kind: RNNT_IN_LOG_PROBS_DENSE (blank_plane: the blank column as a plane of its own, or
// nullptr), RNNT_IN_LOG_PROBS_GATHERED, RNNT_IN_LOGITS_DENSE or RNNT_ALIGN_IN_HAT_LOGITS (dtype: the logits'; the
// log-prob kinds are fp32); another kind is hipErrorInvalidValue.  la: the sweeps that will run on the plane -- the two
// log-prob producers then carry the ring kernel's preparation (kernels.h: RingPrep) and la->prepared says so -- or
// nullptr where none will.
struct PairSource {
    int kind;
    int dtype;
    const void* input;
    const float* blank_plane;
};
hipError_t fill_pair_plane(hipStream_t stream, const PairSource& src, const int* labels, float* ws2, int N, int T, int U,
                           int V, int blank, LatticeArgs* la);

// Steps 2 and 3 of a loss call on a carved workspace whose pair plane is filled (api_loss.hip): the alpha / beta sweeps
// of shape (T, U), then costs, guard and the gradient pairs, written by `writer` into gout (nullptr: the sweeps only).
// offs: the compact layout's cell offsets, nullptr for padded planes; prepared: LatticeArgs::prepared (the producer of
// the pairs carried the ring kernel's RingPrep).
rnntStatus_t sweeps_and_pair_grads(rnntStream_t stream, const Workspace& w, const int* xn, const int* yn, float* costs,
                                   float* gout, int writer, int N, int T, int U, const int64_t* offs,
                                   float fastemit_lambda, int prepared = 0);

}  // namespace rnnt
#pragma GCC visibility pop
