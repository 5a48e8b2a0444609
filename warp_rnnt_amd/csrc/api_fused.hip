// C ABI of libwarp_rnnt_amd.so, the fused family: a producer of its own in front of the loss's sweeps -- or a sweep of its
// own behind one of the loss's producers.  The joint network (include/warp_rnnt_amd.h) and its dropout
// (include/warp_rnnt_amd_joint_dropout.h), the factorised-blank loss (include/warp_rnnt_amd_hat.h), the pruned loss over a
// band of the lattice (include/warp_rnnt_amd_pruned.h), the smoothed first pass of its recipe over the trivial joiner
// (include/warp_rnnt_amd_simple.h), the modified topology and the delay penalty of the two
// (include/warp_rnnt_amd_topology.h), best-path alignments
// (include/warp_rnnt_amd_align.h), the token-and-duration loss (include/warp_rnnt_amd_tdt.h: producer, sweeps and
// gradient kernel all its own), its best-path alignments (include/warp_rnnt_amd_tdt_align.h) and the joint network fused
// into it (include/warp_rnnt_amd_tdt_joint.h), the multi-blank loss (include/warp_rnnt_amd_multiblank.h: producer, sweeps
// and gradient kernel all its own).  Host-side orchestration only: argument checks, workspace carving, launches.
#include "../../include/warp_rnnt_amd_align.h"
#include "../../include/warp_rnnt_amd_hat.h"
#include "../../include/warp_rnnt_amd_joint_dropout.h"
#include "../../include/warp_rnnt_amd_multiblank.h"
#include "../../include/warp_rnnt_amd_pruned.h"
#include "../../include/warp_rnnt_amd_simple.h"
#include "../../include/warp_rnnt_amd_tdt.h"
#include "../../include/warp_rnnt_amd_tdt_align.h"
#include "../../include/warp_rnnt_amd_tdt_joint.h"
#include "../../include/warp_rnnt_amd_topology.h"

#include "align.h"
#include "api_common.h"
#include "hat.h"
#include "multiblank.h"
#include "philox.h"
#include "pruned.h"
#include "simple.h"
#include "tdt.h"
#include "tdt_align.h"
#include "tdt_joint.h"

using namespace rnnt;

namespace {

// The joint network fused into the loss (joint.hip).  Behind the loss layout: W^T (H,Vp) for the backward, then the
// weight kernel's fp32 partials (splits x Vp x H and splits x Vp), splits sized for fp32 (the most a dtype takes).
struct JointWorkspace {
    void* wt;
    float* dw_part;
    float* db_part;
};
JointWorkspace joint_layout(Carver& c, int N, int T, int U, int H, int V) {
    const size_t vp = (size_t)joint_vpad(V), splits = (size_t)joint_w_splits(N, T, U, H, V, RNNT_DTYPE_F32);
    JointWorkspace jw;
    jw.wt = c.take<float>((size_t)H * vp);
    jw.dw_part = c.take<float>(splits * vp * H);
    jw.db_part = c.take<float>(splits * vp);
    return jw;
}
bool joint_args_ok(int dtype, int activation, int N, int T, int U, int H, int V, int blank) {
    return dtype_ok(dtype) && (activation == RNNT_ACT_TANH || activation == RNNT_ACT_RELU) && dims_ok(N, T, U) &&
           H >= 32 && H <= 1024 && H % 32 == 0 && V >= 2 && V <= (1 << 24) && vocab_ok(V, blank);
}
// f, g and the weight are read in 16-byte words, the bias (optional) as floats
inline bool joint_inputs_aligned(const void* f, const void* g, const void* weight, const float* bias) {
    return aligned(f, 16) && aligned(g, 16) && aligned(weight, 16) && aligned(bias, 4);
}

// p, seed: the dropout of include/warp_rnnt_amd_joint_dropout.h (p == 0: none, seed unread)
rnntStatus_t joint_loss(rnntStream_t stream, void* workspace, int dtype, int activation, const void* f, const void* g,
                        const void* weight, const float* bias, const int* labels, const int* xn, const int* yn,
                        float* costs, float* lse, float* grads, int N, int T, int U, int H, int V, int blank,
                        float fastemit_lambda, float p, const uint64_t* seed) {
    if (!joint_args_ok(dtype, activation, N, T, U, H, V, blank)) return RNNT_STATUS_INVALID_ARGUMENT;
    if (!workspace_ok(workspace) || !f || !g || !weight || !xn || !yn || !costs || labels_missing(U, labels) ||
        (grads && !lse))
        return RNNT_STATUS_INVALID_ARGUMENT;
    if (!joint_inputs_aligned(f, g, weight, bias) || !aligned(lse, 8)) return RNNT_STATUS_INVALID_ARGUMENT;
    if (N == 0) return RNNT_STATUS_SUCCESS;
    Carver c(workspace);
    const Workspace w = loss_layout(c, N, T, U);
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
    if (!workspace_ok(workspace) || !f || !g || !weight || !xn || !yn || !lse || !grads || labels_missing(U, labels))
        return RNNT_STATUS_INVALID_ARGUMENT;
    if (!joint_inputs_aligned(f, g, weight, bias) || !aligned(grads, 8) || !aligned(lse, 8))
        return RNNT_STATUS_INVALID_ARGUMENT;
    if (N == 0 || (!df && !dg && !dweight && !dbias)) return RNNT_STATUS_SUCCESS;
    Carver c(workspace);
    loss_layout(c, N, T, U);
    const JointWorkspace jw = joint_layout(c, N, T, U, H, V);
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

// the band of a pruned call (pruned.hip): S label positions per frame, at most the lattice's U; rows of (N,T,S) numbered
// in 32 bits
inline bool pruned_band_ok(int N, int T, int U, int S) {
    return S >= 1 && S <= U && (int64_t)N * T * S < (int64_t)1 << 32;
}

// The simple loss (simple.hip).  Behind the loss layout: the row statistics of am and lm, then the backward's row sums
// (simple.h: SimpleStats).
SimpleStats simple_layout(Carver& c, int N, int T, int U) {
    SimpleStats st;
    st.sa = c.take<float>((size_t)N * T * 4);
    st.sl = c.take<float>((size_t)N * U * 4);
    st.ra = c.take<float>((size_t)N * T * 2);
    st.rl = c.take<float>((size_t)N * U * 4);
    return st;
}
inline bool simple_shape_ok(int dtype, int N, int T, int U, int V, int blank) {
    return dtype_ok(dtype) && dims_ok(N, T, U) && T <= SIMPLE_MAX_ROWS && U <= SIMPLE_MAX_ROWS && V >= 2 &&
           V <= (1 << 24) && vocab_ok(V, blank);
}
// the two smoothing scales: finite, not negative, their fp32 sum at most 1 (false for a NaN); am_only_scale needs q
inline bool simple_scales_ok(float lm_only_scale, float am_only_scale, const float* q) {
    return lm_only_scale >= 0.0f && am_only_scale >= 0.0f && lm_only_scale + am_only_scale <= 1.0f &&
           (am_only_scale == 0.0f || q);
}

// The topology and the delay penalty of the pruned and the simple entries (include/warp_rnnt_amd_topology.h).  The modified
// lattice is the regular one over the sheared cells (t - u, u): its plane has T + 1 rows and is frame-major, and the sweeps
// take T_n - U_n + 1 for the frames of utterance n -- N ints behind the loss layout (pruned.h: launch_modified_terminal).
inline bool topology_ok(int topology, float delay_penalty) {
    return (topology == RNNT_TOPOLOGY_REGULAR || topology == RNNT_TOPOLOGY_MODIFIED) && delay_penalty >= 0.0f &&
           delay_penalty <= 3.402823466e+38f;                                                     // (false for a NaN)
}
// the rows of the lattice's planes
inline int plane_frames(int topology, int T) { return topology == RNNT_TOPOLOGY_MODIFIED ? T + 1 : T; }
inline bool topology_dims_ok(int topology, int N, int T, int U) {
    return dims_ok(N, T, U) && (topology != RNNT_TOPOLOGY_MODIFIED || dims_ok(N, T + 1, U));
}
struct TopologyWorkspace {
    Workspace w;
    int* xs;         // modified: the sheared lattice's frame counts; regular: nullptr
};
TopologyWorkspace topology_layout(Carver& c, int topology, int N, int T, int U) {
    TopologyWorkspace tw;
    tw.w = loss_layout(c, N, plane_frames(topology, T), U);
    tw.xs = topology == RNNT_TOPOLOGY_MODIFIED ? c.take<int>((size_t)N) : nullptr;
    return tw;
}
// Steps 2 and 3 of a loss call on a plane a producer of either topology filled.  clear_terminal: the pairs go to a reader
// that walks them by frames and masks nothing (pruned.h: launch_modified_clear_terminal).
rnntStatus_t topology_sweeps(rnntStream_t stream, const TopologyWorkspace& tw, int topology, const int* xn, const int* yn,
                             float* costs, float* gout, int writer, bool clear_terminal, int N, int T, int U,
                             float fastemit_lambda) {
    if (topology != RNNT_TOPOLOGY_MODIFIED)
        return sweeps_and_pair_grads(stream, tw.w, xn, yn, costs, gout, writer, N, T, U, nullptr, fastemit_lambda);
    if (launch_modified_terminal(stream, xn, yn, tw.xs, tw.w.ws2, N, T, U) != hipSuccess) return RNNT_STATUS_PROLOGUE_FAILED;
    const rnntStatus_t st = sweeps_and_pair_grads(stream, tw.w, tw.xs, yn, costs, gout, WRITE_SKEWED2, N, T + 1, U, nullptr,
                                                  fastemit_lambda);
    if (st != RNNT_STATUS_SUCCESS) return st;
    if (clear_terminal && launch_modified_clear_terminal(stream, xn, yn, gout, N, T, U) != hipSuccess)
        return RNNT_STATUS_GRADS_BLANK_FAILED;
    return RNNT_STATUS_SUCCESS;
}

// Best-path alignments.  Behind the loss layout: the decision words, then the columns parked between column stripes.
struct AlignWorkspace {
    unsigned long long* words;
    float* park;
};
AlignWorkspace align_layout(Carver& c, int N, int T, int U) {
    AlignWorkspace aw;
    aw.words = c.take<unsigned long long>(align_word_count(N, T, U));
    aw.park = c.take<float>(align_park_count(N, T, U));
    return aw;
}

// The token-and-duration loss (tdt.hip): the plane of 2 + D channels, alpha, beta, the log-likelihoods.
struct TdtWorkspace {
    float* plane;
    float* alphas;
    float* betas;
    float* ll;
};
TdtWorkspace tdt_layout(Carver& c, int N, int T, int U, int D) {
    const size_t cells = (size_t)N * T * U;
    TdtWorkspace tw;
    tw.plane = c.take<float>(cells * (size_t)(2 + D));
    tw.alphas = c.take<float>(cells);
    tw.betas = c.take<float>(cells);
    tw.ll = c.take<float>((size_t)N);
    return tw;
}
// the shape of a TDT call: the loss's sizes, a lattice that fits one workgroup, D durations and V tokens with the blank
inline bool tdt_shape_ok(int dtype, int N, int T, int U, int V, int D, int blank) {
    return dtype_ok(dtype) && dims_ok(N, T, U) && U <= TDT_MAX_U && D >= 1 && D <= TDT_MAX_D && V >= 2 && V <= (1 << 24) &&
           vocab_ok(V, blank);
}
inline size_t dtype_size(int dtype) { return dtype == RNNT_DTYPE_F32 ? 4 : 2; }

// Best-path alignments over the TDT lattice (tdt_align.hip): the plane where and as tdt_layout has it, then the decision
// bytes.
struct TdtAlignWorkspace {
    float* plane;
    unsigned char* dec;
};
TdtAlignWorkspace tdt_align_layout(Carver& c, int N, int T, int U, int D) {
    TdtAlignWorkspace aw;
    aw.plane = c.take<float>((size_t)N * T * U * (size_t)(2 + D));
    aw.dec = c.take<unsigned char>(tdt_align_dec_count(N, T, U));
    return aw;
}

// The joint network fused into the TDT loss (tdt_joint.hip).  Behind the TDT layout: W^T (H,Vp) and the weight kernel's fp32
// partials for a weight of V + D rows, as joint_layout has them, in less room: split 0 of d weight goes straight into
// dweight, so there are splits - 1 partials, and W^T -- read by the two kernels in front of the weight kernel, dead when it
// starts -- shares their storage (the larger of the two is reserved).
JointWorkspace tdt_joint_layout(Carver& c, int N, int T, int U, int H, int W) {
    const size_t vp = (size_t)joint_vpad(W), splits = (size_t)joint_w_splits(N, T, U, H, W, RNNT_DTYPE_F32);
    const size_t wt = (size_t)H * vp, parts = (splits - 1) * vp * H;
    JointWorkspace jw;
    jw.dw_part = c.take<float>(wt > parts ? wt : parts);
    jw.wt = jw.dw_part;
    jw.db_part = c.take<float>(splits * vp);
    return jw;
}
inline bool tdt_joint_args_ok(int dtype, int activation, int N, int T, int U, int H, int V, int D, int blank) {
    return tdt_shape_ok(dtype, N, T, U, V, D, blank) && joint_args_ok(dtype, activation, N, T, U, H, V + D, blank);
}

// The multi-blank loss (multiblank.hip): the plane of 1 + B channels, alpha, beta, the log-likelihoods.
struct MbWorkspace {
    float* plane;
    float* alphas;
    float* betas;
    float* ll;
};
MbWorkspace mb_layout(Carver& c, int N, int T, int U, int B) {
    const size_t cells = (size_t)N * T * U;
    MbWorkspace mw;
    mw.plane = c.take<float>(cells * (size_t)(1 + B));
    mw.alphas = c.take<float>(cells);
    mw.betas = c.take<float>(cells);
    mw.ll = c.take<float>((size_t)N);
    return mw;
}
// the shape of a multi-blank call: the loss's sizes, a lattice that fits one workgroup, B blanks and a label beside them
inline bool mb_shape_ok(int dtype, int N, int T, int U, int V, int B) {
    return dtype_ok(dtype) && dims_ok(N, T, U) && U <= MB_MAX_U && B >= 1 && B <= MB_MAX_B && V >= B + 1 && V <= (1 << 24);
}

}  // namespace

extern "C" {

size_t rnnt_amd_joint_workspace_size(int N, int T, int U, int H, int V) {
    if (!joint_args_ok(RNNT_DTYPE_F32, RNNT_ACT_TANH, N, T, U, H, V, 0)) return 0;
    Carver c(nullptr);
    loss_layout(c, N, T, U);
    joint_layout(c, N, T, U, H, V);
    return c.off;
}

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

// include/warp_rnnt_amd_hat.h: the factorised-blank (HAT) loss.  joint_loss's shape above: a producer of its own (hat.hip)
// fills the pair plane, the sweeps and the gradient pairs are the standard ones; the backward is one streaming launch.
rnntStatus_t rnnt_amd_hat_loss_logits(rnntStream_t stream, void* workspace, int dtype, const void* logits,
                                      const int* labels, const int* xn, const int* yn, float* costs, float* grads, int N,
                                      int T, int U, int V, int blank, float fastemit_lambda) {
    if (!dtype_ok(dtype) || !dims_ok(N, T, U) || V < 2 || !vocab_ok(V, blank)) return RNNT_STATUS_INVALID_ARGUMENT;
    if (!workspace_ok(workspace) || !logits || !xn || !yn || !costs || labels_missing(U, labels))
        return RNNT_STATUS_INVALID_ARGUMENT;
    if (N == 0) return RNNT_STATUS_SUCCESS;
    Carver c(workspace);
    const Workspace w = loss_layout(c, N, T, U);
    const PairSource src{RNNT_ALIGN_IN_HAT_LOGITS, dtype, logits, nullptr};
    if (fill_pair_plane(stream, src, labels, w.ws2, N, T, U, V, blank, nullptr) != hipSuccess)
        return RNNT_STATUS_PROLOGUE_FAILED;
    return sweeps_and_pair_grads(stream, w, xn, yn, costs, grads ? grads : w.ws2, WRITE_SKEWED2, N, T, U, nullptr,
                                 fastemit_lambda);
}

rnntStatus_t rnnt_amd_hat_logits_backward(rnntStream_t stream, int dtype, const void* logits, const int* labels,
                                          const float* grads_diagonal, const float* grad_costs, void* dlogits, int N,
                                          int T, int U, int V, int blank) {
    if (!dtype_ok(dtype) || !dims_ok(N, T, U) || V < 2 || !vocab_ok(V, blank)) return RNNT_STATUS_INVALID_ARGUMENT;
    if (!logits || !grads_diagonal || !aligned(grads_diagonal, 8) || !dlogits || labels_missing(U, labels))
        return RNNT_STATUS_INVALID_ARGUMENT;
    if (N == 0) return RNNT_STATUS_SUCCESS;
    if (launch_hat_logits_backward(stream, dtype, logits, labels, grads_diagonal, grad_costs, dlogits, N, T, U, V, blank) !=
        hipSuccess)
        return RNNT_STATUS_EXPAND_FAILED;
    return RNNT_STATUS_SUCCESS;
}

// include/warp_rnnt_amd_pruned.h: the pruned transducer loss.  The HAT entry's shape: a producer of its own (pruned.hip)
// fills the pair plane -- the floor everywhere, the band's pairs over it -- the sweeps and the gradient pairs are the
// standard ones over the (N,T,U) grid; the backward is one streaming launch over the (N,T,S,V) logits.
// include/warp_rnnt_amd_topology.h: the same with a topology and a delay penalty.  RNNT_TOPOLOGY_REGULAR with
// delay_penalty == 0 IS the entry without them.
rnntStatus_t rnnt_amd_pruned_loss_logits_topology(rnntStream_t stream, void* workspace, int dtype, const void* logits,
                                                  const int* labels, const int* starts, const int* xn, const int* yn,
                                                  float* costs, float* grads, int N, int T, int U, int S, int V, int blank,
                                                  float fastemit_lambda, int topology, float delay_penalty) {
    if (!topology_ok(topology, delay_penalty) || !dtype_ok(dtype) || !topology_dims_ok(topology, N, T, U) || V < 2 ||
        !vocab_ok(V, blank) || !pruned_band_ok(N, T, U, S))
        return RNNT_STATUS_INVALID_ARGUMENT;
    if (!workspace_ok(workspace) || !logits || !starts || !xn || !yn || !costs || labels_missing(U, labels))
        return RNNT_STATUS_INVALID_ARGUMENT;
    if (N == 0) return RNNT_STATUS_SUCCESS;
    Carver c(workspace);
    const TopologyWorkspace tw = topology_layout(c, topology, N, T, U);
    if (launch_pruned_pairs(stream, dtype, logits, labels, starts, xn, yn, tw.w.ws2, N, T, U, S, V, blank, topology,
                            delay_penalty) != hipSuccess)
        return RNNT_STATUS_PROLOGUE_FAILED;
    return topology_sweeps(stream, tw, topology, xn, yn, costs, grads ? grads : tw.w.ws2, WRITE_SKEWED2, false, N, T, U,
                           fastemit_lambda);
}

rnntStatus_t rnnt_amd_pruned_loss_logits(rnntStream_t stream, void* workspace, int dtype, const void* logits,
                                         const int* labels, const int* starts, const int* xn, const int* yn, float* costs,
                                         float* grads, int N, int T, int U, int S, int V, int blank,
                                         float fastemit_lambda) {
    return rnnt_amd_pruned_loss_logits_topology(stream, workspace, dtype, logits, labels, starts, xn, yn, costs, grads, N, T,
                                                U, S, V, blank, fastemit_lambda, RNNT_TOPOLOGY_REGULAR, 0.0f);
}

rnntStatus_t rnnt_amd_pruned_logits_backward_topology(rnntStream_t stream, int dtype, const void* logits,
                                                      const int* labels, const int* starts, const int* xn, const int* yn,
                                                      const float* grads_diagonal, const float* grad_costs, void* dlogits,
                                                      int N, int T, int U, int S, int V, int blank, int topology) {
    if (!topology_ok(topology, 0.0f) || !dtype_ok(dtype) || !topology_dims_ok(topology, N, T, U) || V < 2 ||
        !vocab_ok(V, blank) || !pruned_band_ok(N, T, U, S))
        return RNNT_STATUS_INVALID_ARGUMENT;
    if (!logits || !starts || !grads_diagonal || !aligned(grads_diagonal, 8) || !dlogits || labels_missing(U, labels) ||
        (topology == RNNT_TOPOLOGY_MODIFIED && (!xn || !yn)))
        return RNNT_STATUS_INVALID_ARGUMENT;
    if (N == 0) return RNNT_STATUS_SUCCESS;
    if (launch_pruned_logits_backward(stream, dtype, logits, labels, starts, xn, yn, grads_diagonal, grad_costs, dlogits, N,
                                      T, U, S, V, blank, topology) != hipSuccess)
        return RNNT_STATUS_EXPAND_FAILED;
    return RNNT_STATUS_SUCCESS;
}

rnntStatus_t rnnt_amd_pruned_logits_backward(rnntStream_t stream, int dtype, const void* logits, const int* labels,
                                             const int* starts, const float* grads_diagonal, const float* grad_costs,
                                             void* dlogits, int N, int T, int U, int S, int V, int blank) {
    return rnnt_amd_pruned_logits_backward_topology(stream, dtype, logits, labels, starts, nullptr, nullptr, grads_diagonal,
                                                    grad_costs, dlogits, N, T, U, S, V, blank, RNNT_TOPOLOGY_REGULAR);
}

size_t rnnt_amd_pruned_topology_workspace_size(int topology, int N, int T, int U) {
    if (!topology_ok(topology, 0.0f) || !topology_dims_ok(topology, N, T, U)) return 0;
    Carver c(nullptr);
    topology_layout(c, topology, N, T, U);
    return c.off;
}

// include/warp_rnnt_amd_simple.h: the smoothed first pass of the pruned recipe.  The HAT entry's shape with a GEMM in the
// producer (simple.hip): it fills the pair plane and the normaliser plane, the sweeps and the gradient pairs are the
// standard ones, the pairs written row-major for the caller; the backward is the statistics, the row sums and two GEMMs.
// include/warp_rnnt_amd_topology.h: the same with a topology and a delay penalty; RNNT_TOPOLOGY_REGULAR with
// delay_penalty == 0 IS the entry without them.  The modified pairs stay frame-major, (N,T+1,U,2), as the gradient kernel
// writes them in place of the row-major turn, and the backward reads them with a row pitch of T + 1: no copy.
size_t rnnt_amd_simple_topology_workspace_size(int topology, int N, int T, int U) {
    if (!topology_ok(topology, 0.0f) || !topology_dims_ok(topology, N, T, U) || T > SIMPLE_MAX_ROWS || U > SIMPLE_MAX_ROWS)
        return 0;
    Carver c(nullptr);
    topology_layout(c, topology, N, T, U);
    simple_layout(c, N, T, U);
    return c.off;
}

size_t rnnt_amd_simple_workspace_size(int N, int T, int U) {
    return rnnt_amd_simple_topology_workspace_size(RNNT_TOPOLOGY_REGULAR, N, T, U);
}

rnntStatus_t rnnt_amd_simple_loss_topology(rnntStream_t stream, void* workspace, int dtype, const void* am, const void* lm,
                                           const float* q, const int* labels, const int* xn, const int* yn, float* costs,
                                           float* pair_grads, float* znorm, int N, int T, int U, int V, int blank,
                                           float lm_only_scale, float am_only_scale, float fastemit_lambda, int topology,
                                           float delay_penalty) {
    if (!topology_ok(topology, delay_penalty) || !topology_dims_ok(topology, N, T, U) ||
        !simple_shape_ok(dtype, N, T, U, V, blank) || !simple_scales_ok(lm_only_scale, am_only_scale, q))
        return RNNT_STATUS_INVALID_ARGUMENT;
    if (!workspace_ok(workspace) || !am || !lm || !xn || !yn || !costs || labels_missing(U, labels) ||
        (pair_grads && !znorm))
        return RNNT_STATUS_INVALID_ARGUMENT;
    if (!aligned(am, dtype_size(dtype)) || !aligned(lm, dtype_size(dtype)) || !aligned(q, 4) || !aligned(labels, 4) ||
        !aligned(xn, 4) || !aligned(yn, 4) || !aligned(costs, 4) || !aligned(pair_grads, 8) || !aligned(znorm, 4))
        return RNNT_STATUS_INVALID_ARGUMENT;
    if (N == 0) return RNNT_STATUS_SUCCESS;
    Carver c(workspace);
    const TopologyWorkspace tw = topology_layout(c, topology, N, T, U);
    const SimpleStats st = simple_layout(c, N, T, U);
    if (launch_simple_pairs(stream, dtype, am, lm, am_only_scale != 0.0f ? q : nullptr, labels, xn, yn, st, tw.w.ws2, znorm,
                            N, T, U, V, blank, simple_scales(lm_only_scale, am_only_scale), topology,
                            delay_penalty) != hipSuccess)
        return RNNT_STATUS_PROLOGUE_FAILED;
    return topology_sweeps(stream, tw, topology, xn, yn, costs, pair_grads ? pair_grads : tw.w.ws2,
                           pair_grads ? WRITE_ROWMAJOR2 : WRITE_SKEWED2, pair_grads != nullptr, N, T, U, fastemit_lambda);
}

rnntStatus_t rnnt_amd_simple_loss(rnntStream_t stream, void* workspace, int dtype, const void* am, const void* lm,
                                  const float* q, const int* labels, const int* xn, const int* yn, float* costs,
                                  float* pair_grads, float* znorm, int N, int T, int U, int V, int blank,
                                  float lm_only_scale, float am_only_scale, float fastemit_lambda) {
    return rnnt_amd_simple_loss_topology(stream, workspace, dtype, am, lm, q, labels, xn, yn, costs, pair_grads, znorm, N, T,
                                         U, V, blank, lm_only_scale, am_only_scale, fastemit_lambda, RNNT_TOPOLOGY_REGULAR,
                                         0.0f);
}

rnntStatus_t rnnt_amd_simple_backward_topology(rnntStream_t stream, void* workspace, int dtype, const void* am,
                                               const void* lm, const float* q, const int* labels, const int* xn,
                                               const int* yn, const float* pair_grads, const float* znorm,
                                               const float* grad_costs, void* dam, void* dlm, float* dq_partials, int N,
                                               int T, int U, int V, int blank, float lm_only_scale, float am_only_scale,
                                               int topology) {
    if (!topology_ok(topology, 0.0f) || !topology_dims_ok(topology, N, T, U) ||
        !simple_shape_ok(dtype, N, T, U, V, blank) || !simple_scales_ok(lm_only_scale, am_only_scale, q))
        return RNNT_STATUS_INVALID_ARGUMENT;
    if (!workspace_ok(workspace) || !am || !lm || !xn || !yn || !pair_grads || !znorm || !dam || !dlm ||
        labels_missing(U, labels))
        return RNNT_STATUS_INVALID_ARGUMENT;
    if (!aligned(am, dtype_size(dtype)) || !aligned(lm, dtype_size(dtype)) || !aligned(dam, dtype_size(dtype)) ||
        !aligned(dlm, dtype_size(dtype)) || !aligned(q, 4) || !aligned(labels, 4) || !aligned(xn, 4) || !aligned(yn, 4) ||
        !aligned(pair_grads, 8) || !aligned(znorm, 4) || !aligned(grad_costs, 4) || !aligned(dq_partials, 4))
        return RNNT_STATUS_INVALID_ARGUMENT;
    if (N == 0) return RNNT_STATUS_SUCCESS;
    Carver c(workspace);
    topology_layout(c, topology, N, T, U);
    const SimpleStats st = simple_layout(c, N, T, U);
    if (launch_simple_backward(stream, dtype, am, lm, am_only_scale != 0.0f ? q : nullptr, labels, xn, yn, pair_grads,
                               znorm, grad_costs, st, dam, dlm, dq_partials, N, T, U, V, blank,
                               simple_scales(lm_only_scale, am_only_scale), plane_frames(topology, T)) != hipSuccess)
        return RNNT_STATUS_EXPAND_FAILED;
    return RNNT_STATUS_SUCCESS;
}

rnntStatus_t rnnt_amd_simple_backward(rnntStream_t stream, void* workspace, int dtype, const void* am, const void* lm,
                                      const float* q, const int* labels, const int* xn, const int* yn,
                                      const float* pair_grads, const float* znorm, const float* grad_costs, void* dam,
                                      void* dlm, float* dq_partials, int N, int T, int U, int V, int blank,
                                      float lm_only_scale, float am_only_scale) {
    return rnnt_amd_simple_backward_topology(stream, workspace, dtype, am, lm, q, labels, xn, yn, pair_grads, znorm,
                                             grad_costs, dam, dlm, dq_partials, N, T, U, V, blank, lm_only_scale,
                                             am_only_scale, RNNT_TOPOLOGY_REGULAR);
}

// include/warp_rnnt_amd_align.h: best-path alignments.  A producer of the loss fills the pair plane -- and leaves it
// filled -- the max-plus sweep and the trace of align.hip take the place of the alpha / beta sweeps.
size_t rnnt_amd_align_workspace_size(int N, int T, int U) {
    if (!dims_ok(N, T, U)) return 0;
    Carver c(nullptr);
    loss_layout(c, N, T, U);
    align_layout(c, N, T, U);
    return c.off;
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
        (!vocab_ok(V, blank) || (input_kind == RNNT_ALIGN_IN_HAT_LOGITS && V < 2) || labels_missing(U, labels)))
        return RNNT_STATUS_INVALID_ARGUMENT;
    if (N == 0) return RNNT_STATUS_SUCCESS;

    Carver c(workspace);
    const Workspace w = loss_layout(c, N, T, U);
    const AlignWorkspace aw = align_layout(c, N, T, U);
    if (fill_pair_plane(stream, PairSource{input_kind, dtype, input, nullptr}, labels, w.ws2, N, T, U, V, blank, nullptr) !=
        hipSuccess)
        return RNNT_STATUS_PROLOGUE_FAILED;
    if (launch_align_sweep(stream, w.ws2, xn, yn, aw.words, aw.park, scores, N, T, U) != hipSuccess)
        return RNNT_STATUS_WARP_FAILED;
    if (launch_align_trace(stream, aw.words, xn, yn, scores, emit_frames, N, T, U) != hipSuccess)
        return RNNT_STATUS_WARP_FAILED;
    return RNNT_STATUS_SUCCESS;
}

// include/warp_rnnt_amd_tdt.h: the token-and-duration (TDT) loss.  Nothing of the standard lattice serves: tdt.hip's
// producer fills a plane of 2 + D channels, its sweeps write alpha, beta and the costs, its gradient kernel the 2 + D sums
// per cell that the backward -- one streaming launch -- turns into d/d logits.
size_t rnnt_amd_tdt_workspace_size(int N, int T, int U, int D) {
    if (!tdt_shape_ok(RNNT_DTYPE_F32, N, T, U, 2, D, 0)) return 0;
    Carver c(nullptr);
    tdt_layout(c, N, T, U, D);
    return c.off;
}

rnntStatus_t rnnt_amd_tdt_loss_logits(rnntStream_t stream, void* workspace, int dtype, const void* logits,
                                      const int* labels, const int* xn, const int* yn, const int* durations, int D,
                                      float* costs, float* grads, int N, int T, int U, int V, int blank, float sigma,
                                      float fastemit_lambda) {
    if (!tdt_shape_ok(dtype, N, T, U, V, D, blank) || !tdt_durations_ok(durations, D)) return RNNT_STATUS_INVALID_ARGUMENT;
    if (!(sigma >= 0.0f && sigma <= 3.402823466e+38f)) return RNNT_STATUS_INVALID_ARGUMENT;      // (false for a NaN)
    if (!workspace_ok(workspace) || !logits || !xn || !yn || !costs || labels_missing(U, labels))
        return RNNT_STATUS_INVALID_ARGUMENT;
    if (!aligned(logits, dtype_size(dtype)) || !aligned(costs, 4) || !aligned(grads, 4) || !aligned(labels, 4) ||
        !aligned(xn, 4) || !aligned(yn, 4))
        return RNNT_STATUS_INVALID_ARGUMENT;
    if (N == 0) return RNNT_STATUS_SUCCESS;
    Carver c(workspace);
    const TdtWorkspace tw = tdt_layout(c, N, T, U, D);
    const TdtDurations dur = tdt_durations(durations, D);
    if (launch_tdt_plane(stream, dtype, logits, labels, tw.plane, N, T, U, V, D, blank, sigma) != hipSuccess)
        return RNNT_STATUS_PROLOGUE_FAILED;
    if (launch_tdt_sweeps(stream, tw.plane, xn, yn, tw.alphas, grads ? tw.betas : nullptr, tw.ll, costs, dur, N, T, U) !=
        hipSuccess)
        return RNNT_STATUS_WARP_FAILED;
    if (grads && launch_tdt_grads(stream, tw.plane, tw.alphas, tw.betas, tw.ll, xn, yn, grads, dur, N, T, U,
                                  fastemit_lambda) != hipSuccess)
        return RNNT_STATUS_GRADS_BLANK_FAILED;
    return RNNT_STATUS_SUCCESS;
}

rnntStatus_t rnnt_amd_tdt_logits_backward(rnntStream_t stream, int dtype, const void* logits, const int* labels,
                                          const float* grads, const float* grad_costs, void* dlogits, int N, int T, int U,
                                          int V, int D, int blank) {
    if (!tdt_shape_ok(dtype, N, T, U, V, D, blank)) return RNNT_STATUS_INVALID_ARGUMENT;
    if (!logits || !grads || !dlogits || labels_missing(U, labels)) return RNNT_STATUS_INVALID_ARGUMENT;
    if (!aligned(logits, dtype_size(dtype)) || !aligned(dlogits, dtype_size(dtype)) || !aligned(grads, 4) ||
        !aligned(grad_costs, 4) || !aligned(labels, 4))
        return RNNT_STATUS_INVALID_ARGUMENT;
    if (N == 0) return RNNT_STATUS_SUCCESS;
    if (launch_tdt_logits_backward(stream, dtype, logits, labels, grads, grad_costs, dlogits, N, T, U, V, D, blank) !=
        hipSuccess)
        return RNNT_STATUS_EXPAND_FAILED;
    return RNNT_STATUS_SUCCESS;
}

// include/warp_rnnt_amd_tdt_align.h: best-path alignments over the TDT lattice.  The loss's producer fills its plane -- and
// leaves it filled -- the max-plus sweep and the trace of tdt_align.hip take the place of the alpha / beta sweeps.
size_t rnnt_amd_tdt_align_workspace_size(int N, int T, int U, int D) {
    if (rnnt_amd_tdt_workspace_size(N, T, U, D) == 0) return 0;
    Carver c(nullptr);
    tdt_align_layout(c, N, T, U, D);
    return c.off;
}

rnntStatus_t rnnt_amd_tdt_align(rnntStream_t stream, void* workspace, int dtype, const void* logits, const int* labels,
                                const int* xn, const int* yn, const int* durations, int D, float* scores, int* emit_frames,
                                int* emit_durations, int N, int T, int U, int V, int blank, float sigma) {
    if (!tdt_shape_ok(dtype, N, T, U, V, D, blank) || !tdt_durations_ok(durations, D)) return RNNT_STATUS_INVALID_ARGUMENT;
    if (!(sigma >= 0.0f && sigma <= 3.402823466e+38f)) return RNNT_STATUS_INVALID_ARGUMENT;      // (false for a NaN)
    if (!workspace_ok(workspace) || !logits || !xn || !yn || !scores || labels_missing(U, labels) ||
        (U > 1 && (!emit_frames || !emit_durations)))
        return RNNT_STATUS_INVALID_ARGUMENT;
    if (!aligned(logits, dtype_size(dtype)) || !aligned(scores, 4) || !aligned(emit_frames, 4) ||
        !aligned(emit_durations, 4) || !aligned(labels, 4) || !aligned(xn, 4) || !aligned(yn, 4))
        return RNNT_STATUS_INVALID_ARGUMENT;
    if (N == 0) return RNNT_STATUS_SUCCESS;
    Carver c(workspace);
    const TdtAlignWorkspace aw = tdt_align_layout(c, N, T, U, D);
    const TdtDurations dur = tdt_durations(durations, D);
    if (launch_tdt_plane(stream, dtype, logits, labels, aw.plane, N, T, U, V, D, blank, sigma) != hipSuccess)
        return RNNT_STATUS_PROLOGUE_FAILED;
    if (launch_tdt_align_sweep(stream, aw.plane, xn, yn, aw.dec, scores, dur, N, T, U) != hipSuccess)
        return RNNT_STATUS_WARP_FAILED;
    if (launch_tdt_align_trace(stream, aw.dec, xn, yn, scores, emit_frames, emit_durations, dur, N, T, U) != hipSuccess)
        return RNNT_STATUS_WARP_FAILED;
    return RNNT_STATUS_SUCCESS;
}

// include/warp_rnnt_amd_tdt_joint.h: the joint network fused into the TDT loss.  rnnt_amd_tdt_loss_logits's shape with
// tdt_joint.hip's MFMA producer in front: it fills the plane (and the per-cell statistics), the sweeps and the gradient
// kernel of tdt.hip run as they are; the backward recomputes z.
size_t rnnt_amd_tdt_joint_workspace_size(int N, int T, int U, int H, int V, int D) {
    if (!tdt_joint_args_ok(RNNT_DTYPE_F32, RNNT_ACT_TANH, N, T, U, H, V, D, 0)) return 0;
    Carver c(nullptr);
    tdt_layout(c, N, T, U, D);
    tdt_joint_layout(c, N, T, U, H, V + D);
    return c.off;
}

rnntStatus_t rnnt_amd_tdt_joint_loss(rnntStream_t stream, void* workspace, int dtype, int activation, const void* f,
                                     const void* g, const void* weight, const float* bias, const int* labels,
                                     const int* xn, const int* yn, const int* durations, int D, float* costs, float* stats,
                                     float* grads, int N, int T, int U, int H, int V, int blank, float sigma,
                                     float fastemit_lambda, float p, const uint64_t* seed) {
    if (!tdt_joint_args_ok(dtype, activation, N, T, U, H, V, D, blank) || !tdt_durations_ok(durations, D))
        return RNNT_STATUS_INVALID_ARGUMENT;
    if (!(sigma >= 0.0f && sigma <= 3.402823466e+38f) || !dropout_ok(p, seed))       // (false for a NaN)
        return RNNT_STATUS_INVALID_ARGUMENT;
    if (!workspace_ok(workspace) || !f || !g || !weight || !xn || !yn || !costs || labels_missing(U, labels) ||
        (grads && !stats))
        return RNNT_STATUS_INVALID_ARGUMENT;
    if (!joint_inputs_aligned(f, g, weight, bias) || !aligned(stats, 16) || !aligned(grads, 4) || !aligned(costs, 4) ||
        !aligned(labels, 4) || !aligned(xn, 4) || !aligned(yn, 4))
        return RNNT_STATUS_INVALID_ARGUMENT;
    if (N == 0) return RNNT_STATUS_SUCCESS;
    Carver c(workspace);
    const TdtWorkspace tw = tdt_layout(c, N, T, U, D);
    const TdtDurations dur = tdt_durations(durations, D);
    if (launch_tdt_joint_fwd(stream, dtype, activation, f, g, weight, bias, labels, xn, yn, tw.plane,
                             grads ? stats : nullptr, N, T, U, H, V, D, blank, sigma, p,
                             p > 0.0f ? seed : nullptr) != hipSuccess)
        return RNNT_STATUS_PROLOGUE_FAILED;
    if (launch_tdt_sweeps(stream, tw.plane, xn, yn, tw.alphas, grads ? tw.betas : nullptr, tw.ll, costs, dur, N, T, U) !=
        hipSuccess)
        return RNNT_STATUS_WARP_FAILED;
    if (grads && launch_tdt_grads(stream, tw.plane, tw.alphas, tw.betas, tw.ll, xn, yn, grads, dur, N, T, U,
                                  fastemit_lambda) != hipSuccess)
        return RNNT_STATUS_GRADS_BLANK_FAILED;
    return RNNT_STATUS_SUCCESS;
}

rnntStatus_t rnnt_amd_tdt_joint_backward(rnntStream_t stream, void* workspace, int dtype, int activation, const void* f,
                                         const void* g, const void* weight, const float* bias, const int* labels,
                                         const int* xn, const int* yn, const float* stats, const float* grads,
                                         const float* grad_costs, void* df, void* dg, float* dweight, float* dbias, int N,
                                         int T, int U, int H, int V, int D, int blank, float p, const uint64_t* seed) {
    if (!tdt_joint_args_ok(dtype, activation, N, T, U, H, V, D, blank) || !dropout_ok(p, seed))
        return RNNT_STATUS_INVALID_ARGUMENT;
    if (!workspace_ok(workspace) || !f || !g || !weight || !xn || !yn || !stats || !grads || labels_missing(U, labels))
        return RNNT_STATUS_INVALID_ARGUMENT;
    if (!joint_inputs_aligned(f, g, weight, bias) || !aligned(stats, 16) || !aligned(grads, 4) ||
        !aligned(grad_costs, 4) || !aligned(labels, 4) || !aligned(xn, 4) || !aligned(yn, 4))
        return RNNT_STATUS_INVALID_ARGUMENT;
    if (N == 0 || (!df && !dg && !dweight && !dbias)) return RNNT_STATUS_SUCCESS;
    Carver c(workspace);
    tdt_layout(c, N, T, U, D);
    const JointWorkspace jw = tdt_joint_layout(c, N, T, U, H, V + D);
    if (launch_tdt_joint_bwd(stream, dtype, activation, f, g, weight, bias, labels, xn, yn, stats, grads, grad_costs, jw.wt,
                             jw.dw_part, jw.db_part, joint_w_splits(N, T, U, H, V + D, dtype), df, dg, dweight, dbias, N,
                             T, U, H, V, D, blank, p, p > 0.0f ? seed : nullptr) != hipSuccess)
        return RNNT_STATUS_EXPAND_FAILED;
    return RNNT_STATUS_SUCCESS;
}

// include/warp_rnnt_amd_multiblank.h: the multi-blank loss.  As TDT's, nothing of the standard lattice serves:
// multiblank.hip's producer fills a plane of 1 + B channels, its sweeps write alpha, beta and the costs, its gradient kernel
// the 1 + B sums per cell that the backward -- one streaming launch -- turns into d/d logits.
size_t rnnt_amd_multiblank_workspace_size(int N, int T, int U, int B) {
    if (!mb_shape_ok(RNNT_DTYPE_F32, N, T, U, B + 1, B)) return 0;
    Carver c(nullptr);
    mb_layout(c, N, T, U, B);
    return c.off;
}

rnntStatus_t rnnt_amd_multiblank_loss_logits(rnntStream_t stream, void* workspace, int dtype, const void* logits,
                                             const int* labels, const int* xn, const int* yn, const int* blank_ids,
                                             const int* blank_durations, int B, float* costs, float* grads, int N, int T,
                                             int U, int V, float sigma, float fastemit_lambda) {
    if (!mb_shape_ok(dtype, N, T, U, V, B) || !mb_ids_ok(blank_ids, B, V) || !mb_durations_ok(blank_durations, B))
        return RNNT_STATUS_INVALID_ARGUMENT;
    if (!(sigma >= 0.0f && sigma <= 3.402823466e+38f)) return RNNT_STATUS_INVALID_ARGUMENT;      // (false for a NaN)
    if (!workspace_ok(workspace) || !logits || !xn || !yn || !costs || labels_missing(U, labels))
        return RNNT_STATUS_INVALID_ARGUMENT;
    if (!aligned(logits, dtype_size(dtype)) || !aligned(costs, 4) || !aligned(grads, 4) || !aligned(labels, 4) ||
        !aligned(xn, 4) || !aligned(yn, 4))
        return RNNT_STATUS_INVALID_ARGUMENT;
    if (N == 0) return RNNT_STATUS_SUCCESS;
    Carver c(workspace);
    const MbWorkspace mw = mb_layout(c, N, T, U, B);
    const MbBlanks blanks = mb_blanks(blank_ids, blank_durations, B);
    if (launch_mb_plane(stream, dtype, logits, labels, mw.plane, N, T, U, V, blanks, sigma) != hipSuccess)
        return RNNT_STATUS_PROLOGUE_FAILED;
    if (launch_mb_sweeps(stream, mw.plane, xn, yn, mw.alphas, grads ? mw.betas : nullptr, mw.ll, costs, blanks, N, T, U) !=
        hipSuccess)
        return RNNT_STATUS_WARP_FAILED;
    if (grads && launch_mb_grads(stream, mw.plane, mw.alphas, mw.betas, mw.ll, xn, yn, grads, blanks, N, T, U,
                                 fastemit_lambda) != hipSuccess)
        return RNNT_STATUS_GRADS_BLANK_FAILED;
    return RNNT_STATUS_SUCCESS;
}

rnntStatus_t rnnt_amd_multiblank_logits_backward(rnntStream_t stream, int dtype, const void* logits, const int* labels,
                                                 const float* grads, const float* grad_costs, void* dlogits, int N, int T,
                                                 int U, int V, const int* blank_ids, int B) {
    if (!mb_shape_ok(dtype, N, T, U, V, B) || !mb_ids_ok(blank_ids, B, V)) return RNNT_STATUS_INVALID_ARGUMENT;
    if (!logits || !grads || !dlogits || labels_missing(U, labels)) return RNNT_STATUS_INVALID_ARGUMENT;
    if (!aligned(logits, dtype_size(dtype)) || !aligned(dlogits, dtype_size(dtype)) || !aligned(grads, 4) ||
        !aligned(grad_costs, 4) || !aligned(labels, 4))
        return RNNT_STATUS_INVALID_ARGUMENT;
    if (N == 0) return RNNT_STATUS_SUCCESS;
    if (launch_mb_logits_backward(stream, dtype, logits, labels, grads, grad_costs, dlogits, N, T, U, V,
                                  mb_blanks(blank_ids, nullptr, B)) != hipSuccess)
        return RNNT_STATUS_EXPAND_FAILED;
    return RNNT_STATUS_SUCCESS;
}

}  // extern "C"
