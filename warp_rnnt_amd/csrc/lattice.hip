// Alpha / beta lattice sweeps of the RNN-Transducer loss for MI355X (gfx950).
//
// What it computes (per utterance n; maths = SURVEY.md Appendix A; reference
// kernels: core_gather.cu:37-133 (alphas), :135-234 (betas), dense indexing
// core.cu:84-87,116-120,189-192,221-225):
//   alpha[t,u] = lse(alpha[t-1,u] + lpB[t-1,u], alpha[t,u-1] + lpL[t,u-1]),  alpha[0,0] = 0
//   beta [t,u] = lse(beta[t+1,u] + lpB[t,u],    beta[t,u+1] + lpL[t,u]),     beta[T-1,U-1] = lpB[T-1,U-1]
//
// How (nothing like the reference's 32x1 warp tiles ordered by global spin
// locks):
//   * one workgroup per (utterance, direction); lane <-> lattice column,
//     wave w owns columns [64w, 64w+64); up to 16 waves (1024 columns) per
//     pass, wider lattices are swept in column stripes;
//   * true anti-diagonal sweep: at diagonal d every lane computes its cell
//     (d - u, u).  The value a cell needs from its left neighbour moves one
//     lane up with a single DPP `wave_shr:1`; the value it needs from the
//     previous frame is the lane's own register;
//   * wave w runs K diagonals (one "block") behind wave w-1; the boundary
//     column between two waves is handed over through a tiny LDS ring, K
//     values per block, with ONE s_barrier per K diagonals.  No global
//     atomics, no inter-workgroup ordering;
//   * log-probs are read from the diagonal-major workspace (common.h): each
//     diagonal is one contiguous row, K rows are prefetched into registers a
//     block ahead; alphas/betas are written in the same diagonal-major layout
//     with coalesced stores.
//   Critical path: (T_n + U_n - 1) + K*(waves-1) dependent lse steps.
#include <atomic>
#include <cstdlib>
#include <type_traits>

#include "common.h"
#include "kernels.h"
#include "lattice_launch.h"
#include "lattice_single.h"

namespace rnnt {

using namespace single;

template <int LOADER, bool COMPACT>
__global__ void __launch_bounds__(MAXW * WAVE) k_lattice(const LatticeArgs a) {
    __shared__ float mail[MAXW][RING];
    __shared__ float trash[MAXW][MAIL_TRASH];
    // XCD-aware placement: workgroup b runs on XCD b % 8 (MI355X_MICROARCH.md), each XCD has its
    // own L2.  The alpha and the beta sweep of one utterance read the same diagonal-major plane
    // (from opposite ends), so they are given ids b and b+8: same XCD, shared L2 lines.
    // (Speed only; nothing depends on the placement.)
    const unsigned b = blockIdx.x, pairs_total = gridDim.x >> 1;
    const unsigned grp = b >> 4, in = b & 15;
    unsigned n, dir;
    if ((grp << 3) + 8 <= pairs_total) { n = (grp << 3) + (in & 7); dir = in >> 3; }
    else { const unsigned r = b - (grp << 4); n = (grp << 3) + (r >> 1); dir = r & 1; }   // tail group
    if (a.beta_only && !dir) return;
    if (a.redo && a.redo[2 * n + dir] == 0) return;   // launched behind a ring kernel: only the sweeps it flagged
    if (dir)
        sweep<LOADER, true, COMPACT>(a, n, mail, trash);
    else
        sweep<LOADER, false, COMPACT>(a, n, mail, trash);
}

namespace {
// compute units of the stream's device (one query per process and device; 256 on MI355X): the kernels with one
// workgroup per column block want CUs of their own for them
int device_cus(hipStream_t stream) {
    static std::atomic<int> cached[64];
    int dev = 0;
    // the device that owns the stream the kernels go to (not necessarily the current one)
    if (hipStreamGetDevice(stream, &dev) != hipSuccess && hipGetDevice(&dev) != hipSuccess) return 256;
    if (dev < 0 || dev >= 64) return 256;
    int n = cached[dev].load(std::memory_order_relaxed);
    if (n == 0) {
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
        cached[dev].store(n, std::memory_order_relaxed);
    }
    return n;
}

// The knobs of the lattice family, read from the environment once per process -- here and nowhere else.  The shipped
// library reads the first two; the other two exist in the A/B build only (common.h: ab_getenv).
const LatticeKnobs& knobs_from_env() {
    static const LatticeKnobs knobs = [] {
        LatticeKnobs k;
        const char* v = getenv("RNNT_DEBUG_LATTICE_KERNEL");
        if (v && v[0] == 'w') k.pin = v[1] == 's' ? PIN_WS : v[1] == 'd' ? PIN_WD : v[1] == 'l' ? PIN_WL : PIN_AUTO;
        if ((v = getenv("RNNT_WD_K16_FROM_T")) != nullptr) k.k16_from_t = atoi(v);
        if ((v = ab_getenv("RNNT_WL_MAX_BLOCKS")) != nullptr) {
            const int d = atoi(v);
            k.wl_max_blocks = d < 0 ? 0 : (d > WL_MAX_BLOCKS ? WL_MAX_BLOCKS : d);
        }
        k.no_prep_fold = ab_getenv("RNNT_NO_PREP_FOLD") != nullptr;
        return k;
    }();
    return knobs;
}
std::atomic<int>& kernel_override_setting() {
    static std::atomic<int> r{knobs_from_env().pin};
    return r;
}
LatticeKnobs current_knobs() {      // the environment's, with the pin as rnnt_amd_debug_set_lattice_kernel left it
    LatticeKnobs k = knobs_from_env();
    k.pin = kernel_override_setting().load(std::memory_order_relaxed);
    return k;
}

// (compact layout: the native entry's 64-bit cell offsets; a.T / a.U are then the launch bounds Tmax / Umax)
LatticeFacts facts_of(hipStream_t stream, const LatticeArgs& a, int N, int loader, bool folded) {
    // (the other loaders take the single-role kernel whatever the device: no query)
    return LatticeFacts{N, a.T, a.U, loader, a.redo && a.queue, a.mail != nullptr, a.offs32 != nullptr, folded,
                        loader == LOAD_SKEWED ? device_cus(stream) : 0};
}

// the single-role kernel: one workgroup per sweep, 1024-column stripes, every loader; honours a.redo
hipError_t launch_single(hipStream_t stream, const LatticeArgs& a, int N, int loader) {
    int waves = column_blocks(a.U);
    waves = waves < 1 ? 1 : (waves > MAXW ? MAXW : waves);
    const dim3 grid(2 * N), block(waves * WAVE);
    if (is_compact(a)) {   // compact layout: diagonal-major pairs (native path) or row-major pairs (core.h shims)
        if (loader == LOAD_ROWMAJOR2) k_lattice<LOAD_ROWMAJOR2, true><<<grid, block, 0, stream>>>(a);
        else k_lattice<LOAD_SKEWED, true><<<grid, block, 0, stream>>>(a);
        return hipGetLastError();
    }
    switch (loader) {
        case LOAD_SKEWED:    k_lattice<LOAD_SKEWED, false><<<grid, block, 0, stream>>>(a); break;
        case LOAD_ROWMAJOR2: k_lattice<LOAD_ROWMAJOR2, false><<<grid, block, 0, stream>>>(a); break;
        default:             k_lattice<LOAD_DENSE, false><<<grid, block, 0, stream>>>(a); break;
    }
    return hipGetLastError();
}
}  // namespace

static thread_local int g_last_kernel = 0;
int last_lattice_kernel() { return g_last_kernel; }

int lattice_kernel_override() { return kernel_override_setting().load(std::memory_order_relaxed); }

int set_lattice_kernel_override(int k) {
    if (k < PIN_AUTO || k > PIN_WL) return -1;
    return kernel_override_setting().exchange(k, std::memory_order_relaxed);
}

int debug_lattice_plan(int N, int T, int U, int loader, int resources, int cus, int pin, int folded) {
    if (N <= 0 || T < 1 || U < 1 || pin < -1 || pin > PIN_WL) return -1;
    LatticeKnobs k = current_knobs();
    if (pin >= 0) k.pin = pin;
    const LatticeFacts f{N, T, U, loader, (resources & 1) != 0, (resources & 2) != 0, (resources & 4) != 0, folded != 0,
                         cus > 0 ? cus : 256};
    const LatticePlan p = plan_lattice(f, k);
    return p.reported | p.block_diagonals << 8 | (p.kernel == LatticeKernel::WD_RINGS ? 1 : 0) << 16;
}

// Asked BEFORE the producer of the call's pair plane runs: planned as folded.  A parcel that cannot be had (false) leaves
// a.prepared unset, and launch_lattice plans the same call again by the unfolded thresholds.
bool lattice_ring_prep(hipStream_t stream, const LatticeArgs& a, int N, int loader, RingPrep* prep) {
    const LatticeKnobs knobs = current_knobs();
    if (knobs.no_prep_fold || N <= 0) return false;
    const LatticePlan plan = plan_lattice(facts_of(stream, a, N, loader, true), knobs);
    return plan.kernel == LatticeKernel::WD_RINGS && wd_ring_prep(stream, a, N, plan.block_diagonals, prep);
}

hipError_t launch_lattice(hipStream_t stream, const LatticeArgs& a, int N, int loader) {
    if (N <= 0) return hipSuccess;
    LatticeArgs plain = a;          // for the kernels that sweep everything: no redo flags to look at
    plain.redo = nullptr;
    const LatticePlan plan = plan_lattice(facts_of(stream, a, N, loader, a.prepared != 0), current_knobs());
    hipError_t e = hipErrorNotSupported;
    switch (plan.kernel) {
        case LatticeKernel::WD_LONE:
            e = launch_lattice_wd(stream, plain, N, plan.block_diagonals, true);
            break;
        case LatticeKernel::WD_RINGS:
            e = launch_lattice_wd(stream, a, N, plan.block_diagonals, false);
            if (e == hipSuccess) {
                g_last_kernel = plan.reported;
                // ... and behind it a single-workgroup kernel for the sweeps it flagged (normally none: its workgroups
                // read one flag and return, 5 us per call)
                return column_blocks(a.U) <= WS_MAX_BLOCKS ? launch_lattice_ws(stream, a, N)
                                                           : launch_single(stream, a, N, loader);
            }
            if (e != hipErrorNotSupported) return e;
            break;
        case LatticeKernel::WL:
            e = launch_lattice_wl(stream, plain, N, plan.wl_blocks);
            break;
        case LatticeKernel::WS:
            e = launch_lattice_ws(stream, plain, N);
            break;
        case LatticeKernel::SINGLE:
            break;
    }
    if (e != hipErrorNotSupported) { g_last_kernel = plan.reported; return e; }
    g_last_kernel = 4;              // planned, or the last resort of a launcher whose own guards refused the call
    return launch_single(stream, plain, N, loader);
}

}  // namespace rnnt
