// Which of the bit-identical alpha / beta kernels serves a call, decided ONCE, by a pure function of the call's facts and the
// process's knobs: no HIP call, no static, no environment.  launch_lattice (lattice.hip) launches what the plan says,
// lattice_ring_prep asks the same function before the producer runs, rnnt_amd_debug_lattice_plan answers without a launch
// (tests/test_host_lattice_plan.py holds the table).  Why each kernel wins where it does: DESIGN.md section 3.2.
#pragma once
#include <climits>

#include "common.h"

namespace rnnt {

constexpr int WS_MAX_BLOCKS = 8;        // column blocks one k_lattice_ws workgroup sweeps (ws::MAXA is this)
constexpr int WL_MAX_BLOCKS = 5;        // column blocks k_lattice_wl's LDS holds (148 of the CU's 160 KiB)
inline int column_blocks(int U) { return (U + WAVE - 1) / WAVE; }       // 64 lattice columns each: one wave, lane = column

enum LatticePin : int { PIN_AUTO = 0, PIN_WS = 1, PIN_WD = 2, PIN_WL = 3 };      // rnnt_amd_debug_set_lattice_kernel

// what the choice may depend on
struct LatticeFacts {
    int N, T, U;          // launch bounds (compact layout: Tmax, Umax)
    int loader;           // common.h: Loader; only LOAD_SKEWED (diagonal-major) is read by the column-block kernels
    bool flags;           // redo flags and the work queue are there (LatticeArgs::redo, ::queue)
    bool rings;           // hand-over rings are there (LatticeArgs::mail)
    bool offs32;          // compact layout with the reference's 32-bit offsets
    bool folded;          // the ring preparation rides in the launch of the kernel that produces the pair plane (dense and
                          // gathered routes); else it is a launch of its own in front of the sweeps, ~4 us that move wd's
                          // break-even points
    int cus;              // compute units of the device
};

struct LatticeKnobs {
    int pin = PIN_AUTO;              // RNNT_DEBUG_LATTICE_KERNEL / rnnt_amd_debug_set_lattice_kernel
    int k16_from_t = -1;             // RNNT_WD_K16_FROM_T: wd's blocks of 16 diagonals from this T on; -1: by shape
    int wl_max_blocks = WL_MAX_BLOCKS;   // RNNT_WL_MAX_BLOCKS (A/B build): 0 = wl is never chosen, pinned or not
    bool no_prep_fold = false;       // RNNT_NO_PREP_FOLD (A/B build): the ring preparation always a launch of its own
};

enum class LatticeKernel : int {
    WD_LONE,      // k_lattice_wd, one column block per sweep: a plain launch (no rings, no queue, no redo kernel behind)
    WD_RINGS,     // k_lattice_wd with flags, queue and rings; the redo kernel behind it
    WL,           // k_lattice_wl: all column blocks of a sweep in one workgroup, boundary columns through LDS
    WS,           // k_lattice_ws: compute + I/O wave pairs, one workgroup per sweep
    SINGLE        // k_lattice: the single-role kernel, any loader, any width
};

struct LatticePlan {
    LatticeKernel kernel;
    int block_diagonals;   // 8 or 16: which instantiation of k_lattice_wd (and how long its rings are)
    int wl_blocks;         // the max_blocks k_lattice_wl is launched with
    int reported;          // last_lattice_kernel(): 1 ws, 2 wd, 4 single-role, 5 wl
};

#ifdef RNNT_LATTICE_LEGACY      // the `precise` build: the single-role kernel everywhere
constexpr bool PLAN_SINGLE_ONLY = true;
#else
constexpr bool PLAN_SINGLE_ONLY = false;
#endif
#ifdef RNNT_WD_STATS            // the diagnostics build stamps through the rings' tail: it has no plain launch
constexpr bool PLAN_HAS_LONE = false;
#else
constexpr bool PLAN_HAS_LONE = true;
#endif

// Blocks of 16 diagonals from T >= 1024, and from T >= 320 on one column block while every workgroup has a CU of its own
// (tools/lattice_routes.py: profiles/r06_lattice_routes.txt, profiles/r06_k16_threshold.txt).  The knob replaces both.
inline int plan_block_diagonals(const LatticeFacts& f, const LatticeKnobs& k) {
    if (k.k16_from_t >= 0) return f.T >= k.k16_from_t ? 16 : 8;
    if (f.U <= WAVE && f.T >= 320 && 2ll * f.N <= (long long)f.cus) return 16;
    return f.T >= 1024 ? 16 : 8;
}

inline LatticePlan plan_lattice(const LatticeFacts& f, const LatticeKnobs& k) {
    const int bd = plan_block_diagonals(f, k);
    const auto plan = [&](LatticeKernel kernel, int reported, int wl_blocks = 0) {
        return LatticePlan{kernel, bd, wl_blocks, reported};
    };
    if (PLAN_SINGLE_ONLY || f.loader != LOAD_SKEWED) return plan(LatticeKernel::SINGLE, 4);
    const int nA = column_blocks(f.U);
    const long long wgs = 2ll * f.N * nA;                 // wd's workgroups: one per column block and sweep
    const bool wgs_ok = wgs < (1ll << 31);
    // 1. one column block: nothing is handed over, wd's three-wave team beats ws's wave pair at every size
    //    (tools/lattice_routes.py: profiles/r04_lattice_routes_single_block.txt)
    if (PLAN_HAS_LONE && nA == 1 && k.pin != PIN_WS && wgs_ok) return plan(LatticeKernel::WD_LONE, 2);
    // 2. wd with rings: while its workgroups find CUs and the sweep is long enough to recover the launches around it.
    //    from_t: a CU for every workgroup; from_t2: two workgroups per CU.  Measured on the whole loss entry with each
    //    kernel pinned (tools/loss_routes.py, and --fused for the unfolded column: profiles/r06_loss_routes.txt; two
    //    column blocks: profiles/r06_two_block_routes.txt)
    const bool ring_ok = f.flags && !f.offs32 && (nA == 1 || f.rings);
    if (ring_ok && nA >= 2 && wgs_ok && k.pin != PIN_WS && k.pin != PIN_WL) {
        const int from_t = f.folded ? (nA == 2 ? 900 : nA == 3 ? 640 : nA == 4 ? 400 : nA == 5 ? 320 : 128)
                                    : (nA == 2 ? 1200 : nA == 3 ? 1100 : nA == 4 ? 640 : nA == 5 ? 400 : 128);
        const int from_t2 = nA <= 3 ? INT_MAX : nA == 4 ? 1400 : nA == 5 ? 800 : 128;
        const bool by_shape = (wgs <= f.cus && f.T >= from_t) || (wgs <= 2ll * f.cus && f.T >= from_t2);
        // (wider than one ws workgroup sweeps: column blocks, or the single-role kernel's stripes)
        if (k.pin == PIN_WD || nA > WS_MAX_BLOCKS || by_shape) return plan(LatticeKernel::WD_RINGS, 2);
    }
    // 3. wl: needs nothing but the planes, so it also serves the callers without flags and rings.  By itself two column
    //    blocks always, up to five while one workgroup per sweep leaves CUs idle (beyond ~100 utterances ws's ten waves
    //    per workgroup pack the chip better than fifteen: tools/lattice_routes.py, profiles/r05_lattice_routes.txt);
    //    pinned: all it can take.  Not when wd is pinned: a pinned A/B run measures the kernel it names or falls to ws.
    if ((k.pin == PIN_AUTO || k.pin == PIN_WL) && nA >= 2) {
        const int two = k.wl_max_blocks < 2 ? k.wl_max_blocks : 2;
        const int limit = k.pin == PIN_WL || nA <= 2 || f.N <= 96 ? k.wl_max_blocks : two;
        if (nA <= limit && nA <= WL_MAX_BLOCKS) return plan(LatticeKernel::WL, 5, limit);
    }
    // 4. ws while one workgroup sweeps the width, 5. else the single-role kernel's stripes
    if (nA <= WS_MAX_BLOCKS) return plan(LatticeKernel::WS, 1);
    return plan(LatticeKernel::SINGLE, 4);
}

}  // namespace rnnt
