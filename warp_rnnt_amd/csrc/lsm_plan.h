// Which forward log-softmax kernel serves a call, and in which shape, decided ONCE by a pure function of the call's facts and
// the process's knobs: no HIP call, no static, no environment (host-only code may include this).  dispatch_lsm_map (lsm.h)
// and launch_log_softmax_backward (lsm_backward.hip) launch what the plan says, rnnt_amd_debug_lsm_plan answers without a
// launch (tests/test_host_lsm_plan.py holds the table).  Every byte predicate is one of whole four-element vectors (16 bytes
// of fp32, 8 of half), so a V takes the same kernel and the same lanes per row at every storage type: only the rows per
// LDS tile of the fused gather depend on elem_bytes.  The kernels themselves: lsm.h; the measurements stand at the
// thresholds they explain.
#pragma once
#include <cstddef>
#include <cstdint>

#pragma GCC visibility push(hidden)     // the library's own: nothing of this in its dynamic symbol table
namespace rnnt {

// What the log-softmax kernels emit.
enum LsmMode : int {
    LSM_NORM = 0,    // log-softmax rows
    LSM_GATHER = 1,  // diagonal-major (blank,label) log-prob pairs; log-probs never materialise
    LSM_BWD = 2      // d(loss)/d(logits) rows from the gathered gradients:
                     //   dz[v] = s*( [v==blank]gB + [v==label]gL - softmax(z)[v]*(gB+gL) )
};

constexpr int LSM_WAVE = 64;      // (common.h: WAVE; lsm.h checks)
constexpr int SM_THREADS = 256;
constexpr int SM_FLOATS = 3200;   // LDS tile budget in floats: one pass of the 256 threads over a 12.5 KiB tile.  (512 threads x 25 KiB: 2 % faster in the isolated probe, slower in bench.py and in the fused gather mode; two passes per tile or 50 KiB tiles are clearly worse.)
// In the fused gather the shared tile of half-precision logits holds twice the rows: 12.8 KB of HBM per tile, as for fp32
// (c4, bf16: 178 -> 172 us; the fused backward, which also writes the tile back, 287 -> 290 us with it and keeps the
// fp32 row count).  Rows per tile do not touch the bits: the lanes of a row and its reduction tree stay the same.
constexpr int lsm_tile_floats(int mode, int elem_bytes) {
    return mode == LSM_GATHER ? SM_FLOATS * (int)(sizeof(float) / (size_t)elem_bytes) : SM_FLOATS;
}
constexpr int RG_UN = 2;          // k_lsm_regs: groups per half and wave, loads first (1: 500 us, 2: 462-484, 4: 482-498)
constexpr int LG_MAXV = 16384;    // the largest row of the row-per-workgroup kernels (k_lsm_large, k_lsmbwd_large)
constexpr int SMB_THREADS = 256;  // log-softmax backward: two tiles per workgroup, keep the 256-thread shape
constexpr int SMB_FLOATS = 3200;

// what the choice may depend on
struct LsmFacts {
    int mode;             // LsmMode
    int elem_bytes;       // 4 or 2: the storage type of the logits
    int64_t rows;
    int V;
    bool aligned;         // x (and out, where rows are written) start on a four-element vector
    bool compact;         // the row -> cell map is CompactMap: never the diagonal walk
    int T, U;             // dense map: the (T,U) grid of the diagonal walk
    bool plane;           // LSM_NORM: the column plane is written too (LsmBwd::col_out)
};

// The A/B knobs, one field each; the defaults are what the library does when no variable is set.  Read from the
// environment by lsm_knobs() alone, once per process, and only in the build made for A/B runs (common.h: ab_getenv).
struct LsmKnobs {
    bool no_regs = false;         // RNNT_LSM_NO_REGS: the LDS-staged kernel where k_lsm_regs would run
    int regs_xcd = 1;             // RNNT_LSM_REGS_XCD=0: k_lsm_regs in the plain workgroup order
    bool no_lgr = false;          // RNNT_LSM_NO_LGR: the LDS-staged kernel where one row per small workgroup would run
    bool no_rows = false;         // RNNT_LSM_NO_ROWS: the LDS-staged kernel where k_lsm_rows would run
    bool no_diag = false;         // RNNT_LSM_NO_DIAG: consecutive rows per wave for every V
    bool rows_any = false;        // RNNT_LSM_ROWS_ANY: k_lsm_rows for every V % 4 == 0
    bool no_wp = false;           // RNNT_LSM_NO_WP: never the wave-private tiles
    bool wp_fused = false;        // RNNT_LSM_WP_FUSED: the wave-private tiles in the fused modes too
    int lg_xcd = -1;              // RNNT_LG_XCD=0 / 1: the row-per-workgroup order forced; -1: by shape
    int lg_xcd_fused = 0;         // RNNT_LG_XCD_FUSED=1: the contiguous order in the fused modes
    int bwd_xcd = 1;              // RNNT_LSMBWD_XCD=0: k_lsmbwd_large in the plain order
    bool bwd_smallest_cover = false;   // RNNT_LSMBWD_SMALLEST_COVER: its covers before round 3
};
const LsmKnobs& lsm_knobs();      // (lsm_f32.hip: the one reader)

enum class LsmFamily : int {
    REGS = 0,        // k_lsm_regs<KR>: KR rows per 16-byte aligned group, in registers
    LGR = 1,         // k_lsm_large<TH, NV> as one row per SMALL workgroup (128 < V <= 1024)
    ROWS = 2,        // k_lsm_rows<L, Q>: L lanes per row, consecutive rows per wave
    ROWS_DIAG = 3,   // k_lsm_rows_diag<Q>: the same lanes along the diagonals
    SMALL = 4,       // k_lsm_small<L, WP>: LDS tiles of R rows
    LARGE = 5,       // k_lsm_large<TH, NV>: one row per workgroup (1024 < V <= 16384)
    GENERIC = 6      // k_lsm_generic: a wave per row, any V, any alignment
};

// what the launcher needs, and nothing it has to work out again (fields a family does not use are 0)
struct LsmPlan {
    LsmFamily family;
    int KR;                       // REGS
    int L;                        // ROWS, ROWS_DIAG, SMALL: lanes per row
    int Q;                        // ROWS, ROWS_DIAG: float4 per lane (1 ... 4)
    bool WP;                      // SMALL: wave-private tiles
    int TH, NV;                   // LGR, LARGE: threads x float4 per thread cover a row
    unsigned grid, grid_y, grid_z;   // (y, z: the diagonal walk's column blocks and utterances; 1 elsewhere)
    size_t lds_bytes;             // SMALL
    int R, q;                     // SMALL: rows per tile, columns per lane
    int xcd;                      // REGS, LARGE: every XCD streams a contiguous eighth
    int64_t head_rows;            // REGS: the ngroups * KR rows this launch takes; the rest is planned by a second call
};

// rows per group for k_lsm_regs, or 0 when the kernel does not fit V: the largest KR <= 4 with KR*V a multiple of 4 and
// KR*V/4 <= 32 lanes, if it keeps at least 20 of the 32 lanes of a half busy
inline int lsm_regs_rows_per_group(int V) {
    if (V < 4) return 0;
    int best = 0;
    for (int k = 1; k <= 4; ++k)
        if ((k * V) % 4 == 0 && (k * V) / 4 <= 32) best = k;
    return (best && (best * V) / 4 >= 20) ? best : 0;
}
inline unsigned lsm_stream_grid(int64_t chunks) { return ((unsigned)chunks + 7u) & ~7u; }     // (common.h: stream_grid)
// the grid-stride row-per-workgroup kernels: a workgroup per row up to 4 M of them
inline unsigned lsm_row_grid(int64_t rows, int xcd) {
    const unsigned grid = (unsigned)(rows < (1 << 22) ? rows : (1 << 22));
    return xcd ? (grid + 7u) & ~7u : grid;
}

// A REGS plan covers head_rows = (rows / KR) * KR rows; the caller plans the rows left over with f.rows = rows - head_rows
// (and the same `aligned`: the head ends on a group boundary, a whole number of vectors).  That second plan is never REGS
// again: KR is a function of V, aligned and the knobs alone, and fewer than KR rows are left.
inline LsmPlan plan_lsm(const LsmFacts& f, const LsmKnobs& k) {
    const int V = f.V;
    const int64_t rows = f.rows;
    const bool gather = f.mode == LSM_GATHER;
    LsmPlan p{};
    p.grid_y = p.grid_z = 1;
    if (f.mode == LSM_NORM) {
        // rows in registers where the vocabulary allows it
        // (below V = 32 -- four rows per group -- the LDS-staged kernel with its straight-line row pass is the faster one
        //  since round 4: the c4 lattice with V=24 0.584 -> 0.536 ms per step, V=28 0.589-0.605 -> 0.584, c2 0.0343 -> 0.0336;
        //  from V = 32 on this kernel wins inside the step: V=40 0.71 vs 0.73, V=50 0.870 vs 0.893; tools/step_rate.py)
        const int kr = (f.aligned && !k.no_regs && V >= 32) ? lsm_regs_rows_per_group(V) : 0;
        if (kr && rows >= kr) {
            const int64_t ngroups = rows / kr;
            const int64_t per_wg = 4 * RG_UN * 2;               // 4 waves x RG_UN groups x 2 halves
            int64_t grid = (ngroups + per_wg - 1) / per_wg;
            // every XCD streams a contiguous eighth of the tensor (as the row-per-workgroup kernel below; here it costs two
            // scalar instructions): V=50 1.44 GB equal, 5.76 GB 5.66 -> 5.86 TB/s, V=64 6.25 -> 6.40, 100 5.92 -> 6.19, 128
            // 6.15 -> 6.44; the c4 step in bench.py 0.8759 / 0.8781 / 0.8779 -> 0.8726 / 0.8702 / 0.8709 ms, three
            // interleaved pairs (profiles/r04_lsm_xcd_order_ab.txt)
            if (k.regs_xcd) grid = (grid + 7) / 8 * 8;
            if (grid < ((int64_t)1 << 31)) {
                p.family = LsmFamily::REGS;
                p.KR = kr;
                p.grid = (unsigned)grid;
                p.xcd = k.regs_xcd;
                p.head_rows = ngroups * kr;                     // (a group boundary: vector aligned)
                return p;
            }
        }
        // 128 < V <= 1024 whose rows fill a cover of 64 ... 256 threads x one float4 (or an exact 64x2 / 64x3 / 128x2):
        // the row-in-registers kernel, one row per small workgroup, instead of the LDS-staged tiles.  Measured
        // round 3 (tools/lsm_rate.py, 1.44 GB in, TB/s in + out, LDS-staged -> registers; profiles/r03_lsm_midv_probe.txt):
        // V=256 5.82 -> 6.44, 496 5.33 -> 6.12, 500 5.14 -> 5.90, 512 5.77 -> 6.47, 768 5.58 -> 6.15, 980 5.26 -> 6.00,
        // 1000 5.14 -> 6.10, 1024 5.76 -> 6.59; with 94 % of the lanes busy still +4 ... +10 % (484, 724, 964), below
        // that -- and below 98 % for a single wave (V=244: 5.53 -> 5.23) -- the tiles win (V=200, 400, 600: 78 / 59 %).
        if (f.aligned && !k.no_lgr && V % 4 == 0 && V > 128 && V <= 1024) {
            const int nvec = V >> 2, th = (nvec + 63) / 64 * 64;
            int TH = 0, NV = 1;
            if (nvec == 64) TH = 64;
            else if (nvec == 128) TH = 64, NV = 2;
            else if (nvec == 192) TH = 64, NV = 3;
            else if (nvec == 256) TH = 128, NV = 2;
            else if (th == 64 && nvec >= 63) TH = 64;
            else if (th >= 128 && th <= 256 && nvec * 100 >= th * 94) TH = th;
            if (TH) {
                p.family = LsmFamily::LGR;
                p.TH = TH;
                p.NV = NV;
                p.grid = lsm_row_grid(rows, 0);
                return p;
            }
        }
    }
    if (gather) {
        // V % 4 != 0 (c4's own V = 50: rows that pack into 16-byte groups only in twos) stays on the LDS-staged kernel below.
        // Round 5 tried the rows-in-registers loads of k_lsm_regs for it once more, with what round 4 had learnt on
        // k_lsm_rows -- the lane that stores a row's pair asks for its two logits itself, ahead of the group loads, or picks
        // them out of an LDS copy of the groups: whole fused forward at c4 503-512 us (two and four groups per half-wave:
        // 558 / 503; LDS copy 512) against 419-433 for the LDS-staged kernel then, and ~400 since its staging loop issues
        // its loads first (k_lsm_small; the kernel alone 290 -> 225-255 us, 5.6-6.4 TB/s read against 7.0 for a bare
        // read-only stream, tools/ubench/copy_rate.hip, profiles/r05_loads_first_ab.txt).
        // Rows in registers, L lanes per row (k_lsm_rows), against the LDS-staged kernel below -- re-measured after that
        // kernel got its straight-line row pass (forward of the fused entry, N=32, T=500, U=100, us, k_lsm_rows / LDS tiles;
        // tools/fused_rate.py, profiles/r04_lsm_rows_ab.txt section 9): V=32 97 / 127, 64 140 / 146, 128 187 / 197, 256 320 /
        // 341, 320 393 / 404; 448 512 / 522, 480 532 / 554, 500 561 / 583, 512 505 / 587, 544 609 / 753, 640 668 / 749, 768
        // 791 / 812, 896 850 / 930, 1000 986 / 1089, 1024 1016 / 1128; but 96 180 / 163, 160 256 / 237, 192 285 / 262, 224 302 /
        // 290, 352 426 / 418, 384 456 / 426, 400 510 / 485, and everything whose 8- or 16-lane row instructions straddle
        // lines (V=100: 236 / 187, 132: 281 / 257) or needs float2 rows (V=50: 169 / 132).  Rule: the powers of two from 32
        // to 256, and every V % 4 == 0 from 448 on.
        const bool rows_rule = V == 32 || V == 64 || V == 128 || V == 256 || V >= 448;
        if (f.aligned && !k.no_rows && V % 4 == 0 && V >= 32 && V <= 1024 && (rows_rule || k.rows_any)) {
            int L = 8;
            while (L < 64 && L * 16 < V) L <<= 1;
            const int q = (V / 4 + L - 1) / L;         // 1 ... 4
            p.L = L;
            p.Q = q;
            // (the diagonal walk needs the dense (T,U) grid; rows that are one or two whole lines, T >= 16: lsm.h)
            if (!f.compact && V <= 64 && V % 32 == 0 && f.T >= 16 && f.U >= 1 && !k.no_diag) {
                const int64_t N = rows / ((int64_t)f.T * f.U), nub = (f.U + 15) / 16;
                if (N <= 65535 && nub <= 65535) {
                    p.family = LsmFamily::ROWS_DIAG;
                    p.grid = (unsigned)((f.T + 3) / 4);
                    p.grid_y = (unsigned)nub;
                    p.grid_z = (unsigned)N;
                    return p;
                }
            }
            const int64_t rpw = L <= 8 ? 2 * (LSM_WAVE / L) : LSM_WAVE / L;       // RowsShape<L>::RPW
            const int64_t chunks = (rows + 4 * rpw - 1) / (4 * rpw);
            if (chunks < ((int64_t)1 << 31) - 8) {
                p.family = LsmFamily::ROWS;
                p.grid = lsm_stream_grid(chunks);
                return p;
            }
            p.L = p.Q = 0;
        }
    }
    if (f.aligned && V <= 1024) {
        int L = 1;
        while (L < 64 && L * 16 < V) L <<= 1;          // <= 16 columns per lane
        const int rpp = SM_THREADS / L;                // rows per pass, a multiple of 4
        int R = (lsm_tile_floats(f.mode, f.elem_bytes) / V) / rpp * rpp;   // whole passes
        if (R < rpp) R = rpp;
        // wave-private tiles: each wave owns WAVE/L rows (a multiple of 4 for L <= 16), one pass.
        // Plain log-softmax only: measured 2-3 % faster there (0.506 -> 0.493 ms at c4), slower for the fused
        // gather (its one-lane-per-row mapping phase wants all rows of the tile in ONE wave: 0.52 -> 0.556 ms)
        // and for the fused backward (+15 us).
        const bool wp = (L <= 16) && !k.no_wp && (f.mode == LSM_NORM || k.wp_fused);
        if (wp) R = rpp;
        p.family = LsmFamily::SMALL;
        p.L = L;
        p.WP = wp;
        p.R = R;
        p.q = (V + L - 1) / L;
        p.lds_bytes = (size_t)R * V * sizeof(float) + (gather ? (size_t)R * 2 * sizeof(float) : 0);
        p.grid = lsm_stream_grid((rows + R - 1) / R);
        return p;
    }
    if (f.aligned && V % 4 == 0 && V <= LG_MAXV) {
        const int nvec = V >> 2;
        // Which rows an XCD streams (plain log-softmax only).  Workgroups go to the eight XCDs by blockIdx mod 8, so with
        // row = work item every XCD reads every eighth row of one moving front; with xcd each streams a contiguous
        // eighth of the tensor.  Measured (tools/lsm_rate.py, TB/s in + out, every-eighth / contiguous, 1.92 GB in; 8 GB
        // in brackets; profiles/r04_lsm_xcd_order_ab.txt): V=1500 5.9 / 6.2, 3000 6.0 / 6.2 [5.95 / 6.6], 5000 5.8-5.9 /
        // 6.0-6.5 [5.7 / 6.1], 7168 6.2 / 6.4, 8192 6.0-6.2 / 6.3-6.4 [5.8 / 6.2], 16384 5.2-5.4 / 6.0 [5.3 / 6.2];
        // nothing at 2048, 4096, 5120 ... 6144, 12288; WORSE for the three-pass covers of 2048 < V/4 <= 3072 (V=10000:
        // 6.0 / 5.6 [5.9 / 5.6]), which keep the plain order.
        // (fused gather / backward modes: no difference at c3 -- fused forward 0.3196 / 0.3184 / 0.3181 vs 0.3186 / 0.3178 /
        //  0.3190 ms -- so they keep the plain order)
        if (f.mode == LSM_NORM) p.xcd = k.lg_xcd >= 0 ? (k.lg_xcd != 0) : !(nvec > 2048 && nvec <= 3072);
        else p.xcd = k.lg_xcd_fused;
        p.family = LsmFamily::LARGE;
        p.grid = lsm_row_grid(rows, p.xcd);
        if (f.mode == LSM_NORM) {
            // The read + write stream wants about two float4 per thread and (nearly) every thread busy in every pass;
            // workgroups of 512 or 1024 threads (which tile a CU's 2048 exactly) beat the sizes in between.  Round 2
            // (profiles/r02_lsm_large_variants.txt, threads x passes, us for ~1.9 GB in + out): V=3000 256x3 734 /
            // 384x2 663; V=8192 256x8 687 / 1024x2 666; V=10000 512x5 870 / 1024x3 828-834 / 896x3 811; V=16384 512x8
            // 707 / 1024x4 723.  Re-swept in round 3 with the non-temporal policies in place
            // (profiles/r03_xcd_run_order_probe.txt part 3, profiles/r03_lg_cover_ab.txt; TB/s in + out): V=5000 640x2
            // 5.71 / 512x3 5.79-5.82 (c3 in bench.py: 0.696 -> 0.680 ms); V=5120 640x2 5.90 / 512x3 6.10; V=5600 768x2
            // 5.96 / 512x3 6.17; V=6144 768x2 6.23 / 512x3 5.99 / 1024x2 6.11; V=7168 896x2 5.90 / 1024x2 6.16.
            // The thread count is a template parameter on purpose (the same kernel with blockDim.x read at run
            // time: 780 us at V=5000).
            if (nvec > 3072) p.TH = 512, p.NV = 8;
            else if (nvec > 2048) p.TH = (nvec + 383) / 384 * 128, p.NV = 3;      // 768, 896, 1024
            else if (nvec > 1536) p.TH = 1024, p.NV = 2;
            else if (nvec > 1408) p.TH = 768, p.NV = 2;
            else if (nvec > 1024) p.TH = 512, p.NV = 3;
            else {
                const int th = (nvec + 255) / 256 * 128;                        // 256, 384, 512
                p.TH = th < 256 ? 256 : th;
                p.NV = 2;
            }
        } else {
            // read-mostly modes (fused gather, fused backward): the smallest cover, for the residency
            if (V <= 4096) p.TH = 256, p.NV = 4;
            else if (V <= 8192) p.TH = 256, p.NV = 8;
            else p.TH = 512, p.NV = 8;
        }
        return p;
    }
    p.family = LsmFamily::GENERIC;
    p.grid = (unsigned)((rows + 3) / 4);
    return p;
}

// launch_log_softmax_backward (lsm_backward.hip; fp32): the same three shapes -- SMALL (L, q, R, lds_bytes), LARGE (TH, NV,
// xcd), GENERIC.  aligned: dy, y and dx all start on 16 bytes.
inline LsmPlan plan_lsm_backward(int64_t rows, int V, bool aligned, const LsmKnobs& k) {
    LsmPlan p{};
    p.grid_y = p.grid_z = 1;
    if (aligned && V <= 1024) {
        int L = 1;
        while (L < 64 && L * 16 < V) L <<= 1;
        int R = (SMB_FLOATS / V) / 4 * 4;
        if (R < 4) R = 4;
        p.family = LsmFamily::SMALL;
        p.L = L;
        p.R = R;
        p.q = (V + L - 1) / L;
        p.lds_bytes = (size_t)R * V * sizeof(float) * 2;
        p.grid = lsm_stream_grid((rows + R - 1) / R);
        return p;
    }
    if (aligned && V % 4 == 0 && V <= LG_MAXV) {
        // every XCD streams a contiguous eighth of the rows (as the forward kernel): the reference's call chain with the
        // native log-softmax function at c3 2.08 / 2.07 / 2.03 -> 2.03 / 2.03 / 1.99 ms per training step
        p.family = LsmFamily::LARGE;
        p.xcd = k.bwd_xcd;
        p.grid = lsm_row_grid(rows, p.xcd);
        const int nvec = V >> 2;
        if (k.bwd_smallest_cover) {
            if (V <= 4096) p.TH = 256, p.NV = 4;
            else if (V <= 8192) p.TH = 256, p.NV = 8;
            else p.TH = 512, p.NV = 8;
        } else if (nvec > 3072) {
            p.TH = 512, p.NV = 8;
        } else {      // as the forward kernel: two or three passes, (nearly) every thread busy
            const int passes = nvec <= 2048 ? 2 : 3;
            const int th = (nvec + 128 * passes - 1) / (128 * passes) * 128;     // 256 ... 1024 x 2; 768, 896, 1024 x 3
            p.TH = th < 256 ? 256 : th;
            p.NV = passes;
        }
        return p;
    }
    p.family = LsmFamily::GENERIC;
    p.grid = (unsigned)((rows + 3) / 4);
    return p;
}

}  // namespace rnnt
#pragma GCC visibility pop
