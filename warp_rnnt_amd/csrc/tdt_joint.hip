// The joint network fused into the token-and-duration (TDT) loss (rnnt_amd_tdt_joint_loss / rnnt_amd_tdt_joint_backward,
// include/warp_rnnt_amd_tdt_joint.h): z[n,t,u,:] = W act(f[n,t] + g[n,u]) + b with W (V+D, H) --
// rows [0,V) the tokens, row V+i durations[i] -- is formed tile by tile with MFMA and never stored.  The forward writes
// the plane of 2 + D channels that tdt.hip's sweeps and gradient kernel read (they run unchanged behind it) and four floats
// of statistics per cell; the backward recomputes z and forms the TDT dz of include/warp_rnnt_amd_tdt.h, two softmaxes
// per row, in the accumulator registers.
//
// The three kernels are the walks of their twins in joint.hip over the unit of work of joint_tile.h.  What differs is the
// head: token rows v < V feed the online (max, sum) and the (blank, label) pick exactly as there; duration rows are kept
// apart.  Only the one or two 16-row blocks of W that hold duration rows (v0 + 16 > V) touch the duration state: the
// backward fetches (md, lsd) and G_dur there and nowhere else, so the blocks of token rows carry what joint.hip's carry.
#include "joint_tile.h"
#include "tdt.h"
#include "tdt_joint.h"

// every product and sum of the head is rounded on its own, as in tdt.hip (p S - G is not to become one fma)
#pragma clang fp contract(off)

namespace rnnt {

namespace {

// JointArgs with V = the rows of W (V tokens + D durations), pairs / lse / g2 unused
template <bool DROP> struct TdtJointArgs : jargs_t<DROP> {
    int Vt, D;             // token rows [0, Vt), duration rows [Vt, Vt + D)
    float sigma;
    float* plane;          // forward: 2 + D channels of `cells` floats, diagonal-major (tdt.h)
    float4* stats;         // (N,T,U): (m, ls, md, lsd), or nullptr (forward without gradients)
    const float* gplane;   // backward: G_b, G_l, G_dur[0..D) of k_tdt_grads
    size_t cells;
};

template <bool DROP> __device__ __forceinline__ int tdt_label_of(const TdtJointArgs<DROP>& a, int n, int u) {
    return u < a.U - 1 ? safe_label(a.labels[(size_t)n * (a.U - 1) + u], a.Vt, a.blank) : a.blank;
}
// the upstream gradient of utterance n (JointArgs::scale: the dropout arguments have a `scale` of their own in front of it)
__device__ __forceinline__ float upstream(const JointArgs& a, int n) { return a.scale ? a.scale[n] : 1.0f; }
// the diagonal-major address of cell (n,t,u): common.h, tdt.h
template <bool DROP> __device__ __forceinline__ size_t tdt_sk(const TdtJointArgs<DROP>& a, int n, int t, int u) {
    int d = t + u;
    d = d >= a.T ? d % a.T : d;
    return ((size_t)n * a.T + d) * a.U + u;
}

// ---------------------------------------------------------------------------------------------------------------------
// Forward: 4 frames x 4 labels per wave.  Token rows: online max / sum of exponentials per lane group, the normaliser kept
// as two floats (k_joint_fwd has the reasons); -inf contributes nothing.  Duration rows: the lane that owns row V+i keeps
// its logit, the four lane groups are combined by shuffle (the others hold +0, so the sum is the value), then every lane
// takes (max, log sum) in the order i = 0..D-1.
// ---------------------------------------------------------------------------------------------------------------------
template <typename E, int ACT, bool DROP>
__global__ void __launch_bounds__(WAVE * JWAVES) k_tdt_joint_fwd(TdtJointArgs<DROP> a) {
    extern __shared__ __align__(16) unsigned char j_lds[];
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x >> 6;
    const int tt = (a.T + 3) >> 2, tu = (a.U + 3) >> 2;
    const long item = (long)blockIdx.x * a.wpg + wave;
    if (item >= (long)a.N * tt * tu) return;
    const int n = (int)(item / ((long)tt * tu));
    const int rem = (int)(item - (long)n * tt * tu);
    const int t0 = (rem / tu) * 4, u0 = (rem - (rem / tu) * tu) * 4;
    const UttLens len = utt_lens<false>(a.xn, a.yn, n, a.T, a.U);
    const int c = lane & 15, q = lane >> 4;
    const int t = t0 + (c >> 2), u = u0 + (c & 3);
    const bool in_grid = t < a.T && u < a.U, live = t < len.Tn && u < len.Un;
    float tb = 0.0f, tl = 0.0f, dl[TDT_MAX_D];
#pragma unroll
    for (int i = 0; i < TDT_MAX_D; ++i) dl[i] = 0.0f;
    float4 st = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (t0 < len.Tn && u0 < len.Un) {
        E* hs = reinterpret_cast<E*>(j_lds) + (size_t)wave * 16 * hs_pitch<E>(a.H);
        unsigned long long seed = 0;
        if constexpr (DROP) seed = *a.seed;
        stage_h<E, ACT, DROP>(a, n, hs, [&](int cc, int& ct, int& cu) { ct = t0 + (cc >> 2); cu = u0 + (cc & 3); },
                              len.Tn, len.Un, lane, seed);
        const int lab = tdt_label_of(a, n, u < a.U ? u : a.U - 1);
        float m = -INFINITY, s = 0.0f, zb = 0.0f, zl = 0.0f, zd[TDT_MAX_D];
#pragma unroll
        for (int i = 0; i < TDT_MAX_D; ++i) zd[i] = 0.0f;
        for (int v0 = 0; v0 < a.V; v0 += 16) {
            const jf4 acc = z_block<E, false>(a, hs, 0, v0, lane);
            const bool durs = v0 + 16 > a.Vt;            // (the whole wave: the last one or two blocks)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int v = v0 + 4 * q + i;
                if (v < a.Vt) {
                    const float z = acc[i] + (a.bias ? a.bias[v] : 0.0f);
                    if (z > m) { s = s * expf(m - z) + 1.0f; m = z; } else if (z > -INFINITY) { s += expf(z - m); }
                    if (v == a.blank) zb = z;
                    if (v == lab) zl = z;
                } else if (durs && v < a.V) {
                    const float z = acc[i] + (a.bias ? a.bias[v] : 0.0f);
#pragma unroll
                    for (int k = 0; k < TDT_MAX_D; ++k) zd[k] = v - a.Vt == k ? z : zd[k];
                }
            }
        }
        // the four lane groups of a cell: max, rescaled sums (fixed order), and the one group that saw each entry
        float mall = m;
        mall = fmaxf(mall, __shfl_xor(mall, 16, WAVE));
        mall = fmaxf(mall, __shfl_xor(mall, 32, WAVE));
        float sc = m == -INFINITY ? 0.0f : s * expf(m - mall);
        sc += __shfl_xor(sc, 16, WAVE);
        sc += __shfl_xor(sc, 32, WAVE);
        const bool own_b = ((a.blank & 15) >> 2) == q, own_l = ((lab & 15) >> 2) == q;   // (v = v0 + 4q + i)
        float xb = own_b ? zb : 0.0f, xl = own_l ? zl : 0.0f;
        xb += __shfl_xor(xb, 16, WAVE);
        xb += __shfl_xor(xb, 32, WAVE);
        xl += __shfl_xor(xl, 16, WAVE);
        xl += __shfl_xor(xl, 32, WAVE);
        const float logsc = logf(sc);
#pragma unroll
        for (int k = 0; k < TDT_MAX_D; ++k) {
            if (k < a.D) {
                zd[k] += __shfl_xor(zd[k], 16, WAVE);
                zd[k] += __shfl_xor(zd[k], 32, WAVE);
            }
        }
        // (max, log sum) of the durations in the order i = 0..D-1 (tdt.hip: tdt_duration_stats)
        float md = -INFINITY, sd = 0.0f;
#pragma unroll
        for (int k = 0; k < TDT_MAX_D; ++k)
            if (k < a.D) md = fmaxf(md, zd[k]);
#pragma unroll
        for (int k = 0; k < TDT_MAX_D; ++k)
            if (k < a.D) sd += expf(zd[k] - md);
        const float lsd = logf(sd);
        if (live) {
            tb = ((xb - mall) - logsc) - a.sigma;
            tl = ((xl - mall) - logsc) - a.sigma;
#pragma unroll
            for (int k = 0; k < TDT_MAX_D; ++k) dl[k] = (zd[k] - md) - lsd;
            st = make_float4(mall, logsc, md, lsd);
        }
    }
    if (q == 0 && in_grid) {
        const size_t sk = tdt_sk(a, n, t, u);
        a.plane[sk] = tb;
        a.plane[a.cells + sk] = tl;
#pragma unroll
        for (int k = 0; k < TDT_MAX_D; ++k)
            if (k < a.D) a.plane[(size_t)(2 + k) * a.cells + sk] = dl[k];
        if (a.stats) a.stats[((size_t)n * a.T + t) * a.U + u] = st;
    }
}

// What the backward holds of a cell through every block of W: as joint.hip's CellGrad, G_b and G_l times the upstream
// gradient.  The duration side -- (md, lsd), G_dur, and the address and scale they are fetched with -- is NOT here.
struct TdtCell {
    bool live;
    float m, ls, gB, gL;
    int lab;
};
template <bool DROP>
__device__ __forceinline__ TdtCell tdt_cell(const TdtJointArgs<DROP>& a, int n, int t, int u, const UttLens& len) {
    TdtCell cg{t < len.Tn && u < len.Un, 0.0f, 0.0f, 0.0f, 0.0f, a.blank};
    if (cg.live) {
        const float s = upstream(a, n);
        const size_t sk = tdt_sk(a, n, t, u);
        cg.gB = a.gplane[sk] * s;
        cg.gL = a.gplane[a.cells + sk] * s;
        const float2 ml = *reinterpret_cast<const float2*>(a.stats + ((size_t)n * a.T + t) * a.U + u);
        cg.m = ml.x;
        cg.ls = ml.y;
        cg.lab = tdt_label_of(a, n, u);
    }
    return cg;
}
// dz of a token row: go (p S - [v == blank] G_b - [v == label] G_l)
__device__ __forceinline__ float tdt_dz_token(float z, int v, const TdtCell& cg, int blank) {
    float x = cell_prob(z, cg.m, cg.ls) * (cg.gB + cg.gL);
    x = v == blank ? x - cg.gB : x;
    x = v == cg.lab ? x - cg.gL : x;
    return x;
}

// dz of the 16x16 block `z` (rows v0 + 4q + i, column = this lane's cell (n,t,u))
template <bool DROP>
__device__ __forceinline__ jf4 tdt_dz_block(const TdtJointArgs<DROP>& a, jf4 z, int v0, int q, const TdtCell& cg, int n,
                                            int t, int u) {
    jf4 d;
    if (v0 + 16 <= a.Vt) {                        // token rows only (the whole wave)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int v = v0 + 4 * q + i;
            d[i] = cg.live ? tdt_dz_token(z[i] + (a.bias ? a.bias[v] : 0.0f), v, cg, a.blank) : 0.0f;
        }
        return d;
    }
    // a block with duration rows: their statistics and sums are fetched here
    float md = 0.0f, lsd = 0.0f, s = 1.0f;
    size_t sk = 0;
    if (cg.live) {
        const float4 st = a.stats[((size_t)n * a.T + t) * a.U + u];
        md = st.z;
        lsd = st.w;
        s = upstream(a, n);
        sk = tdt_sk(a, n, t, u);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int v = v0 + 4 * q + i;
        float x = 0.0f;
        if (cg.live && v < a.V) {
            const float zz = z[i] + (a.bias ? a.bias[v] : 0.0f);
            if (v < a.Vt) {
                x = tdt_dz_token(zz, v, cg, a.blank);
            } else {
                const float gd = a.gplane[(size_t)(2 + v - a.Vt) * a.cells + sk] * s;
                x = cell_prob(zz, md, lsd) * (cg.gB + cg.gL) - gd;
            }
        }
        d[i] = x;
    }
    return d;
}

// ---------------------------------------------------------------------------------------------------------------------
// Backward to f (SIDE_G = false) or g (true): k_joint_bwd_fg's walk.  Each row of df / dg is written once, by one wave.
// ---------------------------------------------------------------------------------------------------------------------
template <typename E, int ACT, bool SIDE_G, bool DROP>
__global__ void __launch_bounds__(WAVE * JWAVES) k_tdt_joint_bwd_fg(TdtJointArgs<DROP> a, E* out) {
    extern __shared__ __align__(16) unsigned char j_lds[];
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x >> 6;
    const int own_tiles = SIDE_G ? (a.U + 3) >> 2 : (a.T + 3) >> 2;
    const long item = (long)blockIdx.x * a.wpg + wave;
    if (item >= (long)a.N * own_tiles) return;
    const int n = (int)(item / own_tiles);
    const int o0 = (int)(item - (long)n * own_tiles) * 4;
    const UttLens len = utt_lens<false>(a.xn, a.yn, n, a.T, a.U);
    const int own_n = SIDE_G ? len.Un : len.Tn, walk_n = SIDE_G ? len.Tn : len.Un, rows = SIDE_G ? a.U : a.T;
    const int H = a.H, P = hs_pitch<E>(H), q = lane >> 4, c = lane & 15, nb = H >> 4;
    const E* WT = static_cast<const E*>(a.wt);
    E* hs = reinterpret_cast<E*>(j_lds) + (size_t)wave * 16 * P;
    unsigned long long seed = 0;
    if constexpr (DROP) seed = *a.seed;
    float acc[FG_MAXB];
#pragma unroll
    for (int b = 0; b < FG_MAXB; ++b) acc[b] = 0.0f;
    // cell cc of a tile: own index o0 + (cc >> 2), walked index w0 + (cc & 3)
    auto tu_of = [&](int cc, int w0, int& ct, int& cu) {
        const int own = o0 + (cc >> 2), walk = w0 + (cc & 3);
        ct = SIDE_G ? walk : own;
        cu = SIDE_G ? own : walk;
    };
    if (o0 < own_n) {
        for (int w0 = 0; w0 < walk_n; w0 += 4) {
            stage_h<E, ACT, DROP>(a, n, hs, [&](int cc, int& ct, int& cu) { tu_of(cc, w0, ct, cu); }, len.Tn, len.Un,
                                  lane, seed);
            int t, u;
            tu_of(c, w0, t, u);
            const TdtCell cg = tdt_cell(a, n, t, u, len);
            for (int v0 = 0; v0 < a.V; v0 += 16 * ZB<E>) {
                jf4 dz[ZB<E>];
#pragma unroll
                for (int zb = 0; zb < ZB<E>; ++zb) {
                    const jf4 z = z_block<E, false>(a, hs, 0, v0 + 16 * zb, lane);
                    dz[zb] = tdt_dz_block(a, z, v0 + 16 * zb, q, cg, n, t, u);
                }
                const jfrag_t<E> adz = pack_acc<E>(dz);
#pragma unroll
                for (int b = 0; b < FG_MAXB; ++b) {
                    if (b < nb) {
                        const int k = 16 * b + c;
                        jfrag_t<E> bw;
#pragma unroll
                        for (int j = 0; j < EPF<E>; ++j) bw[j] = WT[(size_t)k * a.Vp + v0 + b_slot(j, q)];
                        jf4 dh = {0.0f, 0.0f, 0.0f, 0.0f};
                        dh = mma_k<E>(adz, bw, dh);
                        // dh[r]: cell 4q + r, column k
                        float x = acc[b];
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            if constexpr (DROP) {
                                const E hv = hs[(4 * q + r) * P + k];
                                x += dh[r] * (dropped(hv) ? 0.0f : a.scale * act_bwd<ACT>((float)hv * a.keep));
                            } else {
                                x += dh[r] * act_bwd<ACT>((float)hs[(4 * q + r) * P + k]);
                            }
                        }
                        acc[b] = x;
                    }
                }
            }
            __builtin_amdgcn_wave_barrier();   // (the next tile restages hs)
        }
    }
    const int row = o0 + q;
    if (row < rows) {
        E* o = out + ((size_t)n * rows + row) * H;
        const bool zero = row >= own_n;
#pragma unroll
        for (int b = 0; b < FG_MAXB; ++b)
            if (b < nb) o[16 * b + c] = (E)(zero ? 0.0f : acc[b]);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Backward to W and b: k_joint_bwd_w's walk -- a unit owns a 16-row tile of the V + D rows, a 256-column H tile and a fixed
// range of cell groups; one fp32 result per split, summed in split order.  Split 0 writes its rows straight into dweight
// (nothing, where dweight is not asked for), splits 1.. into the partials dw_part[s - 1]: one partial of Vp x H floats less
// in the workspace, and the sum is the one k_joint_reduce_w forms, started from split 0's value.  Whether the unit's rows
// hold durations is a property of the unit (v0): only those units fetch the duration side of their cells.
// ---------------------------------------------------------------------------------------------------------------------
template <typename E, int ACT, bool DROP>
__global__ void __launch_bounds__(WAVE * JWAVES) k_tdt_joint_bwd_w(TdtJointArgs<DROP> a, int splits, long groups_per_split,
                                                                  float* dweight, float* dw_part, float* db_part) {
    extern __shared__ __align__(16) unsigned char j_lds[];
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x >> 6;
    const int vb = (a.V + 15) >> 4, ht = (a.H + HC_W - 1) / HC_W;
    const long item = (long)blockIdx.x * a.wpg + wave;
    if (item >= (long)vb * ht * splits) return;
    const int s = (int)(item % splits);
    const int h_tile = (int)((item / splits) % ht);
    const int v_tile = (int)(item / ((long)splits * ht));
    const int v0 = v_tile * 16, h0 = h_tile * HC_W;
    const bool durs = v0 + 16 > a.Vt;
    const int H = a.H, P = hs_pitch<E>(H), q = lane >> 4, c = lane & 15;
    const long cells = (long)a.N * a.T * a.U, groups = (cells + CG<E> - 1) / CG<E>;
    E* hs = reinterpret_cast<E*>(j_lds) + (size_t)wave * CG<E> * P;
    jf4 acc[HC_W / 16];
#pragma unroll
    for (int b = 0; b < HC_W / 16; ++b) acc[b] = jf4{0.0f, 0.0f, 0.0f, 0.0f};
    float db = 0.0f;
    unsigned long long seed = 0;
    if constexpr (DROP) seed = *a.seed;
    const long g_end = min(groups, (long)(s + 1) * groups_per_split);
    for (long gi = (long)s * groups_per_split; gi < g_end; ++gi) {
        const long cell0 = gi * CG<E>;
        // this lane's cells: 16 * zb + c; skip groups without a live cell
        bool any = false;
        TdtCell cgs[ZB<E>];
        size_t frow[ZB<E>], grow[ZB<E>];   // rows of f and g of cell 16 zb + c (the staging below fetches them by shuffle)
        [[maybe_unused]] int cn[ZB<E>], ct[ZB<E>], cu[ZB<E>];   // DROP: the cell itself, the mask's counter
        float cmd[ZB<E>], clsd[ZB<E>], csc[ZB<E>];              // durs: (md, lsd), the upstream gradient ...
        unsigned csk[ZB<E>];                                    // ... and the cell's address in a channel of gplane
#pragma unroll
        for (int zb = 0; zb < ZB<E>; ++zb) {
            const long cell = cell0 + 16 * zb + c;
            int n = 0, t = 0, u = 0;
            UttLens len{0, 0, false};
            if (cell < cells) {
                u = (int)(cell % a.U);
                const long fr = cell / a.U;
                t = (int)(fr % a.T);
                n = (int)(fr / a.T);
                len = utt_lens<false>(a.xn, a.yn, n, a.T, a.U);
            }
            cgs[zb] = cell < cells ? tdt_cell(a, n, t, u, len) : TdtCell{false, 0.0f, 0.0f, 0.0f, 0.0f, a.blank};
            frow[zb] = (size_t)n * a.T + t;
            grow[zb] = (size_t)n * a.U + u;
            if constexpr (DROP) { cn[zb] = n; ct[zb] = t; cu[zb] = u; }
            cmd[zb] = clsd[zb] = 0.0f;
            csc[zb] = 1.0f;
            csk[zb] = 0u;
            if (durs && cgs[zb].live) {
                const float4 st = a.stats[cell];
                cmd[zb] = st.z;
                clsd[zb] = st.w;
                csc[zb] = upstream(a, n);
                csk[zb] = (unsigned)tdt_sk(a, n, t, u);      // (cells < 2^32: the C ABI's dims_ok)
            }
            any |= cgs[zb].live;
        }
        if (__ballot(any) == 0) continue;
        // stage the group's activations: rows 16 * zb + cc
#pragma unroll
        for (int zb = 0; zb < ZB<E>; ++zb) {
            E* hz = hs + 16 * zb * P;
            // (per-cell rows and liveness from the lane that holds the cell: a group may straddle utterances)
            const E* f = static_cast<const E*>(a.f);
            const E* g = static_cast<const E*>(a.g);
            const int H4 = H >> 2;
            for (int i = lane; i < 16 * H4; i += WAVE) {
                const int cc = i / H4, k = (i - cc * H4) * 4;
                const bool live = __shfl((int)cgs[zb].live, cc, WAVE) != 0;
                const size_t fr = __shfl((unsigned long long)frow[zb], cc, WAVE);
                const size_t gr = __shfl((unsigned long long)grow[zb], cc, WAVE);
                [[maybe_unused]] int dn = 0, dt = 0, du = 0;
                if constexpr (DROP) {
                    dn = __shfl(cn[zb], cc, WAVE);
                    dt = __shfl(ct[zb], cc, WAVE);
                    du = __shfl(cu[zb], cc, WAVE);
                }
                float o[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                [[maybe_unused]] unsigned m = 15u;
                if (live) {
                    const E* fp = f + fr * H + k;
                    const E* gp = g + gr * H + k;
#pragma unroll
                    for (int j = 0; j < 4; ++j) o[j] = act_fwd<ACT>((float)fp[j] + (float)gp[j]);
                    if constexpr (DROP) m = drop4(a, seed, dn, dt, du, k >> 2, o);
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if constexpr (DROP)
                        hz[cc * P + k + j] = drop_stage<E>(o[j], (m >> j) & 1u);
                    else
                        hz[cc * P + k + j] = (E)o[j];
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        // z with rows = cells (lane: column v = v0 + c, cells 16 zb + 4q + r); dz needs each cell's values, which sit in
        // the lane of the cell's column: fetch them by shuffle (cell 16 zb + 4q + r lives in lane c' = 4q + r)
        jf4 dz[ZB<E>];
#pragma unroll
        for (int zb = 0; zb < ZB<E>; ++zb) {
            const jf4 z = z_block<E, true>(a, hs, 16 * zb, v0, lane);
            const int v = v0 + c;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int src = 4 * q + r;
                TdtCell cg;
                cg.m = __shfl(cgs[zb].m, src, WAVE);
                cg.ls = __shfl(cgs[zb].ls, src, WAVE);
                cg.gB = __shfl(cgs[zb].gB, src, WAVE);
                cg.gL = __shfl(cgs[zb].gL, src, WAVE);
                cg.lab = __shfl(cgs[zb].lab, src, WAVE);
                cg.live = __shfl((int)cgs[zb].live, src, WAVE) != 0;
                float x = 0.0f;
                if (!durs) {
                    if (cg.live) x = tdt_dz_token(z[r] + (a.bias ? a.bias[v] : 0.0f), v, cg, a.blank);
                } else {
                    const float md = __shfl(cmd[zb], src, WAVE), lsd = __shfl(clsd[zb], src, WAVE);
                    const float sc = __shfl(csc[zb], src, WAVE);
                    const unsigned sk = __shfl(csk[zb], src, WAVE);
                    if (cg.live && v < a.V) {
                        const float zz = z[r] + (a.bias ? a.bias[v] : 0.0f);
                        if (v < a.Vt) {
                            x = tdt_dz_token(zz, v, cg, a.blank);
                        } else {
                            const float gd = a.gplane[(size_t)(2 + v - a.Vt) * a.cells + sk] * sc;
                            x = cell_prob(zz, md, lsd) * (cg.gB + cg.gL) - gd;
                        }
                    }
                }
                dz[zb][r] = x;
                db += x;
            }
        }
        // dW[v][k] += sum_cells dz[cell][v] h[cell][k]: A = dz^T (row v = lane column, K slots = the cells of its
        // registers), B = h rows in the same slot order
        const jfrag_t<E> adz = pack_acc<E>(dz);
#pragma unroll
        for (int b = 0; b < HC_W / 16; ++b) {
            const int k = h0 + 16 * b + c;
            if (h0 + 16 * b < H) {
                jfrag_t<E> bh;
#pragma unroll
                for (int j = 0; j < EPF<E>; ++j) bh[j] = hs[b_slot(j, q) * P + k];
                acc[b] = mma_k<E>(adz, bh, acc[b]);
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
    // the result of split s: rows v0 + 4q + r, columns h0 + 16 b + c.  dweight has V + D rows and no padding; a partial Vp
    float* dp = s == 0 ? dweight : dw_part + (size_t)(s - 1) * a.Vp * H;
    const int row_end = s == 0 ? a.V : a.Vp;
    if (dp) {
#pragma unroll
        for (int b = 0; b < HC_W / 16; ++b) {
            if (h0 + 16 * b < H) {
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (v0 + 4 * q + r < row_end) dp[(size_t)(v0 + 4 * q + r) * H + h0 + 16 * b + c] = acc[b][r];
            }
        }
    }
    if (h_tile == 0) {
        db += __shfl_xor(db, 16, WAVE);
        db += __shfl_xor(db, 32, WAVE);
        if (q == 0) db_part[(size_t)s * a.Vp + v0 + c] = db;
    }
}

// dweight += the partials of splits 1.. in split order (split 0 is in it); dbias = the sum of all splits' in split order
__global__ void k_tdt_joint_reduce_w(const float* __restrict__ dw_part, const float* __restrict__ db_part, int splits, int V,
                                     int Vp, int H, float* dweight, float* dbias) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long vh = (long)V * H;
    if (dweight && splits > 1 && i < vh) {
        float x = dweight[i];
        for (int s = 1; s < splits; ++s) x += dw_part[(size_t)(s - 1) * Vp * H + i];
        dweight[i] = x;
    }
    if (dbias && i < V) {
        float x = 0.0f;
        for (int s = 0; s < splits; ++s) x += db_part[(size_t)s * Vp + i];
        dbias[i] = x;
    }
}

template <typename E, int ACT, bool DROP> hipError_t fwd_typed(hipStream_t stream, TdtJointArgs<DROP> a) {
    a.wpg = waves_per_group<E>(16, a.H);
    const long items = (long)a.N * ((a.T + 3) / 4) * ((a.U + 3) / 4);
    const size_t lds = (size_t)a.wpg * 16 * (a.H + EPF<E>) * sizeof(E);
    k_tdt_joint_fwd<E, ACT, DROP><<<blocks_for(items, a.wpg), WAVE * a.wpg, lds, stream>>>(a);
    return hipGetLastError();
}

template <typename E, int ACT, bool DROP>
hipError_t bwd_typed(hipStream_t stream, TdtJointArgs<DROP> a, void* wt, float* dw_part, float* db_part, int splits,
                     void* df, void* dg, float* dweight, float* dbias) {
    // (wt may share its storage with dw_part: the two kernels that read it run in front of the one that writes the partials)
    const long tw = (long)a.H * a.Vp;
    k_joint_transpose_w<E><<<(unsigned)((tw + 255) / 256), 256, 0, stream>>>(static_cast<const E*>(a.w),
                                                                             static_cast<E*>(wt), a.V, a.Vp, a.H);
    a.wt = wt;
    a.wpg = waves_per_group<E>(16, a.H);
    const size_t lds = (size_t)a.wpg * 16 * (a.H + EPF<E>) * sizeof(E);
    if (df) {
        const long items = (long)a.N * ((a.T + 3) / 4);
        k_tdt_joint_bwd_fg<E, ACT, false, DROP><<<blocks_for(items, a.wpg), WAVE * a.wpg, lds, stream>>>(
            a, static_cast<E*>(df));
    }
    if (dg) {
        const long items = (long)a.N * ((a.U + 3) / 4);
        k_tdt_joint_bwd_fg<E, ACT, true, DROP><<<blocks_for(items, a.wpg), WAVE * a.wpg, lds, stream>>>(
            a, static_cast<E*>(dg));
    }
    if (dweight || dbias) {
        TdtJointArgs<DROP> b = a;
        b.wpg = waves_per_group<E>(CG<E>, a.H);
        const size_t lw = (size_t)b.wpg * CG<E> * (a.H + EPF<E>) * sizeof(E);
        const long cells = (long)a.N * a.T * a.U, groups = (cells + CG<E> - 1) / CG<E>;
        const long per = (groups + splits - 1) / splits;
        const long items = (long)((a.V + 15) / 16) * ((a.H + HC_W - 1) / HC_W) * splits;
        k_tdt_joint_bwd_w<E, ACT, DROP><<<blocks_for(items, b.wpg), WAVE * b.wpg, lw, stream>>>(b, splits, per, dweight,
                                                                                              dw_part, db_part);
        const long vh = (long)a.V * a.H;
        k_tdt_joint_reduce_w<<<(unsigned)((vh + 255) / 256), 256, 0, stream>>>(dw_part, db_part, splits, a.V, a.Vp, a.H,
                                                                               dweight, dbias);
    }
    return hipGetLastError();
}

template <bool DROP> hipError_t fwd_drop(hipStream_t stream, int dtype, int act, const TdtJointArgs<DROP>& a) {
    const bool tanh_ = act == RNNT_ACT_TANH;
#define RNNT_TDT_JOINT_FWD(E, A) fwd_typed<E, A, DROP>(stream, a)
    switch (dtype) {
        case RNNT_DTYPE_F32:
            return tanh_ ? RNNT_TDT_JOINT_FWD(float, RNNT_ACT_TANH) : RNNT_TDT_JOINT_FWD(float, RNNT_ACT_RELU);
        case RNNT_DTYPE_BF16:
            return tanh_ ? RNNT_TDT_JOINT_FWD(__bf16, RNNT_ACT_TANH) : RNNT_TDT_JOINT_FWD(__bf16, RNNT_ACT_RELU);
        case RNNT_DTYPE_F16:
            return tanh_ ? RNNT_TDT_JOINT_FWD(_Float16, RNNT_ACT_TANH) : RNNT_TDT_JOINT_FWD(_Float16, RNNT_ACT_RELU);
        default: return hipErrorInvalidValue;
    }
#undef RNNT_TDT_JOINT_FWD
}

template <bool DROP>
hipError_t bwd_drop(hipStream_t stream, int dtype, int act, const TdtJointArgs<DROP>& a, void* wt, float* dw_part,
                    float* db_part, int splits, void* df, void* dg, float* dweight, float* dbias) {
    const bool tanh_ = act == RNNT_ACT_TANH;
#define RNNT_TDT_JOINT_BWD(E, A) bwd_typed<E, A, DROP>(stream, a, wt, dw_part, db_part, splits, df, dg, dweight, dbias)
    switch (dtype) {
        case RNNT_DTYPE_F32:
            return tanh_ ? RNNT_TDT_JOINT_BWD(float, RNNT_ACT_TANH) : RNNT_TDT_JOINT_BWD(float, RNNT_ACT_RELU);
        case RNNT_DTYPE_BF16:
            return tanh_ ? RNNT_TDT_JOINT_BWD(__bf16, RNNT_ACT_TANH) : RNNT_TDT_JOINT_BWD(__bf16, RNNT_ACT_RELU);
        case RNNT_DTYPE_F16:
            return tanh_ ? RNNT_TDT_JOINT_BWD(_Float16, RNNT_ACT_TANH) : RNNT_TDT_JOINT_BWD(_Float16, RNNT_ACT_RELU);
        default: return hipErrorInvalidValue;
    }
#undef RNNT_TDT_JOINT_BWD
}

inline bool tdt_joint_rows_ok(int H, int V, int D, int blank) {
    return H >= 32 && H <= 1024 && H % 32 == 0 && V >= 2 && D >= 1 && D <= TDT_MAX_D && blank >= 0 && blank < V;
}

template <bool DROP>
TdtJointArgs<DROP> tdt_args(const JointArgs& base, float p, const uint64_t* seed, int V, int D, float sigma, float* plane,
                            float* stats, const float* gplane) {
    TdtJointArgs<DROP> a{};
    static_cast<jargs_t<DROP>&>(a) = drop_args<DROP>(base, p, seed);
    a.Vt = V;
    a.D = D;
    a.sigma = sigma;
    a.plane = plane;
    a.stats = reinterpret_cast<float4*>(stats);
    a.gplane = gplane;
    a.cells = (size_t)base.N * base.T * base.U;
    return a;
}

}  // namespace

hipError_t launch_tdt_joint_fwd(hipStream_t stream, int dtype, int act, const void* f, const void* g, const void* w,
                                const float* bias, const int* labels, const int* xn, const int* yn, float* plane,
                                float* stats, int N, int T, int U, int H, int V, int D, int blank, float sigma, float p,
                                const uint64_t* seed) {
    if (!tdt_joint_rows_ok(H, V, D, blank)) return hipErrorInvalidValue;
    if (N == 0) return hipSuccess;
    const JointArgs base{f, g, w, nullptr, bias, labels, xn, yn, nullptr, nullptr, nullptr, nullptr,
                         N, T, U, H, V + D, joint_vpad(V + D), blank, 1};
    return p > 0.0f ? fwd_drop<true>(stream, dtype, act, tdt_args<true>(base, p, seed, V, D, sigma, plane, stats, nullptr))
                    : fwd_drop<false>(stream, dtype, act,
                                      tdt_args<false>(base, p, seed, V, D, sigma, plane, stats, nullptr));
}

hipError_t launch_tdt_joint_bwd(hipStream_t stream, int dtype, int act, const void* f, const void* g, const void* w,
                                const float* bias, const int* labels, const int* xn, const int* yn, const float* stats,
                                const float* gplane, const float* grad_costs, void* wt, float* dw_part, float* db_part,
                                int splits, void* df, void* dg, float* dweight, float* dbias, int N, int T, int U, int H,
                                int V, int D, int blank, float p, const uint64_t* seed) {
    if (!tdt_joint_rows_ok(H, V, D, blank)) return hipErrorInvalidValue;
    if (N == 0) return hipSuccess;
    const JointArgs base{f, g, w, nullptr, bias, labels, xn, yn, nullptr, grad_costs, nullptr, nullptr,
                         N, T, U, H, V + D, joint_vpad(V + D), blank, 1};
    float* st = const_cast<float*>(stats);
    return p > 0.0f ? bwd_drop<true>(stream, dtype, act,
                                     tdt_args<true>(base, p, seed, V, D, 0.0f, nullptr, st, gplane), wt, dw_part,
                                     db_part, splits, df, dg, dweight, dbias)
                    : bwd_drop<false>(stream, dtype, act,
                                      tdt_args<false>(base, p, seed, V, D, 0.0f, nullptr, st, gplane), wt, dw_part,
                                      db_part, splits, df, dg, dweight, dbias);
}

}  // namespace rnnt
