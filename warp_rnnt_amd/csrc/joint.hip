// The joint network fused into the loss (rnnt_amd_joint_loss / rnnt_amd_joint_backward, include/warp_rnnt_amd.h):
// z[n,t,u,:] = W act(f[n,t] + g[n,u]) + b is formed tile by tile with MFMA and never stored; neither act(f+g) (N,T,U,H)
// nor z (N,T,U,V) exists in memory.  DESIGN.md section 3.9.
//
// Every kernel here is built from the unit of work of joint_tile.h -- one wave, sixteen cells, h staged in LDS, two MFMA
// products -- which tdt_joint.hip shares.
#include "joint_tile.h"

namespace rnnt {

namespace {

__device__ __forceinline__ int label_of(const JointArgs& a, int n, int u) {
    return u < a.U - 1 ? safe_label(a.labels[(size_t)n * (a.U - 1) + u], a.V, a.blank) : a.blank;
}

// ---------------------------------------------------------------------------------------------------------------------
// Forward: 4 frames x 4 labels per wave; online max / sum of exponentials per cell, (blank, label) log-probs into the
// diagonal-major pair plane at launch_log_softmax_gather_skewed's addresses, (mall, log sc) per cell.
// The log-normaliser is never formed as ONE float: mall + log sc rounds at ulp(mall) (4e-3 at a bias of 60000), and a
// log-softmax must not change under a shift of its row.  Log-probs are (z - mall) - log sc, the backward's exponent the
// same.  A logit of -inf (a masked vocabulary entry) contributes nothing to max or sum, also
// when it comes before the first finite one; a row needs one finite logit.
// ---------------------------------------------------------------------------------------------------------------------
template <typename E, int ACT, bool DROP>
__global__ void __launch_bounds__(WAVE * JWAVES) k_joint_fwd(jargs_t<DROP> a) {
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
    float2 pair = make_float2(0.0f, 0.0f);
    float2 lse = make_float2(0.0f, 0.0f);
    if (t0 < len.Tn && u0 < len.Un) {
        E* hs = reinterpret_cast<E*>(j_lds) + (size_t)wave * 16 * hs_pitch<E>(a.H);
        unsigned long long seed = 0;
        if constexpr (DROP) seed = *a.seed;
        stage_h<E, ACT, DROP>(a, n, hs, [&](int cc, int& ct, int& cu) { ct = t0 + (cc >> 2); cu = u0 + (cc & 3); },
                              len.Tn, len.Un, lane, seed);
        const int lab = label_of(a, n, u < a.U ? u : a.U - 1);
        float m = -INFINITY, s = 0.0f, zb = 0.0f, zl = 0.0f;
        for (int v0 = 0; v0 < a.V; v0 += 16) {
            const jf4 acc = z_block<E, false>(a, hs, 0, v0, lane);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int v = v0 + 4 * q + i;
                if (v < a.V) {
                    const float z = acc[i] + (a.bias ? a.bias[v] : 0.0f);
                    if (z > m) { s = s * expf(m - z) + 1.0f; m = z; } else if (z > -INFINITY) { s += expf(z - m); }
                    if (v == a.blank) zb = z;
                    if (v == lab) zl = z;
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
        if (live) {
            pair = make_float2((xb - mall) - logsc, (xl - mall) - logsc);
            lse = make_float2(mall, logsc);
        }
    }
    if (q == 0 && in_grid) {
        int d = t + u;
        d = d >= a.T ? d % a.T : d;
        a.pairs[((size_t)n * a.T + d) * a.U + u] = pair;
        if (a.lse) a.lse[((size_t)n * a.T + t) * a.U + u] = lse;
    }
}

// dz of the 16x16 block `z` (rows v0 + 4q + i, column = this lane's cell): the LSM_BWD formula of lsm.h.
__device__ __forceinline__ jf4 dz_block(const JointArgs& a, jf4 z, int v0, int q, bool live, float mall, float logsc,
                                        float gB, float gL, int lab) {
    jf4 d;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int v = v0 + 4 * q + i;
        float x = 0.0f;
        if (live && v < a.V) {
            const float p = cell_prob(z[i] + (a.bias ? a.bias[v] : 0.0f), mall, logsc);
            x = (v == a.blank ? gB : 0.0f) + (v == lab ? gL : 0.0f) - p * (gB + gL);
        }
        d[i] = x;
    }
    return d;
}

struct CellGrad {
    bool live;
    float mall, logsc, gB, gL;   // (the forward's pair: cell_prob)
    int lab;
};
__device__ __forceinline__ CellGrad cell_grad(const JointArgs& a, int n, int t, int u, const UttLens& len) {
    CellGrad cg{t < len.Tn && u < len.Un, 0.0f, 0.0f, 0.0f, 0.0f, a.blank};
    if (cg.live) {
        const float s = a.scale ? a.scale[n] : 1.0f;
        int d = t + u;
        d = d >= a.T ? d % a.T : d;
        const float2 p = a.g2[((size_t)n * a.T + d) * a.U + u];
        cg.gB = p.x * s;
        cg.gL = p.y * s;
        const float2 ml = a.lse[((size_t)n * a.T + t) * a.U + u];
        cg.mall = ml.x;
        cg.logsc = ml.y;
        cg.lab = label_of(a, n, u);
    }
    return cg;
}

// ---------------------------------------------------------------------------------------------------------------------
// Backward to f (SIDE_G = false) or g (true).  A wave owns 4 frames (4 labels) and walks all the utterance's label
// (frame) tiles in order; per tile and V chunk: z, dz, dh = dz W_chunk (MFMA, rows = cells, so lane group q holds the
// wave's own index q and the 4 registers the walked index), then out[q][k] += sum_r dh[r][k] act'(h[4q+r][k]) in
// registers.  Each row of df / dg is written once, by one wave; its bits depend on the utterance's own lengths only.
// ---------------------------------------------------------------------------------------------------------------------
// DROP: d/d(f+g) = dh m scale act'(y), y = h~ / scale recovered from the staged value as h~ (1 - p); m from the sign of a
// staged zero (dropped; never from h~ == 0: a kept tanh(0) has derivative scale).
template <typename E, int ACT, bool SIDE_G, bool DROP>
__global__ void __launch_bounds__(WAVE * JWAVES) k_joint_bwd_fg(jargs_t<DROP> a, E* out) {
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
            const CellGrad cg = cell_grad(a, n, t, u, len);
            for (int v0 = 0; v0 < a.V; v0 += 16 * ZB<E>) {
                jf4 dz[ZB<E>];
#pragma unroll
                for (int zb = 0; zb < ZB<E>; ++zb) {
                    const jf4 z = z_block<E, false>(a, hs, 0, v0 + 16 * zb, lane);
                    dz[zb] = dz_block(a, z, v0 + 16 * zb, q, cg.live, cg.mall, cg.logsc, cg.gB, cg.gL, cg.lab);
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
// Backward to W and b: a unit owns a 16-row V tile, a 256-column H tile and a fixed range of cell groups (split-K over
// cells); per group: z (rows = cells, column = v), dz, dW_tile += dz^T h (MFMA), db_tile += sum dz.  One fp32 partial per
// split, reduced in split order by k_joint_reduce_w.  The split count is a function of the shape only.
// ---------------------------------------------------------------------------------------------------------------------
template <typename E, int ACT, bool DROP>
__global__ void __launch_bounds__(WAVE * JWAVES) k_joint_bwd_w(jargs_t<DROP> a, int splits, long groups_per_split,
                                                              float* dw_part, float* db_part) {
    extern __shared__ __align__(16) unsigned char j_lds[];
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x >> 6;
    const int vb = (a.V + 15) >> 4, ht = (a.H + HC_W - 1) / HC_W;
    const long item = (long)blockIdx.x * a.wpg + wave;
    if (item >= (long)vb * ht * splits) return;
    const int s = (int)(item % splits);
    const int h_tile = (int)((item / splits) % ht);
    const int v_tile = (int)(item / ((long)splits * ht));
    const int v0 = v_tile * 16, h0 = h_tile * HC_W;
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
        CellGrad cgs[ZB<E>];
        size_t frow[ZB<E>], grow[ZB<E>];   // rows of f and g of cell 16 zb + c (the staging below fetches them by shuffle)
        [[maybe_unused]] int cn[ZB<E>], ct[ZB<E>], cu[ZB<E>];   // DROP: the cell itself, the mask's counter
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
            cgs[zb] = cell < cells ? cell_grad(a, n, t, u, len) : CellGrad{false, 0.0f, 0.0f, 0.0f, 0.0f, a.blank};
            frow[zb] = (size_t)n * a.T + t;
            grow[zb] = (size_t)n * a.U + u;
            if constexpr (DROP) { cn[zb] = n; ct[zb] = t; cu[zb] = u; }
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
                const float mall = __shfl(cgs[zb].mall, src, WAVE), logsc = __shfl(cgs[zb].logsc, src, WAVE);
                const float gB = __shfl(cgs[zb].gB, src, WAVE), gL = __shfl(cgs[zb].gL, src, WAVE);
                const int lab = __shfl(cgs[zb].lab, src, WAVE);
                const bool live = __shfl((int)cgs[zb].live, src, WAVE) != 0;
                float x = 0.0f;
                if (live && v < a.V) {
                    const float p = cell_prob(z[r] + (a.bias ? a.bias[v] : 0.0f), mall, logsc);
                    x = (v == a.blank ? gB : 0.0f) + (v == lab ? gL : 0.0f) - p * (gB + gL);
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
    // partial of split s: rows v0 + 4q + r, columns h0 + 16 b + c
    float* dp = dw_part + (size_t)s * a.Vp * H;
#pragma unroll
    for (int b = 0; b < HC_W / 16; ++b) {
        if (h0 + 16 * b < H) {
#pragma unroll
            for (int r = 0; r < 4; ++r) dp[(size_t)(v0 + 4 * q + r) * H + h0 + 16 * b + c] = acc[b][r];
        }
    }
    if (h_tile == 0) {
        db += __shfl_xor(db, 16, WAVE);
        db += __shfl_xor(db, 32, WAVE);
        if (q == 0) db_part[(size_t)s * a.Vp + v0 + c] = db;
    }
}

template <typename E, int ACT, bool DROP> hipError_t fwd_typed(hipStream_t stream, jargs_t<DROP> a) {
    a.wpg = waves_per_group<E>(16, a.H);
    const long items = (long)a.N * ((a.T + 3) / 4) * ((a.U + 3) / 4);
    const size_t lds = (size_t)a.wpg * 16 * (a.H + EPF<E>) * sizeof(E);
    k_joint_fwd<E, ACT, DROP><<<blocks_for(items, a.wpg), WAVE * a.wpg, lds, stream>>>(a);
    return hipGetLastError();
}

template <typename E, int ACT, bool DROP>
hipError_t bwd_typed(hipStream_t stream, jargs_t<DROP> a, void* wt, float* dw_part, float* db_part, int splits, void* df,
                     void* dg, float* dweight, float* dbias) {
    const long tw = (long)a.H * a.Vp;
    k_joint_transpose_w<E><<<(unsigned)((tw + 255) / 256), 256, 0, stream>>>(static_cast<const E*>(a.w),
                                                                             static_cast<E*>(wt), a.V, a.Vp, a.H);
    a.wt = wt;
    a.wpg = waves_per_group<E>(16, a.H);
    const size_t lds = (size_t)a.wpg * 16 * (a.H + EPF<E>) * sizeof(E);
    if (df) {
        const long items = (long)a.N * ((a.T + 3) / 4);
        k_joint_bwd_fg<E, ACT, false, DROP><<<blocks_for(items, a.wpg), WAVE * a.wpg, lds, stream>>>(
            a, static_cast<E*>(df));
    }
    if (dg) {
        const long items = (long)a.N * ((a.U + 3) / 4);
        k_joint_bwd_fg<E, ACT, true, DROP><<<blocks_for(items, a.wpg), WAVE * a.wpg, lds, stream>>>(
            a, static_cast<E*>(dg));
    }
    if (dweight || dbias) {
        jargs_t<DROP> b = a;
        b.wpg = waves_per_group<E>(CG<E>, a.H);
        const size_t lw = (size_t)b.wpg * CG<E> * (a.H + EPF<E>) * sizeof(E);
        const long cells = (long)a.N * a.T * a.U, groups = (cells + CG<E> - 1) / CG<E>;
        const long per = (groups + splits - 1) / splits;
        const long items = (long)((a.V + 15) / 16) * ((a.H + HC_W - 1) / HC_W) * splits;
        k_joint_bwd_w<E, ACT, DROP><<<blocks_for(items, b.wpg), WAVE * b.wpg, lw, stream>>>(b, splits, per, dw_part,
                                                                                          db_part);
        const long vh = (long)a.V * a.H;
        k_joint_reduce_w<<<(unsigned)((vh + 255) / 256), 256, 0, stream>>>(dw_part, db_part, splits, a.V, a.Vp, a.H,
                                                                           dweight, dbias);
    }
    return hipGetLastError();
}

template <bool DROP> hipError_t fwd_drop(hipStream_t stream, int dtype, int act, jargs_t<DROP> a) {
    const bool tanh_ = act == RNNT_ACT_TANH;
#define RNNT_JOINT_FWD(E, A) fwd_typed<E, A, DROP>(stream, a)
    switch (dtype) {
        case RNNT_DTYPE_F32: return tanh_ ? RNNT_JOINT_FWD(float, RNNT_ACT_TANH) : RNNT_JOINT_FWD(float, RNNT_ACT_RELU);
        case RNNT_DTYPE_BF16: return tanh_ ? RNNT_JOINT_FWD(__bf16, RNNT_ACT_TANH) : RNNT_JOINT_FWD(__bf16, RNNT_ACT_RELU);
        default: return tanh_ ? RNNT_JOINT_FWD(_Float16, RNNT_ACT_TANH) : RNNT_JOINT_FWD(_Float16, RNNT_ACT_RELU);
    }
#undef RNNT_JOINT_FWD
}

template <bool DROP>
hipError_t bwd_drop(hipStream_t stream, int dtype, int act, jargs_t<DROP> a, void* wt, float* dw_part, float* db_part,
                    int splits, void* df, void* dg, float* dweight, float* dbias) {
    const bool tanh_ = act == RNNT_ACT_TANH;
#define RNNT_JOINT_BWD(E, A) bwd_typed<E, A, DROP>(stream, a, wt, dw_part, db_part, splits, df, dg, dweight, dbias)
    switch (dtype) {
        case RNNT_DTYPE_F32: return tanh_ ? RNNT_JOINT_BWD(float, RNNT_ACT_TANH) : RNNT_JOINT_BWD(float, RNNT_ACT_RELU);
        case RNNT_DTYPE_BF16: return tanh_ ? RNNT_JOINT_BWD(__bf16, RNNT_ACT_TANH) : RNNT_JOINT_BWD(__bf16, RNNT_ACT_RELU);
        default: return tanh_ ? RNNT_JOINT_BWD(_Float16, RNNT_ACT_TANH) : RNNT_JOINT_BWD(_Float16, RNNT_ACT_RELU);
    }
#undef RNNT_JOINT_BWD
}

}  // namespace

int joint_vpad(int V) { return (V + WT_PITCH - 1) / WT_PITCH * WT_PITCH; }

// Splits of the weight kernel over cell groups: about 1024 units in all, never more groups than there are
int joint_w_splits(int N, int T, int U, int H, int V, int dtype) {
    const int cg = dtype == RNNT_DTYPE_F32 ? 16 : 32;
    const long groups = ((long)N * T * U + cg - 1) / cg;
    const long tiles = (long)((V + 15) / 16) * ((H + HC_W - 1) / HC_W);
    long s = (1024 + tiles - 1) / tiles;
    if (s > 256) s = 256;
    if (s > groups) s = groups;
    return s < 1 ? 1 : (int)s;
}

// p > 0: the dropout kernels with the mask of (seed, p) (philox.h; seed a device word); p == 0: the kernels without
hipError_t launch_joint_fwd(hipStream_t stream, int dtype, int act, const void* f, const void* g, const void* w,
                            const float* bias, const int* labels, const int* xn, const int* yn, float* pairs,
                            float* lse, int N, int T, int U, int H, int V, int blank, float p, const uint64_t* seed) {
    JointArgs a{f, g, w, nullptr, bias, labels, xn, yn, nullptr, nullptr, reinterpret_cast<float2*>(pairs),
                reinterpret_cast<float2*>(lse), N, T, U, H, V, joint_vpad(V), blank, 1};
    return p > 0.0f ? fwd_drop<true>(stream, dtype, act, drop_args<true>(a, p, seed))
                    : fwd_drop<false>(stream, dtype, act, a);
}

hipError_t launch_joint_bwd(hipStream_t stream, int dtype, int act, const void* f, const void* g, const void* w,
                            const float* bias, const int* labels, const int* xn, const int* yn, const float* lse,
                            const float* grads, const float* grad_costs, void* wt, float* dw_part, float* db_part,
                            int splits, void* df, void* dg, float* dweight, float* dbias, int N, int T, int U, int H,
                            int V, int blank, float p, const uint64_t* seed) {
    JointArgs a{f, g, w, nullptr, bias, labels, xn, yn, reinterpret_cast<const float2*>(grads), grad_costs, nullptr,
                reinterpret_cast<float2*>(const_cast<float*>(lse)), N, T, U, H, V, joint_vpad(V), blank, 1};
    return p > 0.0f ? bwd_drop<true>(stream, dtype, act, drop_args<true>(a, p, seed), wt, dw_part, db_part, splits, df,
                                     dg, dweight, dbias)
                    : bwd_drop<false>(stream, dtype, act, a, wt, dw_part, db_part, splits, df, dg, dweight, dbias);
}

}  // namespace rnnt
