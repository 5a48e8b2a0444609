// Body of the large log-softmax kernel family (lsm.h), included into the dense and the compact
// kernel of each instantiation so that the code is the kernel's own: `map` is the row -> cell policy (DenseMap or
// CompactMap) the including kernel declares.  Not a header of its own.
    constexpr bool GATHER = MODE == LSM_GATHER;
    __shared__ float red[LG_THREADS / WAVE];
    // bw.xcd: every XCD (workgroups go to them by blockIdx mod 8; the grid is a multiple of 8) streams a contiguous
    // eighth of the rows instead of every eighth row -- see dispatch_lsm
    const size_t per_xcd = ((size_t)rows + 7) / 8;
    const size_t items = bw.xcd ? per_xcd * 8 : (size_t)rows;
    for (size_t it = blockIdx.x; it < items; it += gridDim.x) {
    const size_t row = bw.xcd ? (it & 7) * per_xcd + (it >> 3) : it;
    if (row >= (size_t)rows) continue;
    const E* src = x + row * V;
    const int nvec = V >> 2;
    // How a lane's LG_MAXVEC loads are issued (round 5).  As first written -- load and running maximum together under
    // `if (j < nvec)` -- every load sits in a branch of its own with an s_waitcnt vmcnt(0) behind it: LG_MAXVEC memory
    // round trips per row, one after the other.  Measured against two loads-first forms (tools/ab_kernels.py, three
    // interleaved rounds, profiles/r05_loads_first_ab.txt):
    //   * the read-mostly FUSED modes gain 5-7 % from all loads issued unconditionally at an index clamped into the row,
    //     what lies beyond the row replaced by -inf afterwards (c3: fused forward 317 -> 300 us, fused backward 739 -> 689);
    //   * the plain log-softmax -- a read and a write stream at the rate of a copy -- does not: V = 5000 629 -> 647 us,
    //     4096 596 -> 606, 2048 590 -> 594, nothing at 1000, 3000, 8192; only the three-pass covers of 768 threads and more
    //     gain (c5's V = 10000: 693 -> 674 clamped, -> 665 with the loads alone under their predicates and the maxima
    //     behind them), so those take the predicated form and everything else stays as it was.
    constexpr bool CLAMPED = MODE != LSM_NORM;
    constexpr bool PREDICATED = MODE == LSM_NORM && LG_THREADS >= 768;
    float4 v[LG_MAXVEC];
    float mx = -__builtin_inff();
    if constexpr (CLAMPED || PREDICATED) {
#pragma unroll
        for (int i = 0; i < LG_MAXVEC; ++i) {
            const int j = (int)threadIdx.x + i * LG_THREADS;
            if constexpr (CLAMPED) {
                v[i] = lsm_ld4<true>(src, min(j, nvec - 1));
            } else {
                if (j < nvec) v[i] = lsm_ld4<true>(src, j);
            }
        }
    }
    // what the fused modes need besides the row, requested behind it instead of after the reductions
    [[maybe_unused]] CellMap m = {0, 0, 0};
    [[maybe_unused]] float2 side = make_float2(0.0f, 0.0f);      // GATHER: the row's (blank, label) logits; BWD: its gradient pair
    [[maybe_unused]] float sc = 1.0f;
    if constexpr (MODE != LSM_NORM) {
        map.chunk((int64_t)row, (int64_t)row);      // (compact rows: one search per row)
        m = map.at(row, V, blank);
        if constexpr (GATHER) {
            const E* xr = x + row * V;
            side = make_float2(lsm_ld1(xr + blank), lsm_ld1(xr + m.label));
        } else {
            side = map.pair(bw, m);
            sc = map.scale(bw, m);
        }
    }
#pragma unroll
    for (int i = 0; i < LG_MAXVEC; ++i) {
        const int j = (int)threadIdx.x + i * LG_THREADS;
        if constexpr (CLAMPED || PREDICATED) {
            if (j >= nvec) {
                const float ninf = -__builtin_inff();
                v[i] = make_float4(ninf, ninf, ninf, ninf);
            }
            mx = fmaxf(fmaxf(mx, fmaxf(v[i].x, v[i].y)), fmaxf(v[i].z, v[i].w));
        } else {
            if (j < nvec) {
                v[i] = lsm_ld4<true>(src, j);
                mx = fmaxf(fmaxf(mx, fmaxf(v[i].x, v[i].y)), fmaxf(v[i].z, v[i].w));
            }
        }
    }
    mx = block_reduce<LG_THREADS>(mx, true, red);
    const float mb = -mx * LOG2E;
    float s = 0.0f;
#pragma unroll
    for (int i = 0; i < LG_MAXVEC; ++i) {
        const int j = threadIdx.x + i * LG_THREADS;
        if (j < nvec)
            s += (__builtin_amdgcn_exp2f(__builtin_fmaf(v[i].x, LOG2E, mb)) + __builtin_amdgcn_exp2f(__builtin_fmaf(v[i].y, LOG2E, mb))) +
                 (__builtin_amdgcn_exp2f(__builtin_fmaf(v[i].z, LOG2E, mb)) + __builtin_amdgcn_exp2f(__builtin_fmaf(v[i].w, LOG2E, mb)));
    }
    s = block_reduce<LG_THREADS>(s, false, red);
    const float ls = lsm_log_sum(logf(s), mx, mb);
    if constexpr (GATHER) {
        if (threadIdx.x == 0) map.put(out, m, make_float2((side.x - mx) - ls, (side.y - mx) - ls));
    } else if constexpr (MODE == LSM_BWD) {
        const float2 g = side;
        // CLAMP: the pair stays unscaled -- the row is clamped behind the two additions and scaled behind the clamp
        const float gB = CLAMP ? g.x : g.x * sc, gL = CLAMP ? g.y : g.y * sc, gs = gB + gL;
        const float gq = gs / s;                                 // p_j = e_j / s (lsm_log_sum)
        LsmOut<MODE, E>* dst = out + row * V;
#pragma unroll
        for (int i = 0; i < LG_MAXVEC; ++i) {
            const int j = threadIdx.x + i * LG_THREADS;
            if (j < nvec) {
                float o[4] = {v[i].x, v[i].y, v[i].z, v[i].w};
#pragma unroll
                for (int cc = 0; cc < 4; ++cc) {
                    const int e = 4 * j + cc;
                    float d = -__builtin_amdgcn_exp2f(__builtin_fmaf(o[cc], LOG2E, mb)) * gq;
                    d += (e == blank) ? gB : 0.0f;
                    d += (e == m.label) ? gL : 0.0f;
                    if constexpr (CLAMP) d = lsm_clamp_scale(d, bw.clamp, sc);
                    o[cc] = d;
                }
                lsm_st4<true>(dst, j, make_float4(o[0], o[1], o[2], o[3]));
            }
        }
    } else {
        float* dst = out + row * V;
#pragma unroll
        for (int i = 0; i < LG_MAXVEC; ++i) {
            const int j = threadIdx.x + i * LG_THREADS;
            if (j < nvec) {
                const float4 r = make_float4((v[i].x - mx) - ls, (v[i].y - mx) - ls, (v[i].z - mx) - ls,
                                             (v[i].w - mx) - ls);
                lsm_st4<true>(dst, j, r);
                // the column plane (LsmBwd::col_out): the one lane that holds the column stores it (a row per workgroup:
                // 4 bytes beside 4V)
                if (bw.col_out && j == (bw.col >> 2)) {
                    const int c = bw.col & 3;
                    bw.col_out[row] = c == 0 ? r.x : (c == 1 ? r.y : (c == 2 ? r.z : r.w));
                }
            }
        }
    }
    }
