// Body of the small log-softmax kernel family (lsm.h), included into the dense and the compact
// kernel of each instantiation so that the code is the kernel's own: `map` is the row -> cell policy (DenseMap or
// CompactMap) the including kernel declares.  Not a header of its own.
    constexpr bool GATHER = MODE == LSM_GATHER;
    extern __shared__ __attribute__((aligned(16))) float tile[];
    float2* stat = reinterpret_cast<float2*>(tile + (size_t)R * V);   // GATHER: (max, log-sum) per row
    const int tid = threadIdx.x;
    const int64_t row0 = (int64_t)stream_block() * R;
    if (row0 >= rows) return;
    const int nrows = (int)min((int64_t)R, rows - row0);
    map.chunk(row0, row0 + nrows - 1);
    const int nel = nrows * V;                      // floats in this chunk
    const E* src = x + row0 * V;                    // vector aligned: R % 4 == 0 (out may alias x)
    // wave-private view of the same tile: rows [wr0, wr0 + wn) of the chunk
    constexpr int RW = (WAVE / L) > 0 ? (WAVE / L) : 1;
    const int lane = tid & (WAVE - 1);
    const int wr0 = (tid >> 6) * RW;
    const int wn = min(max(nrows - wr0, 0), RW);
    const int wel = wn * V, wvec = wel >> 2;
    float* wtile = tile + wr0 * V;

    // ---- stage: the tile is a plain copy of the chunk ----
    const int nvec = nel >> 2;
    // fused backward: the gradient pair (and scale) of the row this thread works on first, requested before the tile
    [[maybe_unused]] CellMap pm = {0, 0, 0};
    [[maybe_unused]] float2 pg = make_float2(0.0f, 0.0f);
    [[maybe_unused]] float psc = 1.0f;
    if constexpr (MODE == LSM_BWD) {
        pm = map.at((size_t)(row0 + min(tid / L, nrows - 1)), V, blank);
        pg = map.pair(bw, pm);
        psc = map.scale(bw, pm);
    }
    // LOADS FIRST (round 5).  Written as `for (i ...) tile[i] = load(src + i)` the compiler emits load, s_waitcnt vmcnt(0),
    // ds_write per iteration: a wave had ONE 16-byte load per lane in flight at a time and paid the memory latency three
    // to four times per tile -- 1 KB per wave in flight, 32 KB per CU, which at ~1.5 us of loaded latency is the 5.2 TB/s
    // the fused gather ran at (read-only streams reach 7.0, tools/ubench/copy_rate.hip).  A tile is at most four passes
    // of the threads that stage it (SM_FLOATS, and V <= 16 L for the wave-private form): all of a lane's loads are
    // issued before the first of them is written to LDS -- unconditionally, at an index clamped into the tile, and so are
    // the LDS writes (lanes past the end rewrite the tile's last 16 bytes with the bytes that are there).  A predicate per
    // load comes out as a branch per load with a conservative wait at every join; predicates on the writes alone and the
    // compiler sinks the loads into them.
    constexpr int STAGE_UN = WP ? 4 : (sm_floats<E, MODE>() / 4 + SM_THREADS - 1) / SM_THREADS;   // (3200 floats, 256 threads: 4)
    if constexpr (WP) {
        const E* wsrc = src + (size_t)wr0 * V;
        for (int base = lane; base < wvec; base += STAGE_UN * WAVE) {
            float4 sv[STAGE_UN];
#pragma unroll
            for (int k = 0; k < STAGE_UN; ++k)
                sv[k] = lsm_ld4<RNNT_LSM_NT_MODE(MODE)>(wsrc, min(base + k * WAVE, wvec - 1));
#pragma unroll
            for (int k = 0; k < STAGE_UN; ++k)
                reinterpret_cast<float4*>(wtile)[min(base + k * WAVE, wvec - 1)] = sv[k];
        }
        for (int e = (wvec << 2) + lane; e < wel; e += WAVE) wtile[e] = lsm_ld1(wsrc + e);
        wave_sync_lds();
    } else {
        for (int base = tid; base < nvec; base += STAGE_UN * SM_THREADS) {
            float4 sv[STAGE_UN];
#pragma unroll
            for (int k = 0; k < STAGE_UN; ++k)
                sv[k] = lsm_ld4<RNNT_LSM_NT_MODE(MODE)>(src, min(base + k * SM_THREADS, nvec - 1));
#pragma unroll
            for (int k = 0; k < STAGE_UN; ++k)
                reinterpret_cast<float4*>(tile)[min(base + k * SM_THREADS, nvec - 1)] = sv[k];
        }
        for (int e = (nvec << 2) + tid; e < nel; e += SM_THREADS) tile[e] = lsm_ld1(src + e);   // last chunk only
        __syncthreads();
    }

    // ---- per-row max / sum(exp) / normalise: L lanes per row, lane h owns columns h, h+L, ... ----
    constexpr int RPP = SM_THREADS / L;             // rows per pass
    const int h = tid % L, rr = tid / L;
    const int ctail = h + (q - 1) * L;              // this lane's last column, may be >= V
    const bool tail_ok = ctail < V;
    // One row: the lane's q values are read ONCE into registers by a straight-line sequence (all LDS reads in flight
    // together), reduced, and -- in the modes that rewrite the row -- written back from the registers.  QC = q as a
    // compile-time constant (9 ... 16: what the launcher's choice of L gives for V > 16); the run-time loops of the first
    // version waited for every LDS read of the max pass on its own (~9 instructions and one LDS latency per element) and
    // read every element a second time for the sum.
    auto one_row = [&](auto QC, const int r) {
        constexpr int Q = decltype(QC)::value;
        float* row = tile + r * V;
        float v[Q];
#pragma unroll
        for (int i = 0; i < Q - 1; ++i) v[i] = row[h + i * L];
        v[Q - 1] = tail_ok ? row[ctail] : -__builtin_inff();
        float mx = v[0];
#pragma unroll
        for (int i = 1; i < Q; ++i) mx = fmaxf(mx, v[i]);
        mx = group_max<L>(mx);
        const float mb = -mx * LOG2E;
        float s = 0.0f;
#pragma unroll
        for (int i = 0; i < Q; ++i) s += __builtin_amdgcn_exp2f(__builtin_fmaf(v[i], LOG2E, mb));   // (exp2(-inf) = 0)
        s = group_sum<L>(s);
        const float ls = lsm_log_sum(__builtin_amdgcn_logf(s) * LN2, mx, mb);
        if constexpr (GATHER) {
            if (h == 0) stat[r] = make_float2(mx, ls);
        } else if constexpr (MODE == LSM_BWD) {
            const bool first = r == rr;                // (the row whose pair was requested up front)
            const CellMap m = first ? pm : map.at((size_t)(row0 + r), V, blank);
            const float sc = first ? psc : map.scale(bw, m);
            const float2 g = first ? pg : map.pair(bw, m);
            if constexpr (CLAMP) {
                // the clamp behind the sum and in front of the scale: the pair stays unscaled, every lane clamps and scales
                // what it writes, and lane 0 forms the two one-hot entries whole -- from the logits still in the tile --
                // and puts them over the row's behind the row pass (lsm_hot_clamped)
                const float gB = g.x, gL = g.y, gs = gB + gL;
                const float gq = gs * __builtin_amdgcn_rcpf(s);
                float hb = 0.0f, hl = 0.0f;
                if (h == 0) lsm_hot_clamped(row[blank], row[m.label], m.label == blank, mb, gq, gB, gL, bw.clamp, sc, hb, hl);
#pragma unroll
                for (int i = 0; i < Q - 1; ++i)
                    row[h + i * L] = lsm_clamp(-__builtin_amdgcn_exp2f(__builtin_fmaf(v[i], LOG2E, mb)) * gq, bw.clamp) * sc;
                if (tail_ok)
                    row[ctail] = lsm_clamp(-__builtin_amdgcn_exp2f(__builtin_fmaf(v[Q - 1], LOG2E, mb)) * gq, bw.clamp) * sc;
                if (h == 0) { row[blank] = hb; row[m.label] = hl; }
            } else {
            const float gB = g.x * sc, gL = g.y * sc, gs = gB + gL;
            const float gq = gs * __builtin_amdgcn_rcpf(s);      // p_j = e_j / s (lsm_log_sum)
#pragma unroll
            for (int i = 0; i < Q - 1; ++i)
                row[h + i * L] = -__builtin_amdgcn_exp2f(__builtin_fmaf(v[i], LOG2E, mb)) * gq;
            if (tail_ok) row[ctail] = -__builtin_amdgcn_exp2f(__builtin_fmaf(v[Q - 1], LOG2E, mb)) * gq;
            // the L lanes of a row sit in one wave and LDS operations of a wave retire in order
            if (h == 0) { row[blank] += gB; row[m.label] += gL; }
            }
        } else {
#pragma unroll
            for (int i = 0; i < Q - 1; ++i) row[h + i * L] = (v[i] - mx) - ls;
            if (tail_ok) row[ctail] = (v[Q - 1] - mx) - ls;
        }
    };
    auto all_rows = [&](auto QC) {
        for (int r = rr; r < nrows; r += RPP) one_row(QC, r);
    };
    switch (q) {
#define LSM_Q(QQ) case QQ: all_rows(std::integral_constant<int, QQ>{}); break;
        LSM_Q(9) LSM_Q(10) LSM_Q(11) LSM_Q(12) LSM_Q(13) LSM_Q(14) LSM_Q(15) LSM_Q(16)
#undef LSM_Q
        default:      // q <= 8 (V <= 16, or rows shorter than the lane cover): run-time loops
    for (int r = rr; r < nrows; r += RPP) {
        float* row = tile + r * V;
        float mx = -__builtin_inff();
        for (int i = 0, c = h; i < q - 1; ++i, c += L) mx = fmaxf(mx, row[c]);
        if (tail_ok) mx = fmaxf(mx, row[ctail]);
        mx = group_max<L>(mx);
        const float mb = -mx * LOG2E;
        float s = 0.0f;
        for (int i = 0, c = h; i < q - 1; ++i, c += L) s += __builtin_amdgcn_exp2f(__builtin_fmaf(row[c], LOG2E, mb));
        if (tail_ok) s += __builtin_amdgcn_exp2f(__builtin_fmaf(row[ctail], LOG2E, mb));
        s = group_sum<L>(s);
        const float ls = lsm_log_sum(__builtin_amdgcn_logf(s) * LN2, mx, mb);
        if constexpr (GATHER) {
            if (h == 0) stat[r] = make_float2(mx, ls);
        } else if constexpr (MODE == LSM_BWD) {
            const CellMap m = map.at((size_t)(row0 + r), V, blank);
            const float sc = map.scale(bw, m);
            const float2 g = map.pair(bw, m);
            if constexpr (CLAMP) {       // (as in the straight-line form above)
                const float gB = g.x, gL = g.y, gs = gB + gL;
                const float gq = gs * __builtin_amdgcn_rcpf(s);
                float hb = 0.0f, hl = 0.0f;
                if (h == 0) lsm_hot_clamped(row[blank], row[m.label], m.label == blank, mb, gq, gB, gL, bw.clamp, sc, hb, hl);
                for (int i = 0, c = h; i < q - 1; ++i, c += L)
                    row[c] = lsm_clamp(-__builtin_amdgcn_exp2f(__builtin_fmaf(row[c], LOG2E, mb)) * gq, bw.clamp) * sc;
                if (tail_ok)
                    row[ctail] = lsm_clamp(-__builtin_amdgcn_exp2f(__builtin_fmaf(row[ctail], LOG2E, mb)) * gq, bw.clamp) * sc;
                if (h == 0) { row[blank] = hb; row[m.label] = hl; }
            } else {
            const float gB = g.x * sc, gL = g.y * sc, gs = gB + gL;
            const float gq = gs * __builtin_amdgcn_rcpf(s);      // p_j = e_j / s (lsm_log_sum)
            for (int i = 0, c = h; i < q - 1; ++i, c += L)
                row[c] = -__builtin_amdgcn_exp2f(__builtin_fmaf(row[c], LOG2E, mb)) * gq;
            if (tail_ok) row[ctail] = -__builtin_amdgcn_exp2f(__builtin_fmaf(row[ctail], LOG2E, mb)) * gq;
            // the L lanes of a row sit in one wave and LDS operations of a wave retire in order
            if (h == 0) { row[blank] += gB; row[m.label] += gL; }
            }
        } else {
            for (int i = 0, c = h; i < q - 1; ++i, c += L) row[c] = (row[c] - mx) - ls;
            if (tail_ok) row[ctail] = (row[ctail] - mx) - ls;
        }
    }
    }
    if constexpr (GATHER && WP) {
        wave_sync_lds();
        for (int r = wr0 + lane; r < wr0 + wn; r += WAVE) {
            const CellMap m = map.at((size_t)(row0 + r), V, blank);
            const float2 st = stat[r];
            const float* row = tile + r * V;
            map.put(out, m, make_float2((row[blank] - st.x) - st.y, (row[m.label] - st.x) - st.y));
        }
    } else if constexpr (GATHER) {
        // one lane per row with all lanes busy (the per-row index arithmetic costs ~60 instructions;
        // doing it inside the L-lane row loop ran it with a quarter of the lanes)
        __syncthreads();
        for (int r = tid; r < nrows; r += SM_THREADS) {
            const CellMap m = map.at((size_t)(row0 + r), V, blank);
            const float2 st = stat[r];
            const float* row = tile + r * V;
            const float2 pr = make_float2((row[blank] - st.x) - st.y, (row[m.label] - st.x) - st.y);
            // (written through, sc1: +38 us at c4 -- scattered 8-byte stores need L2 to merge them.  Timing probes that sent
            // the pairs into a 64 KB region that stays in L2, or stored them in row-major order as coalesced 512-byte runs:
            // the gather's stores cost 40-55 us in any shape)
            map.put(out, m, pr);
        }
    } else if constexpr (WP) {
        wave_sync_lds();
        // the column plane (LsmBwd::col_out): the wave's rows are consecutive, so is its slice of the plane
        if constexpr (MODE == LSM_NORM) {
            if (bw.col_out)
                for (int r = lane; r < wn; r += WAVE) bw.col_out[row0 + wr0 + r] = wtile[r * V + bw.col];
        }
        LsmOut<MODE, E>* wdst = out + (row0 + wr0) * V;
        if constexpr (std::is_same_v<E, float>) {
            for (int i = lane; i < wvec; i += WAVE)
                RNNT_LSM_STORE(reinterpret_cast<float4*>(wdst) + i, reinterpret_cast<const float4*>(wtile)[i]);
            for (int e = (wvec << 2) + lane; e < wel; e += WAVE) wdst[e] = wtile[e];
        } else {
            for (int i = lane; i < wvec; i += WAVE)
                lsm_st4<RNNT_LSM_NT_MODE(MODE)>(wdst, i, reinterpret_cast<const float4*>(wtile)[i]);
            for (int e = (wvec << 2) + lane; e < wel; e += WAVE) lsm_st1(wdst + e, wtile[e]);
        }
    } else {
        __syncthreads();
        if constexpr (MODE == LSM_NORM) {      // the column plane: one contiguous run per workgroup
            if (bw.col_out)
                for (int r = tid; r < nrows; r += SM_THREADS) bw.col_out[row0 + r] = tile[r * V + bw.col];
        }
        LsmOut<MODE, E>* dst = out + row0 * V;
        if constexpr (std::is_same_v<E, float>) {
            for (int i = tid; i < nvec; i += SM_THREADS)
                RNNT_LSM_STORE(reinterpret_cast<float4*>(dst) + i, reinterpret_cast<const float4*>(tile)[i]);
            for (int e = (nvec << 2) + tid; e < nel; e += SM_THREADS) dst[e] = tile[e];
        } else {
            for (int i = tid; i < nvec; i += SM_THREADS)
                lsm_st4<RNNT_LSM_NT_MODE(MODE)>(dst, i, reinterpret_cast<const float4*>(tile)[i]);
            for (int e = (nvec << 2) + tid; e < nel; e += SM_THREADS) lsm_st1(dst + e, tile[e]);
        }
    }
