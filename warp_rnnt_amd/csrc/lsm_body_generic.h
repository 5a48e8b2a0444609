// Body of the generic log-softmax kernel family (lsm.h), included into the dense and the compact
// kernel of each instantiation so that the code is the kernel's own: `map` is the row -> cell policy (DenseMap or
// CompactMap) the including kernel declares.  Not a header of its own.
    constexpr bool GATHER = MODE == LSM_GATHER;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int lane = threadIdx.x & 63;
    if constexpr (decltype(map)::COMPACT) map.chunk(row, row);
    const E* xr = x + row * V;
    float mx = -__builtin_inff();
    for (int c = lane; c < V; c += WAVE) mx = fmaxf(mx, lsm_ld1(xr + c));
    mx = group_max<WAVE>(mx);
    float s = 0.0f;
    for (int c = lane; c < V; c += WAVE) s += expf(lsm_ld1(xr + c) - mx);
    s = group_sum<WAVE>(s);
    const float ls = logf(s);
    if constexpr (GATHER) {
        if (lane == 0) {
            const CellMap m = map.at((size_t)row, V, blank);
            map.put(out, m, make_float2((lsm_ld1(xr + blank) - mx) - ls, (lsm_ld1(xr + m.label) - mx) - ls));
        }
    } else if constexpr (MODE == LSM_BWD) {
        const CellMap m = map.at((size_t)row, V, blank);
        const float sc = map.scale(bw, m);
        const float2 g = map.pair(bw, m);
        // CLAMP: the pair stays unscaled -- the row is clamped behind the two additions and scaled behind the clamp
        const float gB = CLAMP ? g.x : g.x * sc, gL = CLAMP ? g.y : g.y * sc, gs = gB + gL;
        LsmOut<MODE, E>* o = out + row * V;
        for (int c = lane; c < V; c += WAVE) {
            float d = -expf((lsm_ld1(xr + c) - mx) - ls) * gs;
            d += (c == blank) ? gB : 0.0f;
            d += (c == m.label) ? gL : 0.0f;
            if constexpr (CLAMP) d = lsm_clamp_scale(d, bw.clamp, sc);
            lsm_st1(o + c, d);
        }
    } else {
        float* o = out + row * V;
        for (int c = lane; c < V; c += WAVE) {
            const float r = (lsm_ld1(xr + c) - mx) - ls;
            o[c] = r;
            if (bw.col_out && c == bw.col) bw.col_out[row] = r;      // the column plane (LsmBwd::col_out)
        }
    }
