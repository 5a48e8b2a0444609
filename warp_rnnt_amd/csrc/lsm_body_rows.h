// Body of the rows log-softmax kernel family (lsm.h), included into the dense and the compact
// kernel of each instantiation so that the code is the kernel's own: `map` is the row -> cell policy (DenseMap or
// CompactMap) the including kernel declares.  Not a header of its own.
    constexpr int MODE = LSM_GATHER, VEC = 4;
    constexpr int UN = RowsShape<L>::UN, RW = RowsShape<L>::RW, RPW = RowsShape<L>::RPW;
    const int lane = threadIdx.x & 63, h = lane % L, rr = lane / L;
    // wave-uniform values kept in scalar registers (the 64-bit row arithmetic runs on the scalar unit)
    const int64_t row0 = ((int64_t)stream_block() * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6)) * RPW;
    if (row0 >= rows) return;
    const bool last_ok = (h + (Q - 1) * L) * VEC < V;   // the lane's last float4 is part of the row
    const bool whole = row0 + RPW <= rows;              // (uniform) every row of this wave exists
    if constexpr (decltype(map)::COMPACT) map.chunk(row0, min(row0 + RPW, rows) - 1);
    const E* const wave_src = x + row0 * V;
    const unsigned lane_off = (unsigned)rr * (unsigned)V + (unsigned)h * VEC;      // floats inside a pass
    // lane l < RPW owns the pair of row row0 + l.  Its two logits are requested FIRST, next to the row loads that bring
    // the same lines (asked for after the rows have streamed through, they are fetched a second time: forward 252 vs 216
    // us at V = 128, profiles/r04_lsm_rows_ab.txt)
    CellMap cm = {0, 0, 0};
    float xb = 0.0f, xl = 0.0f;
    const bool own = lane < RPW && row0 + lane < rows;
    if (own) {
        cm = map.at((size_t)(row0 + lane), V, blank);
        const E* xr = x + (row0 + lane) * V;
        xb = lsm_ld1(xr + blank);
        xl = lsm_ld1(xr + cm.label);
    }
    const E* src[UN];
#pragma unroll
    for (int p = 0; p < UN; ++p) {
        src[p] = wave_src + (size_t)(p * RW) * V + lane_off;
        // (rows past the end of the tensor -- last wave only -- re-read the last row and are dropped at the stores)
        if (!whole && row0 + p * RW + rr >= rows) src[p] = x + (rows - 1) * V + h * VEC;
    }
    float mx[UN], ls[UN];
    lsm_rows_stats<E, L, Q, MODE>(src, last_ok, mx, ls);
    float m, lg;
    lsm_rows_stats_of_lane<L>(lane, mx, ls, m, lg);
    if (own) map.put(out, cm, make_float2((xb - m) - lg, (xl - m) - lg));
