// Best-path alignments on the pruned band (include/warp_rnnt_amd_pruned_align.h has the definition).
//
// Two launches.  The producer is the pruned loss's row arithmetic -- row_stats of row_chunks.h, the HAT row of hat.h, the
// delay penalty in the expression pruned.hip uses -- with another store: the pair of row (n,t,s) goes to (n,t,s) of a
// band-compact (N,T,S,2) plane, (-inf,-inf) where the row's cell is not in the band.  No floor, no (N,T,U) plane.
//
// The sweep is frame-synchronous: one wave per utterance, lane s is band position s, T_n steps.  Per frame the wave
// fetches the previous frame's v + blank at s + c(t) - c(t-1) (one ds_bpermute; none when the band did not move), relaxes
// along s through DPP wave_shr:1 rounds until nothing changes (regular topology; the fixed point of the rounds is the
// definition's chain of adds, bit for bit: fp add and the compare are monotone), and keeps __ballot(by_label) as the
// frame's decision word.  No load sits in that chain: the pairs and starts of PA_CHUNK = 64 frames are asked for, in
// coalesced 8-byte loads, while the chunk before them is swept; they wait in registers and go to LDS when that chunk is
// done, and a frame's pair is read from LDS one frame ahead.  The decision words of a chunk sit in lane f of a register
// and leave in one coalesced store behind the staging, so the wait for the staged loads never waits for a store.
// The same wave then walks back from the end cell: per frame one decision word and one start, read 64 frames at a time,
// the run of labels of a frame found with one count-leading-zeros and written by as many lanes.  The wave owns the
// utterance: nothing passes between workgroups, no atomics, no hand-written instructions.
#include "pruned_align.h"

#include "hat.h"
#include "pruned.h"
#include "row_chunks.h"
#include "../../include/warp_rnnt_amd.h"

// every sum below is rounded on its own
#pragma clang fp contract(off)

namespace rnnt {
namespace {

constexpr float PA_NEG_INF = -__builtin_inff();

// Where row `row` of (N,T,S) lies in the lattice of its utterance.  live: the cell is in the band -- u in [0,U), t < T_n,
// u <= U_n, lengths the entry takes; the sum is formed in 64 bits so that no start wraps into the grid.  has_label: u < U_n.
struct BandRow {
    int n, t, label;
    bool live, has_label;
};
__device__ __forceinline__ BandRow band_row(size_t row, const int* __restrict__ labels, const int* __restrict__ starts,
                                            const int* __restrict__ xn, const int* __restrict__ yn, int T, int U, int S,
                                            int V, int blank, bool read_label) {
    const unsigned r32 = (unsigned)row;                // N*T*S < 2^32 is checked by the C ABI
    const unsigned frame = r32 / (unsigned)S;          // n*T + t
    const int s = (int)(r32 - frame * (unsigned)S);
    const unsigned n = frame / (unsigned)T;
    const int t = (int)(frame - n * (unsigned)T);
    const int Tn = xn[n], Un = yn[n];
    const long long u = (long long)starts[frame] + s;
    BandRow c;
    c.n = (int)n;
    c.t = t;
    c.live = Tn >= 1 && Tn <= T && Un >= 0 && Un < U && t < Tn && u >= 0 && u < (long long)U && u <= (long long)Un;
    c.has_label = c.live && u < (long long)Un;
    c.label = blank;
    if (c.has_label && read_label) c.label = safe_label(labels[(size_t)n * (U - 1) + (int)u], V, blank);
    return c;
}

__device__ __forceinline__ float band_penalty(float dp, int Tn, int t) { return dp * (0.5f * (float)(Tn - 1) - (float)t); }

template <typename E, int G, int ACC, bool HAT, bool REGS>
__global__ void __launch_bounds__(ROW_THREADS)
k_band_pairs(const E* __restrict__ x, const int* __restrict__ labels, const int* __restrict__ starts,
             const int* __restrict__ xn, const int* __restrict__ yn, float2* __restrict__ out, size_t rows, int T, int U,
             int S, int V, int blank, float dp) {
    static_assert(!HAT || REGS || G == WAVE, "HAT's long form is a wave per row");
    const size_t row = (size_t)blockIdx.x * (ROW_THREADS / G) + threadIdx.x / G;
    if (row >= rows) return;
    const int lane = threadIdx.x % G;
    const BandRow c = band_row(row, labels, starts, xn, yn, T, U, S, V, blank, true);
    if (!c.live) {                                     // (the whole group: no lane of it is asked for a shuffle below)
        if (lane == 0) out[row] = make_float2(PA_NEG_INF, PA_NEG_INF);
        return;
    }
    const E* xr = x + row * (size_t)V;
    const float zb = (float)xr[blank], zl = (float)xr[c.label];
    float m, ls;
    float2 p;
    if constexpr (HAT) {
        if constexpr (REGS) {
            float z[2][ROW_CHUNK];
            hat_small_stats<E, G, ACC>(xr, lane, V, blank, z, m, ls);
        } else {
            hat_wave_stats<E, ACC, true>(xr, lane, V, blank, m, ls);
        }
        p = hat_pair(zb, zl, c.label, blank, m, ls);
    } else {
        row_stats<E, G, ACC, true>(xr, lane, V, V, [](int) { return false; }, m, ls);
        p = make_float2((zb - m) - ls, (zl - m) - ls);
    }
    if (dp != 0.0f) p.y = p.y + band_penalty(dp, xn[c.n], c.t);
    if (!c.has_label) p.y = PA_NEG_INF;
    if (lane == 0) out[row] = p;
}

// ready-made pairs: a lane per row
__global__ void __launch_bounds__(ROW_THREADS)
k_band_pairs_ready(const float2* __restrict__ in, const int* __restrict__ starts, const int* __restrict__ xn,
                   const int* __restrict__ yn, float2* __restrict__ out, size_t rows, int T, int U, int S, float dp) {
    const size_t row = (size_t)blockIdx.x * ROW_THREADS + threadIdx.x;
    if (row >= rows) return;
    const BandRow c = band_row(row, nullptr, starts, xn, yn, T, U, S, 0, 0, false);
    float2 p = make_float2(PA_NEG_INF, PA_NEG_INF);
    if (c.live) {
        p = in[row];
        if (dp != 0.0f) p.y = p.y + band_penalty(dp, xn[c.n], c.t);
        if (!c.has_label) p.y = PA_NEG_INF;
    }
    out[row] = p;
}

template <typename E>
hipError_t band_pairs_logits(hipStream_t stream, bool hat, const E* x, const int* labels, const int* starts, const int* xn,
                             const int* yn, float2* out, size_t rows, int T, int U, int S, int V, int blank, float dp) {
    const int G = row_group(V);
    const unsigned grid = row_grid(rows, G);
    return row_dispatch<E>(G, row_access<E>(V, x, nullptr), [&](auto g, auto acc) {
        constexpr int GG = decltype(g)::value, ACC = decltype(acc)::value;
        // (HAT's form is a function of V alone, as in pruned_hat.hip: a row's bits are that unit's)
        if (!hat)
            k_band_pairs<E, GG, ACC, false, false><<<grid, ROW_THREADS, 0, stream>>>(x, labels, starts, xn, yn, out, rows, T,
                                                                                    U, S, V, blank, dp);
        else if (V <= HAT_SMALL_V)
            k_band_pairs<E, GG, ACC, true, true><<<grid, ROW_THREADS, 0, stream>>>(x, labels, starts, xn, yn, out, rows, T, U,
                                                                                  S, V, blank, dp);
        else if constexpr (GG == WAVE)
            k_band_pairs<E, WAVE, ACC, true, false><<<grid, ROW_THREADS, 0, stream>>>(x, labels, starts, xn, yn, out, rows,
                                                                                     T, U, S, V, blank, dp);
    });
}

// ---------------------------------------------------------------------------------------------------------
// The sweep and the walk back
// ---------------------------------------------------------------------------------------------------------

// lane s takes lane s-1's value, lane 0 takes -inf: one DPP move
__device__ __forceinline__ float pa_shr1(float x) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, PA_NEG_INF),
                                                                 __builtin_bit_cast(int, x), 0x138, 0xf, 0xf, false));
}
// lane s takes lane s+off's value; -inf where that is no band position
__device__ __forceinline__ float pa_fetch(float w, int lane, int off, int S) {
    const int src = lane + off;
    const float r = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute((src & (WAVE - 1)) << 2, __builtin_bit_cast(int, w)));
    return src >= 0 && src < S ? r : PA_NEG_INF;
}
// c - cp of two starts nobody validated, in 64 bits, cut to where every lane's source is out of range anyway
__device__ __forceinline__ int pa_delta(int c, int cp) {
    const long long d = (long long)c - (long long)cp;
    return (int)(d > WAVE + 1 ? WAVE + 1 : d < -(WAVE + 1) ? -(WAVE + 1) : d);
}
__device__ __forceinline__ unsigned long long pa_readlane64(unsigned long long w, int j) {
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)w, j);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(w >> 32), j);
    return ((unsigned long long)hi << 32) | lo;
}

// blockIdx.x: the utterance; one wave.  SB: the bucket of S (S <= SB): the staged chunk is SB float2 per lane.
template <int SB, int TOPO>
__global__ void __launch_bounds__(WAVE)
k_band_sweep(const float2* __restrict__ pairs, const int* __restrict__ starts, const int* __restrict__ xn,
             const int* __restrict__ yn, unsigned long long* __restrict__ words, float* __restrict__ scores,
             int* __restrict__ emit_frames, int T, int U, int S) {
    __shared__ float2 lp[PA_CHUNK * SB];               // pairs of the chunk's frames: frame f, position s at f * S + s
    __shared__ int lc[PA_CHUNK];                       // ... and their starts
    constexpr bool MOD = TOPO == TOPO_MODIFIED;
    const int n = blockIdx.x, lane = threadIdx.x;
    const int Tn = xn[n], Un = yn[n];
    int* frames = emit_frames + (size_t)n * (U - 1);
    if (Tn < 1 || Tn > T || Un < 0 || Un >= U) {       // (the whole wave)
        if (lane == 0) scores[n] = __builtin_nanf("");
        for (int u = lane; u < U - 1; u += WAVE) frames[u] = -1;
        return;
    }
    const float2* pn = pairs + (size_t)n * T * S;
    const int* cn = starts + (size_t)n * T;
    unsigned long long* wn = words + (size_t)n * pruned_align_words(T, TOPO);
    // the pair of band position `lane` of the chunk's frame f (lanes past the band: -inf, through an address of the band's)
    const auto frame_pair = [&](int f) {
        const float2 q = lp[f * S + min(lane, S - 1)];
        return make_float2(lane < S ? q.x : PA_NEG_INF, lane < S ? q.y : PA_NEG_INF);
    };

    float2 st[SB];
    int stc = 0;
    const auto stage_load = [&](int t0) {              // frames t0 .. of the utterance: elements j * 64 + lane of the chunk
        const int nf = min(PA_CHUNK, Tn - t0), count = nf * S;
        const float2* src = pn + (size_t)t0 * S;
#pragma unroll
        for (int j = 0; j < SB; ++j) {
            if (j >= S) continue;                      // (the wave's: elements from 64 S on belong to no frame of a chunk)
            const int idx = j * WAVE + lane;
            const float2 q = src[min(idx, count - 1)]; // (an address inside the chunk for every lane: no select of pointers)
            st[j].x = idx < count ? q.x : PA_NEG_INF;
            st[j].y = idx < count ? q.y : PA_NEG_INF;
        }
        stc = cn[t0 + min(lane, nf - 1)];
    };
    const auto stage_store = [&]() {
#pragma unroll
        for (int j = 0; j < SB; ++j)
            if (j < S) lp[j * WAVE + lane] = st[j];
        lc[lane] = stc;
    };

    float wb = PA_NEG_INF, wl = PA_NEG_INF;            // v + blank, v + label of the frame behind, per band position
    int cprev = 0;
    stage_load(0);
    stage_store();
    for (int t0 = 0; t0 < Tn; t0 += PA_CHUNK) {
        const int nf = min(PA_CHUNK, Tn - t0);
        const bool more = t0 + PA_CHUNK < Tn;
        if (more) stage_load(t0 + PA_CHUNK);           // in flight while this chunk is swept
        unsigned long long mine = 0;                   // lane f: the decision word of frame t0 + f
        float2 cur = frame_pair(0);
        int ccur = lc[0];
        for (int f = 0; f < nf; ++f) {
            // a frame ahead: out of LDS before this frame's chain needs it (behind the chunk's last frame: that frame again)
            const int fn = min(f + 1, nf - 1);
            const float2 nxt = frame_pair(fn);
            const int cnxt = lc[fn];
            const int t = t0 + f;
            const long long u = (long long)ccur + lane;
            const int delta = pa_delta(ccur, cprev);
            float cb, v;
            bool by;
            if (t == 0)
                cb = lane < S && u == 0 ? 0.0f : PA_NEG_INF;
            else
                cb = delta == 0 ? wb : pa_fetch(wb, lane, delta, S);
            if constexpr (MOD) {
                const float cl = t == 0 ? PA_NEG_INF : pa_fetch(wl, lane, delta - 1, S);
                by = cl > cb;
                v = by ? cl : cb;
            } else {
                float cand = PA_NEG_INF;
                v = cb;
                for (int r = 1; r < S; ++r) {          // lanes <= r are final after round r; cand is then final for them too
                    cand = pa_shr1(v + cur.y);
                    cand = lane < S ? cand : PA_NEG_INF;
                    const float nv = cand > v ? cand : v;
                    const bool changed = __ballot(nv != v) != 0;
                    v = nv;
                    if (!changed) break;
                }
                by = t == 0 ? u > 0 : cand > cb;
            }
            wb = v + cur.x;
            wl = v + cur.y;
            const unsigned long long word = __ballot(by && lane < S);
            mine = lane == f ? word : mine;
            cprev = ccur;
            cur = nxt;
            ccur = cnxt;
        }
        if (more) stage_store();                       // (behind this chunk's last LDS read: one wave, LDS in order)
        if (lane < nf) wn[t0 + lane] = mine;
    }

    float score;
    if constexpr (MOD) {                               // frame T_n holds the end cell alone: a band that starts at U_n
        const int delta = pa_delta(Un, cprev);
        const float cb = pa_fetch(wb, lane, delta, S), cl = pa_fetch(wl, lane, delta - 1, S);
        const bool by = cl > cb;
        score = __shfl(by ? cl : cb, 0, WAVE);
        const unsigned long long word = __ballot(by) & 1ull;
        if (lane == 0) wn[Tn] = word;
    } else {
        const long long so = (long long)Un - cprev;
        score = __shfl(wb, (int)(so & (WAVE - 1)), WAVE);
        score = so >= 0 && so < S ? score : PA_NEG_INF;
    }
    if (lane == 0) scores[n] = score;
    const bool path = score > PA_NEG_INF;
    for (int u = (path ? Un : 0) + lane; u < U - 1; u += WAVE) frames[u] = -1;
    if (!path) return;
    __syncthreads();                                   // the decision words are read back by other lanes than wrote them

    // from the end cell: lane j of a chunk holds frame t - j.  Regular: the frame's run of labels is the run of set bits
    // from the cell's bit down; modified: the cell's bit, and the label's frame is the one its edge consumes.
    int t = MOD ? Tn : Tn - 1, u = Un;
    const int tend = MOD ? 1 : 0;
    bool walking = u > 0;
    while (walking && t >= tend) {
        const int tj = t - lane;
        unsigned long long w = 0;
        int c = 0;
        if (tj >= tend) {
            w = wn[tj];
            c = MOD && tj == Tn ? Un : cn[tj];
        }
        const int count = min(WAVE, t - tend + 1);
        for (int j = 0; j < count; ++j) {
            const unsigned long long wj = pa_readlane64(w, j);
            const long long s = (long long)u - __builtin_amdgcn_readlane(c, j);
            if (s < 0 || s >= S) {                     // (not on a path of finite score: only keeps a walk inside its rows)
                walking = false;
                break;
            }
            int k;
            if constexpr (MOD) {
                k = (int)((wj >> s) & 1ull);
            } else {
                const unsigned long long x = ~(wj << (63 - s));
                k = x == 0 ? 64 : __clzll((long long)x);
            }
            k = min(k, u);
            if (lane < k) frames[u - 1 - lane] = t - j - (MOD ? 1 : 0);
            u -= k;
            if (u == 0) {
                walking = false;
                break;
            }
        }
        t -= count;
    }
}

template <int SB>
void band_sweep_bucket(hipStream_t stream, const float2* pairs, const int* starts, const int* xn, const int* yn,
                       unsigned long long* words, float* scores, int* emit_frames, int N, int T, int U, int S,
                       int topology) {
    if (topology == TOPO_MODIFIED)
        k_band_sweep<SB, TOPO_MODIFIED><<<N, WAVE, 0, stream>>>(pairs, starts, xn, yn, words, scores, emit_frames, T, U, S);
    else
        k_band_sweep<SB, TOPO_REGULAR><<<N, WAVE, 0, stream>>>(pairs, starts, xn, yn, words, scores, emit_frames, T, U, S);
}

}  // namespace

hipError_t launch_band_pairs(hipStream_t stream, int kind, int dtype, const void* input, const int* labels,
                             const int* starts, const int* xn, const int* yn, float* pairs, int N, int T, int U, int S, int V,
                             int blank, float delay_penalty) {
    if (N < 0 || T < 1 || U < 1 || S < 1 || S > U || (unsigned long long)N * T * S >= (1ull << 32) || !starts || !xn || !yn)
        return hipErrorInvalidValue;
    const size_t rows = (size_t)N * T * S;
    if (rows == 0) return hipSuccess;
    float2* out = reinterpret_cast<float2*>(pairs);
    if (kind == PA_IN_PAIRS) {
        if (dtype != RNNT_DTYPE_F32) return hipErrorInvalidValue;
        k_band_pairs_ready<<<(unsigned)((rows + ROW_THREADS - 1) / ROW_THREADS), ROW_THREADS, 0, stream>>>(
            static_cast<const float2*>(input), starts, xn, yn, out, rows, T, U, S, delay_penalty);
        return hipGetLastError();
    }
    if ((kind != PA_IN_LOGITS && kind != PA_IN_HAT_LOGITS) || V < 2 || blank < 0 || blank >= V) return hipErrorInvalidValue;
    return row_typed(dtype, input, nullptr, [&](auto* x, auto*) {
        return band_pairs_logits(stream, kind == PA_IN_HAT_LOGITS, x, labels, starts, xn, yn, out, rows, T, U, S, V, blank,
                                 delay_penalty);
    });
}

hipError_t launch_band_sweep(hipStream_t stream, const float* pairs, const int* starts, const int* xn, const int* yn,
                             unsigned long long* words, float* scores, int* emit_frames, int N, int T, int U, int S,
                             int topology) {
    if (N < 0 || T < 1 || U < 1 || S < 1 || S > PA_MAX_S || (topology != TOPO_REGULAR && topology != TOPO_MODIFIED))
        return hipErrorInvalidValue;
    if (N == 0) return hipSuccess;
    const float2* p = reinterpret_cast<const float2*>(pairs);
    if (S <= 8) band_sweep_bucket<8>(stream, p, starts, xn, yn, words, scores, emit_frames, N, T, U, S, topology);
    else if (S <= 16) band_sweep_bucket<16>(stream, p, starts, xn, yn, words, scores, emit_frames, N, T, U, S, topology);
    else if (S <= 32) band_sweep_bucket<32>(stream, p, starts, xn, yn, words, scores, emit_frames, N, T, U, S, topology);
    else band_sweep_bucket<64>(stream, p, starts, xn, yn, words, scores, emit_frames, N, T, U, S, topology);
    return hipGetLastError();
}

}  // namespace rnnt
