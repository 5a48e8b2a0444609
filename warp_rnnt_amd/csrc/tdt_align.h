// Launch interface of the best-path kernels over the token-and-duration (TDT) lattice (tdt_align.hip) for the C ABI of
// include/warp_rnnt_amd_tdt_align.h.  The producer is tdt.hip's launch_tdt_plane, unchanged; the duration set and its
// bounds are tdt.h's.
//
// The definition.  Per cell the plane holds, in fp32, tb = tok[blank] and tl = tok[labels[u]] (sigma already subtracted
// from both) and dur[i].  For utterance n, T_n = xn[n], U_n = yn[n].  Everything is in fp32, every add is rounded on its
// own, and the association is the one k_tdt_sweep uses: weight first, then v + weight.
//
//     v(0,0) = 0, code(0,0) = 255
//     for every other cell (t,u), 0 <= t < T_n, 0 <= u <= U_n, and for the end cell (T_n, U_n):
//         best = -inf, code = 255
//         for i = 0..D-1, d = durations[i]:            (durations in the order given; blank before label)
//             if d > 0 and t-d >= 0:                    c = v(t-d,u)   + (tb(t-d,u)   + dur_i(t-d,u));     if c > best: best = c, code = 2i
//             if u > 0 and t-d >= 0 and t < T_n:        c = v(t-d,u-1) + (tl(t-d,u-1) + dur_i(t-d,u-1));   if c > best: best = c, code = 2i+1
//         v(t,u) = best
//     scores[n] = v(T_n, U_n)                           (only blank edges reach the end cell)
//
// A candidate replaces the running best only when strictly greater, so a tie stays with the earlier candidate; a cell
// that nothing finite reaches keeps code 255.  The path is read back from the end cell along the codes: code k is edge
// i = k >> 1 of kind k & 1, leading back to (t - durations[i], u - (k & 1)).  For the label edge out of (t,u) with
// duration d, emit_frames[n,u] = t and emit_durations[n,u] = d; both are -1 for U_n <= u < U-1.  An utterance whose score
// is -inf has no path and gets -1 in both rows.  A finite score implies finite v and a valid code on every cell of the
// path.  Among all paths of maximal score the rule returns the one whose sequence of codes, read from the last edge to
// the first, is lexicographically smallest.  -inf logits are legal, NaN input is unspecified; lengths outside
// [1,T] x [0,U-1] give a NaN score and -1 rows, and nothing outside that utterance's own outputs is read or written.
#pragma once
#include <hip/hip_runtime.h>

#include "tdt.h"

namespace rnnt {

constexpr unsigned char TDT_ALIGN_NO_EDGE = 255;          // the code of (0,0) and of a cell that nothing finite reaches

// decision bytes: dec[n][d][u] with d = t + u in [0, T+U), the code of cell (d-u, u); written for every cell of the
// utterance's window and for its end cell, unspecified elsewhere
inline size_t tdt_align_dec_count(int N, int T, int U) { return (size_t)N * ((size_t)T + U) * U; }

// The max-plus sweep over launch_tdt_plane's plane: dec as above, scores[n] = v(T_n, U_n) (NaN for an utterance whose
// lengths are out of range).  One workgroup per utterance, U <= TDT_MAX_U.
hipError_t launch_tdt_align_sweep(hipStream_t stream, const float* plane, const int* xn, const int* yn, unsigned char* dec,
                                  float* scores, const TdtDurations& dur, int N, int T, int U);
// The path of every utterance from dec and scores: emit_frames, emit_durations (N,U-1), the -1 tails, -1 throughout where
// scores[n] is -inf or the lengths are out of range.  One wave per utterance.
hipError_t launch_tdt_align_trace(hipStream_t stream, const unsigned char* dec, const int* xn, const int* yn,
                                  const float* scores, int* emit_frames, int* emit_durations, const TdtDurations& dur, int N,
                                  int T, int U);

}  // namespace rnnt
