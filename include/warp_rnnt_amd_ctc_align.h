/* Best-path (Viterbi) forced alignment of the CTC lattice: additive entries of libwarp_rnnt_amd.so (they did not move the
 * C-ABI version -- nothing that was there moves).
 *
 * What rnnt_amd_align, rnnt_amd_tdt_align and rnnt_amd_pruned_align give the transducer lattices, for the CTC head of
 * warp_rnnt_amd_ctc.h: the score of the best path, the token of every frame on it and the frame at which every label starts.
 *
 * inputs (N,T,V) of `dtype`, batch-major and contiguous; labels (N,L) int32, padded; xn, yn (N,) int32: the frames T_n and
 * the labels L_n of utterance n.  A label that is no index of [0,V) is read as the blank, as the CTC loss reads it.
 *
 * States.  Utterance n has the states s = 0 .. 2 L_n: even s = 2 l is the blank in front of label l (l = L_n: the final
 * blank), odd s = 2 l + 1 is label l.  token(l) = labels[n,l] as read above.
 *
 * Emissions.  e(t,s) = E[n,t,0] for even s and E[n,t,1+l] for s = 2 l + 1, with E (N,T,L+1) fp32, FLOOR = -1e30f:
 *
 *     RNNT_CTC_ALIGN_IN_LOGITS     the plane the CTC loss forms from the same logits, bit for bit (warp_rnnt_amd_ctc.h,
 *                                  "Emissions"): E[n,t,k] = max(((float)z[v] - m) - ls, FLOOR)
 *     RNNT_CTC_ALIGN_IN_LOG_PROBS  the values as they are, not normalised: E[n,t,k] = max((float)lp[n,t,v], FLOOR)
 *
 * (v = blank for k = 0, token(k-1) otherwise).  Only the columns k <= L_n of the rows t < T_n are read and written.
 *
 * Recurrence, fp32, one add per state and frame, each rounded on its own:
 *
 *     v(0,0) = e(0,0);  v(0,1) = e(0,1) if L_n > 0;  every other v(0,s) = FLOOR
 *     t > 0:  stay = v(t-1,s)
 *             step = v(t-1,s-1)           (s > 0, else FLOOR)
 *             skip = v(t-1,s-2)           (s odd, s >= 3, token(l) != token(l-1); else FLOOR)
 *             d(t,s) = 0 if stay >= step and stay >= skip,  else 1 if step >= skip,  else 2
 *             v(t,s) = max(e(t,s) + (the chosen one), FLOOR)
 *     end:    the final blank 2 L_n if L_n == 0 or v(T_n-1, 2 L_n) >= v(T_n-1, 2 L_n - 1), else the last label 2 L_n - 1
 *     score = v(T_n-1, end)
 *
 * One tie rule everywhere: of equal predecessors the one with the highest state index wins.  Every value is finite.
 *
 * Walk back.  s(T_n-1) = end, s(t-1) = s(t) - d(t, s(t)).
 *
 *     scores[n]         = score
 *     frame_tokens[n,t] = blank for even s(t), token(l) for s(t) = 2 l + 1;  -1 for t >= T_n
 *     emit_frames[n,l]  = the first frame t with s(t) = 2 l + 1;             -1 for l >= L_n
 *
 * A score at or below FLOOR / 2 means no path -- T_n < L_n + the adjacent repeats, or every path runs through a masked
 * (-inf) entry: the score is written as -inf and both rows as -1.  Lengths outside 1 <= xn[n] <= T, 0 <= yn[n] <= L: nothing
 * of the utterance is read, its score is NaN and both rows are -1.  Nothing outside an utterance's own outputs is written
 * for it, and its bits do not depend on the batch around it.  NaN input is unspecified.
 *
 * Decision words.  One wave of 64 lanes works on an utterance; lane j owns the K = 1, 2, 4, 8 or 16 (the least power of two
 * with 64 K >= L + 1) label positions j K .. j K + K - 1, that is the states 2 j K .. 2 j K + 2 K - 1.  The word of (n, t, j),
 * at index (n T + t) 64 + j of the decisions, holds d(t, 2 j K + q) in its bits 2 q and 2 q + 1: 32-bit words for K <= 8,
 * 64-bit words for K = 16.  Written for 1 <= t < T_n of an utterance with lengths the entry takes, unspecified elsewhere.
 * The walk back takes the frames in blocks of 128 (64-bit words: 64).
 *
 * Shapes: N >= 0, T >= 1, 1 <= L <= 1023, 2 <= V <= 16384, 0 <= blank < V, N*T*(L+1) < 2^31.  Everything else -- and an
 * unknown input_kind or dtype, a null inputs / labels / xn / yn / scores / frame_tokens / emit_frames, a workspace that is
 * null or off a multiple of 256 bytes, inputs off a multiple of their element size, labels / xn / yn / scores /
 * frame_tokens / emit_frames off a multiple of 4 -- comes back as RNNT_STATUS_INVALID_ARGUMENT before any HIP call.  N == 0
 * succeeds without a launch.  A failed emission launch: RNNT_STATUS_PROLOGUE_FAILED; a failed sweep launch:
 * RNNT_STATUS_WARP_FAILED.  The call only enqueues (no read-back, no allocation, no memset): it can be captured into a graph.
 */
#ifndef WARP_RNNT_AMD_CTC_ALIGN_H
#define WARP_RNNT_AMD_CTC_ALIGN_H

#include "warp_rnnt_amd.h"

/* input_kind: what `inputs` holds */
#define RNNT_CTC_ALIGN_IN_LOGITS 0    /* (N,T,V) logits of `dtype` */
#define RNNT_CTC_ALIGN_IN_LOG_PROBS 1 /* (N,T,V) log-probs of `dtype` */

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of the workspace, a function of the shape alone; 0 for a shape the entry refuses.  Every piece on a multiple of 256
 * bytes:
 *     offset 0:                        (m, ls) per row (N,T,2) fp32, written for RNNT_CTC_ALIGN_IN_LOGITS only;
 *     offset round_up(8*N*T, 256):     the emission plane E (N,T,L+1) fp32, still there when the call returns;
 *     behind it (round_up(4*N*T*(L+1), 256) more): the decision words, N*T*64 of 4 bytes (L <= 511) or 8 bytes. */
size_t rnnt_amd_ctc_align_workspace_size(int N, int T, int L, int V);

rnntStatus_t rnnt_amd_ctc_align(rnntStream_t stream, void *workspace, int input_kind, int dtype, const void *inputs,
                                const int *labels, const int *xn, const int *yn, float *scores /* (N,) */,
                                int *frame_tokens /* (N,T) */, int *emit_frames /* (N,L) */, int N, int T, int L, int V,
                                int blank);

#ifdef __cplusplus
}
#endif
#endif /* WARP_RNNT_AMD_CTC_ALIGN_H */
