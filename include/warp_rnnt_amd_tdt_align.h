/* Best-path alignments over the token-and-duration (TDT) lattice: additive entries of libwarp_rnnt_amd.so (they did not
 * move the C-ABI version -- nothing that was there moves).
 *
 * Logits (N,T,U,V+D), durations, blank and sigma exactly as rnnt_amd_tdt_loss_logits reads them
 * (warp_rnnt_amd_tdt.h).  The loss's producer fills its plane; per cell the plane holds, in fp32:
 *
 *     tb = tok[blank]
 *     tl = tok[labels[u]], with sigma already subtracted from both
 *     dur[i]
 *
 * For utterance n, T_n = xn[n], U_n = yn[n].  Everything is in fp32, every add is rounded on its own, and the association
 * is the one the loss's alpha sweep uses: weight first, then v + weight.
 *
 *     v(0,0) = 0, code(0,0) = 255
 *     for every other cell (t,u), 0 <= t < T_n, 0 <= u <= U_n, and for the end cell (T_n, U_n):
 *         best = -inf, code = 255
 *         for i = 0..D-1, d = durations[i]:            (durations in the order given; blank before label)
 *             if d > 0 and t-d >= 0:                    c = v(t-d,u)   + (tb(t-d,u)   + dur_i(t-d,u));     if c > best: best = c, code = 2i
 *             if u > 0 and t-d >= 0 and t < T_n:        c = v(t-d,u-1) + (tl(t-d,u-1) + dur_i(t-d,u-1));   if c > best: best = c, code = 2i+1
 *         v(t,u) = best
 *     scores[n] = v(T_n, U_n)                           (only blank edges reach the end cell)
 *
 * A candidate replaces the running best only when strictly greater, so a tie stays with the earlier candidate.  A cell
 * that nothing finite reaches keeps code 255.  The path is read back from the end cell along the codes: code k is edge
 * i = k >> 1 of kind k & 1, leading back to (t - durations[i], u - (k & 1)).  For the label edge out of (t,u) with
 * duration d, emit_frames[n,u] = t and emit_durations[n,u] = d; both are -1 for U_n <= u < U-1.  An utterance whose score
 * is -inf has no path and gets -1 in both rows -- for example T_n <= U_n when 0 is not among the durations, or masked
 * logits.  A finite score implies finite v and a valid code on every cell of the path.  Among all paths of maximal score
 * the rule returns the one whose sequence of codes, read from the last edge to the first, is lexicographically smallest.
 *
 * -inf logits are legal; NaN input is unspecified.  An utterance with xn[n] outside [1,T] or yn[n] outside [0,U-1] gets
 * scores[n] = NaN and -1 rows, and nothing outside that utterance's own outputs is read or written.
 *
 * Refused with RNNT_STATUS_INVALID_ARGUMENT before any HIP call, as by rnnt_amd_tdt_loss_logits: an unknown dtype,
 * durations that are not D distinct integers in [0,8] with 1 among them, V < 2, a blank outside [0,V), U > 1024 or sizes
 * rnnt_amd_tdt_workspace_size refuses, sigma < 0 or not finite, a null or misaligned workspace, a null or misaligned
 * logits / scores, a misaligned emit_frames / emit_durations / labels / xn / yn, a null xn / yn / durations, U > 1 without
 * labels or without either output row.  N == 0 succeeds without a launch.  A failed producer launch:
 * RNNT_STATUS_PROLOGUE_FAILED; a failed sweep or trace launch: RNNT_STATUS_WARP_FAILED.  The call only enqueues (no
 * read-back, no allocation): it can be captured into a graph.
 */
#ifndef WARP_RNNT_AMD_TDT_ALIGN_H
#define WARP_RNNT_AMD_TDT_ALIGN_H

#include "warp_rnnt_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of workspace for (N,T,U,D): a function of the shape alone; 0 for whatever rnnt_amd_tdt_workspace_size refuses.
 * With cells = N*T*U and every piece on a multiple of 256 bytes:
 *     offset 0:                               the plane, (2+D) channels of `cells` fp32 -- tb, tl, dur[0..D) -- each in the
 *                                             diagonal-major cell order sk(n,t,u) = (n*T + (t+u) mod T)*U + u: bit for bit
 *                                             what rnnt_amd_tdt_loss_logits leaves at offset 0 of its own workspace, and
 *                                             still there when the call returns;
 *     offset round_up(4*(2+D)*cells, 256):    the decision bytes dec[n][d][u], d = t+u in [0, T+U), N*(T+U)*U of them:
 *                                             the code of cell (d-u, u), written for every cell of the utterance's window
 *                                             and for its end cell; unspecified elsewhere. */
size_t rnnt_amd_tdt_align_workspace_size(int N, int T, int U, int D);

/* durations: D integers in HOST memory, read during the call. */
rnntStatus_t rnnt_amd_tdt_align(rnntStream_t stream, void *workspace, int dtype, const void *logits, const int *labels,
                                const int *xn, const int *yn, const int *durations /* host */, int D,
                                float *scores /* (N,) */, int *emit_frames, int *emit_durations /* (N,U-1); NULL iff U == 1 */,
                                int N, int T, int U, int V, int blank, float sigma);

#ifdef __cplusplus
}
#endif
#endif /* WARP_RNNT_AMD_TDT_ALIGN_H */
