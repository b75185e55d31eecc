/*
 * mgp_pathwise.h -- C ABI of libmgp's pathwise-training entry points: what a bound built on pathwise posterior
 * samples needs beyond mgp.h.  Same conventions as mgp.h (device pointers, row-major, contiguous, 0 or a negative
 * MGP_E_* code, work enqueued on the handle's stream); the functions live in the same libmgp.so.
 */
#ifndef MGP_PATHWISE_H
#define MGP_PATHWISE_H

#include "mgp.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Backward pass of mgp_rff_sample (csrc/rff_grad.hip; the reference differentiates cggp/rff.py:48-73 by TensorFlow's
 * tape).  With phi_nl = theta_l . x_n and the cotangent G(s, n) of out(s, n):
 *     q(n, l)      = scale * sum_s G(s, n) (W[s, L + l] cos phi_nl - W[s, l] sin phi_nl)
 *     dtheta[l, d] = sum_n q(n, l) x_n[d]          [L, D]
 *     dX[n, d]     = sum_l q(n, l) theta_l[d]      [N, D]
 * X [N, D], theta [L, D] (radians), W [S, 2L] (cos block first), G [S, N] (g_layout = MGP_ROWS) or [N, S] (MGP_COLS).
 * Either output may be NULL, not both (MGP_E_BADARG).  The derivative in `scale` needs no kernel: sum(G o out) / scale.
 * fp64 only (anything else: MGP_E_DTYPE); 1 <= D <= MGP_FUSED_MAX_D and 1 <= S <= 8 (else MGP_E_BADARG, the message
 * names the value); N, L >= 0 (MGP_E_SHAPE); scale finite.  N = 0 writes zeros to dtheta and nothing to dX; L = 0 writes
 * zeros to dX and nothing to dtheta.
 *
 * Arithmetic: the phases are the forward's bit for bit (theta / (2 pi) formed once, the fma chain over d in
 * revolutions, t - rint(t) exact, the polynomial pair after the quadrant split: csrc/rff_math.h).  For dtheta a lane
 * owns a basis and the records [x_n | G(:, n)] are streamed; for dX a lane owns a row and the forward's basis records
 * [theta_l / (2 pi) | W[:, l] | W[:, L + l]] are streamed, the factor 2 pi scale applied once at the end.  The streamed
 * side is cut into `chunks` equal pieces (the last may be shorter):
 *     owners  = 256 * (D <= 8 ? 2 : 1)                       owned points per workgroup
 *     blocks  = ceil(owned / owners)
 *     chunks  = blocks >= 4 CUs ? 1 : min(ceil(4 CUs / blocks), ceil(streamed / 32), 256)
 *     len     = ceil(streamed / chunks),  chunks = ceil(streamed / len)
 * One output element is a chain of at most `len` fmas, then (chunks > 1) `chunks` additions in chunk order and one
 * multiplication.  No atomics: two calls give the same bits.
 *
 * Error (u = 2^-53): |dtheta[l, d] - exact| <= u (8 (1 + max_nl sum_d |x_nd theta_ld|) + 2 S + D + len + chunks + 4)
 *                                               |scale| sum_n sum_s |G(s, n)| (|W[s, l]| + |W[s, L + l]|) |x_n[d]|
 * -- the per-feature bound of rff_math.h, the roundings of the 2 S products and fmas of q's two sums, the D-term
 * phase chain (already inside the feature bound; counted again for the products q x_d), the accumulation chain, and 4
 * for the two products of q, the final scaling and (dX) theta / (2 pi) 2 pi -- and the same for dX with theta_l[d] in
 * place of x_n[d] and the sum over l.  tests/test_gpu_rff_vjp.py holds every output to it.
 *
 * Scratch: arenas "gen" (the streamed records: 8 N (DP + S) + 256 bytes for dtheta, 8 L (DP + 2 S) + 256 for dX, DP
 * the smallest of 4, 8, 16, 32 that is >= D) and, where chunks > 1, "ws" (8 chunks owned D bytes); both are counted by
 * mgp_workspace_bytes and come from the fixed pool of mgp_create_ex when there is one (MGP_E_NOMEM if it does not fit,
 * never an allocation). */
int mgp_rff_sample_vjp(mgp_handle* h, int dtype, const void* X, int64_t N, int32_t D, const void* theta, int64_t L,
                       const void* W, int32_t S, double scale, const void* G, int g_layout,
                       void* dtheta /* or NULL */, void* dX /* or NULL */);

/* MGP_RFF_ANYD: OR into out_layout of mgp_rff_sample or g_layout of mgp_rff_sample_vjp (csrc/rff_anyd.hip).  The flag
 * is stripped and the layout word checked as without it (any other bit: MGP_E_BADARG).  With the flag, fp64,
 * MGP_FUSED_MAX_D < D <= MGP_MAX_D and 1 <= S <= 8, the call takes the fused any-D route below: no [N, 2L] feature
 * panel, forward or backward.  With the flag and anything else -- fp32, D <= MGP_FUSED_MAX_D, S > 8 -- the code is
 * exactly that of the plain call, with its bits and its refusals (forward: S > 8 is the panel route; backward: S > 8 is
 * MGP_E_BADARG naming S, fp32 is MGP_E_DTYPE).  Without the flag nothing changes: mgp_rff_sample_vjp still refuses
 * D > MGP_FUSED_MAX_D.  Empty inputs as on the plain calls (forward: N = 0 writes nothing, L = 0 writes zeros; backward:
 * N = 0 writes zeros to dtheta and nothing to dX, L = 0 the reverse; both outputs NULL: MGP_E_BADARG).
 *
 * Tile scheme: a 16 x 16 tile of phases in revolutions, t = sum_d x_d theta_d / (2 pi), comes out of
 * v_mfma_f64_16x16x4_f64.  Both point sets are packed per call in MFMA fragment order, zero padded to K = 4 KS columns,
 * KS = ceil(D / 4), and to whole tiles of 16 points; K is walked in slices of 8 k-steps, k ascending, one accumulator
 * per pair; the streamed side goes through LDS, every lane loads the owned side as its own operand; rff_math.h turns
 * the phase into sin / cos as on every route.  The tile then goes back in as the B operand of the contraction.  A
 * workgroup of four waves owns 64 points and streams the other side in tiles of 16:
 *     forward   owned rows n, streamed bases l:  out^T[s, n] += Wc^T[s, l] cos[l, n] + Ws^T[s, l] sin[l, n], S padded to 16
 *     dtheta    owned bases l, streamed rows n:  dtheta^T[d, l] += X^T[d, n] q[n, l]
 *     dX        owned rows n, streamed bases l:  dX^T[d, n] += theta^T[d, l] q[l, n]
 * with q = cos a - sin b, a = sum_s G_s W[s, L + l] and b = sum_s G_s W[s, l] two small matrix products over s; `scale`
 * is applied once at the end.  dtheta and dX are one kernel with the roles swapped; asking for both runs it twice.  The
 * output accumulator of a wave is ceil(D / 16) tiles of four doubles per lane (rounded up to one of 3, 4, 5, 6, 8, 10,
 * 12, 16; a padded tile multiplies zeros); above D = 256 the output dimensions are taken in groups = ceil(D / 256) equal
 * groups of at most 256 (1 group on the forward) and every group recomputes the phases.
 * Slots past the end of either point set are exact zeros in every fragment, weight and coordinate and are never stored.
 *
 * Split rule: the streamed side is cut into `nsplit` runs of `tps` tiles (the last may be shorter),
 *     wg      = ceil(owned / 64) * groups
 *     stiles  = ceil(streamed / 16)
 *     nsplit  = wg >= 2 CUs ? 1 : max(1, min(ceil(2 CUs / wg), ceil(stiles / 16), 256))
 *     tps     = ceil(stiles / nsplit),  nsplit = ceil(stiles / tps),  len = 16 tps
 * Every split writes a partial; a finish kernel adds the partials in split order and scales.  No float atomics: two
 * calls give the same bits.  Everything is packed per call: nothing is kept on the handle between calls.
 *
 * Scratch: the arena "gen" alone, counted by mgp_workspace_bytes, with a(x) = x rounded up to a multiple of 256,
 * To = ceil(owned / 16), Ts = ceil(streamed / 16), DT = 16 ceil(D / 16):
 *     forward   a(512 KS To) + a(512 KS Ts) + a(4096 Ts)              + (nsplit > 1 ? a(64 nsplit N) : 0)
 *     backward  a(512 KS To) + a(512 KS Ts) + a(2048 To) + a(2048 Ts) + (nsplit > 1 ? a(8 nsplit owned DT) : 0)
 * bytes, for both outputs the larger of the two passes, reserved once.  MGP_E_NOMEM from a fixed pool that is too
 * small, never an allocation.
 *
 * Error (u = 2^-53, K = 4 KS, P = max_nl sum_d |x_nd theta_ld|), per output element:
 *     |out(s, n) - exact|     <= u (8 + (K + 2) P + 2 len + nsplit + 2) |scale| sum_l (|W[s, l]| + |W[s, L + l]|)
 *     |dtheta[l, d] - exact|  <= u (8 + (K + 2) P + S + len + nsplit + 4)
 *                                |scale| sum_n sum_s |G(s, n)| (|W[s, l]| + |W[s, L + l]|) |x_n[d]|
 * and the same for dX with theta_l[d] in place of x_n[d] and the sum over l -- the sums of absolute terms of the bound
 * above.  8 + (K + 2) P is the per-feature bound of rff_math.h with its fma-chain term replaced by the order-free bound
 * of a K-term sum (the order in which the hardware adds the four products of a k-step is not documented): 1 u for
 * theta / (2 pi), K u for the products and additions, 1 u of slack for second-order terms, all relative to sum_d |x_d
 * theta_d|; 8 u for the argument scaling and the polynomials.  S (backward) is the order-free bound of the S-term sums
 * a and b; `len` the longest accumulation chain of one split, one product and one addition per streamed point (two on
 * the forward: the cos and the sin term), again order-free; `nsplit` the additions of the finish kernel; and 2
 * (forward) or 4 (backward) for the final scaling, the two products and the subtraction of q, and slack.
 * tests/test_gpu_rff_anyd.py holds every output to it. */
enum { MGP_RFF_ANYD = 16 };

#ifdef __cplusplus
}
#endif

#endif /* MGP_PATHWISE_H */
