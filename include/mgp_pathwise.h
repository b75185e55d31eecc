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

#ifdef __cplusplus
}
#endif

#endif /* MGP_PATHWISE_H */
