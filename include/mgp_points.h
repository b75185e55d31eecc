/*
 * mgp_points.h -- C ABI of libmgp's dense-cotangent kernel VJP in the points: what training needs beyond mgp.h once
 * the inducing inputs of a dense model are trainable.  Same conventions as mgp.h (device pointers, row-major, 0 or a
 * negative MGP_E_* code, work enqueued on the handle's stream); the function lives in the same libmgp.so.
 */
#ifndef MGP_POINTS_H
#define MGP_POINTS_H

#include "mgp.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The VJP of a dense kernel block K = k(A, B) [na, nb] at a dense cotangent G = dL/dK (row-major, leading dimension
 * ldg >= nb), in the hyper-parameters and in the points, each pair evaluated without any [., ., D] temporary.  With
 * a = A / l, b = B / l, r2 from direct differences, f = k / variance and f' = df/dr2 as mgp_k_dense_vjp forms them:
 *     dvariance        = sum_ij G_ij f_ij
 *     dlengthscales[d] = variance (-2 / l_d) sum_ij G_ij f'_ij (a_id - b_jd)^2
 *     dA[i, d]         = variance ( 2 / l_d) sum_j  G_ij f'_ij (a_id - b_jd)
 *     dB[j, d]         = variance (-2 / l_d) sum_i  G_ij f'_ij (a_id - b_jd)
 * dvariance and dlengthscales[0:D] are host doubles (entries >= D are not touched) and are mgp_k_dense_vjp's
 * quantities; dA [na, D] and dB [nb, D] are device buffers, contiguous, and either may be NULL: not computed.  A and B
 * may be the same pointer: dA + dB is then the derivative of sum_ij G_ij k(z_i, z_j) in Z.  A, B and G are not written.
 *
 * fp64 only (MGP_E_DTYPE); 1 <= D <= MGP_MAX_D and na, nb >= 0 (MGP_E_SHAPE); ldg < nb: MGP_E_SHAPE; NULL dvariance
 * or dlengthscales: MGP_E_BADARG; na = 0 or nb = 0 writes zeros to every output that is not NULL.  Synchronises the
 * stream (it returns host doubles).
 *
 * panel_rows: rows of A per panel.  0 = the library's rule R0 below (no scratch panel above 256 MiB); > 0 = that many
 * (the last panel may be shorter; any value is legal, small ones are for tests), except that above MGP_FUSED_MAX_D a
 * panel never has more than 2^21 rows (its row tiles are a grid dimension); < 0: MGP_E_SHAPE.  The caps of 256 MiB on
 * H and H^T and of 128 MiB on one block of dA partials are properties of R0: a positive panel_rows larger than R0
 * lifts them, and the scratch is then whatever the formula below gives for that R.
 *
 * The Matern slopes are exactly 0 at GPflow's r2 floor of 1e-36, so a pair of coincident points adds exactly 0 to
 * dlengthscales, dA and dB and never a NaN.  No float atomics: every sum is taken in a fixed order, two calls give the
 * same bits, and row shards of A (with the matching rows of G) add up to the whole in dvariance, dlengthscales and dB
 * up to rounding.
 *
 * D <= MGP_FUSED_MAX_D (DP = D padded to 2, 4, 8, 16 or 32): per panel two pair kernels, one whose lanes own a column
 * (dB, dlengthscales, dvariance) and one whose lanes own a row (dA); G is read twice.
 * D > MGP_FUSED_MAX_D: per panel a slope kernel reads G once and writes H = G f' [R, nb] and, when dA is wanted,
 * H^T [nb, R]; kernels whose lanes own a point and a slice of 32 dimensions read H (dB, dlengthscales) and H^T (dA).
 *
 * Scratch, one arena of the handle (counted by mgp_workspace_bytes, MGP_E_NOMEM from a fixed pool that is too small),
 * with al(x) = x rounded up to 256, c(x, y) = ceil(x / y), R = min(na, panel_rows or R0) and (D > 32) at most 2^21,
 * W = DP or (D > 32) D, S = 1 or (D > 32) c(D, 32), dA? and dB? 1 when that output is wanted and 0 otherwise:
 *     R0  = 2^24 / DP                                              D <= 32
 *         = max(16, min(2^25 / nb, 2^24 / D) rounded down to 16), at most 2^21          D > 32
 *     Bb  = max(1, min(c(4 CUs, c(nb, 256) S), c(R, 32), dB? ? 2^24 / (nb W) : inf))    row blocks
 *     Ba  = max(1, min(c(4 CUs, c(R, 256) S), c(nb, 32), 2^24 / (R W)))                 column blocks
 *     bytes = dB? al(8 Bb nb W) + dA? al(8 Ba R W) + dB? al(8 nb W)
 *           + al(8 Bb c(nb, 256) (DP + 1)) + al(8 (DP + 1))                                       D <= 32
 *           + al(8 Bb c(nb, 256) 32 S) + al(8 c(nb, 64) c(R, 64)) + al(8 (32 S + 1))
 *           + (1 + dA?) al(8 R nb)                                                                D > 32
 * (CUs = the device's compute units, 256 on an MI355X): O((na + nb) D) plus block partials, and the [blocks, ., W]
 * partials of dA and of dB never exceed 128 MiB each unless one block alone does, which R0 excludes for dA.  Nothing
 * of size na x nb x D exists. */
int mgp_k_dense_vjp_points(mgp_handle* h, const mgp_kernel* k, const void* A, int64_t na, const void* B, int64_t nb,
                           const void* G, int64_t ldg, int64_t panel_rows, double* dvariance, double* dlengthscales,
                           void* dA, void* dB);

#ifdef __cplusplus
}
#endif

#endif /* MGP_POINTS_H */
