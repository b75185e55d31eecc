/*
 * mgp_anyd.h -- C ABI of libmgp's any-dimension training entry points: what SGPR training needs beyond mgp.h once the
 * inputs have more than MGP_FUSED_MAX_D dimensions.  Same conventions as mgp.h (device pointers, row-major,
 * contiguous, 0 or a negative MGP_E_* code, work enqueued on the handle's stream); the functions live in the same
 * libmgp.so.
 */
#ifndef MGP_ANYD_H
#define MGP_ANYD_H

#include "mgp.h"

#ifdef __cplusplus
extern "C" {
#endif

/* mgp_kmn_knm_vjp at any input dimension 1 <= D <= MGP_MAX_D, with the row panel as an argument.  Arguments, outputs,
 * argument checks and error codes are mgp_kmn_knm_vjp's (mgp.h): the cotangent of K = k(X, Z) is
 *     W = K (Gq + Gq^T) + Y Gb^T                          (Gq = NULL: W = Y Gb^T alone, P >= 1 with Y and Gb required)
 * and dvariance, dlengthscales[0:D] (host doubles; entries >= D are not touched) and dZ [M, D] (device, may be NULL:
 * not computed) are its contractions with the kernel's derivatives.  fp64 only (MGP_E_DTYPE); N >= 0, M >= 1, P >= 0
 * (MGP_E_SHAPE); N = 0 writes zeros.  Synchronises the stream.
 *
 * panel_rows: 0 = the rule of mgp_kmn_knm_vjp (at most 256 MiB of K per row panel); > 0 = that many rows of X per
 * panel (the last panel may be shorter; any value is legal, small ones are for tests); < 0: MGP_E_SHAPE.
 *
 * D <= MGP_FUSED_MAX_D: the implementation behind mgp_kmn_knm_vjp (csrc/kmn_grad.hip); with panel_rows = 0 the
 * results are that entry point's bit for bit.
 *
 * D > MGP_FUSED_MAX_D (csrc/kmn_grad_generic.hip), per row panel:
 *   1. K_panel = k(X_panel, Z), direct differences, dimensions staged 16 at a time     (not formed when Gq = NULL)
 *   2. W_panel = K_panel (Gq + Gq^T) [+ Y_panel Gb^T] by the fp64 MFMA NT GEMM         (Gq = NULL: Y_panel Gb^T alone)
 *   3. slope kernel: r2 of every pair again over the dimension slices (64 x 64 tiles, 4 x 4 pairs per thread), the
 *      W f share of dvariance, and H = W f' written over W
 *   4. pair kernel: a lane owns one column m and one slice of 32 dimensions (z_m's slice and its 2 x 32 sums in
 *      registers), the rows of its row block staged through LDS; it reads H_nm once per slice and adds
 *      H (a - b)^2 to the lengthscale sums and H (a - b) to dZ's
 *   5. the row-block partials are added to running sums in block order
 * and at the end dl_d = variance (-2 / l_d) sum, dZ[m, d] = variance (-2 / l_d) sum.  No float atomics: every sum is
 * taken in a fixed order, two calls give the same bits, and row shards of X (and Y) add up to the whole up to
 * rounding.  Matern-1/2 adds exactly 0 to dlengthscales and dZ for a pair at GPflow's r2 floor of 1e-36.
 *
 * Scratch (D > MGP_FUSED_MAX_D), one arena of the handle (counted by mgp_workspace_bytes, MGP_E_NOMEM from a fixed
 * pool that is too small): 16 R M + 8 M^2 bytes of panels (8 R M when Gq = NULL), R = the panel rows, plus
 * 8 (B M D [dZ only] + B C S 32 + T + M D [dZ only] + D + 1) + 2048 bytes of partials, C = ceil(M / 256),
 * S = ceil(D / 32), T = ceil(R / 64) ceil(M / 64) and B = the row blocks of a panel,
 *     B <= min(ceil(4 CUs / (C S)), ceil(R / 32), dZ ? max(1, 2^27 / (8 M D)) : unbounded)
 * so the [B, M, D] partials of dZ never exceed 128 MiB unless one [M, D] block alone does: at M = 4096, D = 512 the
 * partials and running sums of this route stay below the 256 MiB of the panel they serve. */
int mgp_kmn_knm_vjp_anyd(mgp_handle* h, const mgp_kernel* k, const void* X, int64_t N, const void* Z, int64_t M,
                         const void* Gq, const void* Y, const void* Gb, int32_t P, int64_t panel_rows,
                         double* dvariance, double* dlengthscales, void* dZ);

#ifdef __cplusplus
}
#endif

#endif /* MGP_ANYD_H */
