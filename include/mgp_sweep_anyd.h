/*
 * mgp_sweep_anyd.h -- C ABI of libmgp's fused matrix-free sweeps at any input dimension: K_nm v, K_mn w and
 * (K_xx + s2 I) v without a kernel panel in memory once the inputs have more than MGP_FUSED_MAX_D dimensions.  Same
 * conventions as mgp.h (device pointers, row-major, contiguous, 0 or a negative MGP_E_* code, work enqueued on the
 * handle's stream); the functions live in the same libmgp.so.
 *
 * Opt-in: the plain names (mgp_knm_matvec, mgp_kmn_matvec, mgp_kxx_matvec) and the plain operator kinds keep their
 * dispatch -- above MGP_FUSED_MAX_D they write k(A_chunk, B_chunk) panels (direct differences) and multiply them.
 *
 * fp64 and D > MGP_FUSED_MAX_D (csrc/sweep_anyd.hip): the squared distance comes out of the fp64 matrix cores in its
 * expansion form, -s = 2 a.b - |a|^2 - |b|^2, with the K dimension of the product augmented by |a|^2, 1 / -1, -|b|^2
 * and walked in slices of 32 columns; the profile is applied once, after the last slice.  The expansion form cancels:
 * its error grows with |a|^2 + |b|^2 (so with D for data of a given spread), where the panel route's direct
 * differences do not -- the reason these names are opt-in.  No float atomics: two calls give the same bits, and row
 * shards of the streamed set add up to the whole up to rounding.
 * fp32, or D <= MGP_FUSED_MAX_D: exactly the code of the plain name or kind, and its bits.
 *
 * Scratch (fused route): the `ws` arena of the handle alone (counted by mgp_workspace_bytes; MGP_E_NOMEM from a fixed
 * pool that is too small), 8 (na + nb + [chunks > 1] chunks na RC) bytes for na owned and nb streamed points -- the
 * two squared-norm vectors and the per-chunk partials of the widest column pass RC (8, 4, 2 or 1).  The generic-D
 * arena (`gen`) is never touched.
 */
#ifndef MGP_SWEEP_ANYD_H
#define MGP_SWEEP_ANYD_H

#include "mgp.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Operator kinds of mgp_operator.kind, beside those of mgp.h.  Fields, checks, error codes and empty-input behaviour
 * are those of MGP_OP_SGPR, MGP_OP_KMM_LAMBDA and MGP_OP_KXX_NOISE (for MGP_OP_SGPR_ANYD the multi-rank fields too: the
 * collective is untouched, only the two local sweeps change); mgp_pcg_solve, mgp_pcg_solve_record and
 * mgp_operator_apply take them.  Inside a solve MGP_OP_SGPR_ANYD defers exactly as MGP_OP_SGPR does (the fused update
 * reads the all-reduced partial of a collective in place): the deferral concerns the collective, not the sweeps. */
enum { MGP_OP_SGPR_ANYD = 5, MGP_OP_KMM_LAMBDA_ANYD = 6, MGP_OP_KXX_NOISE_ANYD = 7 };

/* MGP_OP_KMM_LAMBDA_WIDE_ANYD: the many-column form of (k(Z, Z) + diag lambda) above MGP_FUSED_MAX_D dimensions,
 * out[Bt, M] = P[Bt, M] (k(Z, Z) + diag lambda) with no kernel panel in memory (csrc/kmm_wide_anyd.hip).  Fields
 * (kernel, Z, M == n, lambda), checks, error codes and empty-input behaviour are those of MGP_OP_KMM_LAMBDA;
 * mgp_operator_apply, mgp_pcg_solve and mgp_pcg_solve_record take it wherever they take MGP_OP_KMM_LAMBDA_WIDE, with
 * the same gate word inside a solve, where Z is packed once before the loop and the pack held to the end of the solve.
 *
 * fp64 and MGP_FUSED_MAX_D < D <= MGP_MAX_D: a workgroup owns 64 output elements and all right-hand sides of a group
 * of at most 256 (more go in groups of 256 and a remainder), forms every 16 x 16 tile of -s = 2 a.b - |a|^2 - |b|^2
 * on the fp64 matrix cores as mgp_sweep_anyd.h's sweeps do (K = D + 2 in slices of 32 columns, k ascending, the
 * profile once after the last slice) and contracts the profiled tile with the 16 x r panel of P on the matrix cores
 * too: every kernel value is evaluated once per group, not once per 8 right-hand sides.  When ceil(M / 64) workgroups
 * leave compute units idle the streamed side is split; the splits' tiles are added in split order.  No float atomics:
 * two calls give the same bits.
 * fp64 and D <= MGP_FUSED_MAX_D: exactly the code of MGP_OP_KMM_LAMBDA_WIDE, and its bits.
 * fp32: exactly the code of MGP_OP_KMM_LAMBDA, and its bits.
 *
 * Scratch (fp64, D > MGP_FUSED_MAX_D): the `prj` arena of the handle alone (counted by mgp_workspace_bytes;
 * MGP_E_NOMEM from a fixed pool that is too small, never an allocation),
 *     bytes = align256(8 * 64 * KS * ceil(M / 16)) + align256(8 * nsplit * 64 * ceil(M / 64) * RP),
 * KS = ceil((D + 2) / 4), RP = min(Bt, 256) rounded up to a multiple of 16, align256 = rounding up to 256 bytes, and
 *     nsplit = ceil(M / rows),  rows = ceil(ceil(M / s) / 32) * 32,  s = clamp(ceil(2 CUs / ceil(M / 64)), 1, ceil(M / 256))
 * -- the pack of Z (scaled points, squared norms, in matrix-core operand order) and the split tiles of the widest group.
 *
 * Error bound.  The distance is the expansion form, so a kernel value carries the per-pair error of mgp_sweep_anyd.h's
 * sweeps, which grows with |a|^2 + |b|^2 -- the reason the kind is opt-in.  With u = 2^-53,
 *     |out[b, j] - exact| <= sum_i |P[b, i]| pairbound(i, j) + u (terms + nsplit + 3) sum_i |P[b, i] K[i, j]|
 *                            + 2 u |lambda_j P[b, j]|,
 * pairbound(i, j) = K[i, j] times the relative bound of one pair: (D + 6) u (|a_i| + |b_j|)^2-type distance error
 * through the profile plus 8 u of function error (tests/pair_reference.py: pair_bound); terms = rows, the longest chain
 * of products accumulated into one output by one split; nsplit for the sum of the splits; 3 for the rounding of the
 * product with the variance, of lambda_j P[b, j] and of the final sum. */
enum { MGP_OP_KMM_LAMBDA_WIDE_ANYD = 8 };

/* out [N, R] = k(X, Z) V: the arguments, checks and layouts of mgp_knm_matvec. */
int mgp_knm_matvec_anyd(mgp_handle* h, const mgp_kernel* k, const void* X, int64_t N, const void* Z, int64_t M,
                        const void* V, int32_t R, int v_layout, void* out, int out_layout);

/* out [M, R] = k(Z, X) W: the arguments, checks and layouts of mgp_kmn_matvec.  The N streamed rows are cut into
 * chunks whose partials are added in chunk order. */
int mgp_kmn_matvec_anyd(mgp_handle* h, const mgp_kernel* k, const void* X, int64_t N, const void* Z, int64_t M,
                        const void* W, int32_t R, int w_layout, void* out, int out_layout);

/* out [N, R] = (k(X, X) + s2 I) V: the arguments, checks and layouts of mgp_kxx_matvec (every ordered pair is
 * evaluated: the plain sweep with s2 V as its addend). */
int mgp_kxx_matvec_anyd(mgp_handle* h, const mgp_kernel* k, const void* X, int64_t N, double s2, const void* V,
                        int32_t R, int v_layout, void* out, int out_layout);

#ifdef __cplusplus
}
#endif

#endif /* MGP_SWEEP_ANYD_H */
