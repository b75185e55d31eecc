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
