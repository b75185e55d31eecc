/*
 * mgp_predict.h -- C ABI of libmgp's whole-test-set predictive variance of the sparse models: the quadratic form
 * q[b] = k(xs_b, Z) C k(Z, xs_b) for one symmetric [M, M] matrix C that does not depend on the test rows, so that
 * var(xs_b) = k(xs_b, xs_b) - q[b] (reference models.py:343-345, the CDGP variance with C = (K_mm + Lambda)^-1; GPflow
 * SGPR.predict_f with C = K_mm^-1 - s2 S^-1).  Same conventions as mgp.h (device pointers, row-major, contiguous, 0 or
 * a negative MGP_E_* code, work enqueued on the handle's stream); the function lives in the same libmgp.so.  mgp.h and
 * MGP_VERSION are untouched.
 *
 * Definition: q[b] = sum_i C_ii k_bi^2 + 2 sum_{i<j} C_ij k_bi k_bj with k_bi = k(xs_b, z_i) (variance included).  The
 * upper triangle of C defines the form: entries with i > j and the columns M ... ldc-1 of a row are never read, on
 * either route, so callers need not symmetrise C.  C is row-major with ldc >= M.
 *
 * fp64 and D <= MGP_FUSED_MAX_D (csrc/quadform.hip): k(Xs, Z) is never materialised.  A workgroup owns t = 128 test
 * rows and one block J of c = 128 columns of C; it walks i = 0 ... end of block J in steps of 16, evaluates the
 * 16 x 128 kernel panel once per step on the vector ALU (the expansion-form distance and profiles of mgp_kmn_knm,
 * values as mgp_k_dense to rounding) and contracts it with the 16 x 128 panel of C, masked to i < j, on the fp64 matrix
 * cores.  When the walk passes a 16-column tile of its own block that tile is final: it is doubled exactly, C_jj k_bj
 * is added and the result is dotted with k_bj.  Block J is paired with block nJ-1-J in one workgroup (nJ = ceil(M / c))
 * so that every workgroup walks nJ + 1 blocks; the per-block row sums [nJ, B'] go to the arena and a second kernel
 * adds them in block order and scales by variance^2.  No float atomics: two calls give the same bits.
 * fp32 or D > MGP_FUSED_MAX_D: the generic route -- the symmetric matrix built from the upper triangle of C, row panels
 * of at most 256 MiB of k(Xs, Z) through mgp_k_dense, the NT GEMM of the panel with that matrix and a row dot.  The
 * same results to rounding, equally deterministic.
 *
 * Scratch (arenas of the handle, each counted by mgp_workspace_bytes; MGP_E_NOMEM from a fixed pool that is too small,
 * with q untouched; a growing handle rounds an arena up by a quarter, a fixed pool starts each arena on a multiple of
 * 256).  Fused route, the arena of mgp_knm_project ("prj") alone: 8 nJ min(B', 2^16) rounded up to 256, plus
 * 8 M (D' + 1) bytes, B' = B rounded up to t, D' = D rounded up to 2, 4, 8, 16 or 32 (test rows go in chunks of 2^16).
 * Generic route, two arenas: in "prj" elem (M^2 + 2 p M) + 256 bytes with p = min(B, max(64, 2^28 / (elem M))) panel rows;
 * and in the reduction arena "ws" the contraction slices of the NT GEMM, s elem p M bytes when the product has fewer
 * than 2 CUs tiles of 128 x 128 -- s = min(8, ceil(2 CUs / (ceil(M / 128) ceil(p / 128)))) lowered until a slice holds
 * at least 256 of the M terms (and, for aligned operands, until 16 s divides M) -- and nothing when s = 1, so nothing
 * below M = 512; at most 8 elem p M.  mgp_k_dense takes no scratch at any D: the generic-D arena ("gen") is never touched.
 *
 * The call does not synchronise the stream (a fixed pool whose "prj" arena has to move, or a growing arena that has to
 * be reallocated, waits for the work queued on it first).
 */
#ifndef MGP_PREDICT_H
#define MGP_PREDICT_H

#include "mgp.h"

#ifdef __cplusplus
extern "C" {
#endif

/* q [B] = the form above for the rows of Xs [B, D] against Z [M, D].  B = 0 writes nothing; M = 0 writes zeros.  A NULL
 * handle, kernel or q, or ldc < M, is MGP_E_BADARG; a negative size MGP_E_SHAPE.  q must not alias an input. */
int mgp_knm_quadform(mgp_handle* h, const mgp_kernel* k, const void* Xs, int64_t B, const void* Z, int64_t M,
                     const void* C, int64_t ldc, void* q);

#ifdef __cplusplus
}
#endif

#endif /* MGP_PREDICT_H */
