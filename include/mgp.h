/*
 * mgp.h -- C ABI of libmgp (MI355X / gfx950 HIP kernels for the CG + kernel-matvec path).
 *
 * Drop-in boundary of SURVEY.md §8(b).  The reference (awav/conjugate-gradient-sparse-gp)
 * has no FFI of its own: its boundary is the Python call surface of cggp/conjugate_gradient.py,
 * cggp/models.py and cggp/distance.py.  Each entry point below names the reference
 * interface (file:line under /root/reference) whose arithmetic it replaces; the Python
 * host side (conjugate-gradient-sparse-gp_amd/cggp) binds these with ctypes and mirrors the
 * reference's names and argument meaning on top.
 *
 * Conventions
 *  - plain pointers and sizes only; every data pointer is a DEVICE pointer unless a
 *    parameter says "host"; row-major, contiguous, base aligned to the element size (8 bytes
 *    fp64 / int64, 4 bytes fp32): any contiguous slice of an allocation is a valid argument.  A
 *    wider alignment is never required; where a kernel has a 16- or 32-byte vector form, the host
 *    selects it only when every pointer it loads through is so aligned (csrc/dense.hip), and the
 *    result meets the same bound either way.  Writes stay inside the documented extent of an
 *    output and inputs are never modified (tests/test_gpu_buffer_contract.py checks every entry
 *    point at both alignments between guard bands).
 *  - the caller owns every buffer it passes.  The library owns only its handle and a
 *    device workspace that it grows on demand (never while a stream capture is active).
 *  - every function returns 0 on success or a negative MGP_E_* code and never throws or
 *    exits; mgp_last_error() gives the message.  CG non-convergence is NOT an error (the
 *    reference returns the last iterate silently, conjugate_gradient.py:93-98); it is
 *    reported through mgp_cg_stats.
 *  - all work is enqueued on the handle's stream (mgp_set_stream); the only host
 *    synchronisations are the convergence poll of mgp_pcg_solve and explicit stats readback.
 *  - a handle is not thread-safe; distinct handles are independent.
 */
#ifndef MGP_H
#define MGP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MGP_VERSION 210 /* 0.2.1: + mgp_profile_read_clocks (0.2.0: mgp_comm, mgp_operator.comm, mgp_create_ex) */
#define MGP_MAX_D 512      /* input dimensions the library accepts (capacity of mgp_kernel) */
#define MGP_FUSED_MAX_D 32 /* up to here the fused register-resident kernels run; above, every entry point takes
                            * the generic route (csrc/generic.hip): products through row-chunked explicit kernel
                            * panels + the NT GEMM (the reference's dense form), nearest-centre, the kernel VJP
                            * and the k^2 column sum tile by tile with the dimensions staged through LDS */

enum { MGP_OK = 0, MGP_E_BADARG = -1, MGP_E_SHAPE = -2, MGP_E_DTYPE = -3, MGP_E_HIP = -4,
       MGP_E_COMM = -5, MGP_E_NOMEM = -6 };

enum { MGP_F32 = 0, MGP_F64 = 1 };

/* GPflow stationary kernels reachable in the reference (cggp/cli_utils.py:105-108,455-473;
 * cg_test.py:14): K2 of SURVEY §8a. */
enum { MGP_SE = 0, MGP_MATERN12 = 1, MGP_MATERN32 = 2, MGP_MATERN52 = 3 };

/* layout of a batch of vectors: MGP_COLS = [n, R] (the facade layout of
 * ConjugateGradient.__call__, conjugate_gradient.py:180-212), MGP_ROWS = [R, n] (the
 * function-level layout of conjugate_gradient(), conjugate_gradient.py:24-32). */
enum { MGP_COLS = 0, MGP_ROWS = 1 };

/* MGP_PRE_LOWRANK: diagonal plus low rank, z = diag_inv o r - (r B^T) B for each row of the batch, applied inside the
 * device CG loop (mgp_lowrank_apply's kernels, gated).  It reuses three fields of mgp_precond: diag_inv = D^-1 [n],
 * dense_inv = B [k, n] row-major, num_blocks = k >= 1.  For P = D + L^T L (L [k, n], e.g. mgp_kxx_pivchol's factor and
 * D = s2 I) pass B = C^-1 L D^-1 with C C^T = I_k + L D^-1 L^T (Woodbury); P^-1 must be positive definite.
 * MGP_PRE_LOWRANK_WIDE: the many-column form of MGP_PRE_LOWRANK -- the same fields, the same checks, the same meaning,
 * the same place in the loop of mgp_pcg_solve, results equal to rounding; mgp_pcg_solve_record does not take it
 * (MGP_E_BADARG).  Only the kernels that form z differ: the right-hand sides go in groups of at most 256 and both
 * products run on the fp64 matrix cores -- T [b, k] = R B^T with n split over the workgroups and the per-split tiles
 * added in split order by a second kernel, then Z = diag_inv o R - T B with the diagonal term fused into the store, so
 * a step is three launches per 256 right-hand sides where MGP_PRE_LOWRANK makes three per 16.  No float atomics: two
 * calls are bit-identical.  Any k in 1 .. 1024 and any n >= 1.  fp32 takes exactly the code of MGP_PRE_LOWRANK and
 * gives its bits.  Scratch, the arena of mgp_kxx_pivchol ("pch"; counted by mgp_workspace_bytes; MGP_E_NOMEM from a
 * fixed pool that is too small): 8 (s + 1) b' k' bytes for the widest group, b = min(Bt, 256) right-hand sides,
 * b' = b rounded up to the row tile t (t = 32 for b <= 32, 64 for b <= 64, else 128), k' = k rounded up to 64 and
 * s = min(ceil(4 CUs / ((b' / t) (k' / 64))), ceil(n / 256)) the splits of n (each a multiple of 16 columns) -- at
 * most 8 (4 CUs + 64) 128 64 bytes (256 CUs: 68 MiB), whatever n. */
enum { MGP_PRE_EYE = 0, MGP_PRE_JACOBI = 1, MGP_PRE_BLOCK = 2, MGP_PRE_DENSE = 3, MGP_PRE_CALLBACK = 4,
       MGP_PRE_LOWRANK = 5, MGP_PRE_LOWRANK_WIDE = 6 };

/* MGP_OP_KXX_NOISE: (k(X,X) + s2 I) applied matrix-free with each unordered pair evaluated once (mgp_kxx_matvec);
 * fields kernel, X, N, s2 and n == N; single rank: `allreduce` / `comm` set is MGP_E_BADARG
 * MGP_OP_KMM_LAMBDA_WIDE: the many-column form of MGP_OP_KMM_LAMBDA -- the same fields (kernel, Z, M == n, lambda), the
 * same checks, the same meaning out[Bt, M] = P[Bt, M] (k(Z, Z) + diag(lambda)), results equal to rounding.  The right-hand
 * sides go in groups of at most 256 through the kernel of mgp_knm_project (Xs = X = Z, R = P as MGP_ROWS), so each
 * kernel value is evaluated once per group on the vector ALU and contracted with the whole group on the fp64 matrix
 * cores, where the sweep of MGP_OP_KMM_LAMBDA evaluates it once per 8 right-hand sides; a second kernel adds the split
 * tiles in a fixed order, scales, adds lambda_i P[b, i] and writes out (no float atomics: two calls are bit-identical).
 * It pays from some tens of right-hand sides on (DESIGN 4.15 has the table).  Fallbacks: fp32 or D > MGP_FUSED_MAX_D take
 * exactly the code of MGP_OP_KMM_LAMBDA and give its bits.  mgp_pcg_solve / mgp_pcg_solve_record pack Z once, before the
 * loop; mgp_operator_apply packs per call.  Scratch, the arena of mgp_knm_project ("prj"; MGP_E_NOMEM from a fixed pool
 * that is too small): 8 M (D' + 1) rounded up to 256, plus 8 t r' (min(M', 2^16) / t + s) rounded up to 256 bytes for
 * the widest group, r = min(Bt, 256) columns (and Bt mod 256 when Bt > 256), r' = r rounded up to 16, t = 128 for
 * r <= 128 and 64 above, M' = M rounded up to t, D' = D rounded up to 2, 4, 8, 16 or 32, s <= 4 CUs + 1 the workgroups
 * added by the split -- at most 8 M (D' + 1) + 512 r' (1024 + 4 CUs + 1) + 512 bytes.
 * MGP_OP_KXX_NOISE_SYM_ANYD: MGP_OP_KXX_NOISE above MGP_FUSED_MAX_D dimensions on the fp64 matrix cores -- the same
 * fields (kernel, X, N == n, s2), the same checks, the same meaning out[Bt, N] = P[Bt, N] (k(X, X) + s2 I), for fp64 and
 * MGP_FUSED_MAX_D < D <= MGP_MAX_D with no kernel panel in memory (csrc/kxx_sym_anyd.hip).  Rows go in blocks of
 * TB = 128 points; every unordered pair of blocks {I, (I + d) mod nb}, d = 0 .. nb/2, is evaluated once (the diagonal
 * block whole, feeding only its own rows) and each profiled 16 x 16 tile is contracted twice, with the right-hand sides
 * of both blocks, for up to 16 right-hand sides at once; more go in groups of 16 plus a remainder.  The distance is
 * the expansion form of mgp_sweep_anyd.h (K = D + 2 on v_mfma_f64_16x16x4_f64 in slices of 32 columns, k ascending, the
 * profile once after the last slice).  Partial sums go to slots with one writer per slot and row, added in slot order
 * by a second kernel that scales by the variance and adds s2 P: no float atomics, two calls are bit-identical.
 * mgp_pcg_solve / mgp_pcg_solve_record pack X once, before the loop, and hold the pack to the end of the solve;
 * mgp_operator_apply packs per call, so X may change in place between calls.  Every launch reads the gate word;
 * N = 0 or Bt = 0 writes nothing.  Fallbacks: fp32 or D <= MGP_FUSED_MAX_D take exactly the code of MGP_OP_KXX_NOISE
 * and give its bits.
 * Scratch, the arena of mgp_kxx_matvec alone ("kxx"; counted by mgp_workspace_bytes; MGP_E_NOMEM from a fixed pool that
 * is too small, nothing is allocated then):
 *     bytes = align256(8 * 64 * KS * N' / 16) + 2 * align256(8 * 16 * N') + align256(8 * (S + ceil(S / DC)) * N' * r)
 * with N' = N rounded up to 128, KS = ceil((D + 2) / 4), r = min(Bt, 16) (with Bt > 16 and Bt mod 16 > 0 the last
 * term is the larger of the terms of r = 16 and r = Bt mod 16), nb = N' / 128, nd = nb/2 + 1,
 * DC = min(ceil(nd / min(max(ceil(2 CUs / nb), 1), nd)), maxs - 1) the values of d one workgroup chains,
 * maxs = min(max(2, 2^29 / (8 N' r)), 32768) and S = min(nd, max(1, maxs / (DC + 1)) DC) the values of d per launch:
 * the slots of a launch stay inside 2^29 bytes (two slots where one exceeds 2^28), as those of mgp_kxx_matvec.
 * Error, for every element, u = 2^-53:
 *     |out[b, i] - exact| <= sum_j |P[b, j]| pairbound(i, j) + u (terms + slots + 3) sum_j |P[b, j] K[i, j]|
 *                            + 2 u |s2 P[b, i]|
 * pairbound(i, j) the bound of the expansion-form distance through the profile (tests/pair_reference.py's pair_bound,
 * as for MGP_OP_KMM_LAMBDA_WIDE_ANYD); terms = 128 DC, the longest chain of products one accumulator takes on the
 * matrix cores (the DC blocks a workgroup streams past the block it keeps, padding included; the chain of the streamed
 * side -- 32 products per wave and 3 sums of waves -- is shorter); slots = nd + ceil(nd / DC) + 2 ceil(nd / S), the
 * sums of the finish kernel over every launch (a slot per d, one per chunk, the running sum); 3 = the product with the variance, the product s2 P[b, i] and the last sum.
 * The distance cancels where a direct difference does not: this error is why the kind is opt-in. */
enum { MGP_OP_DENSE = 0, MGP_OP_SGPR = 1, MGP_OP_KMM_LAMBDA = 2, MGP_OP_KXX_NOISE = 3, MGP_OP_KMM_LAMBDA_WIDE = 4,
       MGP_OP_KXX_NOISE_SYM_ANYD = 9 };

typedef struct mgp_handle mgp_handle;
/* one RCCL communicator rank (wraps ncclComm_t); see "collectives" below */
typedef struct mgp_comm mgp_comm;

/* Kernel hyper-parameters (host memory).  lengthscales has D entries (ARD; repeat the
 * value for an isotropic kernel).  Replaces gpflow.kernels.* parameter objects. */
typedef struct {
  int32_t kind;  /* MGP_SE ... */
  int32_t dtype; /* MGP_F32 | MGP_F64: element type of every data pointer of the call */
  int32_t D;
  int32_t reserved;
  double variance;
  double lengthscales[MGP_MAX_D];
} mgp_kernel;

/* Optional collective hook (rehearsal of the N > 1 path without RCCL, e.g. gloo with host staging):
 * sum `count` elements of `buf` (device) in place over all ranks, enqueued on `stream`.  Used only
 * for the [Bt*M + 1] partial product of the row-sharded SGPR operator -- one call per
 * operator application.  The native path is `mgp_operator.comm` (RCCL, no callback). */
typedef int (*mgp_allreduce_fn)(void* ctx, void* buf, size_t count, int dtype, void* stream);

/* Linear operator handed to mgp_pcg_solve (the `matrix` argument of
 * conjugate_gradient(), conjugate_gradient.py:24-27, generalised to matrix-free forms). */
typedef struct {
  int32_t kind;  /* MGP_OP_* */
  int32_t dtype;
  int64_t n;     /* operator is n x n */
  /* MGP_OP_DENSE: explicit symmetric matrix A [n,n] */
  const void* A;
  /* MGP_OP_SGPR: S = s2 * Kmm_j + K_mn K_nm with K_nm matrix-free over the local row shard.
   * Kmm_j [M,M] dense = k(Z,Z) + jitter I (replicated).  n = M. */
  const mgp_kernel* kernel;
  const void* X; int64_t N;
  const void* Z; int64_t M;
  const void* Kmm;
  double s2;
  /* MGP_OP_KMM_LAMBDA, MGP_OP_KMM_LAMBDA_WIDE: (k(Z,Z) + diag(lambda)) applied matrix-free; lambda [M] device */
  const void* lambda;
  mgp_allreduce_fn allreduce; void* allreduce_ctx;
  /* MGP_OP_SGPR with the `allreduce` hook, optional: caller-owned device buffer of Bt_max*M + 1
   * elements that receives the local partial K_mn(K_nm p) and the agreement word (below) before
   * the collective, so a host-side collective can address it as its own tensor; NULL = library
   * scratch. */
  void* partial_buf;
  /* MGP_OP_SGPR, multi-rank: rows [kmm_row_begin, kmm_row_end) of Kmm whose s2*Kmm.p contribution
   * THIS rank adds to its partial (the slabs of all ranks must tile [0,M)); 0,0 = all rows. */
  int64_t kmm_row_begin, kmm_row_end;
  /* MGP_OP_SGPR, multi-rank, native: RCCL communicator of this rank.  With `allreduce == NULL` and
   * `comm != NULL` every operator application issues ONE ncclAllReduce(sum) of Bt*M + 1 elements on
   * the handle's stream -- the [Bt,M] partial plus one agreement word: inside mgp_pcg_solve each
   * rank contributes its `active` flag there, and an iteration is carried out only if the sum says
   * every rank is active, so all ranks leave the loop on the same iteration by construction. */
  mgp_comm* comm;
  /* number of ranks the `allreduce` hook sums over (the agreement word is compared with it);
   * ignored with `comm`, which knows its own size */
  int32_t world_size; int32_t reserved;
} mgp_operator;

/* MGP_PRE_CALLBACK: the caller's own preconditioner, the protocol of CGPreconditioner.__call__(vec, mat)
 * (conjugate_gradient.py:125-128, used at :77,:89).  Once per CG step, between the two halves of the
 * update, the library copies the residual batch r [Bt, n] into `cb_r` and calls `apply`, which must
 * ENQUEUE on `stream` work that leaves z = M^-1 r in `cb_z` (both buffers caller-owned device memory);
 * rz = sum(z * r) is formed by the library (the reference recomputes it the same way).  The loop stays
 * device resident: steps enqueued past convergence are gated off and their z is ignored.  Non-zero
 * return aborts the solve with MGP_E_BADARG. */
typedef int (*mgp_precond_fn)(void* ctx, const void* r, void* z, int64_t Bt, int64_t n, void* stream);

typedef struct {
  int32_t kind;               /* MGP_PRE_* */
  int32_t block_size;         /* MGP_PRE_BLOCK: bs */
  int64_t num_blocks;         /* MGP_PRE_BLOCK: nb; MGP_PRE_LOWRANK: k, the rows of B */
  const void* diag_inv;       /* MGP_PRE_JACOBI: 1/diag(A) [n] device; MGP_PRE_LOWRANK: D^-1 [n] device */
  const int64_t* block_index; /* MGP_PRE_BLOCK: [nb, bs] int64 device */
  const void* block_inv;      /* MGP_PRE_BLOCK: inverse of A[idx,idx], [nb, bs, bs] device */
  const void* dense_inv;      /* MGP_PRE_DENSE: symmetric P^-1 [n, n] device; z = r @ P^-1; MGP_PRE_LOWRANK: B [k, n] device */
  mgp_precond_fn apply;       /* MGP_PRE_CALLBACK */
  void* apply_ctx;
  void* cb_r;                 /* MGP_PRE_CALLBACK: [Bt, n] device, receives r before every call */
  void* cb_z;                 /* MGP_PRE_CALLBACK: [Bt, n] device, z left there by `apply` */
} mgp_precond;

typedef struct {
  int32_t iterations; /* CG steps taken == reference stats_steps (conjugate_gradient.py:96) */
  int32_t converged;  /* 1 iff all_b(0.5*||r_b||^2 <= thr) at exit */
  double seconds;     /* wall time of the solve (host clock around the enqueue + poll) */
} mgp_cg_stats;

/* ---- handle ------------------------------------------------------------------------- */
int mgp_version(void);
int mgp_create(mgp_handle** out, int device);
/* As mgp_create, with the device workspace fixed up front: one allocation of `workspace_bytes`
 * serves every internal arena (sweep partials, CG state, operator scratch) and the library never
 * calls hipMalloc/hipFree afterwards -- a request that does not fit fails with MGP_E_NOMEM
 * (mgp_last_error names the shortfall).  workspace_bytes == 0 behaves as mgp_create (arenas grow
 * on demand).  mgp_workspace_bytes reports what a handle holds now: run the workload once on a
 * growing handle, read it, and create the production handle with that figure. */
int mgp_create_ex(mgp_handle** out, int device, size_t workspace_bytes);
size_t mgp_workspace_bytes(const mgp_handle* h);
/* Diagnosis: bytes one reused arena of the handle holds now -- "ws", "cg", "opws", "kxx", "kgrad", "pch", "prj", "gen" or
 * "pack" (both slots); 0 for any other name.  An arena that a call reserved from is non-zero afterwards (growing handle
 * and fixed pool alike), which is how tests/test_gpu_buffer_contract.py knows which arenas an entry point reaches. */
size_t mgp_arena_bytes(const mgp_handle* h, const char* name);
int mgp_destroy(mgp_handle* h);
/* The stream every later call enqueues on.  Work enqueued through one handle executes in call order, also when the
 * stream changes in between: the handle's scratch is shared by all of its calls and invisible to the caller, who
 * therefore cannot order two streams' use of it.  When hip_stream differs from the current stream, an event of the
 * handle's own is recorded on the outgoing stream and the incoming stream waits for it (so the outgoing stream must
 * still exist); the host does not wait.  Setting the stream that is already set costs nothing. */
int mgp_set_stream(mgp_handle* h, void* hip_stream);
const char* mgp_last_error(mgp_handle* h);
/* name of the gfx arch the device code was built for, e.g. "gfx950" */
const char* mgp_build_arch(void);

/* ---- matrix-free kernel products --------------------------
 * out[N,R] = k(X,Z) V      replaces Kuf(...)^T @ a, cggp/models.py:334,351 (and :273,:157)
 * V, out layouts given by v_layout / out_layout (MGP_COLS: [M,R]/[N,R]; MGP_ROWS: [R,M]/[R,N]).
 * An empty contraction set (M = 0 here, N = 0 in mgp_kmn_matvec: no inducing points / a rank without rows) is not an
 * error: the output is written as zeros, what the reference's dense [B,0].[0,R] product gives. */
int mgp_knm_matvec(mgp_handle* h, const mgp_kernel* k, const void* X, int64_t N, const void* Z,
                   int64_t M, const void* V, int32_t R, int v_layout, void* out, int out_layout);
/* out[M,R] = k(Z,X) W = K_nm^T W   (W [N,R]); deterministic two-stage reduction over row
 * blocks (no float atomics).  The transpose product of models.py:343 / the SGPR A A^T term. */
int mgp_kmn_matvec(mgp_handle* h, const mgp_kernel* k, const void* X, int64_t N, const void* Z,
                   int64_t M, const void* W, int32_t R, int w_layout, void* out, int out_layout);
/* out[na, ld>=nb] = k(A,B) (+ jitter on the diagonal, + diag_add[i] on the diagonal when
 * non-NULL).  Replaces gpflow Kuu/Kuf + add_diagonal: models.py:300-301,333-337, utils.py:11-17. */
int mgp_k_dense(mgp_handle* h, const mgp_kernel* k, const void* A, int64_t na, const void* B,
                int64_t nb, void* out, int64_t ld, double jitter, const void* diag_add);
/* out[M,M] = K_mn K_nm = k(Z,X) k(X,Z): fp64 MFMA contraction, K row panels generated on the
 * fly (row S1: GPflow SGPR's A A^T, 2 N M^2 flop). */
int mgp_kmn_knm(mgp_handle* h, const mgp_kernel* k, const void* X, int64_t N, const void* Z,
                int64_t M, void* out);

/* out[M] = sum_i k(x_i, z_m)^2 = diag(K_mn K_nm): the N-sized part of diag(S) for the Jacobi
 * preconditioner of the SGPR normal equations (build-side addition, no reference counterpart). */
int mgp_kmn_sq_colsum(mgp_handle* h, const mgp_kernel* k, const void* X, int64_t N, const void* Z,
                      int64_t M, void* out);

/* ---- symmetric self-product: the exact GP regression operator ------------------------------------------------
 * out[N,R] = (k(X,X) + s2 I) V, matrix-free.  The reference's exact baseline is GPflow's GPR (gpr_class,
 * cggp/cli_utils.py:449-452; create_gpr_model, cli_utils.py:171-184), which forms this N x N matrix and factors it;
 * here it is the operator of a CG solve (MGP_OP_KXX_NOISE) for N far beyond a dense K.  Layouts and the empty input
 * follow mgp_knm_matvec (N = 0 writes nothing).  One right-hand side, fp64, D <= MGP_FUSED_MAX_D, N >= 2^16: each
 * unordered pair {i, j} is evaluated once and feeds both rows (csrc/kxx.hip), the same expansion-form distance and exp2
 * arithmetic as the sweep; deterministic (no float atomics, fixed summation order).  Otherwise (several columns, small
 * N, fp32, D > 32; or MGP_KXX=plain in the environment) the sweep k(X,X) V plus s2 V (mgp_knm_matvec with Z = X),
 * which measured faster there.  MGP_KXX=sym takes the symmetric kernel wherever it can (fp64, D <= 32).
 * Scratch, one arena of the handle (counted by mgp_workspace_bytes; MGP_E_NOMEM from a fixed pool that is too small):
 * at most max(2^29, 128 N') + 8 N' (D' + 17) + 256 bytes, N' = N rounded up to 1024, D' = D rounded up to 4, 8, 16
 * or 32 -- O(N), nothing N x N (N = 2^20, D = 32, R = 8: 904 MiB). */
int mgp_kxx_matvec(mgp_handle* h, const mgp_kernel* k, const void* X, int64_t N, double s2, const void* V, int32_t R,
                   int v_layout, void* out, int out_layout);
/* Rank-k partial pivoted Cholesky K ~= L^T L of K = k(X, X) (no noise term), matrix-free: the factor behind the
 * MGP_PRE_LOWRANK preconditioner of the MGP_OP_KXX_NOISE system (Harbrecht et al. 2012; Gardner et al. 2018).  With
 * d = diag K = variance, step i takes p_i = argmax_j d_j (lowest index on ties), stops with *rank_out = i if
 * sum_j d_j <= rel_tol N variance or d_{p_i} <= 0, else writes
 *   L[i, :] = (k(x_{p_i}, X) - sum_{j<i} L[j, p_i] L[j, :]) / sqrt(d_{p_i}),   d <- max(d - L[i, :]^2, 0),
 * with d_{p_i} = 0 and L[i, c] = 0 exactly wherever d_c is 0 (every earlier pivot).  L [max_rank, N] row-major and
 * piv [max_rank] (int64) are device buffers of the caller, rows and entries from *rank_out on are left untouched;
 * diag [N] (device, may be NULL) receives the final d; rank_out is a host pointer.  Rows of K come from the kernel on
 * the fly (direct differences, GPflow's profiles, as mgp_k_dense_vjp forms them); nothing N x N is held.  fp64 only
 * (fp32: MGP_E_DTYPE), any D <= MGP_MAX_D, 1 <= max_rank <= 1024 (clamped to N), rel_tol >= 0, N >= 0 (N = 0: rank 0).
 * One launch per step, the pivot never visits the host: every workgroup reduces the step partials of the launch
 * before it, in a fixed order, so two calls give bit-identical L and piv; about 4 k^2 N bytes are streamed.
 * Scratch, one arena of the handle (counted by mgp_workspace_bytes; MGP_E_NOMEM from a fixed pool that is too small;
 * a growing handle rounds an arena up by a quarter): at most 8 N + 32 KiB.  Synchronises the stream. */
int mgp_kxx_pivchol(mgp_handle* h, const mgp_kernel* k, const void* X, int64_t N, int32_t max_rank, double rel_tol,
                    void* L, int64_t* piv, void* diag, int32_t* rank_out);
/* Z[Bt, n] = diag_inv o R - (R B^T) B for the rows of R [Bt, n], B [k, n] row-major, diag_inv [n]: one application of
 * the MGP_PRE_LOWRANK preconditioner (fp64 and fp32; k >= 1; n = 0 or Bt = 0 writes nothing; not in place).  R B^T is
 * reduced over n in two stages in a fixed order (no float atomics): two calls are bit-identical.  B is streamed twice
 * per 16 rows of the batch (2 elem k n bytes; bandwidth-bound).  Scratch, the arena of mgp_kxx_pivchol:
 * (ceil(n / c) + 1) b k elements, b = min(Bt, 16), c = 2048 / b' columns, b' = b rounded up to 1, 2, 4, 8 or 16. */
int mgp_lowrank_apply(mgp_handle* h, int dtype, const void* diag_inv, const void* B, int64_t k, int64_t n,
                      const void* R, int64_t Bt, void* Z);
/* proj[B, r] = k(Xs, X) R and sqnorm[b] = sum_j proj[b, j]^2 for a wide dense R ([N, r] MGP_COLS or [r, N] MGP_ROWS):
 * the query of a Lanczos variance cache, var(x*) = k(x*, x*) - |k(x*, X) R|^2 with R = Q^T C^-T, T = C C^T (Pleiss et
 * al. 2018).  proj is row-major [B, r]; either output may be NULL, not both (MGP_E_BADARG).  B = 0 writes nothing;
 * N = 0 or r = 0 writes zeros.  k(Xs, X) is never materialised on the fused route -- fp64, D <= MGP_FUSED_MAX_D,
 * r <= 256: a workgroup owns a tile of test rows (t = 128 for r <= 128, 64 above) and all r columns (padded to 16),
 * evaluates each kernel value once (the expansion-form distance and profiles of mgp_kmn_knm, values as mgp_k_dense to
 * rounding) and contracts on the fp64 matrix cores; N is split over the grid when B alone does not fill the chip and
 * the per-split tiles are added in a fixed order by a second kernel that also forms sqnorm (csrc/project.hip; no float
 * atomics, two calls are bit-identical).  fp32, D > 32 or r > 256: row panels of at most 256 MiB of k(Xs, X) through
 * mgp_k_dense, the NT GEMM and a row-square-sum kernel; the same results to rounding, equally deterministic.
 * Scratch, one arena of the handle (counted by mgp_workspace_bytes; MGP_E_NOMEM from a fixed pool that is too small; a
 * growing handle rounds an arena up by a quarter): fused, 8 t r' (min(B', 2^16) / t + s) + 8 N (D' + 1) + 256 bytes
 * with B' = B rounded up to t, r' = r rounded up to 16, D' = D rounded up to 2, 4, 8, 16 or 32 and s <= 4 CUs + 1 the
 * workgroups added by the split -- at most 512 r' (1024 + 4 CUs + 1) + 8 N (D' + 1) + 256 bytes (256 CUs, r = 256:
 * 257 MiB + O(N D)); generic, elem (r N [MGP_COLS only] + c min(N, 16384) + c r [proj NULL only]) + 256 bytes,
 * c = min(B, max(64, 2^28 / (elem min(N, 16384)))) panel rows, and up to 8 c r elements of the NT GEMM's contraction
 * slices in the reduction arena it shares with the other entry points. */
int mgp_knm_project(mgp_handle* h, const mgp_kernel* k, const void* Xs, int64_t B, const void* X, int64_t N,
                    const void* R, int32_t r, int r_layout, void* proj, void* sqnorm);
/* Hyper-parameter bilinear forms of K = k(X, X) (no noise term): for theta = variance and each ARD lengthscale,
 *   dvariance = sum_r u_r^T (dK/dvariance) v_r,   dlengthscales[d] = sum_r u_r^T (dK/dl_d) v_r   (host doubles)
 * -- the gradient of the exact-GP marginal likelihood without dK/dtheta or any N x N matrix (callers fold weights into
 * U).  U, V [N, R] (MGP_COLS) or [R, N] (MGP_ROWS), R >= 1.  Diagonal terms count (dk_ii/dvariance = 1, dk_ii/dl = 0).
 * fp64, D <= MGP_FUSED_MAX_D: each unordered pair once with c_ij = sum_r (u_ri v_rj + u_rj v_ri), direct differences,
 * workgroup partials added in a fixed order (csrc/kxx_grad.hip; two calls are bit-identical).  Scratch, one arena of
 * the handle: 8 N' (D' + 2 C) + 64 CUs (D' + 1) bytes, N' = N rounded up to 256, D' = D rounded up to 4, 8, 16 or 32,
 * C = 16 (8 for D' = 32 and Matern-1/2) -- O(N D).  fp32, D > 32 (or MGP_KXX_GRAD=panel in the environment): row panels of at most
 * 256 MB of G = U[rows] V^T through mgp_k_dense_vjp.  N = 0 writes zeros.  Synchronises the stream. */
int mgp_kxx_grad(mgp_handle* h, const mgp_kernel* k, const void* X, int64_t N, const void* U, const void* V, int32_t R,
                 int layout, double* dvariance, double* dlengthscales);
/* VJP of (theta, Z) -> (Q, B) = (K_mn K_nm, K_mn Y), K = k(X, Z) [N, M], at the cotangents Gq [M, M] and Gb [M, P]
 * -- the N-sized part of the gradient of Titsias' collapsed bound (GPflow SGPR.elbo, which depends on the data only
 * through Q, K_mn y and y^T y); mgp_k_dense_vjp would need the [N, M] cotangent W = K (Gq + Gq^T) + Y Gb^T.  Returns
 *   dvariance = sum_nm W_nm dk_nm/dvariance,  dlengthscales[d] = sum_nm W_nm dk_nm/dl_d     (host doubles, ARD)
 *   dZ[m, d]  = sum_n  W_nm dk_nm/dz_md                                                     ([M, D] device, row-major)
 * Y [N, P] and Gb may be NULL with P = 0; dZ may be NULL (not computed).  Gq need not be symmetric: Gq + Gq^T is used
 * (Gq = NULL: see the last paragraph).
 * fp64 only (fp32: MGP_E_DTYPE), D <= MGP_FUSED_MAX_D (else MGP_E_BADARG), N >= 0, M >= 1, P >= 0; N = 0 writes zeros.
 * dk/dr2 as mgp_k_dense_vjp forms it, r2 from direct differences; Matern-1/2 adds 0 to the lengthscales and to dZ
 * below GPflow's r2 floor of 1e-36 (a data row equal to an inducing point gives no NaN).  Row panels of at most 256 MiB
 * of K: k(X_panel, Z) (direct differences), W_panel by the fp64 MFMA NT GEMM, then one pair kernel reduces W_panel against
 * the kernel's derivatives into workgroup partials that are added in a fixed order (csrc/kmn_grad.hip): no float
 * atomics, two calls are bit-identical, and the results for row shards of X (and Y) add up to the whole up to
 * rounding.  Scratch, one arena of the handle (counted by mgp_workspace_bytes, MGP_E_NOMEM from a fixed pool that is
 * too small): 16 R M + 8 M^2 + 8 (4 CUs + B) (D' + 1) + (dZ ? 8 M D' (4 CUs / B + 2) : 0) + 2048 bytes, R = the
 * panel rows (min(N, 2^25 / M) rounded down to 16, at least 16), B = ceil(M / 256), D' = D rounded up to 4, 8, 16
 * or 32 -- at most 512 MiB + 8 M^2 + O(CUs (M + 256) D'), nothing N x M beyond one row panel.  Synchronises the
 * stream.
 * Gq = NULL means Gq = 0: the cotangent of K is W = Y Gb^T alone, of rank P, and P >= 1 with Y and Gb is required
 * (MGP_E_BADARG otherwise).  Nothing [M, M] is read, written or reserved.  X and Z may be the same buffer (with
 * Y = [U | V], Gb = [V | U] the call differentiates sum_r u_r^T k(Z, Z) v_r: dZ in both arguments of k, dvariance and
 * dlengthscales twice mgp_kxx_grad's); coincident points and the diagonal pairs add 0 to dlengthscales and dZ, never a
 * NaN.  Same arithmetic, determinism and shard additivity as above.  P <= 12 (MGP_KVJP_P_FUSED at build time): a
 * fused pair kernel forms W_nm = sum_p Y_np Gb_mp on the fly in passes of at most C = 16 columns (8 for Matern-1/2)
 * that add to the running sums in pass order; scratch 8 R' (D' + C) + 8 (4 CUs + B) (D' + 1) +
 * (dZ ? 8 M D' (4 CUs / B + 2) : 0) + 1280 bytes, R' = min(N, 2^23 / (D' + C)) -- at most 64 MiB +
 * O(CUs (M + 256) D').  Larger P: row panels of W by the NT GEMM and the pair kernel above; scratch 8 R M + the same
 * partials, R as above -- at most 256 MiB + O(CUs (M + 256) D'). */
int mgp_kmn_knm_vjp(mgp_handle* h, const mgp_kernel* k, const void* X, int64_t N, const void* Z, int64_t M,
                    const void* Gq, const void* Y, const void* Gb, int32_t P, double* dvariance, double* dlengthscales,
                    void* dZ);

/* ---- dense symmetric product (row M2: `state.p @ A`, conjugate_gradient.py:65) ---------
 * out[Bt,n] = P[Bt,n] @ A[n,n] for SYMMETRIC A (CG requires it; computed as rows of A dotted
 * with p_b, i.e. P @ A^T).  For Bt = 1 and n >= 1024 only the upper triangle of A (in 64x64
 * tiles, diagonal tiles whole) is read: each tile serves both A_IJ p_J and A_IJ^T p_I. */
int mgp_symm_matmul(mgp_handle* h, int dtype, const void* A, int64_t n, const void* P,
                    int64_t Bt, void* out);

/* ---- preconditioned batched CG (rows CG1, CG3-CG5) -------------------------------------
 * Solves V A = B for row batches B [Bt,n] starting from V0 (NULL = zeros), exactly the
 * recurrence of conjugate_gradient.py:59-98: stop when all_b(0.5||r_b||^2 <= thr) or
 * i >= max_iterations; gamma = 0 where p.Ap <= min_float; beta-term = 0 where rz <= min_float;
 * residual refresh + direction restart when i % max_steps_cycle == max_steps_cycle-1.
 * err_out [Bt] receives 0.5*rz_final (stats_error, :97).  check_every = iterations enqueued
 * between convergence polls (device-side gating keeps the step count exact). */
int mgp_pcg_solve(mgp_handle* h, const mgp_operator* op, const mgp_precond* pre, const void* B,
                  const void* V0, int64_t Bt, double error_threshold, int64_t max_iterations,
                  int64_t max_steps_cycle, double min_float, int32_t check_every, void* V_out,
                  void* err_out, mgp_cg_stats* stats);
/* mgp_pcg_solve that also records, for every CG step k actually taken (steps gated off after convergence write
 * nothing; k < coef_steps), coef[k, b, 0:3] = (gamma, beta, 0.5 rz after the step) in the operator's dtype -- the
 * coefficients a stochastic Lanczos quadrature builds the Lanczos tridiagonal of column b from.  Preconditioner
 * MGP_PRE_EYE (or NULL) or MGP_PRE_LOWRANK, else MGP_E_BADARG; with MGP_PRE_LOWRANK beta = (r.z)_new / (r.z)_old and T
 * is the Lanczos tridiagonal of P^-1/2 A P^-1/2 started at P^-1/2 b.  The record is defined up to the first residual refresh: pass
 * max_steps_cycle > max_iterations.  Never takes the register-resident dense route.  coef [coef_steps, Bt, 3] device,
 * coef_steps >= 0. */
int mgp_pcg_solve_record(mgp_handle* h, const mgp_operator* op, const mgp_precond* pre, const void* B,
                         const void* V0, int64_t Bt, double error_threshold, int64_t max_iterations,
                         int64_t max_steps_cycle, double min_float, int32_t check_every, void* V_out,
                         void* err_out, mgp_cg_stats* stats, void* coef, int64_t coef_steps);
/* one application of an operator: out[Bt,n] = P[Bt,n] @ Op (used by tests and the bench) */
int mgp_operator_apply(mgp_handle* h, const mgp_operator* op, const void* P, int64_t Bt, void* out);
/* the matrix-free (Kmm + Lambda) product by name (row M2, `p @ A` with A = add_diagonal(Kuu, lambda),
 * models.py:301,337): out[R,M] = V[R,M] @ (k(Z,Z) + diag(lambda)); lambda [M] on the device */
int mgp_kmm_lambda_matvec(mgp_handle* h, const mgp_kernel* k, const void* Z, int64_t M, const void* lambda,
                          const void* V, int64_t R, void* out);

/* ---- reductions used by the model surface ----------------------------------------------
 * out[c] = sum_r A[r,c]*B[r,c] (axis 0, like tf.reduce_sum(Kmn * W, axis=0), models.py:343) */
int mgp_colwise_dot(mgp_handle* h, int dtype, const void* A, const void* B, int64_t rows,
                    int64_t cols, void* out);
/* *out = sum(A*B) over count elements (host double); Hutchinson trace, models.py:313 */
int mgp_dot_all(mgp_handle* h, int dtype, const void* A, const void* B, int64_t count, double* out);

/* ---- collectives: RCCL over xGMI, one communicator rank per GPU ----------------
 * The reference has no collective; these are the build's own multi-GPU boundary.
 * Two ways to form the communicator:
 *  - one process per GPU (torch.distributed.run): rank 0 calls mgp_comm_unique_id, ships the
 *    MGP_COMM_ID_BYTES to the other ranks by any channel, every rank calls mgp_comm_init_rank;
 *  - one process driving ndev devices: mgp_comm_init_all(ndev, devs, comms) (ncclCommInitAll).
 * mgp_allreduce_sum: in-place sum of `count` elements of `buf` (device) over the ranks, enqueued on
 * `stream`; calls for several communicators of one process must be bracketed by
 * mgp_comm_group_begin/end.  Errors: negative code, text via mgp_comm_last_error (thread local). */
#define MGP_COMM_ID_BYTES 128
int mgp_comm_unique_id(void* id_out);
int mgp_comm_init_rank(mgp_comm** out, int device, int nranks, int rank, const void* id);
int mgp_comm_init_all(int ndev, const int* devs, mgp_comm** comms);
int mgp_comm_destroy(mgp_comm* c);
int mgp_comm_size(const mgp_comm* c);
int mgp_comm_rank(const mgp_comm* c);
int mgp_comm_group_begin(void);
int mgp_comm_group_end(void);
int mgp_allreduce_sum(void* buf, size_t count, int dtype, mgp_comm* comm, void* stream);
const char* mgp_comm_last_error(void);

/* ---- next row F1: nearest-centre assignment + cluster statistics (optimize.py:41-98) ----
 * idx[i] = argmin_m d(Z_m, X_i) (first index on ties), dist type 0 = squared euclidean on raw
 * inputs (ops.square_distance, optimize.py:50), 1 = euclidean (distance.py:9-11, same argmin),
 * 2 = covariance, 3 = correlation (distance.py:15-30; kernel required).  best[i] = the distance.
 * sums[M], counts[M] accumulate y and 1 per cluster in deterministic order. */
int mgp_nearest_center(mgp_handle* h, const mgp_kernel* k, int dist_type, const void* X, int64_t N,
                       const void* Z, int64_t M, int64_t* idx, void* best);
int mgp_cluster_stats(mgp_handle* h, int dtype, const int64_t* idx, const void* y, int64_t N,
                      int64_t M, void* sums, void* counts);
/* the same sums for C columns at once when the caller has grouped the rows: order [N] = row indices
 * sorted (stably) by cluster, offsets [M+1] = start of every cluster's run in `order`;
 * sums[M,C] = per-cluster column sums of Y [N,C], summed in a fixed order (N C work, against the
 * N M of the sweep above: the k-means centroid update, selection.py:58-63, and optimize.py:61-78) */
int mgp_segment_sums(mgp_handle* h, int dtype, const int64_t* order, const int64_t* offsets, const void* Y,
                     int64_t N, int64_t C, int64_t M, void* sums);

/* ---- next row F2: hyper-parameter gradient of a kernel block ---------------------------------
 * Given G = dL/dK for K = k(A,B) [na, nb] (leading dimension ldg), returns (host doubles)
 * dL/dvariance and dL/dlengthscales[D] -- the vector-Jacobian product autodiff takes through
 * gpflow's kernel in the reference's training step (cggp/optimize.py:198-254 over
 * cggp/models.py:125-134,293-354).  Fused reduction; synchronises the stream. */
int mgp_k_dense_vjp(mgp_handle* h, const mgp_kernel* k, const void* A, int64_t na, const void* B,
                    int64_t nb, const void* G, int64_t ldg, double* dvariance, double* dlengthscales);

/* ---- random Fourier features (the reference's cggp/rff.py; csrc/rff.hip) -------------------------
 * theta [L, D] spectral frequencies in radians (the library forms theta / 2 pi itself), X [N, D], any D <= MGP_MAX_D.
 * Phases are reduced in revolutions, so |theta x| of 1e6 rad and more keeps the accuracy of the dot product: per
 * feature |err| <= 8 u (1 + sum_d |x_d theta_d|), u the unit roundoff of the dtype.
 * mgp_rff_features: out[n, 0:L] = cos(theta x_n), out[n, L:2L] = sin(theta x_n), rows ld >= 2L apart
 *   (basis_vectors, rff.py:48-57).
 * mgp_rff_sample: out(s, n) = scale * sum_l (W[s, l] cos(theta_l x_n) + W[s, L + l] sin(theta_l x_n)), W [S, 2L]
 *   (cos block first); out [S, N] (MGP_ROWS) or [N, S] (MGP_COLS) (rff_sample, rff.py:60-73).  D <= 32 and S <= 8: one
 *   fused sweep, deterministic; otherwise feature panels in row chunks of <= ~256 MB and a GEMM against W.
 * N = 0 writes nothing; L = 0 writes zeros (mgp_rff_sample). */
int mgp_rff_features(mgp_handle* h, int dtype, const void* X, int64_t N, int32_t D, const void* theta, int64_t L,
                     void* out, int64_t ld);
int mgp_rff_sample(mgp_handle* h, int dtype, const void* X, int64_t N, int32_t D, const void* theta, int64_t L,
                   const void* W, int32_t S, double scale, void* out, int out_layout);

/* ---- measurement (bench.py): HIP events around every launch of the fused sweep kernel ------
 * While enabled, each sweep launch is bracketed by two events on the handle's stream;
 * mgp_profile_read synchronises the stream, returns the number of bracketed launches and the
 * sum of their durations in milliseconds, and resets the counters.  Enabling reserves a 4 MB block for
 * the clock stamps below as one more arena of the workspace: counted by mgp_workspace_bytes, taken from
 * the fixed pool of mgp_create_ex (MGP_E_NOMEM if it does not fit) -- no allocation outside it. */
int mgp_profile_enable(mgp_handle* h, int on);
int mgp_profile_read(mgp_handle* h, int64_t* launches, double* total_ms);
/* as mgp_profile_read, but one duration per bracketed launch (the first `capacity` of them) so the
 * caller can report median / percentiles; *launches receives the number recorded. */
int mgp_profile_read_each(mgp_handle* h, double* ms_out, int64_t capacity, int64_t* launches);
/* Shader clock the bracketed sweep launches ran at (bench-only): while profiling is on, up to 16 workgroups of each
 * launch stamp the constant 100 MHz counter and the shader-clock counter at their start and at the end of their loop;
 * this returns one value in MHz per stamped workgroup (the first `capacity` of them) and their number. */
int mgp_profile_read_clocks(mgp_handle* h, double* mhz_out, int64_t capacity, int64_t* samples);

/* ---- next row F3: cover-tree clustering (host code, no GPU, no handle) ----------------------
 * Replaces the reference's CoverTree class (cggp/covertree.py:26-179), which
 * covertree_update_inducing_parameters (cggp/optimize.py:19-38) turns into inducing inputs,
 * cluster means and counts.  x is a HOST pointer [N, D] row-major fp64.  spatial_resolution > 0
 * derives the level count as the reference does (:54-56), otherwise num_levels is used.  The tree
 * keeps row indices into x (x is only read during the build).  Levels are read back flat:
 * level_nodes gives centres [n, D], the parent's position in the level above (-1 for the root) and
 * the number of rows held; level_rows gives CSR offsets [n+1] and the concatenated row indices
 * (rows may be NULL to get the offsets only).  Errors: mgp_host_last_error() (thread local). */
typedef struct mgp_covertree mgp_covertree;
const char* mgp_host_last_error(void);
int mgp_covertree_build(const double* x, int64_t N, int D, double spatial_resolution, int num_levels, int lloyds,
                        int voronoi, mgp_covertree** out);
/* The same construction -- the same tree, node for node and bit for bit -- with its four all-pairs-shaped passes (the
 * ball of a seed, the rows a new centre takes, the per-level Voronoi reassignment, the r-neighbour test of the new
 * centres) as device filters over `x_dev`, the fp64 device copy of the same [N, D] rows; the sequential acceptance of
 * centres and every mean stay on the host (csrc/covertree_dev.hip).  For inputs where almost every node is an
 * r-neighbour of every other (D >= ~6) the host version scans nearly all rows per centre. */
int mgp_covertree_build_device(mgp_handle* h, const double* x, const double* x_dev, int64_t N, int D,
                               double spatial_resolution, int num_levels, int lloyds, int voronoi, mgp_covertree** out);
void mgp_covertree_destroy(mgp_covertree* t);
int mgp_covertree_num_levels(const mgp_covertree* t);
int64_t mgp_covertree_level_size(const mgp_covertree* t, int level);
double mgp_covertree_level_radius(const mgp_covertree* t, int level);
int mgp_covertree_level_nodes(const mgp_covertree* t, int level, double* points, int64_t* parent, int64_t* counts);
int mgp_covertree_level_rows(const mgp_covertree* t, int level, int64_t* offsets, int64_t* rows);

#ifdef __cplusplus
}
#endif
#endif /* MGP_H */
