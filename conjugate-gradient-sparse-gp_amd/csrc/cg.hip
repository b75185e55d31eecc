// cg.hip -- device-resident batched preconditioned conjugate gradient (rows CG1, CG3-CG5).
//
// Restates the recurrence of cggp/conjugate_gradient.py:59-98 with every scalar
// (gamma, beta, rz, the stopping test) kept on the device:
//
//   while any_b(0.5 ||r_b||^2 > thr) and i < max_it:                  (:59-62)
//       Ap = p @ A                                                     (:65)   operator kernel(s)
//       gamma = rz / (p . Ap), 0 where p.Ap <= min_float               (:66-68)  \
//       v += gamma p ; r -= gamma Ap   (or r = b - v @ A on a refresh) (:69-76)   | cg_update_kernel
//       z, rz' = M^-1 r ; p = z + p rz'/rz (0 where rz <= min_float)   (:77-84)  /  one block per RHS
//
// The host never sees a scalar: a device word `active` gates every kernel of an iteration, so
// `check_every` iterations can be enqueued back to back and the ones after convergence are
// no-ops -- the step count stays exactly the reference's.  The host polls `active` once per
// batch.  Vectors are [Bt, n] row-major (the function-level layout, :24-32); one workgroup owns
// one right-hand side, dot products are wavefront shuffles + one LDS hop.
//
// Host side: apply_operator (A.p for every operator kind) and pcg_solve_t, which reads decode_precond -> routes ->
// CgArena -> CgSolve::start -> one of run_persist / run_dense1_pipelined / run_polled -> statistics (read_ctrl: the one
// poll of the control word; enqueue_batch: the one batch body).  An operator form that leaves A.p somewhere other than
// `out` says so through the MgpApLoc* it was handed (mgp_common.h), never through the handle.
#include <chrono>
#include <cstdio>

#include "../../include/mgp_sweep_anyd.h"
#include "mgp_common.h"

namespace {

using CgCtrl = MgpCgCtrl;  // mgp_common.h (shared with cg_dense1.hip)

template <typename T>
__device__ __forceinline__ T block_sum(T v, T* red) {
  v = mgp_wave_sum(v);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();  // red reuse
  if (lane == 0) red[wave] = v;
  __syncthreads();
  T s = 0;
  const int nw = blockDim.x >> 6;
  for (int w = 0; w < nw; ++w) s += red[w];  // fixed order: deterministic
  return s;
}

struct PrecondDev {
  int kind;
  int bs;
  long nb;
  const void* diag_inv;
  const long* block_index;
  const void* block_inv;
};

// z = M^-1 r for one RHS row (all threads of the block cooperate); returns nothing, z in memory
template <typename T>
__device__ void apply_precond(const PrecondDev& pc, const T* __restrict__ r, T* __restrict__ z, long n) {
  if (pc.kind == MGP_PRE_JACOBI) {
    const T* dinv = (const T*)pc.diag_inv;
    for (long j = threadIdx.x; j < n; j += blockDim.x) z[j] = r[j] * dinv[j];
  } else {  // MGP_PRE_BLOCK: uncovered indices pass through, covered ones get Binv_k r[idx_k]
    for (long j = threadIdx.x; j < n; j += blockDim.x) z[j] = r[j];
    __syncthreads();
    const T* binv = (const T*)pc.block_inv;
    const long tot = pc.nb * pc.bs;
    for (long e = threadIdx.x; e < tot; e += blockDim.x) {
      const long k = e / pc.bs, a = e - k * pc.bs;
      const long* idx = pc.block_index + k * pc.bs;
      const T* row = binv + (k * pc.bs + a) * pc.bs;
      T s = 0;
      for (int c = 0; c < pc.bs; ++c) s = mgp_fma(row[c], r[idx[c]], s);
      z[idx[a]] = s;
    }
  }
  __syncthreads();
}

// r = b - av (av may be null => r = b); z, rz, p, stopping flag.  Also used for the refresh step.
template <typename T>
__global__ __launch_bounds__(256) void cg_init_kernel(const T* __restrict__ b, const T* __restrict__ av,
                                                      T* __restrict__ r, T* __restrict__ z, T* __restrict__ p,
                                                      T* __restrict__ rz, int* __restrict__ over,
                                                      T* __restrict__ err, long n, T thr, PrecondDev pc) {
  __shared__ T red[8];
  const long off = (long)blockIdx.x * n;
  for (long j = threadIdx.x; j < n; j += blockDim.x) r[off + j] = av ? b[off + j] - av[off + j] : b[off + j];
  __syncthreads();
  const T* zz = r + off;
  if (pc.kind != MGP_PRE_EYE) {
    apply_precond<T>(pc, r + off, z + off, n);
    zz = z + off;
  }
  T s_rz = 0, s_rr = 0;
  for (long j = threadIdx.x; j < n; j += blockDim.x) {
    const T rv = r[off + j], zv = zz[j];
    p[off + j] = zv;
    s_rz = mgp_fma(zv, rv, s_rz);
    s_rr = mgp_fma(rv, rv, s_rr);
  }
  s_rz = block_sum(s_rz, red);
  s_rr = block_sum(s_rr, red);
  if (threadIdx.x == 0) {
    rz[blockIdx.x] = s_rz;
    err[blockIdx.x] = (T)0.5 * s_rz;
    over[blockIdx.x] = ((T)0.5 * s_rr > thr) ? 1 : 0;
  }
}

// Generic step pieces (refresh steps, block / dense preconditioners).  The kernel's `mode`:
enum UpdateMode : int {
  UPD_STEP = 0,            // first half (gamma, v, r -= gamma Ap) + native preconditioner + second half
  UPD_STEP_KEEP_R = 1,     // first half without the r update (a residual refresh follows)
  UPD_RESTART = 2,         // native preconditioner + second half with beta = 0 (after a refresh: p = z)
  UPD_FIRST_HALF = 3,      // first half only, with the r update (z from outside the kernel follows)
  UPD_SECOND_HALF = 4,     // second half with z already in memory, normal beta
  UPD_SECOND_RESTART = 5,  // second half with z already in memory, beta = 0 (start-up and refresh: p = z)
};
// `force` bypasses the gate (start-up of the dense-preconditioner path).
// Block size: 256 threads per right-hand side up to n = 8192, 1024 beyond (the fused kernel covers n <= 8192; one
// 256-thread workgroup per right-hand side was a cliff for larger systems).
// NTB is the launch bound AND the launch size (256 or 1024): small systems keep the register budget of a 256-thread
// workgroup (one 1024-thread bound capped it for every launch).
template <typename T, int NTB>
__global__ __launch_bounds__(NTB) void cg_update_kernel(const CgCtrl* __restrict__ ctrl, T* __restrict__ v,
                                                        T* __restrict__ r, T* __restrict__ p,
                                                        T* __restrict__ z, const T* __restrict__ ap,
                                                        T* __restrict__ rz, int* __restrict__ over,
                                                        T* __restrict__ err, long n, T thr, T min_float,
                                                        PrecondDev pc, int mode, int force,
                                                        T* __restrict__ coef, long coef_steps) {
  if (!force && ctrl->active == 0) return;
  __shared__ T red[16];
  const long off = (long)blockIdx.x * n;
  const T rz_old = rz[blockIdx.x];
  const bool first = mode == 0 || mode == 1 || mode == 3;
  T gamma = 0;
  if (first) {
    T d = 0;
    for (long j = threadIdx.x; j < n; j += blockDim.x) d = mgp_fma(p[off + j], ap[off + j], d);
    d = block_sum(d, red);
    gamma = (d <= min_float) ? (T)0 : rz_old / d;
    for (long j = threadIdx.x; j < n; j += blockDim.x) {
      v[off + j] = mgp_fma(gamma, p[off + j], v[off + j]);
      if (mode != 1) r[off + j] = mgp_fma(-gamma, ap[off + j], r[off + j]);
    }
    // recording solve on the split-update route: the step length is known here, beta and rz in mode 4
    if (mode == 3 && coef != nullptr && threadIdx.x == 0 && ctrl->iters < coef_steps)
      coef[((long)ctrl->iters * gridDim.x + blockIdx.x) * 3] = gamma;
    if (mode != 0) return;
    __syncthreads();
  }
  const T* zz = r + off;
  if (mode >= 4) {
    zz = z + off;  // computed by the dense preconditioner product
  } else if (pc.kind != MGP_PRE_EYE) {
    apply_precond<T>(pc, r + off, z + off, n);
    zz = z + off;
  }
  T s_rz = 0, s_rr = 0;
  for (long j = threadIdx.x; j < n; j += blockDim.x) {
    const T rv = r[off + j], zv = zz[j];
    s_rz = mgp_fma(zv, rv, s_rz);
    s_rr = mgp_fma(rv, rv, s_rr);
  }
  s_rz = block_sum(s_rz, red);
  s_rr = block_sum(s_rr, red);
  const T beta = (mode == 2 || mode == 5 || rz_old <= min_float) ? (T)0 : s_rz / rz_old;
  // p = z where the beta-term is dropped (:79-84): a select, not 0 * p -- at start-up (mode 5) p is
  // whatever the arena held, and 0 * Inf/NaN would poison the direction
  const bool drop = mode == 2 || mode == 5 || rz_old <= min_float;
  for (long j = threadIdx.x; j < n; j += blockDim.x) p[off + j] = drop ? zz[j] : mgp_fma(beta, p[off + j], zz[j]);
  if (threadIdx.x == 0) {
    // recording solve (modes 0 and 4; the step index is the counter cg_advance_kernel moves after this launch)
    if (coef != nullptr && (mode == 0 || mode == 4) && ctrl->iters < coef_steps) {
      T* c = coef + ((long)ctrl->iters * gridDim.x + blockIdx.x) * 3;
      if (mode == 0) c[0] = gamma;
      c[1] = beta;
      c[2] = (T)0.5 * s_rz;
    }
    rz[blockIdx.x] = s_rz;
    err[blockIdx.x] = (T)0.5 * s_rz;
    over[blockIdx.x] = ((T)0.5 * s_rr > thr) ? 1 : 0;
  }
}

// Fused common-case step (no refresh, Eye or Jacobi): the whole update of one RHS with its
// elements held in registers (EPT per thread), two block reductions instead of four, and the
// iteration bookkeeping (`any` over the RHS flags, step counter, next gate) done by the last
// workgroup to arrive -- write-through flag + ticket, no extra launch.
template <typename T, int EPT, int NT>
__global__ __launch_bounds__(NT) void cg_update_fused_kernel(CgCtrl* __restrict__ ctrl, T* __restrict__ v,
                                                             T* __restrict__ r, T* __restrict__ p,
                                                             const T* __restrict__ ap, T* __restrict__ rz,
                                                             int* __restrict__ over, T* __restrict__ err, long n,
                                                             T thr, T min_float, const T* __restrict__ dinv,
                                                             int max_it, int ap_slices, long ap_stride,
                                                             const T* __restrict__ agree, int world,
                                                             T* __restrict__ coef, long coef_steps) {
  // multi-rank SGPR operator: `ap` is the all-reduced partial itself and `agree` the word behind it -- the sum of
  // the ranks' gate words.  Unless every rank computed this application nobody uses it: the gate closes and all
  // ranks leave the loop on the same iteration (what finish_allreduce_kernel did in a launch of its own).
  // Tested BEFORE the gate word: in this branch workgroup 0 clears ctrl->active, and no workgroup of the launch may be
  // reading that word at its entry meanwhile -- here none does, every one of them leaves on `agree`.  The
  // other writer of ctrl->active, the last arriver below, runs after every workgroup has passed this point.
  if (agree != nullptr && *agree != (T)world) {
    if (blockIdx.x == 0 && threadIdx.x == 0) ctrl->active = 0;
    return;
  }
  if (ctrl->active == 0) return;
  __shared__ T red[2][NT / 64];
  __shared__ int last_flag;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const long off = (long)blockIdx.x * n;
  const T rz_old = rz[blockIdx.x];
  T pv[EPT], av[EPT], rv[EPT], vv[EPT], dv[EPT];
  T d = 0;
#pragma unroll
  for (int e = 0; e < EPT; ++e) {
    const long j = (long)e * NT + t;
    const bool ok = j < n;
    pv[e] = ok ? p[off + j] : (T)0;
    av[e] = ok ? ap[off + j] : (T)0;
    rv[e] = ok ? r[off + j] : (T)0;
    // the solution and the Jacobi diagonal are not needed before gamma is known, but requested now: behind the
    // block reduction they were a third dependent round trip to memory in a kernel that is nothing but latency
    vv[e] = ok ? v[off + j] : (T)0;
    dv[e] = (dinv != nullptr && ok) ? dinv[j] : (T)0;
  }
  if (ap_slices > 1) {
    // A.p left as contraction slices by the skinny product (at most 8): every slice of every element is requested
    // before the first is used -- one workgroup per right-hand side is latency-bound, a load-add chain per element
    // cost what the separate reduce launch had -- then added in slice order, as skinny_reduce_kernel does
    T sl[7][EPT];
#pragma unroll
    for (int z = 1; z < 8; ++z)
#pragma unroll
      for (int e = 0; e < EPT; ++e) {
        const long j = (long)e * NT + t;
        sl[z - 1][e] = (z < ap_slices && j < n) ? ap[(long)z * ap_stride + off + j] : (T)0;
      }
#pragma unroll
    for (int z = 1; z < 8; ++z)
      if (z < ap_slices) {
#pragma unroll
        for (int e = 0; e < EPT; ++e) av[e] += sl[z - 1][e];
      }
  }
#pragma unroll
  for (int e = 0; e < EPT; ++e) d = mgp_fma(pv[e], av[e], d);
  d = mgp_wave_sum(d);
  if (lane == 0) red[0][wave] = d;
  __syncthreads();
  d = 0;
#pragma unroll
  for (int w = 0; w < NT / 64; ++w) d += red[0][w];
  const T gamma = (d <= min_float) ? (T)0 : rz_old / d;
  T s_rz = 0, s_rr = 0;
  T zv[EPT];
#pragma unroll
  for (int e = 0; e < EPT; ++e) {
    const long j = (long)e * NT + t;
    if (j < n) v[off + j] = mgp_fma(gamma, pv[e], vv[e]);
    rv[e] = mgp_fma(-gamma, av[e], rv[e]);
    zv[e] = dinv != nullptr ? rv[e] * dv[e] : rv[e];
    s_rz = mgp_fma(zv[e], rv[e], s_rz);
    s_rr = mgp_fma(rv[e], rv[e], s_rr);
  }
  s_rz = mgp_wave_sum(s_rz);
  s_rr = mgp_wave_sum(s_rr);
  __syncthreads();  // red[0] fully read
  if (lane == 0) {
    red[0][wave] = s_rz;
    red[1][wave] = s_rr;
  }
  __syncthreads();
  s_rz = 0;
  s_rr = 0;
#pragma unroll
  for (int w = 0; w < NT / 64; ++w) {
    s_rz += red[0][w];
    s_rr += red[1][w];
  }
  const T beta = (rz_old <= min_float) ? (T)0 : s_rz / rz_old;
#pragma unroll
  for (int e = 0; e < EPT; ++e) {
    const long j = (long)e * NT + t;
    if (j < n) {
      r[off + j] = rv[e];
      p[off + j] = (rz_old <= min_float) ? zv[e] : mgp_fma(beta, pv[e], zv[e]);
    }
  }
  if (t == 0) {
    // recording solve: step index = the counter the last arriver below moves, read before this workgroup's ticket
    if (coef != nullptr) {
      const int it = ctrl->iters;
      if (it < coef_steps) {
        T* c = coef + ((long)it * gridDim.x + blockIdx.x) * 3;
        c[0] = gamma;
        c[1] = beta;
        c[2] = (T)0.5 * s_rz;
      }
    }
    rz[blockIdx.x] = s_rz;
    err[blockIdx.x] = (T)0.5 * s_rz;
    __hip_atomic_store(&over[blockIdx.x], ((T)0.5 * s_rr > thr) ? 1 : 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (gridDim.x == 1) {
      last_flag = 1;  // one right-hand side: nothing to hand over
    } else {
      // hand-off without fences (cdna_hip_programming.md G16, sc1 form): the flag above is a
      // write-through store of this lane, drained here, then the ticket; the last arriver reads the
      // flags with sc1 loads behind the barrier.  (__threadfence() on both sides cost ~3.5 us each.)
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      const unsigned tk = atomicAdd(&ctrl->ticket, 1u);
      last_flag = (tk == gridDim.x - 1) ? 1 : 0;
    }
  }
  __syncthreads();
  if (last_flag) {  // last workgroup to arrive: every flag has been published
    __shared__ int any;
    if (t == 0) any = 0;
    __syncthreads();
    int a = 0;
    for (long b = t; b < (long)gridDim.x; b += NT)
      a |= __hip_atomic_load(&over[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (a) atomicOr(&any, 1);
    __syncthreads();
    if (t == 0) {
      const int it = ctrl->iters + 1;
      ctrl->iters = it;
      ctrl->ticket = 0;
      ctrl->active = (any && it < max_it) ? 1 : 0;
    }
  }
}

// r = b - av, gated (refresh step, conjugate_gradient.py:72-75)
template <typename T>
__global__ __launch_bounds__(256) void cg_residual_kernel(const CgCtrl* __restrict__ ctrl,
                                                          const T* __restrict__ b, const T* __restrict__ av,
                                                          T* __restrict__ r, long total, int force) {
  if (!force && ctrl->active == 0) return;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < total) r[i] = av ? b[i] - av[i] : b[i];
}

__global__ void cg_advance_kernel(CgCtrl* ctrl, const int* __restrict__ over, long Bt, int inc, int max_it) {
  __shared__ int any;
  if (inc && ctrl->active == 0) return;  // uniform: every thread reads the same word
  if (threadIdx.x == 0) any = 0;
  __syncthreads();
  int a = 0;
  for (long b = threadIdx.x; b < Bt; b += blockDim.x) a |= over[b];
  if (a) atomicOr(&any, 1);
  __syncthreads();
  if (threadIdx.x == 0) {
    const int it = ctrl->iters + inc;
    ctrl->iters = it;
    ctrl->active = (any && it < max_it) ? 1 : 0;
  }
}

// t[b, j] += a * x[b, j] for the columns j in [rb, re)
template <typename T>
__global__ __launch_bounds__(256) void add_rows_slab_kernel(const int* __restrict__ gate, T a, const T* __restrict__ x,
                                                            T* __restrict__ t, long n, long total, long rb, long re) {
  if (gate != nullptr && *gate == 0) return;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const long j = i % n;
  if (j >= rb && j < re) t[i] = mgp_fma(a, x[i], t[i]);
}

// out[b, j] += lam[j] * p[b, j]
template <typename T>
__global__ __launch_bounds__(256) void add_diag_prod_kernel(const int* __restrict__ gate, const T* __restrict__ lam,
                                                            const T* __restrict__ p, T* __restrict__ out, long n,
                                                            long total) {
  if (gate != nullptr && *gate == 0) return;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < total) out[i] = mgp_fma(lam[i % n], p[i], out[i]);
}

// Multi-rank agreement: the word behind the [Bt,M] partial carries this rank's gate
// (1 = it computed this application) through the all-reduce; the sum equals the number of ranks
// iff every rank did.
template <typename T>
__global__ void put_gate_word_kernel(const int* __restrict__ gate, T* __restrict__ word) {
  *word = (gate == nullptr || *gate != 0) ? (T)1 : (T)0;
}

// After the all-reduce: out = reduced partial when every rank took part; otherwise nobody uses this
// application and the local gate closes, so all ranks leave the CG loop on the same iteration.
template <typename T>
__global__ __launch_bounds__(256) void finish_allreduce_kernel(int* __restrict__ gate, const T* __restrict__ tt,
                                                               T* __restrict__ out, long tot, int world) {
  const int a = gate == nullptr ? 1 : *gate;
  if (!a) return;
  if (tt[tot] != (T)world) {  // exact: a sum of at most `world` ones
    if (gate != nullptr && blockIdx.x == 0 && threadIdx.x == 0) *gate = 0;
    return;
  }
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < tot) out[i] = tt[i];
}

inline unsigned nblk(long total) { return (unsigned)((total + 255) / 256); }

// out[Bt, n] = P[Bt, n] @ Op ; gate may be null.  loc (MgpApLoc, mgp_common.h): null = finished into out; else the
// skinny product may leave its slices and the collective SGPR operator, under a gate, its all-reduced partial
template <typename T>
int apply_operator(mgp_handle* h, const mgp_operator* op, const T* P, long Bt, T* out, const int* gate,
                   MgpApLoc* loc = nullptr) {
  const long n = op->n;
  if (loc != nullptr) *loc = MgpApLoc{out, 1, 0, nullptr, 0};
  switch (op->kind) {
    case MGP_OP_DENSE:
      return mgp_symm_matmul_gated(h, op->dtype, op->A, n, P, Bt, out, gate, loc);
    case MGP_OP_KMM_LAMBDA_WIDE_ANYD:  // the many-column form above 32 dimensions (kmm_wide_anyd.hip); else as the next kind
      if (mgp_kmm_wide_anyd_serves(op->kernel))
        return mgp_kmm_wide_anyd_apply(h, op->kernel, op->Z, op->M, op->lambda, P, Bt, out, gate);
      [[fallthrough]];
    case MGP_OP_KMM_LAMBDA_WIDE:  // the many-column form (project.hip); fp32 and D > 32 take the sweep form below
      if (mgp_kmm_wide_serves(op->kernel))
        return mgp_kmm_wide_apply(h, op->kernel, op->Z, op->M, op->lambda, P, Bt, out, gate);
      [[fallthrough]];
    case MGP_OP_KMM_LAMBDA_ANYD:  // the fused any-D sweep where it serves (sweep_anyd.hip), else the code below
    case MGP_OP_KMM_LAMBDA: {
      MGP_TRY((op->kind == MGP_OP_KMM_LAMBDA_ANYD ? mgp_sweep_anyd : mgp_sweep)(
          h, op->kernel, op->Z, op->M, op->Z, op->M, VecView{P, 1, n}, (int)Bt, VecViewMut{out, 1, n}, 0.0,
          VecView{nullptr, 0, 0}, gate));
      hipLaunchKernelGGL((add_diag_prod_kernel<T>), dim3(nblk(Bt * n)), dim3(256), 0, h->stream, gate,
                         (const T*)op->lambda, P, out, n, Bt * n);
      MGP_LAUNCH_CHECK(h);
      return MGP_OK;
    }
    case MGP_OP_KXX_NOISE:  // (k(X,X) + s2 I) p, each unordered pair once (kxx.hip); rows of P are the right-hand sides
      return mgp_kxx(h, op->kernel, op->X, n, op->s2, VecView{P, 1, n}, (int)Bt, VecViewMut{out, 1, n}, gate);
    case MGP_OP_KXX_NOISE_ANYD:
      return mgp_kxx_anyd(h, op->kernel, op->X, n, op->s2, VecView{P, 1, n}, (int)Bt, VecViewMut{out, 1, n}, gate);
    case MGP_OP_KXX_NOISE_SYM_ANYD:  // each unordered pair once on the matrix cores (kxx_sym_anyd.hip); else MGP_OP_KXX_NOISE
      return mgp_kxx_sym_anyd(h, op->kernel, op->X, n, op->s2, P, Bt, out, gate);
    case MGP_OP_SGPR_ANYD:  // the two local sweeps by the fused any-D kernel where it serves; everything else as below
    case MGP_OP_SGPR: {
      const auto sweep = op->kind == MGP_OP_SGPR_ANYD ? mgp_sweep_anyd : mgp_sweep;
      // u[Bt,N] = (K_nm p^T)^T ; t[Bt,M] = (K_mn u^T)^T over the local rows ; the replicated
      // s2*Kmm.p term is added as this rank's row slab of it, so ONE all-reduce of t finishes S.p
      const long N = op->N, M = op->M;
      const bool coll = op->allreduce != nullptr || op->comm != nullptr;
      // operator arena: u [Bt,N] | partial [Bt,M] + agreement word (padded to 2) | Kmm.p [Bt,M] (only for Bt > 1)
      const size_t need = ((size_t)Bt * N + 2 * (size_t)Bt * M + 2) * sizeof(T);
      MGP_TRY(mgp_reserve(h, &h->opws, &h->opws_bytes, need));
      T* u = (T*)h->opws;
      // the collective works on the caller's buffer when one is given; single rank: straight into out
      T* tt = coll ? (op->partial_buf ? (T*)op->partial_buf : u + Bt * N) : out;
      long rb = op->kmm_row_begin, re = op->kmm_row_end;
      if (rb == 0 && re == 0) re = M;  // unset: this rank owns every row of Kmm
      bool word_written = false;
      // One right-hand side: this rank's slab of Kmm.p does not depend on the sweeps -- it goes to a stream of its own,
      // forked when p is ready, and comes back as the addend of the K_mn sweep: 31 us of HBM streaming at M = 4096
      // beside 2.3 ms of vector-ALU-bound sweep instead of behind it
      // (worth its two events from ~50 MB of slab on: one rank's share of 8 at M = 4096 is 17 MB = 4 us, measured 5 us slower)
      const bool aside = Bt == 1 && N > 0 && re > rb &&
                         (h->kmm_aside > 1 || (h->kmm_aside == 1 && (size_t)(re - rb) * M * sizeof(T) >= ((size_t)48 << 20)));
      if (aside) {
        if (!h->aside_stream) MGP_HIP(h, hipStreamCreateWithFlags(&h->aside_stream, hipStreamNonBlocking));
        for (int e = 0; e < 2; ++e)
          if (!h->aside_ev[e]) MGP_HIP(h, hipEventCreateWithFlags(&h->aside_ev[e], hipEventDisableTiming));
        T* kmp = u + Bt * N + Bt * M + 2;
        hipStream_t main_stream = h->stream;
        MGP_HIP(h, hipEventRecord(h->aside_ev[0], main_stream));
        MGP_HIP(h, hipStreamWaitEvent(h->aside_stream, h->aside_ev[0], 0));
        h->stream = h->aside_stream;
        word_written = coll && h->fuse_agree;  // the slab product also writes this rank's agreement word behind the partial
        int rc = MGP_OK;
        if (rb == 0 && re == M && !word_written) {  // every row is this rank's: written, not accumulated
          rc = mgp_symm_gemv_assign(h, op->dtype, op->Kmm, M, P, kmp, gate);
        } else {
          if (hipMemsetAsync(kmp, 0, (size_t)M * sizeof(T), h->stream) != hipSuccess) rc = mgp_fail(h, MGP_E_HIP, "memset of Kmm.p failed");
          if (rc == MGP_OK)
            rc = mgp_symm_gemv_rows_acc(h, op->dtype, op->Kmm, M, P, rb, re, 1.0, kmp, gate,
                                        word_written ? (void*)(tt + Bt * M) : nullptr);
        }
        h->stream = main_stream;
        MGP_TRY(rc);
        MGP_HIP(h, hipEventRecord(h->aside_ev[1], h->aside_stream));
        MGP_TRY(sweep(h, op->kernel, op->X, N, op->Z, M, VecView{P, 1, M}, (int)Bt, VecViewMut{u, 1, N}, 0.0,
                          VecView{nullptr, 0, 0}, gate));
        MGP_HIP(h, hipStreamWaitEvent(main_stream, h->aside_ev[1], 0));
        MGP_TRY(sweep(h, op->kernel, op->Z, M, op->X, N, VecView{u, 1, N}, (int)Bt, VecViewMut{tt, 1, M}, op->s2,
                          VecView{kmp, 1, M}, gate));
      } else if (N > 0) {
        MGP_TRY(sweep(h, op->kernel, op->X, N, op->Z, M, VecView{P, 1, M}, (int)Bt, VecViewMut{u, 1, N}, 0.0,
                          VecView{nullptr, 0, 0}, gate));
        MGP_TRY(sweep(h, op->kernel, op->Z, M, op->X, N, VecView{u, 1, N}, (int)Bt, VecViewMut{tt, 1, M}, 0.0,
                          VecView{nullptr, 0, 0}, gate));
      } else {
        MGP_HIP(h, hipMemsetAsync(tt, 0, (size_t)Bt * M * sizeof(T), h->stream));
      }
      if (aside) {
        // Kmm.p is the K_mn sweep's addend already
      } else if (Bt == 1) {
        // with a collective the slab product also writes this rank's agreement word behind the partial
        word_written = coll && re > rb && h->fuse_agree;
        MGP_TRY(mgp_symm_gemv_rows_acc(h, op->dtype, op->Kmm, M, P, rb, re, op->s2, tt, gate,
                                       word_written ? (void*)(tt + Bt * M) : nullptr));
      } else {
        // several RHS: full replicated product, then only this rank's slab of it is added
        T* kmp = u + Bt * N + Bt * M + 2;
        MGP_TRY(mgp_symm_matmul_gated(h, op->dtype, op->Kmm, M, P, Bt, kmp, gate));
        hipLaunchKernelGGL((add_rows_slab_kernel<T>), dim3(nblk(Bt * M)), dim3(256), 0, h->stream, gate, (T)op->s2,
                           (const T*)kmp, tt, M, Bt * M, rb, re);
        MGP_LAUNCH_CHECK(h);
      }
      if (coll) {
        const long tot = Bt * M;
        if (!word_written) {
          hipLaunchKernelGGL((put_gate_word_kernel<T>), dim3(1), dim3(1), 0, h->stream, gate, tt + tot);
          MGP_LAUNCH_CHECK(h);
        }
        if (op->allreduce) {  // rehearsal hook (gloo with host staging); never used with RCCL
          const int rc = op->allreduce(op->allreduce_ctx, tt, (size_t)(tot + 1), op->dtype, (void*)h->stream);
          if (rc != 0) return mgp_fail(h, MGP_E_COMM, "allreduce callback returned %d", rc);
        } else {  // native: one ncclAllReduce on the solve's stream
          MGP_TRY(mgp_comm_allreduce_on(h, op->comm, tt, (size_t)(tot + 1), op->dtype));
        }
        const int world = op->comm ? mgp_comm_size(op->comm) : op->world_size;
        if (loc != nullptr && gate != nullptr) {  // the fused update tests the word and reads the partial in place
          *loc = MgpApLoc{tt, 1, 0, tt + tot, world};
          return MGP_OK;
        }
        hipLaunchKernelGGL((finish_allreduce_kernel<T>), dim3(nblk(tot)), dim3(256), 0, h->stream, (int*)gate,
                           (const T*)tt, out, tot, world);
        MGP_LAUNCH_CHECK(h);
      }
      return MGP_OK;
    }
    default:
      return mgp_fail(h, MGP_E_BADARG, "unknown operator kind %d", op->kind);
  }
}

int check_operator(mgp_handle* h, const mgp_operator* op) {
  if (!op) return mgp_fail(h, MGP_E_BADARG, "operator is NULL");
  if (op->dtype != MGP_F32 && op->dtype != MGP_F64) return mgp_fail(h, MGP_E_DTYPE, "bad operator dtype");
  if (op->n <= 0) return mgp_fail(h, MGP_E_SHAPE, "operator n must be > 0");
  const bool sgpr = op->kind == MGP_OP_SGPR || op->kind == MGP_OP_SGPR_ANYD;
  if (op->kind == MGP_OP_DENSE) {
    if (!op->A) return mgp_fail(h, MGP_E_BADARG, "dense operator without matrix");
  } else if (sgpr || op->kind == MGP_OP_KMM_LAMBDA || op->kind == MGP_OP_KMM_LAMBDA_WIDE ||
             op->kind == MGP_OP_KMM_LAMBDA_ANYD || op->kind == MGP_OP_KMM_LAMBDA_WIDE_ANYD) {
    MGP_TRY(mgp_check_kernel(h, op->kernel));
    if (op->kernel->dtype != op->dtype) return mgp_fail(h, MGP_E_DTYPE, "operator/kernel dtype mismatch");
    if (op->M != op->n || !op->Z) return mgp_fail(h, MGP_E_SHAPE, "operator needs Z with M == n");
    if (sgpr && (!op->Kmm || op->N < 0 || (op->N > 0 && !op->X)))
      return mgp_fail(h, MGP_E_BADARG, "SGPR operator needs X and Kmm");
    if (!sgpr && !op->lambda) return mgp_fail(h, MGP_E_BADARG, "needs lambda");
    if (sgpr && op->allreduce && op->comm)
      return mgp_fail(h, MGP_E_BADARG, "give either the allreduce hook or a communicator, not both");
    if (sgpr && op->allreduce && op->world_size < 1)
      return mgp_fail(h, MGP_E_BADARG, "allreduce hook needs world_size >= 1");
  } else if (op->kind == MGP_OP_KXX_NOISE || op->kind == MGP_OP_KXX_NOISE_ANYD ||
             op->kind == MGP_OP_KXX_NOISE_SYM_ANYD) {
    MGP_TRY(mgp_check_kernel(h, op->kernel));
    if (op->kernel->dtype != op->dtype) return mgp_fail(h, MGP_E_DTYPE, "operator/kernel dtype mismatch");
    if (op->N != op->n || !op->X) return mgp_fail(h, MGP_E_SHAPE, "K_XX operator needs X with N == n");
    if (!(op->s2 >= 0.0)) return mgp_fail(h, MGP_E_BADARG, "K_XX operator needs s2 >= 0");
    if (op->allreduce || op->comm) return mgp_fail(h, MGP_E_BADARG, "K_XX operator is single-rank (no allreduce / comm)");
  } else {
    return mgp_fail(h, MGP_E_BADARG, "unknown operator kind %d", op->kind);
  }
  return MGP_OK;
}

constexpr int kRetryWithoutPersist = 1;  // internal: never crosses the C ABI

// ------------------------------------------------------------------ the pieces of pcg_solve_t
// The caller's mgp_precond: the form the update kernels apply themselves (`dev`; the identity when z comes from outside
// them) or one of the three external forms
struct CgPrecond {
  PrecondDev dev{MGP_PRE_EYE, 0, 0, nullptr, nullptr, nullptr};
  const void* dense_inv = nullptr;       // MGP_PRE_DENSE: z = r @ Pinv through the symmetric product kernels
  const mgp_precond* cb = nullptr;       // MGP_PRE_CALLBACK: z produced by the caller's function, same step structure
  const mgp_precond* lowrank = nullptr;  // MGP_PRE_LOWRANK: z = diag_inv o r - (r B^T) B (pivchol.hip)
  bool lowrank_wide = false;             // MGP_PRE_LOWRANK_WIDE: the same z by the many-column kernels
  bool dense_pre = false, need_z = false;  // z comes from outside the update kernels; z lives in the arena
};

int decode_precond(mgp_handle* h, const mgp_precond* pre, CgPrecond& c) {
  if (pre) {
    c.dev.kind = pre->kind;
    if (pre->kind == MGP_PRE_JACOBI) {
      if (!pre->diag_inv) return mgp_fail(h, MGP_E_BADARG, "jacobi preconditioner without diag_inv");
      c.dev.diag_inv = pre->diag_inv;
    } else if (pre->kind == MGP_PRE_BLOCK) {
      if (!pre->block_index || !pre->block_inv || pre->block_size <= 0 || pre->num_blocks < 0)
        return mgp_fail(h, MGP_E_BADARG, "block preconditioner incomplete");
      c.dev.bs = pre->block_size;
      c.dev.nb = pre->num_blocks;
      c.dev.block_index = (const long*)pre->block_index;
      c.dev.block_inv = pre->block_inv;
    } else if (pre->kind == MGP_PRE_DENSE) {
      if (!pre->dense_inv) return mgp_fail(h, MGP_E_BADARG, "dense preconditioner without matrix");
      c.dense_inv = pre->dense_inv;
    } else if (pre->kind == MGP_PRE_CALLBACK) {
      if (!pre->apply || !pre->cb_r || !pre->cb_z)
        return mgp_fail(h, MGP_E_BADARG, "callback preconditioner needs apply, cb_r and cb_z");
      c.cb = pre;
    } else if (pre->kind == MGP_PRE_LOWRANK || pre->kind == MGP_PRE_LOWRANK_WIDE) {
      if (!pre->diag_inv || !pre->dense_inv || pre->num_blocks < 1)
        return mgp_fail(h, MGP_E_BADARG, "low-rank preconditioner needs diag_inv, B (dense_inv) and k (num_blocks) >= 1");
      c.lowrank = pre;
      c.lowrank_wide = pre->kind == MGP_PRE_LOWRANK_WIDE;
    } else if (pre->kind != MGP_PRE_EYE) {
      return mgp_fail(h, MGP_E_BADARG, "unknown preconditioner kind %d", pre->kind);
    }
  }
  c.dense_pre = c.dense_inv != nullptr || c.cb != nullptr || c.lowrank != nullptr;
  c.need_z = c.dev.kind != MGP_PRE_EYE && c.cb == nullptr;  // dense: z = r @ Pinv lives in the arena
  if (c.dense_pre) c.dev.kind = MGP_PRE_EYE;                // the update kernels never apply it themselves
  return MGP_OK;
}

// The CG arena (h->cg): r, p, ap, [z], rz[Bt], over[Bt] (int), ctrl, then the arena of cg_dense1.hip (tile shares,
// chunk shares, two direction buffers).  The byte count and the pointers are written here and nowhere else.
template <typename T>
struct CgArena {
  T *r, *p, *ap, *z, *rz;
  int* over;
  CgCtrl* ctrl;
  void* d1_arena;  // 16-byte aligned, as is ctrl
  // 64: the control word and the two round-ups to 16 bytes below
  static size_t bytes(long tot, long Bt, bool need_z, size_t d1_bytes) {
    return (size_t)tot * sizeof(T) * (need_z ? 4 : 3) + (size_t)Bt * sizeof(T) + (size_t)Bt * sizeof(int) + 64 + d1_bytes;
  }
  CgArena(void* base, long tot, long Bt, bool need_z) {
    r = (T*)base;
    p = r + tot;
    ap = p + tot;
    z = need_z ? ap + tot : nullptr;
    rz = (need_z ? z : ap) + tot;
    over = (int*)(rz + Bt);
    ctrl = (CgCtrl*)(((uintptr_t)(over + Bt) + 15) & ~(uintptr_t)15);
    d1_arena = (void*)(((uintptr_t)(ctrl + 1) + 15) & ~(uintptr_t)15);
  }
};

// the device control word on the host: every earlier launch of the stream has finished when this returns
int read_ctrl(mgp_handle* h, const CgCtrl* ctrl, CgCtrl* host) {
  MGP_HIP(h, hipMemcpyAsync(h->host_flag, ctrl, sizeof(CgCtrl), hipMemcpyDeviceToHost, h->stream));
  MGP_HIP(h, hipStreamSynchronize(h->stream));
  memcpy(host, h->host_flag, sizeof(CgCtrl));
  return MGP_OK;
}

// Fused update kernel: (elements per thread, threads) by system size, one workgroup per right-hand side with its
// elements in registers
template <typename T>
struct FusedTier {
  long max_n;
  unsigned nt;
  decltype(&cg_update_fused_kernel<T, 1, 256>) kernel;
};
template <typename T>
constexpr FusedTier<T> kFusedTiers[] = {
    {256, 256, cg_update_fused_kernel<T, 1, 256>},    {512, 256, cg_update_fused_kernel<T, 2, 256>},
    {1024, 1024, cg_update_fused_kernel<T, 1, 1024>}, {2048, 1024, cg_update_fused_kernel<T, 2, 1024>},
    {4096, 1024, cg_update_fused_kernel<T, 4, 1024>}, {8192, 1024, cg_update_fused_kernel<T, 8, 1024>}};
constexpr long kFusedMaxN = 8192;

// One solve: its arguments, its routes and its arena, and the launches of a step.
template <typename T>
struct CgSolve {
  mgp_handle* h;
  const mgp_operator* op;
  const T* B;
  long Bt, n, tot, max_it, cycle, check_every, coef_steps;
  double thr, min_float;
  T *V, *err_out, *coef;
  hipStream_t s;
  CgPrecond pre;
  CgArena<T> a;
  T* z;                // the arena's, or the callback's own buffer
  bool dense1, fused;  // the tile scheme of cg_dense1.hip; cg_update_fused_kernel serves the steps without a refresh
  MgpDense1 d1;
  long enq = 0;  // iterations enqueued so far (index of the next one)
  CgCtrl host{1, 0};

  // z = M^-1 r for the preconditioners applied outside the update kernels
  int external_z(const int* gate) {
    if (pre.cb) {
      MGP_HIP(h, hipMemcpyAsync(pre.cb->cb_r, a.r, (size_t)tot * sizeof(T), hipMemcpyDeviceToDevice, s));
      const int rc = pre.cb->apply(pre.cb->apply_ctx, pre.cb->cb_r, pre.cb->cb_z, Bt, n, (void*)s);
      if (rc != 0) return mgp_fail(h, MGP_E_BADARG, "preconditioner callback returned %d", rc);
      return MGP_OK;
    }
    if (pre.lowrank)
      return (pre.lowrank_wide ? mgp_lowrank_wide_apply_gated : mgp_lowrank_apply_gated)(
          h, op->dtype, pre.lowrank->diag_inv, pre.lowrank->dense_inv, pre.lowrank->num_blocks, n, a.r, Bt, z, gate);
    return mgp_symm_matmul_gated(h, op->dtype, pre.dense_inv, n, a.r, Bt, z, gate);
  }

  // generic update kernel: 256 threads per right-hand side up to n = 8192, 1024 beyond
  int update(UpdateMode mode, bool force = false) {
    const bool records = mode == UPD_STEP || mode == UPD_FIRST_HALF || mode == UPD_SECOND_HALF;  // the recording solve
    hipLaunchKernelGGL((n > 8192 ? cg_update_kernel<T, 1024> : cg_update_kernel<T, 256>), dim3((unsigned)Bt),
                       dim3(n > 8192 ? 1024 : 256), 0, s, a.ctrl, V, a.r, a.p, z, a.ap, a.rz, a.over, err_out, n, (T)thr,
                       (T)min_float, pre.dev, (int)mode, force ? 1 : 0, records ? coef : (T*)nullptr,
                       records ? coef_steps : 0L);
    MGP_LAUNCH_CHECK(h);
    return MGP_OK;
  }

  int advance(int inc) {
    hipLaunchKernelGGL(cg_advance_kernel, dim3(1), dim3(256), 0, s, a.ctrl, a.over, Bt, inc, (int)max_it);
    MGP_LAUNCH_CHECK(h);
    return MGP_OK;
  }

  // whole step in one launch, bookkeeping included; A.p is read from wherever the operator left it
  int fused_update(const MgpApLoc& ap) {
    const T* dinv = pre.dev.kind == MGP_PRE_JACOBI ? (const T*)pre.dev.diag_inv : nullptr;
    const FusedTier<T>* t = kFusedTiers<T>;
    while (n > t->max_n) ++t;  // ends: n <= kFusedMaxN
    hipLaunchKernelGGL(t->kernel, dim3((unsigned)Bt), dim3(t->nt), 0, s, a.ctrl, V, a.r, a.p, (const T*)ap.src, a.rz, a.over,
                       err_out, n, (T)thr, (T)min_float, dinv, (int)max_it, ap.slices, ap.stride, (const T*)ap.agree,
                       ap.world, coef, coef_steps);
    MGP_LAUNCH_CHECK(h);
    return MGP_OK;
  }

  // iteration i of the polled loop, every launch gated by the device word
  int step(long i) {
    const int* gate = &a.ctrl->active;
    const bool reset = (i % cycle) == (cycle - 1);  // :71 (i == state.i while active)
    const bool fuse = fused && !reset;
    // only the fused update can read A.p from somewhere else: the skinny product's slices (dense operator) or the
    // all-reduced partial of the collective SGPR operator, each where its durable switch allows
    // (MGP_OP_SGPR_ANYD defers as MGP_OP_SGPR does: the deferral concerns the collective, not the two local sweeps)
    const bool sgpr = op->kind == MGP_OP_SGPR || op->kind == MGP_OP_SGPR_ANYD;
    const bool may_defer = fuse && ((op->kind == MGP_OP_DENSE && h->skinny_defer) || (sgpr && h->fuse_agree));
    MgpApLoc ap{a.ap, 1, 0, nullptr, 0};
    MGP_TRY(apply_operator<T>(h, op, a.p, Bt, a.ap, gate, may_defer ? &ap : nullptr));
    if (fuse) return fused_update(ap);
    if (!reset) {
      if (!pre.dense_pre) {
        MGP_TRY(update(UPD_STEP));
      } else {
        MGP_TRY(update(UPD_FIRST_HALF));
        MGP_TRY(external_z(gate));
        MGP_TRY(update(UPD_SECOND_HALF));
      }
    } else {  // r = b - vA (:72-75), p = z
      MGP_TRY(update(UPD_STEP_KEEP_R));
      MGP_TRY(apply_operator<T>(h, op, V, Bt, a.ap, gate));
      hipLaunchKernelGGL((cg_residual_kernel<T>), dim3(nblk(tot)), dim3(256), 0, s, a.ctrl, B, a.ap, a.r, tot, 0);
      MGP_LAUNCH_CHECK(h);
      if (pre.dense_pre) MGP_TRY(external_z(gate));
      MGP_TRY(update(pre.dense_pre ? UPD_SECOND_RESTART : UPD_RESTART));
    }
    return advance(1);
  }

  // up to check_every iterations back to back; on the tile scheme its statistics launch closes the batch
  int enqueue_batch() {
    long batch = check_every;
    if (enq + batch > max_it) batch = max_it - enq;
    if (dense1) {
      for (long q = 0; q < batch; ++q, ++enq) MGP_TRY(mgp_dense1_step(h, &d1, enq + 1));
      return mgp_dense1_finish(h, &d1, a.rz, err_out, a.over);
    }
    for (long q = 0; q < batch; ++q, ++enq) MGP_TRY(step(enq));
    return MGP_OK;
  }

  // r_0, z_0, p_1, the flags and the first gate.  `persist`: the register-resident solve runs here, whole.
  int start(const T* V0, bool persist) {
    MGP_HIP(h, hipMemsetAsync(a.ctrl, 0, sizeof(CgCtrl), s));
    const T* av = nullptr;
    if (V0) {
      if (V != V0) MGP_HIP(h, hipMemcpyAsync(V, V0, (size_t)tot * sizeof(T), hipMemcpyDeviceToDevice, s));
      MGP_TRY(apply_operator<T>(h, op, V, Bt, a.ap, nullptr));  // vA (:87)
      av = a.ap;
    } else {
      MGP_HIP(h, hipMemsetAsync(V, 0, (size_t)tot * sizeof(T), s));
    }
    if (dense1) {
      MGP_TRY(mgp_dense1_begin(h, &d1, op->dtype, op->A, n, B, av, V, a.r,
                               pre.dev.kind == MGP_PRE_JACOBI ? pre.dev.diag_inv : nullptr, a.ctrl, a.d1_arena, thr,
                               min_float, max_it, persist ? 1 : 0, (int)Bt));
      MGP_TRY(mgp_dense1_finish(h, &d1, a.rz, err_out, a.over));  // statistics of r_0 and the first gate
      if (persist) {
        MGP_TRY(mgp_dense1_persist_run(h, &d1));
        MGP_TRY(mgp_dense1_finish(h, &d1, a.rz, err_out, a.over));  // final statistics; closes the gate
      }
      return MGP_OK;
    }
    if (!pre.dense_pre) {
      hipLaunchKernelGGL((cg_init_kernel<T>), dim3((unsigned)Bt), dim3(256), 0, s, B, av, a.r, z, a.p, a.rz, a.over,
                         err_out, n, (T)thr, pre.dev);
      MGP_LAUNCH_CHECK(h);
    } else {  // r = b - vA ; z = r @ Pinv ; p = z, rz = z.r, flags
      hipLaunchKernelGGL((cg_residual_kernel<T>), dim3(nblk(tot)), dim3(256), 0, s, a.ctrl, B, av, a.r, tot, 1);
      MGP_LAUNCH_CHECK(h);
      MGP_TRY(external_z(nullptr));
      MGP_TRY(update(UPD_SECOND_RESTART, true));
    }
    return advance(0);
  }

  // n <= 4096: the whole solve ran in one launch (start); what is left is its verdict.  A hand-off ran out of its poll
  // budget (a workgroup was not resident: the chip was shared): the caller retries this solve with the two-launch form
  int run_persist() {
    MGP_TRY(read_ctrl(h, a.ctrl, &host));
    return host.pad ? kRetryWithoutPersist : MGP_OK;
  }

  // Tile scheme, one polled batch stays in flight: the device works on batch i + 1 while the host waits for the
  // control word of batch i (every poll drained the stream, ~20 us each, 10 of them in a 248-step solve).  When a
  // batch reports the end, the one behind it is already enqueued -- its launches are gated off on the device.
  int run_dense1_pipelined() {
    MGP_TRY(read_ctrl(h, a.ctrl, &host));
    for (int e = 0; e < 2; ++e)
      if (!h->poll_ev[e]) MGP_HIP(h, hipEventCreateWithFlags(&h->poll_ev[e], hipEventDisableTiming));
    CgCtrl* slots = (CgCtrl*)h->host_flag;  // 64 pinned bytes: two control words fit behind the first
    int inflight = 0, wr = 0, rd = 0;
    bool more = host.active != 0;
    while (more || inflight > 0) {
      while (more && inflight < 2 && enq < max_it) {
        MGP_TRY(enqueue_batch());
        MGP_HIP(h, hipMemcpyAsync(&slots[1 + wr], a.ctrl, sizeof(CgCtrl), hipMemcpyDeviceToHost, s));
        MGP_HIP(h, hipEventRecord(h->poll_ev[wr], s));
        wr ^= 1;
        ++inflight;
      }
      if (inflight == 0) break;
      MGP_HIP(h, hipEventSynchronize(h->poll_ev[rd]));
      memcpy(&host, &slots[1 + rd], sizeof(CgCtrl));
      rd ^= 1;
      --inflight;
      if (host.pad) return mgp_fail(h, MGP_E_HIP, "dense CG: a hand-off inside the iteration kernel timed out");
      if (!host.active || enq >= max_it) more = false;
      if (!host.active) break;  // what is still in flight does nothing (device gate); no need to wait for it
    }
    return MGP_OK;
  }

  // every other route: poll, then enqueue the next batch while the device word says go on
  int run_polled() {
    for (;;) {
      MGP_TRY(read_ctrl(h, a.ctrl, &host));
      if (dense1 && host.pad) return mgp_fail(h, MGP_E_HIP, "dense CG: a hand-off inside the iteration kernel timed out");
      if (!host.active || enq >= max_it) return MGP_OK;
      MGP_TRY(enqueue_batch());
    }
  }

  int statistics(mgp_cg_stats* stats, std::chrono::steady_clock::time_point t0) {
    if (!stats) return MGP_OK;
    stats->iterations = host.iters;
    int any = 0;  // converged iff no RHS is over threshold: `active` == 0 below the cap says so; at the cap, look at the flags
    if (host.iters >= max_it) {
      std::vector<int> f((size_t)Bt);
      MGP_HIP(h, hipMemcpyAsync(f.data(), a.over, (size_t)Bt * sizeof(int), hipMemcpyDeviceToHost, s));
      MGP_HIP(h, hipStreamSynchronize(s));
      for (long b = 0; b < Bt; ++b) any |= f[b];
    }
    stats->converged = any ? 0 : 1;
    stats->seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return MGP_OK;
  }
};

// decode the preconditioner, pick the routes, lay out the arena, start up, run one of three drivers, statistics
template <typename T>
int pcg_solve_t(mgp_handle* h, const mgp_operator* op, const mgp_precond* pre, const T* B, const T* V0, long Bt,
                double thr, long max_it, long cycle, double min_float, int check_every, T* V, T* err_out,
                mgp_cg_stats* stats, T* coef, long coef_steps, bool allow_persist) {
  const auto t0 = std::chrono::steady_clock::now();
  const long n = op->n, tot = Bt * n;
  PackHold pack_hold(h);  // the operator's X / Z / kernel are constant for the whole solve
  CgPrecond pc;
  MGP_TRY(decode_precond(h, pre, pc));
  // Routes.  Up to d1_cols right-hand sides on a dense matrix, no residual refresh inside the solve: the tile scheme of
  // cg_dense1.hip -- up to 8 where the full matrix fits the chip (n <= 2048: the register-resident form carries the
  // columns for 16 fused multiply-adds each), else where it was measured faster than the skinny product: 4, 6 above 4096
  const long d1_cols = h->cg_dense1_cols > 0 ? h->cg_dense1_cols
                       : ((allow_persist && mgp_dense1_persist_eligible(h, n, 8))   ? 8
                          : (allow_persist && mgp_dense1_persist_eligible(h, n, 6)) ? 6
                                                                                    : (n <= 4096 ? 4 : 6));
  const bool dense1 = op->kind == MGP_OP_DENSE && Bt >= 1 && Bt <= d1_cols && !pc.dense_pre &&
                      pc.dev.kind != MGP_PRE_BLOCK && cycle > max_it && mgp_dense1_eligible(h, n) && coef == nullptr;
  // n <= 4096: the whole solve in one launch, the upper triangle of A in registers (cg_dense1.hip)
  const bool persist = dense1 && allow_persist && mgp_dense1_persist_eligible(h, n, Bt);
  const bool fused = pc.dev.kind != MGP_PRE_BLOCK && !pc.dense_pre && Bt < 2147483647L && n <= kFusedMaxN;
  MGP_TRY(mgp_reserve(h, &h->cg, &h->cg_bytes,
                      CgArena<T>::bytes(tot, Bt, pc.need_z, dense1 ? mgp_dense1_bytes(h, op->dtype, n, Bt) : 0)));
  const CgArena<T> arena(h->cg, tot, Bt, pc.need_z);
  CgSolve<T> cg{h, op, B, /*Bt=*/Bt, /*n=*/n, /*tot=*/tot, /*max_it=*/max_it, /*cycle=*/cycle,
                /*check_every=*/check_every < 1 ? 1L : (long)check_every, /*coef_steps=*/coef_steps,
                /*thr=*/thr, /*min_float=*/min_float, /*V=*/V, /*err_out=*/err_out, /*coef=*/coef, /*s=*/h->stream,
                /*pre=*/pc, /*a=*/arena, /*z=*/pc.cb ? (T*)pc.cb->cb_z : arena.z, /*dense1=*/dense1, /*fused=*/fused};
  // many-column (K_mm + Lambda): the arena for the widest group and the pack of Z before the loop, nothing inside it
  WideHold wide_hold(h);
  if (op->kind == MGP_OP_KMM_LAMBDA_WIDE_ANYD && mgp_kmm_wide_anyd_serves(op->kernel)) {
    MGP_TRY(mgp_kmm_wide_anyd_prepare(h, op->kernel, op->Z, op->M, Bt, nullptr));
    wide_hold.hold(op->Z, op->M);
  } else if ((op->kind == MGP_OP_KMM_LAMBDA_WIDE || op->kind == MGP_OP_KMM_LAMBDA_WIDE_ANYD) &&
             mgp_kmm_wide_serves(op->kernel)) {
    MGP_TRY(mgp_kmm_wide_prepare(h, op->kernel, op->Z, op->M, Bt, nullptr));
    wide_hold.hold(op->Z, op->M);
  }
  // the symmetric operator above 32 dimensions: the same for X and the kxx arena
  SymHold sym_hold(h);
  if (op->kind == MGP_OP_KXX_NOISE_SYM_ANYD && mgp_kxx_sym_anyd_serves(op->kernel)) {
    MGP_TRY(mgp_kxx_sym_anyd_prepare(h, op->kernel, op->X, op->N, Bt, nullptr));
    sym_hold.hold(op->X, op->N);
  }
  MGP_TRY(cg.start(V0, persist));
  MGP_TRY(persist ? cg.run_persist() : (dense1 && h->poll_pipeline) ? cg.run_dense1_pipelined() : cg.run_polled());
  return cg.statistics(stats, t0);
}

int pcg_solve_entry(mgp_handle* h, const mgp_operator* op, const mgp_precond* pre, const void* B, const void* V0,
                    int64_t Bt, double error_threshold, int64_t max_iterations, int64_t max_steps_cycle,
                    double min_float, int32_t check_every, void* V_out, void* err_out, mgp_cg_stats* stats, void* coef,
                    int64_t coef_steps) {
  if (!h) return MGP_E_BADARG;
  MGP_TRY(check_operator(h, op));
  if (Bt < 0) return mgp_fail(h, MGP_E_SHAPE, "Bt < 0");
  if (stats) {
    stats->iterations = 0;
    stats->converged = 1;
    stats->seconds = 0.0;
  }
  if (Bt == 0) return MGP_OK;
  if (!B || !V_out || !err_out) return mgp_fail(h, MGP_E_BADARG, "NULL data pointer");
  if (max_iterations < 0) return mgp_fail(h, MGP_E_BADARG, "max_iterations < 0");
  if (max_steps_cycle < 1) return mgp_fail(h, MGP_E_BADARG, "max_steps_cycle < 1");
  if (Bt > 2147483647L) return mgp_fail(h, MGP_E_SHAPE, "Bt too large");
  auto run = [&](bool allow_persist) -> int {
    return mgp_with_dtype(op->dtype, [&](auto t) {
      using T = decltype(t);
      return pcg_solve_t<T>(h, op, pre, (const T*)B, (const T*)V0, Bt, error_threshold, max_iterations, max_steps_cycle,
                            min_float, check_every, (T*)V_out, (T*)err_out, stats, (T*)coef, coef_steps, allow_persist);
    });
  };
  int rc = run(true);
  if (rc == kRetryWithoutPersist) {
    if (V0 != nullptr && V0 == V_out)
      return mgp_fail(h, MGP_E_HIP, "dense CG: a hand-off between resident workgroups timed out (is the GPU shared?) and "
                                    "the initial solution was overwritten in place; set MGP_CG_DENSE1=1");
    fprintf(stderr, "libmgp: dense CG: a hand-off between resident workgroups timed out (is the GPU shared?); this solve "
                    "runs again with two launches per iteration\n");
    rc = run(false);  // the solve again, from its inputs, two launches per iteration
  }
  return rc;
}

}  // namespace

extern "C" int mgp_pcg_solve(mgp_handle* h, const mgp_operator* op, const mgp_precond* pre, const void* B,
                             const void* V0, int64_t Bt, double error_threshold, int64_t max_iterations,
                             int64_t max_steps_cycle, double min_float, int32_t check_every, void* V_out,
                             void* err_out, mgp_cg_stats* stats) {
  return pcg_solve_entry(h, op, pre, B, V0, Bt, error_threshold, max_iterations, max_steps_cycle, min_float,
                         check_every, V_out, err_out, stats, nullptr, 0);
}

// Recording solve (stochastic Lanczos quadrature): the update kernels write (gamma, beta, 0.5 rz) of every step taken
// into coef[step, b] -- the fused and mode-0 kernels with the identity, the split update (modes 3 and 4) with
// MGP_PRE_LOWRANK; the register-resident dense route is not taken (pcg_solve_t).
extern "C" int mgp_pcg_solve_record(mgp_handle* h, const mgp_operator* op, const mgp_precond* pre, const void* B,
                                    const void* V0, int64_t Bt, double error_threshold, int64_t max_iterations,
                                    int64_t max_steps_cycle, double min_float, int32_t check_every, void* V_out,
                                    void* err_out, mgp_cg_stats* stats, void* coef, int64_t coef_steps) {
  if (!h) return MGP_E_BADARG;
  if (pre != nullptr && pre->kind != MGP_PRE_EYE && pre->kind != MGP_PRE_LOWRANK)
    return mgp_fail(h, MGP_E_BADARG, "recording solve: only the identity (MGP_PRE_EYE) and MGP_PRE_LOWRANK preconditioners");
  if (coef == nullptr) return mgp_fail(h, MGP_E_BADARG, "recording solve: coef is NULL");
  if (coef_steps < 0) return mgp_fail(h, MGP_E_BADARG, "recording solve: coef_steps < 0");
  return pcg_solve_entry(h, op, pre, B, V0, Bt, error_threshold, max_iterations, max_steps_cycle, min_float,
                         check_every, V_out, err_out, stats, coef, coef_steps);
}

extern "C" int mgp_operator_apply(mgp_handle* h, const mgp_operator* op, const void* P, int64_t Bt, void* out) {
  if (!h) return MGP_E_BADARG;
  MGP_TRY(check_operator(h, op));
  if (Bt <= 0) return Bt == 0 ? MGP_OK : mgp_fail(h, MGP_E_SHAPE, "Bt < 0");
  if (!P || !out) return mgp_fail(h, MGP_E_BADARG, "NULL data pointer");
  return mgp_with_dtype(op->dtype, [&](auto t) {
    using T = decltype(t);
    return apply_operator<T>(h, op, (const T*)P, Bt, (T*)out, nullptr);
  });
}

// Named form of the matrix-free (Kmm + Lambda) product (SURVEY 8b lists it as its own entry point):
// out[R, M] = V[R, M] @ (k(Z, Z) + diag(lambda)), rows = right-hand sides, nothing M x M materialised.
extern "C" int mgp_kmm_lambda_matvec(mgp_handle* h, const mgp_kernel* k, const void* Z, int64_t M,
                                     const void* lambda, const void* V, int64_t R, void* out) {
  if (!h) return MGP_E_BADARG;
  MGP_TRY(mgp_check_kernel(h, k));
  mgp_operator op;
  memset(&op, 0, sizeof(op));
  op.kind = MGP_OP_KMM_LAMBDA;
  op.dtype = k->dtype;
  op.n = M;
  op.kernel = k;
  op.Z = Z;
  op.M = M;
  op.lambda = lambda;
  return mgp_operator_apply(h, &op, V, R, out);
}
