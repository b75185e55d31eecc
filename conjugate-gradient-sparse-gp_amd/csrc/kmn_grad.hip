// kmn_grad.hip -- VJP of (theta, Z) -> (Q, B) = (K_mn K_nm, K_mn Y), K = k(X, Z): the N-sized part of the gradient of
// Titsias' collapsed bound (SGPR), which depends on the data only through Q, B = K_mn y and y^T y.
//
// With cotangents Gq [M, M] and Gb [M, P] the cotangent of K [N, M] is
//     W = K (Gq + Gq^T) + Y Gb^T
// and the outputs are the contractions of W with the kernel's derivatives:
//     dvariance   = sum_nm W_nm f(r2_nm)                                       (f = k / variance)
//     dl_d        = variance (-2 / l_d) sum_nm W_nm f'(r2_nm) (a_nd - b_md)^2    (a = x / l, b = z / l)
//     dZ_md       = variance (-2 / l_d) sum_n  W_nm f'(r2_nm) (a_nd - b_md)
// with f' = df/dr2 as grad.hip forms it (Matern-1/2: 0 at GPflow's 1e-36 floor, so a data row equal to an inducing
// point adds nothing to the lengthscales or to dZ, and never a NaN) and r2 from direct differences: a gradient
// amplifies the cancellation of the expansion form.
//
// Form: rows of X are cut into panels of at most 256 MiB of K.  Per panel
//   1. K_panel = k(X_panel, Z)                         kvjp_kpanel_kernel, direct differences
//   2. W_panel = K_panel (Gq + Gq^T)                   the fp64 MFMA NT GEMM of dense.hip (G2 = Gq + Gq^T is exactly
//                                                      symmetric, so K G2^T = K G2); 2 rows M^2 flop
//   3. W_panel += Y_panel Gb^T                         the same GEMM with accumulate, contraction length P
//   4. kvjp_pairs_kernel: one lane per column m (z_m in registers), rows staged through LDS; each pair reads W_nm once
//      and adds to D + 1 workgroup sums and, with dZ, D per-column sums of its row block
//   5. kvjp_fold_kernel: the row-block partials of the panel are added in block order to running sums
// so nothing N x M outlives a panel.  Every sum is taken in a fixed order (no float atomics): two calls are
// bit-identical.  The W round trip through HBM costs ~3 rows M 8 bytes per panel (write, read-modify-write, read) on
// top of a GEMM of 2 rows M^2 flop; at C3 everything but the main GEMM measured ~69 of 594 ms.
#include <vector>

#include "mgp_common.h"

namespace {

constexpr int kVjpThreads = 256;  // columns per workgroup of the pair kernel
constexpr int kVjpTR = 32;        // rows staged per LDS tile

// G2 = Gq + Gq^T (G2[i, j] and G2[j, i] are the same two addends: exactly symmetric)
__global__ __launch_bounds__(256) void kvjp_sym_kernel(const double* __restrict__ Gq, long M, double* __restrict__ G2) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= M * M) return;
  const long i = e / M, j = e - i * M;
  G2[e] = Gq[i * M + j] + Gq[j * M + i];
}

// K_panel[n, m] = variance f(r2_nm), r2 from direct differences as in the pair kernel (the expansion form's
// cancellation, amplified by the square root of the Matern profiles, would put ~1e-8 into K at coincident points).
// grid (column blocks of 256, row blocks of kVjpTR rows); one lane per column, rows staged through LDS.
template <int DP, int KIND>
__global__ __launch_bounds__(kVjpThreads) void kvjp_kpanel_kernel(const double* __restrict__ Xp, long rows,
                                                                  const double* __restrict__ Z, long M, int D,
                                                                  SweepParams prm, double* __restrict__ Kp) {
  __shared__ double xs[kVjpTR * DP];
  const int t = threadIdx.x;
  const long m = (long)blockIdx.x * kVjpThreads + t;
  const long i0 = (long)blockIdx.y * kVjpTR;
  for (int e = t; e < kVjpTR * DP; e += kVjpThreads) {
    const long i = i0 + e / DP;
    const int d = e % DP;
    xs[e] = (i < rows && d < D) ? Xp[i * D + d] * prm.inv_ls[d] : 0.0;
  }
  __syncthreads();
  if (m >= M) return;
  double b[DP];
#pragma unroll
  for (int d = 0; d < DP; ++d) b[d] = d < D ? Z[m * D + d] * prm.inv_ls[d] : 0.0;
  const int lim = rows - i0 < kVjpTR ? (int)(rows - i0) : kVjpTR;
  for (int ii = 0; ii < lim; ++ii) {
    double r2 = 0.0;
#pragma unroll
    for (int d = 0; d < DP; ++d) {
      const double df = xs[ii * DP + d] - b[d];
      r2 = mgp_fma(df, df, r2);
    }
    double f, fp;
    mgp_profile_slope<KIND>(r2, f, fp);
    Kp[(i0 + ii) * M + m] = prm.variance * f;
  }
}

// grid (column blocks of 256, row blocks of rows_per_block rows of the panel).  part_s[blk][DP + 1] (DP lengthscale
// sums, then the variance sum), blk = blockIdx.y * gridDim.x + blockIdx.x; with DZ part_z[blockIdx.y][M][DP].
template <int DP, int KIND, bool DZ>
__global__ __launch_bounds__(kVjpThreads) void kvjp_pairs_kernel(const double* __restrict__ Xp, long rows,
                                                                 const double* __restrict__ Z, long M, int D,
                                                                 SweepParams prm, const double* __restrict__ W,
                                                                 long rows_per_block, double* __restrict__ part_s,
                                                                 double* __restrict__ part_z) {
  __shared__ double xs[kVjpTR * DP];
  __shared__ double red[kVjpThreads / 64][DP + 1];
  const int t = threadIdx.x;
  const long m = (long)blockIdx.x * kVjpThreads + t;
  const bool live = m < M;
  const long ib = (long)blockIdx.y * rows_per_block;
  const long ie = ib + rows_per_block < rows ? ib + rows_per_block : rows;
  double b[DP];
  {
    const long mc = live ? m : M - 1;
#pragma unroll
    for (int d = 0; d < DP; ++d) b[d] = d < D ? Z[mc * D + d] * prm.inv_ls[d] : 0.0;
  }
  double accl[DP], accz[DP], accv = 0.0;
#pragma unroll
  for (int d = 0; d < DP; ++d) accl[d] = accz[d] = 0.0;
  for (long i0 = ib; i0 < ie; i0 += kVjpTR) {
    __syncthreads();
    for (int e = t; e < kVjpTR * DP; e += kVjpThreads) {
      const long i = i0 + e / DP;
      const int d = e % DP;
      xs[e] = (i < ie && d < D) ? Xp[i * D + d] * prm.inv_ls[d] : 0.0;
    }
    __syncthreads();
    if (live) {
      const int lim = (ie - i0) < kVjpTR ? (int)(ie - i0) : kVjpTR;
      const double* wp = W + i0 * M + m;
      for (int ii = 0; ii < lim; ++ii) {
        const double w = wp[(long)ii * M];
        const double* xr = &xs[ii * DP];
        double r2 = 0.0;
#pragma unroll
        for (int d = 0; d < DP; ++d) {
          const double df = xr[d] - b[d];
          r2 = mgp_fma(df, df, r2);
        }
        double f, fp;
        mgp_profile_slope<KIND>(r2, f, fp);
        accv = mgp_fma(w, f, accv);
        const double g = w * fp;
#pragma unroll
        for (int d = 0; d < DP; ++d) {
          const double df = xr[d] - b[d];
          const double gd = g * df;
          accl[d] = mgp_fma(gd, df, accl[d]);
          if (DZ) accz[d] += gd;
        }
      }
    }
  }
  if (DZ && live) {
    double* oz = part_z + ((long)blockIdx.y * M + m) * DP;
#pragma unroll
    for (int d = 0; d < DP; ++d) oz[d] = accz[d];
  }
  // workgroup sum of the DP + 1 scalars: wave butterflies, then the four waves in order
  const int lane = t & 63, wave = t >> 6;
#pragma unroll
  for (int d = 0; d <= DP; ++d) {
    const double v = mgp_wave_sum(d < DP ? accl[d] : accv);
    if (lane == 0) red[wave][d] = v;
  }
  __syncthreads();
  if (t <= DP) {
    const long blk = (long)blockIdx.y * gridDim.x + blockIdx.x;
    part_s[blk * (DP + 1) + t] = (red[0][t] + red[1][t]) + (red[2][t] + red[3][t]);
  }
}

// running sums += the panel's partials, each element summed over the blocks in block order
template <int DP>
__global__ __launch_bounds__(256) void kvjp_fold_kernel(const double* __restrict__ part_s, long nblk,
                                                        const double* __restrict__ part_z, long nrb, long M, int dz,
                                                        double* __restrict__ accs, double* __restrict__ accz) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  const long nz = dz ? M * DP : 0;
  if (e < nz) {
    double s = 0.0;
    for (long r = 0; r < nrb; ++r) s += part_z[r * M * DP + e];
    accz[e] += s;
  } else if (e < nz + DP + 1) {
    const int q = (int)(e - nz);
    double s = 0.0;
    for (long b = 0; b < nblk; ++b) s += part_s[b * (DP + 1) + q];
    accs[q] += s;
  }
}

// dZ[m, d] = scale_d accz[m, d]  (scale_d = variance * -2 / l_d, passed in prm.inv_ls)
template <int DP>
__global__ __launch_bounds__(256) void kvjp_dz_kernel(const double* __restrict__ accz, long M, int D, SweepParams sc,
                                                      double* __restrict__ dZ) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= M * D) return;
  const long m = e / D;
  const int d = (int)(e - m * D);
  dZ[e] = sc.inv_ls[d] * accz[m * DP + d];
}

template <int DP, int KIND>
int kvjp_run(mgp_handle* h, const mgp_kernel* k, const double* X, long N, const double* Z, long M, const double* Gq,
             const double* Y, const double* Gb, int P, double* dvar, double* dls, double* dZ) {
  const int D = k->D;
  SweepParams prm = mgp_make_params(k);
  for (int d = 0; d < MGP_FUSED_MAX_D; ++d) prm.inv_ls[d] = d < D ? 1.0 / k->lengthscales[d] : 0.0;
  // row panel: at most 256 MiB of K (and as much of W)
  long rows = (long)(((size_t)256 << 20) / ((size_t)M * 8));
  rows = rows < 16 ? 16 : rows / 16 * 16;
  if (rows > N) rows = N;
  const long ncb = (M + kVjpThreads - 1) / kVjpThreads;
  long nrb_max = (4L * h->num_cus + ncb - 1) / ncb;  // row blocks of a full panel: ~4 workgroups per CU
  const long rb_cap = (rows + kVjpTR - 1) / kVjpTR;
  if (nrb_max > rb_cap) nrb_max = rb_cap;
  if (nrb_max < 1) nrb_max = 1;
  const bool want_dz = dZ != nullptr;
  // arena: K panel | W panel | G2 | part_s | part_z | accs | accz  (each 256-byte aligned)
  auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
  const size_t b_panel = al((size_t)rows * M * 8), b_g2 = al((size_t)M * M * 8);
  const size_t b_ps = al((size_t)ncb * nrb_max * (DP + 1) * 8);
  const size_t b_pz = want_dz ? al((size_t)nrb_max * M * DP * 8) : 0;
  const size_t b_as = al((size_t)(DP + 1) * 8), b_az = want_dz ? al((size_t)M * DP * 8) : 0;
  MGP_TRY(mgp_reserve(h, &h->kgrad, &h->kgrad_bytes, 2 * b_panel + b_g2 + b_ps + b_pz + b_as + b_az));
  char* base = (char*)h->kgrad;
  double* Kp = (double*)base;
  double* Wp = (double*)(base + b_panel);
  double* G2 = (double*)(base + 2 * b_panel);
  double* part_s = (double*)(base + 2 * b_panel + b_g2);
  double* part_z = want_dz ? (double*)(base + 2 * b_panel + b_g2 + b_ps) : nullptr;
  double* accs = (double*)(base + 2 * b_panel + b_g2 + b_ps + b_pz);
  double* accz = want_dz ? (double*)(base + 2 * b_panel + b_g2 + b_ps + b_pz + b_as) : nullptr;
  MGP_HIP(h, hipMemsetAsync(accs, 0, (size_t)(DP + 1) * 8, h->stream));
  if (want_dz) MGP_HIP(h, hipMemsetAsync(accz, 0, (size_t)M * DP * 8, h->stream));
  hipLaunchKernelGGL(kvjp_sym_kernel, dim3((unsigned)((M * M + 255) / 256)), dim3(256), 0, h->stream, Gq, M, G2);
  MGP_LAUNCH_CHECK(h);
  for (long i0 = 0; i0 < N; i0 += rows) {
    const long nr = N - i0 < rows ? N - i0 : rows;
    const double* Xp = X + i0 * D;
    hipLaunchKernelGGL((kvjp_kpanel_kernel<DP, KIND>), dim3((unsigned)ncb, (unsigned)((nr + kVjpTR - 1) / kVjpTR)),
                       dim3(kVjpThreads), 0, h->stream, Xp, nr, Z, M, D, prm, Kp);
    MGP_LAUNCH_CHECK(h);
    MGP_TRY(mgp_gemm_nt(h, MGP_F64, Kp, M, nr, G2, M, M, M, Wp, M, 0, nullptr));
    if (P > 0) MGP_TRY(mgp_gemm_nt(h, MGP_F64, Y + i0 * P, P, nr, Gb, P, M, P, Wp, M, 1, nullptr));
    long nrb = nrb_max, rpb = (nr + nrb - 1) / nrb;
    rpb = (rpb + kVjpTR - 1) / kVjpTR * kVjpTR;
    nrb = (nr + rpb - 1) / rpb;
    const dim3 grid((unsigned)ncb, (unsigned)nrb);
    if (want_dz)
      hipLaunchKernelGGL((kvjp_pairs_kernel<DP, KIND, true>), grid, dim3(kVjpThreads), 0, h->stream, Xp, nr, Z, M, D,
                         prm, (const double*)Wp, rpb, part_s, part_z);
    else
      hipLaunchKernelGGL((kvjp_pairs_kernel<DP, KIND, false>), grid, dim3(kVjpThreads), 0, h->stream, Xp, nr, Z, M, D,
                         prm, (const double*)Wp, rpb, part_s, part_z);
    MGP_LAUNCH_CHECK(h);
    const long nfold = (want_dz ? M * DP : 0) + DP + 1;
    hipLaunchKernelGGL((kvjp_fold_kernel<DP>), dim3((unsigned)((nfold + 255) / 256)), dim3(256), 0, h->stream,
                       (const double*)part_s, ncb * nrb, (const double*)part_z, nrb, M, want_dz ? 1 : 0, accs, accz);
    MGP_LAUNCH_CHECK(h);
  }
  SweepParams sc = prm;
  for (int d = 0; d < MGP_FUSED_MAX_D; ++d) sc.inv_ls[d] = d < D ? k->variance * (-2.0 / k->lengthscales[d]) : 0.0;
  if (want_dz) {
    hipLaunchKernelGGL((kvjp_dz_kernel<DP>), dim3((unsigned)((M * D + 255) / 256)), dim3(256), 0, h->stream,
                       (const double*)accz, M, D, sc, dZ);
    MGP_LAUNCH_CHECK(h);
  }
  std::vector<double> host(DP + 1);
  MGP_HIP(h, hipMemcpyAsync(host.data(), accs, host.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  MGP_HIP(h, hipStreamSynchronize(h->stream));
  *dvar = host[DP];
  for (int d = 0; d < D; ++d) dls[d] = sc.inv_ls[d] * host[d];
  return MGP_OK;
}

}  // namespace

extern "C" int mgp_kmn_knm_vjp(mgp_handle* h, const mgp_kernel* k, const void* X, int64_t N, const void* Z, int64_t M,
                               const void* Gq, const void* Y, const void* Gb, int32_t P, double* dvariance,
                               double* dlengthscales, void* dZ) {
  MGP_TRY(mgp_check_kernel(h, k));
  if (!dvariance || !dlengthscales) return mgp_fail(h, MGP_E_BADARG, "NULL output");
  *dvariance = 0.0;
  for (int d = 0; d < k->D; ++d) dlengthscales[d] = 0.0;
  if (k->dtype != MGP_F64) return mgp_fail(h, MGP_E_DTYPE, "kmn_knm_vjp: fp64 only");
  if (k->D > MGP_FUSED_MAX_D) return mgp_fail(h, MGP_E_BADARG, "kmn_knm_vjp: D = %d > %d", k->D, MGP_FUSED_MAX_D);
  if (N < 0 || M < 1 || P < 0) return mgp_fail(h, MGP_E_SHAPE, "kmn_knm_vjp: N >= 0, M >= 1, P >= 0 required");
  if (!Z || !Gq) return mgp_fail(h, MGP_E_BADARG, "NULL data pointer");
  if (N == 0) {
    if (dZ) {
      MGP_HIP(h, hipMemsetAsync(dZ, 0, (size_t)M * k->D * 8, h->stream));
      MGP_HIP(h, hipStreamSynchronize(h->stream));
    }
    return MGP_OK;
  }
  if (!X) return mgp_fail(h, MGP_E_BADARG, "NULL data pointer");
  if (P > 0 && (!Y || !Gb)) return mgp_fail(h, MGP_E_BADARG, "kmn_knm_vjp: P > 0 needs Y and Gb");
  const double *Xd = (const double*)X, *Zd = (const double*)Z, *Gqd = (const double*)Gq;
  const double *Yd = P > 0 ? (const double*)Y : nullptr, *Gbd = P > 0 ? (const double*)Gb : nullptr;
  double* dZd = (double*)dZ;
  return mgp_with_kind(k->kind, [&](auto kind) {
    return mgp_with_dp<4>(k->D, [&](auto dp) {
      return kvjp_run<decltype(dp)::value, decltype(kind)::value>(h, k, Xd, N, Zd, M, Gqd, Yd, Gbd, P, dvariance,
                                                                  dlengthscales, dZd);
    });
  });
}
