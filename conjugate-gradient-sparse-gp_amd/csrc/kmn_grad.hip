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
//
// Gq == NULL (CDGP's trainable inducing inputs): W = Y Gb^T alone, of rank P.  Steps 1-3 and G2 fall away:
// up to kVjpPFused columns a fused pair kernel forms W_nm on the fly (kvjp_fused_kernel), beyond that W_panel is the
// one GEMM of step 3 without accumulate; steps 4-5 and the tail are shared.
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

// ---- Gq == NULL: the cotangent of K is W = Y Gb^T alone, of rank P -------------------------------------------------
// Fused form (P <= kVjpPFused): W is never stored.  A lane owns column m (b = z_m / l and Gb[m, p0:p0+PC] in
// registers); the rows of its block come by wave-uniform (scalar) loads from the pack XY[n][DP + PC] =
// (x_n / l, Y[n, p0:p0+PC]), the way kxx_grad_kernel streams block J, and each pair forms c = sum_p y_p gb_p on the
// fly.  Columns beyond PC are further passes over the pairs.  Panel form (larger P): W_panel = Y_panel Gb^T by the
// GEMM and kvjp_pairs_kernel, i.e. kvjp_run below without G2 and the K panel.  kVjpPFused is where the fused form
// stopped taking at most 0.9 of the panel form's time; -DMGP_KVJP_P_FUSED=<P> builds the other side of
// that comparison (0: panels always).
#ifndef MGP_KVJP_P_FUSED
#define MGP_KVJP_P_FUSED 12
#endif
constexpr int kVjpPFused = MGP_KVJP_P_FUSED;

// widest column pass of the fused form (kernel-resource-usage: no scratch and no SGPR spills at these widths; at 16
// columns Matern-1/2's division leaves too few SGPRs for a row, as in kxx_grad.hip)
constexpr int kvjp_pc_max(int DP, int KIND) { return KIND != 1 ? 16 : 8; }

// XY[i, 0:DP] = x_i / l (zeros for d >= D), XY[i, DP:DP+PC] = Y[i, p0:p0+pc] (zeros for the pad columns)
template <int DP, int PC>
__global__ __launch_bounds__(256) void kvjp_pack_xy_kernel(const double* __restrict__ Xp, long rows, int D,
                                                           SweepParams prm, const double* __restrict__ Yp, int P,
                                                           int p0, int pc, double* __restrict__ XY) {
  constexpr int RW = DP + PC;
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= rows * RW) return;
  const long i = e / RW;
  const int c = (int)(e - i * RW);
  double w = 0.0;
  if (c < DP) {
    if (c < D) w = Xp[i * D + c] * prm.inv_ls[c];
  } else if (c - DP < pc) {
    w = Yp[i * P + p0 + (c - DP)];
  }
  XY[e] = w;
}

// grid (column blocks of 256, row blocks of rows_per_block rows); partials laid out as kvjp_pairs_kernel's
template <int DP, int KIND, int PC>
__global__ __launch_bounds__(kVjpThreads) void kvjp_fused_kernel(const double* __restrict__ XY, long rows,
                                                                 const double* __restrict__ Z, long M, int D,
                                                                 SweepParams prm, const double* __restrict__ Gb, int P,
                                                                 int p0, int pc, long rows_per_block, int want_dz,
                                                                 double* __restrict__ part_s,
                                                                 double* __restrict__ part_z) {
  constexpr int RW = DP + PC;
  __shared__ double red[kVjpThreads / 64][DP + 1];
  const int t = threadIdx.x;
  const long m = (long)blockIdx.x * kVjpThreads + t;
  const bool live = m < M;
  const long ib = (long)blockIdx.y * rows_per_block;
  const long ie = ib + rows_per_block < rows ? ib + rows_per_block : rows;
  double b[DP], gb[PC];
  {
    const long mc = live ? m : M - 1;  // a lane past M carries gb = 0: every term it forms is 0
#pragma unroll
    for (int d = 0; d < DP; ++d) b[d] = d < D ? Z[mc * D + d] * prm.inv_ls[d] : 0.0;
#pragma unroll
    for (int q = 0; q < PC; ++q) gb[q] = (live && q < pc) ? Gb[mc * P + p0 + q] : 0.0;
  }
  double accl[DP], accz[DP], accv = 0.0;
#pragma unroll
  for (int d = 0; d < DP; ++d) accl[d] = accz[d] = 0.0;
  const double* rp = XY + ib * RW;  // wave-uniform: scalar loads
  for (long i = ib; i < ie; ++i) {
    double df[DP], r2 = 0.0;
#pragma unroll
    for (int d = 0; d < DP; ++d) {
      df[d] = rp[d] - b[d];
      r2 = mgp_fma(df[d], df[d], r2);
    }
    // the row's DP + PC streamed values fit the SGPR file at every instantiated width (no spills), so the scalar loads
    // of a row issue together and are waited for once; kxx_grad_kernel streams twice as many and has to stage them
    double c = 0.0;
#pragma unroll
    for (int q = 0; q < PC; ++q) c = mgp_fma(rp[DP + q], gb[q], c);
    double f, fp;
    mgp_profile_slope<KIND>(r2, f, fp);
    accv = mgp_fma(c, f, accv);
    const double g = c * fp;
#pragma unroll
    for (int d = 0; d < DP; ++d) {
      const double gd = g * df[d];
      accl[d] = mgp_fma(gd, df[d], accl[d]);
      accz[d] += gd;
    }
    rp += RW;
  }
  if (want_dz && live) {
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

template <int DP, int KIND, int PC>
int kvjp_fused_pass(mgp_handle* h, const double* Xp, long nr, const double* Z, long M, int D, const SweepParams& prm,
                    const double* Yp, const double* Gb, int P, int p0, int pc, dim3 grid, long rpb, int want_dz,
                    double* XY, double* part_s, double* part_z) {
  hipLaunchKernelGGL((kvjp_pack_xy_kernel<DP, PC>), dim3((unsigned)((nr * (DP + PC) + 255) / 256)), dim3(256), 0,
                     h->stream, Xp, nr, D, prm, Yp, P, p0, pc, XY);
  MGP_LAUNCH_CHECK(h);
  hipLaunchKernelGGL((kvjp_fused_kernel<DP, KIND, PC>), grid, dim3(kVjpThreads), 0, h->stream, (const double*)XY, nr, Z,
                     M, D, prm, Gb, P, p0, pc, rpb, want_dz, part_s, part_z);
  MGP_LAUNCH_CHECK(h);
  return MGP_OK;
}

// the tail shared by the three routes: dZ from the running column sums, the D + 1 scalars to the host
template <int DP>
int kvjp_finish(mgp_handle* h, const mgp_kernel* k, const SweepParams& prm, long M, const double* accs,
                const double* accz, double* dvar, double* dls, double* dZ) {
  const int D = k->D;
  SweepParams sc = prm;
  for (int d = 0; d < MGP_FUSED_MAX_D; ++d) sc.inv_ls[d] = d < D ? k->variance * (-2.0 / k->lengthscales[d]) : 0.0;
  if (dZ) {
    hipLaunchKernelGGL((kvjp_dz_kernel<DP>), dim3((unsigned)((M * D + 255) / 256)), dim3(256), 0, h->stream, accz, M, D,
                       sc, dZ);
    MGP_LAUNCH_CHECK(h);
  }
  std::vector<double> host(DP + 1);
  MGP_HIP(h, hipMemcpyAsync(host.data(), accs, host.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  MGP_HIP(h, hipStreamSynchronize(h->stream));
  *dvar = host[DP];
  for (int d = 0; d < D; ++d) dls[d] = sc.inv_ls[d] * host[d];
  return MGP_OK;
}

// Row blocks: at most ~4 workgroups per CU over the ncb column blocks (the partial arrays are sized by this bound),
// and for a chunk of nr rows whole multiples of kVjpTR rows per block.
inline long kvjp_max_row_blocks(const mgp_handle* h, long rows, long ncb) {
  long n = (4L * h->num_cus + ncb - 1) / ncb;
  const long cap = (rows + kVjpTR - 1) / kVjpTR;
  if (n > cap) n = cap;
  return n < 1 ? 1 : n;
}
inline void kvjp_row_blocks(long nr, long nrb_max, long* nrb, long* rpb) {
  long r = (nr + nrb_max - 1) / nrb_max;
  r = (r + kVjpTR - 1) / kVjpTR * kVjpTR;
  *rpb = r;
  *nrb = (nr + r - 1) / r;
}

template <int DP, int KIND>
int kvjp_rank_fused(mgp_handle* h, const mgp_kernel* k, const double* X, long N, const double* Z, long M,
                    const double* Y, const double* Gb, int P, long panel_rows, double* dvar, double* dls, double* dZ) {
  const int D = k->D;
  SweepParams prm = mgp_make_params(k);
  for (int d = 0; d < MGP_FUSED_MAX_D; ++d) prm.inv_ls[d] = d < D ? 1.0 / k->lengthscales[d] : 0.0;
  constexpr int PCM = kvjp_pc_max(DP, KIND);
  // row chunk: at most 64 MiB of pack (panel_rows > 0: that many rows)
  long rows = panel_rows > 0 ? panel_rows : (long)(((size_t)64 << 20) / ((size_t)(DP + PCM) * 8));
  if (rows > N) rows = N;
  const long ncb = (M + kVjpThreads - 1) / kVjpThreads;
  const long nrb_max = kvjp_max_row_blocks(h, rows, ncb);
  const bool want_dz = dZ != nullptr;
  // arena: XY | part_s | part_z | accs | accz  (each 256-byte aligned)
  auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
  const size_t b_xy = al((size_t)rows * (DP + PCM) * 8);
  const size_t b_ps = al((size_t)ncb * nrb_max * (DP + 1) * 8);
  const size_t b_pz = want_dz ? al((size_t)nrb_max * M * DP * 8) : 0;
  const size_t b_as = al((size_t)(DP + 1) * 8), b_az = want_dz ? al((size_t)M * DP * 8) : 0;
  MGP_TRY(mgp_reserve(h, &h->kgrad, &h->kgrad_bytes, b_xy + b_ps + b_pz + b_as + b_az));
  char* base = (char*)h->kgrad;
  double* XY = (double*)base;
  double* part_s = (double*)(base + b_xy);
  double* part_z = want_dz ? (double*)(base + b_xy + b_ps) : nullptr;
  double* accs = (double*)(base + b_xy + b_ps + b_pz);
  double* accz = want_dz ? (double*)(base + b_xy + b_ps + b_pz + b_as) : nullptr;
  MGP_HIP(h, hipMemsetAsync(accs, 0, (size_t)(DP + 1) * 8, h->stream));
  if (want_dz) MGP_HIP(h, hipMemsetAsync(accz, 0, (size_t)M * DP * 8, h->stream));
  for (long i0 = 0; i0 < N; i0 += rows) {
    const long nr = N - i0 < rows ? N - i0 : rows;
    long nrb, rpb;
    kvjp_row_blocks(nr, nrb_max, &nrb, &rpb);
    const dim3 grid((unsigned)ncb, (unsigned)nrb);
    const double *Xp = X + i0 * D, *Yp = Y + i0 * P;
    for (int p0 = 0; p0 < P;) {
      const int left = P - p0;
      // the pass's width: the narrowest of 2, 4, 8, PCM that holds what is left (pc live columns, the rest zeros)
      const int w = left > 8 ? PCM : (left > 4 ? 8 : (left > 2 ? 4 : 2));
      const int pc = left < w ? left : w;
      const int dz = want_dz ? 1 : 0;
      switch (w) {
        case 16:
          MGP_TRY((kvjp_fused_pass<DP, KIND, kvjp_pc_max(DP, KIND)>(h, Xp, nr, Z, M, D, prm, Yp, Gb, P, p0, pc, grid,
                                                                     rpb, dz, XY, part_s, part_z)));
          break;
        case 8:
          MGP_TRY((kvjp_fused_pass<DP, KIND, 8>(h, Xp, nr, Z, M, D, prm, Yp, Gb, P, p0, pc, grid, rpb, dz, XY, part_s,
                                                part_z)));
          break;
        case 4:
          MGP_TRY((kvjp_fused_pass<DP, KIND, 4>(h, Xp, nr, Z, M, D, prm, Yp, Gb, P, p0, pc, grid, rpb, dz, XY, part_s,
                                                part_z)));
          break;
        default:
          MGP_TRY((kvjp_fused_pass<DP, KIND, 2>(h, Xp, nr, Z, M, D, prm, Yp, Gb, P, p0, pc, grid, rpb, dz, XY, part_s,
                                                part_z)));
          break;
      }
      const long nfold = (want_dz ? M * DP : 0) + DP + 1;
      hipLaunchKernelGGL((kvjp_fold_kernel<DP>), dim3((unsigned)((nfold + 255) / 256)), dim3(256), 0, h->stream,
                         (const double*)part_s, ncb * nrb, (const double*)part_z, nrb, M, dz, accs, accz);
      MGP_LAUNCH_CHECK(h);
      p0 += pc;
    }
  }
  return kvjp_finish<DP>(h, k, prm, M, accs, accz, dvar, dls, dZ);
}

template <int DP, int KIND>
int kvjp_rank_panel(mgp_handle* h, const mgp_kernel* k, const double* X, long N, const double* Z, long M,
                    const double* Y, const double* Gb, int P, long panel_rows, double* dvar, double* dls, double* dZ) {
  const int D = k->D;
  SweepParams prm = mgp_make_params(k);
  for (int d = 0; d < MGP_FUSED_MAX_D; ++d) prm.inv_ls[d] = d < D ? 1.0 / k->lengthscales[d] : 0.0;
  // row panel: at most 256 MiB of W (panel_rows > 0: that many rows)
  long rows = (long)(((size_t)256 << 20) / ((size_t)M * 8));
  rows = rows < 16 ? 16 : rows / 16 * 16;
  if (panel_rows > 0) rows = panel_rows;
  if (rows > N) rows = N;
  const long ncb = (M + kVjpThreads - 1) / kVjpThreads;
  const long nrb_max = kvjp_max_row_blocks(h, rows, ncb);
  const bool want_dz = dZ != nullptr;
  // arena: W panel | part_s | part_z | accs | accz  (each 256-byte aligned)
  auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
  const size_t b_panel = al((size_t)rows * M * 8);
  const size_t b_ps = al((size_t)ncb * nrb_max * (DP + 1) * 8);
  const size_t b_pz = want_dz ? al((size_t)nrb_max * M * DP * 8) : 0;
  const size_t b_as = al((size_t)(DP + 1) * 8), b_az = want_dz ? al((size_t)M * DP * 8) : 0;
  MGP_TRY(mgp_reserve(h, &h->kgrad, &h->kgrad_bytes, b_panel + b_ps + b_pz + b_as + b_az));
  char* base = (char*)h->kgrad;
  double* Wp = (double*)base;
  double* part_s = (double*)(base + b_panel);
  double* part_z = want_dz ? (double*)(base + b_panel + b_ps) : nullptr;
  double* accs = (double*)(base + b_panel + b_ps + b_pz);
  double* accz = want_dz ? (double*)(base + b_panel + b_ps + b_pz + b_as) : nullptr;
  MGP_HIP(h, hipMemsetAsync(accs, 0, (size_t)(DP + 1) * 8, h->stream));
  if (want_dz) MGP_HIP(h, hipMemsetAsync(accz, 0, (size_t)M * DP * 8, h->stream));
  for (long i0 = 0; i0 < N; i0 += rows) {
    const long nr = N - i0 < rows ? N - i0 : rows;
    const double* Xp = X + i0 * D;
    MGP_TRY(mgp_gemm_nt(h, MGP_F64, Y + i0 * P, P, nr, Gb, P, M, P, Wp, M, 0, nullptr));
    long nrb, rpb;
    kvjp_row_blocks(nr, nrb_max, &nrb, &rpb);
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
  return kvjp_finish<DP>(h, k, prm, M, accs, accz, dvar, dls, dZ);
}

template <int DP, int KIND>
int kvjp_run(mgp_handle* h, const mgp_kernel* k, const double* X, long N, const double* Z, long M, const double* Gq,
             const double* Y, const double* Gb, int P, long panel_rows, double* dvar, double* dls, double* dZ) {
  const int D = k->D;
  SweepParams prm = mgp_make_params(k);
  for (int d = 0; d < MGP_FUSED_MAX_D; ++d) prm.inv_ls[d] = d < D ? 1.0 / k->lengthscales[d] : 0.0;
  // row panel: at most 256 MiB of K (and as much of W); panel_rows > 0: that many rows
  long rows = (long)(((size_t)256 << 20) / ((size_t)M * 8));
  rows = rows < 16 ? 16 : rows / 16 * 16;
  if (panel_rows > 0) rows = panel_rows;
  if (rows > N) rows = N;
  const long ncb = (M + kVjpThreads - 1) / kVjpThreads;
  const long nrb_max = kvjp_max_row_blocks(h, rows, ncb);
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
    long nrb, rpb;
    kvjp_row_blocks(nr, nrb_max, &nrb, &rpb);
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
  return kvjp_finish<DP>(h, k, prm, M, accs, accz, dvar, dls, dZ);
}

}  // namespace

int mgp_kvjp_symmetrize(mgp_handle* h, const double* Gq, long M, double* G2) {
  hipLaunchKernelGGL(kvjp_sym_kernel, dim3((unsigned)((M * M + 255) / 256)), dim3(256), 0, h->stream, Gq, M, G2);
  MGP_LAUNCH_CHECK(h);
  return MGP_OK;
}

int mgp_kvjp_check(mgp_handle* h, const mgp_kernel* k, const void* X, int64_t N, const void* Z, int64_t M,
                   const void* Gq, const void* Y, const void* Gb, int32_t P, int max_d, double* dvariance,
                   double* dlengthscales, void* dZ, int* done) {
  *done = 0;
  MGP_TRY(mgp_check_kernel(h, k));
  if (!dvariance || !dlengthscales) return mgp_fail(h, MGP_E_BADARG, "NULL output");
  *dvariance = 0.0;
  for (int d = 0; d < k->D; ++d) dlengthscales[d] = 0.0;
  if (k->dtype != MGP_F64) return mgp_fail(h, MGP_E_DTYPE, "kmn_knm_vjp: fp64 only");
  if (k->D > max_d) return mgp_fail(h, MGP_E_BADARG, "kmn_knm_vjp: D = %d > %d", k->D, max_d);
  if (N < 0 || M < 1 || P < 0) return mgp_fail(h, MGP_E_SHAPE, "kmn_knm_vjp: N >= 0, M >= 1, P >= 0 required");
  if (!Z) return mgp_fail(h, MGP_E_BADARG, "NULL data pointer");
  if (!Gq && (P < 1 || !Gb)) return mgp_fail(h, MGP_E_BADARG, "kmn_knm_vjp: Gq = NULL needs P >= 1 with Y and Gb");
  if (N == 0) {
    if (dZ) {
      MGP_HIP(h, hipMemsetAsync(dZ, 0, (size_t)M * k->D * 8, h->stream));
      MGP_HIP(h, hipStreamSynchronize(h->stream));
    }
    *done = 1;
    return MGP_OK;
  }
  if (!X) return mgp_fail(h, MGP_E_BADARG, "NULL data pointer");
  if (P > 0 && (!Y || !Gb)) return mgp_fail(h, MGP_E_BADARG, "kmn_knm_vjp: P > 0 needs Y and Gb");
  return MGP_OK;
}

int mgp_kvjp_fused_d(mgp_handle* h, const mgp_kernel* k, const double* Xd, long N, const double* Zd, long M,
                     const double* Gqd, const double* Yd, const double* Gbd, int P, long panel_rows, double* dvariance,
                     double* dlengthscales, double* dZd) {
  if (!Gqd)  // W = Y Gb^T alone: fused up to kVjpPFused columns, row panels of W beyond
    return mgp_with_kind(k->kind, [&](auto kind) {
      return mgp_with_dp<4>(k->D, [&](auto dp) {
        constexpr int DP = decltype(dp)::value, KIND = decltype(kind)::value;
        if (P <= kVjpPFused)
          return kvjp_rank_fused<DP, KIND>(h, k, Xd, N, Zd, M, Yd, Gbd, P, panel_rows, dvariance, dlengthscales, dZd);
        return kvjp_rank_panel<DP, KIND>(h, k, Xd, N, Zd, M, Yd, Gbd, P, panel_rows, dvariance, dlengthscales, dZd);
      });
    });
  return mgp_with_kind(k->kind, [&](auto kind) {
    return mgp_with_dp<4>(k->D, [&](auto dp) {
      return kvjp_run<decltype(dp)::value, decltype(kind)::value>(h, k, Xd, N, Zd, M, Gqd, Yd, Gbd, P, panel_rows,
                                                                  dvariance, dlengthscales, dZd);
    });
  });
}

extern "C" int mgp_kmn_knm_vjp(mgp_handle* h, const mgp_kernel* k, const void* X, int64_t N, const void* Z, int64_t M,
                               const void* Gq, const void* Y, const void* Gb, int32_t P, double* dvariance,
                               double* dlengthscales, void* dZ) {
  int done = 0;
  MGP_TRY(mgp_kvjp_check(h, k, X, N, Z, M, Gq, Y, Gb, P, MGP_FUSED_MAX_D, dvariance, dlengthscales, dZ, &done));
  if (done) return MGP_OK;
  return mgp_kvjp_fused_d(h, k, (const double*)X, N, (const double*)Z, M, (const double*)Gq,
                          P > 0 ? (const double*)Y : nullptr, P > 0 ? (const double*)Gb : nullptr, P, 0, dvariance,
                          dlengthscales, (double*)dZ);
}
