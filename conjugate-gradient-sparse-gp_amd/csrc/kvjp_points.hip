// kvjp_points.hip -- mgp_k_dense_vjp_points (include/mgp_points.h): the VJP of a dense kernel block K = k(A, B) at a
// dense cotangent G [na, nb] (leading dimension ldg), in the hyper-parameters AND in the points:
//     dvariance = sum_ij G_ij f_ij                                      (f = k / variance)
//     dl_d      = variance (-2 / l_d) sum_ij G_ij f'_ij (a_id - b_jd)^2   (a = A / l, b = B / l, f' = df/dr2)
//     dA_id     = variance ( 2 / l_d) sum_j  G_ij f'_ij (a_id - b_jd)
//     dB_jd     = variance (-2 / l_d) sum_i  G_ij f'_ij (a_id - b_jd)
// with f, f' from mgp_profile_slope (Matern slopes exactly 0 at GPflow's r2 floor) and r2 from direct differences.
// Nothing of size na x nb x D exists anywhere; rows of A are walked in panels.
//
// D <= MGP_FUSED_MAX_D, per row panel:
//   kpts_col_kernel<DP, KIND, DZ>   the scheme of kmn_grad.hip's kvjp_pairs_kernel with W := G at leading dimension ldg:
//                                   a lane owns column j (b_j, its DP column sums and the DP + 1 scalar sums in
//                                   registers), rows staged through LDS kTile at a time and read as broadcasts
//   kpts_row_kernel<DP, KIND, V2>   a lane owns row i (a_i and its DP sums in registers), columns staged through LDS
//                                   kTile at a time and read as broadcasts; the lane reads its own G[i, j0 : j0 + CH]
//                                   by contiguous loads, 128-bit ones (V2) when G and ldg allow 16-byte alignment: a
//                                   lane consumes whole 128-byte lines (CH = 16; 8 at DP = 32 and 4 for Matern-1/2,
//                                   whose lines are finished over 2 and 4 trips)
//   Each kernel evaluates the pair; G is read from memory twice per call.  A coalesced [256 x 32] tile of G read
//   transposed from LDS would be 64 KB + padding per workgroup, one workgroup per CU: the per-lane form needs no LDS
//   for G and leaves the LDS pipe to the broadcasts.
// D > MGP_FUSED_MAX_D, per row panel (the two-stage form of kmn_grad_generic.hip):
//   kpts_slope_kernel<KIND, TR>     64 x 64 tiles, 4 x 4 pairs per thread, r2 over 16-dimension LDS stages; the G f
//                                   share of dvariance per tile, H = G f' to a scratch panel [rows, nb] and, with TR
//                                   (dA wanted), H^T [nb, rows] through a padded LDS tile.  G is read once.
//   kpts_slice_kernel<LS, DZ>       a lane owns one point and one slice of 32 dimensions: on (A panel, B, H) the
//                                   lengthscale sums and dB's, on (B, A panel, H^T) dA's -- the same kernel, so the
//                                   row side needs no pair kernel of its own
// Block partials are folded in block order (kpts_fold_kernel, kpts_fold_scalars_kernel): no float atomics, every sum has
// a fixed order, two calls give the same bits.  dA of a panel is complete when the panel is (all columns seen) and is
// written then; dB and the scalars continue in running sums over the panels.
#include <cstdint>
#include <vector>

#include "../../include/mgp_points.h"
#include "mgp_common.h"

namespace {

constexpr int kThreads = 256;  // points a workgroup of a pair kernel owns
constexpr int kTile = 32;      // streamed points per LDS stage
constexpr int GT = 64;         // tile edge of the slope kernel
constexpr int GK = 16;         // dimensions per LDS stage of the slope kernel
constexpr int kSliceD = 32;    // dimensions a lane of the slice kernel owns

// ---- D <= 32 ---------------------------------------------------------------------------------------------------------
// grid (column blocks of 256, row blocks of rows_per_block rows of the panel).  part_s[blk][DP + 1] (DP lengthscale
// sums, then the variance sum), blk = blockIdx.y * gridDim.x + blockIdx.x; with DZ part_b[blockIdx.y][nb][DP].
template <int DP, int KIND, bool DZ>
__global__ __launch_bounds__(kThreads) void kpts_col_kernel(const double* __restrict__ Ap, long rows,
                                                            const double* __restrict__ B, long nb, int D,
                                                            SweepParams prm, const double* __restrict__ G, long ldg,
                                                            long rows_per_block, double* __restrict__ part_s,
                                                            double* __restrict__ part_b) {
  __shared__ double xs[kTile * DP];
  __shared__ double red[kThreads / 64][DP + 1];
  const int t = threadIdx.x;
  const long m = (long)blockIdx.x * kThreads + t;
  const bool live = m < nb;
  const long ib = (long)blockIdx.y * rows_per_block;
  const long ie = ib + rows_per_block < rows ? ib + rows_per_block : rows;
  double b[DP];
  {
    const long mc = live ? m : nb - 1;
#pragma unroll
    for (int d = 0; d < DP; ++d) b[d] = d < D ? B[mc * D + d] * prm.inv_ls[d] : 0.0;
  }
  double accl[DP], accz[DP], accv = 0.0;
#pragma unroll
  for (int d = 0; d < DP; ++d) accl[d] = accz[d] = 0.0;
  for (long i0 = ib; i0 < ie; i0 += kTile) {
    __syncthreads();
    for (int e = t; e < kTile * DP; e += kThreads) {
      const long i = i0 + e / DP;
      const int d = e % DP;
      xs[e] = (i < ie && d < D) ? Ap[i * D + d] * prm.inv_ls[d] : 0.0;
    }
    __syncthreads();
    if (live) {
      const int lim = (ie - i0) < kTile ? (int)(ie - i0) : kTile;
      const double* gp = G + i0 * ldg + m;
      for (int ii = 0; ii < lim; ++ii) {
        const double w = gp[(long)ii * ldg];
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
    double* oz = part_b + ((long)blockIdx.y * nb + m) * DP;
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

// grid (row blocks of 256 rows of the panel, column blocks of cols_per_block columns).  part_a[blockIdx.y][rows][DP]:
// the lane's row sums of G f' (a - b) over the columns of its block, columns in ascending order.
template <int DP, int KIND, bool V2>
__global__ __launch_bounds__(kThreads) void kpts_row_kernel(const double* __restrict__ Ap, long rows,
                                                            const double* __restrict__ B, long nb, int D,
                                                            SweepParams prm, const double* __restrict__ G, long ldg,
                                                            long cols_per_block, double* __restrict__ part_a) {
  // elements of G a lane loads at a time (Matern-1/2: its slope divides, and more than 4 unrolled divisions spill)
  constexpr int CH = KIND == 1 ? 4 : (DP >= 32 ? 8 : 16);
  __shared__ double bs[kTile * DP];
  const int t = threadIdx.x;
  const long i = (long)blockIdx.x * kThreads + t;
  const bool live = i < rows;
  const long jb = (long)blockIdx.y * cols_per_block;
  const long je = jb + cols_per_block < nb ? jb + cols_per_block : nb;
  double a[DP], acc[DP];
  {
    const long ic = live ? i : rows - 1;
#pragma unroll
    for (int d = 0; d < DP; ++d) {
      a[d] = d < D ? Ap[ic * D + d] * prm.inv_ls[d] : 0.0;
      acc[d] = 0.0;
    }
  }
  for (long j0 = jb; j0 < je; j0 += kTile) {
    __syncthreads();
    for (int e = t; e < kTile * DP; e += kThreads) {
      const long j = j0 + e / DP;
      const int d = e % DP;
      bs[e] = (j < je && d < D) ? B[j * D + d] * prm.inv_ls[d] : 0.0;
    }
    __syncthreads();
    if (live) {
      const int lim = (je - j0) < kTile ? (int)(je - j0) : kTile;
      const double* gp = G + i * ldg + j0;
      for (int c0 = 0; c0 < lim; c0 += CH) {
        double g[CH];
        if (V2 && c0 + CH <= lim) {
#pragma unroll
          for (int q = 0; q < CH / 2; ++q) {
            const double2 v = reinterpret_cast<const double2*>(gp + c0)[q];
            g[2 * q] = v.x;
            g[2 * q + 1] = v.y;
          }
        } else {
#pragma unroll
          for (int q = 0; q < CH; ++q) g[q] = c0 + q < lim ? gp[c0 + q] : 0.0;  // beyond lim: bs is 0 there, adds 0
        }
#pragma unroll
        for (int q = 0; q < CH; ++q) {
          const double* br = &bs[(c0 + q) * DP];
          double r2 = 0.0;
#pragma unroll
          for (int d = 0; d < DP; ++d) {
            const double df = a[d] - br[d];
            r2 = mgp_fma(df, df, r2);
          }
          double f, fp;
          mgp_profile_slope<KIND>(r2, f, fp);
          const double hh = g[q] * fp;
#pragma unroll
          for (int d = 0; d < DP; ++d) acc[d] = mgp_fma(hh, a[d] - br[d], acc[d]);
        }
      }
    }
  }
  if (live) {
    double* oa = part_a + ((long)blockIdx.y * rows + i) * DP;
#pragma unroll
    for (int d = 0; d < DP; ++d) oa[d] = acc[d];
  }
}

// ---- D > 32 ----------------------------------------------------------------------------------------------------------
// H[i, j] = G[i, j] f'(r2_ij) (panel rows, leading dimension nb), with TR also Ht[j, i] (leading dimension rows), and
// part_v[tile] = the tile's sum of G f.  grid (column tiles, row tiles).
template <int KIND, bool TR>
__global__ __launch_bounds__(256) void kpts_slope_kernel(const double* __restrict__ Ap, long rows,
                                                         const double* __restrict__ B, long nb, int D,
                                                         const double* __restrict__ inv_ls,
                                                         const double* __restrict__ G, long ldg,
                                                         double* __restrict__ H, double* __restrict__ Ht,
                                                         double* __restrict__ part_v) {
  __shared__ double As[GT][GK + 1];
  __shared__ double Bs[GT][GK + 1];
  __shared__ double Ts[TR ? GT : 1][GT + 1];  // the tile of H, read transposed (stride 65: no bank conflicts)
  __shared__ double red[4];
  const int t = threadIdx.x, tx = t & 15, ty = t >> 4, lane = t & 63, wave = t >> 6;
  const long i0 = (long)blockIdx.y * GT, j0 = (long)blockIdx.x * GT;
  double r2[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) r2[a][b] = 0;
  for (int d0 = 0; d0 < D; d0 += GK) {
    __syncthreads();
    for (int e = t; e < GT * GK; e += 256) {
      const int r = e / GK, d = e % GK;
      const double sc = d0 + d < D ? inv_ls[d0 + d] : 0.0;
      As[r][d] = (i0 + r < rows && d0 + d < D) ? Ap[(i0 + r) * D + d0 + d] * sc : 0.0;
      Bs[r][d] = (j0 + r < nb && d0 + d < D) ? B[(j0 + r) * D + d0 + d] * sc : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int d = 0; d < GK; ++d) {
      double av[4], bv[4];
#pragma unroll
      for (int a = 0; a < 4; ++a) av[a] = As[ty * 4 + a][d];
#pragma unroll
      for (int b = 0; b < 4; ++b) bv[b] = Bs[tx + 16 * b][d];
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const double df = av[a] - bv[b];
          r2[a][b] = mgp_fma(df, df, r2[a][b]);
        }
    }
  }
  double gf = 0.0;
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const long i = i0 + ty * 4 + a;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const long j = j0 + tx + 16 * b;
      double hv = 0.0;
      if (i < rows && j < nb) {
        const double w = G[i * ldg + j];
        double f, fp;
        mgp_profile_slope<KIND>(r2[a][b], f, fp);
        gf = mgp_fma(w, f, gf);
        hv = w * fp;
        H[i * nb + j] = hv;
      }
      if (TR) Ts[ty * 4 + a][tx + 16 * b] = hv;
    }
  }
  if (TR) {
    __syncthreads();
    for (int e = t; e < GT * GT; e += 256) {
      const int jj = e / GT, ii = e % GT;
      if (i0 + ii < rows && j0 + jj < nb) Ht[(j0 + jj) * rows + i0 + ii] = Ts[ii][jj];
    }
  }
  const double v = mgp_wave_sum(gf);
  if (lane == 0) red[wave] = v;
  __syncthreads();
  if (t == 0) part_v[(long)blockIdx.y * gridDim.x + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// The scheme of kmn_grad_generic.hip's kvjp_pairs_generic_kernel with the leading dimension of H as an argument and
// the lengthscale sums optional.  Owners are the rows of Z [M, D], streamed are the rows of Xp [rows, D]; H is
// [rows, ldh] with the owner index contiguous.  grid (owner blocks of 256, slices of 32 dimensions, blocks of
// rows_per_block streamed rows).  Sums of H (x - z)^2 to part_l[(blockIdx.z * gridDim.x + blockIdx.x)][nsl * 32] (LS),
// of H (x - z) to part_z[blockIdx.z][M][D] (DZ).
template <bool LS, bool DZ>
__global__ __launch_bounds__(kThreads) void kpts_slice_kernel(const double* __restrict__ Xp, long rows,
                                                              const double* __restrict__ Z, long M, int D,
                                                              const double* __restrict__ inv_ls,
                                                              const double* __restrict__ H, long ldh,
                                                              long rows_per_block, double* __restrict__ part_l,
                                                              double* __restrict__ part_z) {
  __shared__ double xs[kTile * kSliceD];
  __shared__ double red[kThreads / 64][kSliceD];
  const int t = threadIdx.x;
  const long m = (long)blockIdx.x * kThreads + t;
  const bool live = m < M;
  const int d0 = (int)blockIdx.y * kSliceD;
  const long ib = (long)blockIdx.z * rows_per_block;
  const long ie = ib + rows_per_block < rows ? ib + rows_per_block : rows;
  double b[kSliceD];
  {
    const long mc = live ? m : M - 1;
#pragma unroll
    for (int d = 0; d < kSliceD; ++d) b[d] = d0 + d < D ? Z[mc * D + d0 + d] * inv_ls[d0 + d] : 0.0;
  }
  double accl[kSliceD], accz[kSliceD];
#pragma unroll
  for (int d = 0; d < kSliceD; ++d) accl[d] = accz[d] = 0.0;
  for (long i0 = ib; i0 < ie; i0 += kTile) {
    __syncthreads();
    for (int e = t; e < kTile * kSliceD; e += kThreads) {
      const long i = i0 + e / kSliceD;
      const int d = d0 + e % kSliceD;
      xs[e] = (i < ie && d < D) ? Xp[i * D + d] * inv_ls[d] : 0.0;
    }
    __syncthreads();
    if (live) {
      const int lim = (ie - i0) < kTile ? (int)(ie - i0) : kTile;
      const double* hp = H + i0 * ldh + m;
      for (int ii = 0; ii < lim; ++ii) {
        const double g = hp[(long)ii * ldh];
        const double* xr = &xs[ii * kSliceD];
#pragma unroll
        for (int d = 0; d < kSliceD; ++d) {
          const double df = xr[d] - b[d];
          const double gd = g * df;
          if (LS) accl[d] = mgp_fma(gd, df, accl[d]);
          if (DZ) accz[d] += gd;
        }
      }
    }
  }
  if (DZ && live) {
    double* oz = part_z + ((long)blockIdx.z * M + m) * D + d0;
#pragma unroll
    for (int d = 0; d < kSliceD; ++d)
      if (d0 + d < D) oz[d] = accz[d];
  }
  if (LS) {
    const int lane = t & 63, wave = t >> 6;
#pragma unroll
    for (int d = 0; d < kSliceD; ++d) {
      const double v = mgp_wave_sum(accl[d]);
      if (lane == 0) red[wave][d] = v;
    }
    __syncthreads();
    if (t < kSliceD) {
      const long blk = (long)blockIdx.z * gridDim.x + blockIdx.x;
      part_l[(blk * gridDim.y + blockIdx.y) * kSliceD + t] = (red[0][t] + red[1][t]) + (red[2][t] + red[3][t]);
    }
  }
}

// ---- folds -----------------------------------------------------------------------------------------------------------
// s[p, d] = sum over the blocks, in block order, of part[b][p][0:W] (d < D).  With acc [npts][W]: the running sum
// continues from it and is left in it.  With out [npts, D]: out = coef * inv_d * s, inv_d = 1 / l_d from inv_dev or,
// when that is null, from prm.
__global__ __launch_bounds__(256) void kpts_fold_kernel(const double* __restrict__ part, long nblk, long npts, int W,
                                                        int D, double* __restrict__ acc, double* __restrict__ out,
                                                        SweepParams prm, const double* __restrict__ inv_dev,
                                                        double coef) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= npts * D) return;
  const long p = e / D;
  const int d = (int)(e - p * D);
  double s = 0.0;
  for (long b = 0; b < nblk; ++b) s += part[(b * npts + p) * W + d];
  if (acc) {
    s = acc[p * W + d] + s;
    acc[p * W + d] = s;
  }
  if (out) out[e] = coef * (inv_dev ? inv_dev[d] : prm.inv_ls[d]) * s;
}

// accs[q] += sum over the blocks of part_l[b * ncols + q], q < ncols, in block order; accs[vidx] += the sum of the nvb
// tile partials of dvariance (lane t adds tiles t, t + 256, ... in order, then wave butterflies and the four waves in
// order).  One workgroup.
__global__ __launch_bounds__(256) void kpts_fold_scalars_kernel(const double* __restrict__ part_l, long nlb, int ncols,
                                                                const double* __restrict__ part_v, long nvb, int vidx,
                                                                double* __restrict__ accs) {
  __shared__ double red[4];
  const int t = threadIdx.x;
  for (int q = t; q < ncols; q += 256) {
    double s = 0.0;
    for (long b = 0; b < nlb; ++b) s += part_l[b * ncols + q];
    accs[q] += s;
  }
  if (nvb > 0) {
    double s = 0.0;
    for (long q = t; q < nvb; q += 256) s += part_v[q];
    s = mgp_wave_sum(s);
    if ((t & 63) == 0) red[t >> 6] = s;
    __syncthreads();
    if (t == 0) accs[vidx] += (red[0] + red[1]) + (red[2] + red[3]);
  }
}

// ---- host ------------------------------------------------------------------------------------------------------------
inline size_t al(size_t b) { return (b + 255) & ~(size_t)255; }
inline long cdiv(long a, long b) { return (a + b - 1) / b; }

// blocks of the streamed side: enough workgroups for 4 per CU, at least one stage each, and (want_pts) the
// [blocks][owners][W] partials at most 128 MiB unless one block alone is more
inline long kpts_max_blocks(const mgp_handle* h, long owner_groups, long streamed, long owners, long W, bool want_pts) {
  long n = cdiv(4L * h->num_cus, owner_groups);
  const long cap = cdiv(streamed, kTile);
  if (n > cap) n = cap;
  if (want_pts) {
    const long capz = (long)(((size_t)128 << 20) / ((size_t)owners * W * 8));
    if (n > capz) n = capz;
  }
  return n < 1 ? 1 : n;
}
// streamed points per block (a multiple of kTile) and the blocks that gives
inline void kpts_blocks(long streamed, long nmax, long* nblk, long* per) {
  long p = cdiv(streamed, nmax);
  p = cdiv(p, kTile) * kTile;
  *per = p;
  *nblk = cdiv(streamed, p);
}

template <int DP, int KIND>
int kpts_fused_run(mgp_handle* h, const mgp_kernel* k, const double* A, long na, const double* B, long nb,
                   const double* G, long ldg, long panel_rows, double* dvar, double* dls, double* dA, double* dB) {
  const int D = k->D;
  SweepParams prm;
  for (int d = 0; d < MGP_FUSED_MAX_D; ++d) prm.inv_ls[d] = d < D ? 1.0 / k->lengthscales[d] : 0.0;
  prm.variance = k->variance;
  prm.clamp = 0.0;
  long rows = (1L << 24) / DP;  // one [rows, DP] block of dA partials is at most 128 MiB
  if (panel_rows > 0) rows = panel_rows;
  if (rows > na) rows = na;
  const bool want_a = dA != nullptr, want_b = dB != nullptr;
  const long ncb = cdiv(nb, kThreads), nrg = cdiv(rows, kThreads);
  const long nrb_max = kpts_max_blocks(h, ncb, rows, nb, DP, want_b);
  const long nkb_max = kpts_max_blocks(h, nrg, nb, rows, DP, true);
  // arena: part_b | part_a | part_s | accs | accb
  const size_t b_pb = want_b ? al((size_t)nrb_max * nb * DP * 8) : 0;
  const size_t b_pa = want_a ? al((size_t)nkb_max * rows * DP * 8) : 0;
  const size_t b_ps = al((size_t)nrb_max * ncb * (DP + 1) * 8), b_as = al((size_t)(DP + 1) * 8);
  const size_t b_ab = want_b ? al((size_t)nb * DP * 8) : 0;
  MGP_TRY(mgp_reserve(h, &h->kgrad, &h->kgrad_bytes, b_pb + b_pa + b_ps + b_as + b_ab));
  char* q = (char*)h->kgrad;
  double* part_b = want_b ? (double*)q : nullptr;
  double* part_a = want_a ? (double*)(q + b_pb) : nullptr;
  double* part_s = (double*)(q + b_pb + b_pa);
  double* accs = (double*)(q + b_pb + b_pa + b_ps);
  double* accb = want_b ? (double*)(q + b_pb + b_pa + b_ps + b_as) : nullptr;
  MGP_HIP(h, hipMemsetAsync(accs, 0, (size_t)(DP + 1) * 8, h->stream));
  if (want_b) MGP_HIP(h, hipMemsetAsync(accb, 0, (size_t)nb * DP * 8, h->stream));
  const bool v2 = ((uintptr_t)G % 16 == 0) && (ldg % 2 == 0);
  const double two_var = 2.0 * k->variance;
  for (long i0 = 0; i0 < na; i0 += rows) {
    const long nr = na - i0 < rows ? na - i0 : rows;
    const bool last = i0 + nr >= na;
    const double* Ap = A + i0 * D;
    const double* Gp = G + i0 * ldg;
    long nrb, rpb;
    kpts_blocks(nr, nrb_max, &nrb, &rpb);
    const dim3 cgrid((unsigned)ncb, (unsigned)nrb);
    if (want_b)
      hipLaunchKernelGGL((kpts_col_kernel<DP, KIND, true>), cgrid, dim3(kThreads), 0, h->stream, Ap, nr, B, nb, D, prm,
                         Gp, ldg, rpb, part_s, part_b);
    else
      hipLaunchKernelGGL((kpts_col_kernel<DP, KIND, false>), cgrid, dim3(kThreads), 0, h->stream, Ap, nr, B, nb, D, prm,
                         Gp, ldg, rpb, part_s, part_b);
    MGP_LAUNCH_CHECK(h);
    hipLaunchKernelGGL(kpts_fold_scalars_kernel, dim3(1), dim3(256), 0, h->stream, (const double*)part_s, nrb * ncb,
                       DP + 1, (const double*)nullptr, 0L, DP, accs);
    MGP_LAUNCH_CHECK(h);
    if (want_b) {
      hipLaunchKernelGGL(kpts_fold_kernel, dim3((unsigned)cdiv(nb * D, 256)), dim3(256), 0, h->stream,
                         (const double*)part_b, nrb, nb, DP, D, accb, last ? dB : (double*)nullptr, prm,
                         (const double*)nullptr, -two_var);
      MGP_LAUNCH_CHECK(h);
    }
    if (want_a) {
      long nkb, cpb;
      kpts_blocks(nb, nkb_max, &nkb, &cpb);
      const dim3 rgrid((unsigned)cdiv(nr, kThreads), (unsigned)nkb);
      if (v2)
        hipLaunchKernelGGL((kpts_row_kernel<DP, KIND, true>), rgrid, dim3(kThreads), 0, h->stream, Ap, nr, B, nb, D,
                           prm, Gp, ldg, cpb, part_a);
      else
        hipLaunchKernelGGL((kpts_row_kernel<DP, KIND, false>), rgrid, dim3(kThreads), 0, h->stream, Ap, nr, B, nb, D,
                           prm, Gp, ldg, cpb, part_a);
      MGP_LAUNCH_CHECK(h);
      hipLaunchKernelGGL(kpts_fold_kernel, dim3((unsigned)cdiv(nr * D, 256)), dim3(256), 0, h->stream,
                         (const double*)part_a, nkb, nr, DP, D, (double*)nullptr, dA + i0 * D, prm,
                         (const double*)nullptr, two_var);
      MGP_LAUNCH_CHECK(h);
    }
  }
  return mgp_fold_vjp_partials(h, accs, 1, DP + 1, k, dvar, dls);
}

template <int KIND>
int kpts_generic_run(mgp_handle* h, const mgp_kernel* k, const double* A, long na, const double* B, long nb,
                     const double* G, long ldg, long panel_rows, double* dvar, double* dls, double* dA, double* dB) {
  const int D = k->D;
  double inv[MGP_MAX_D];
  for (int d = 0; d < D; ++d) inv[d] = 1.0 / k->lengthscales[d];
  long rows = (long)(((size_t)256 << 20) / ((size_t)nb * 8));  // H (and H^T): at most 256 MiB
  const long rows_a = (long)(((size_t)128 << 20) / ((size_t)D * 8));  // one [rows, D] block of dA partials: 128 MiB
  if (rows > rows_a) rows = rows_a;
  rows = rows < 16 ? 16 : rows / 16 * 16;
  if (panel_rows > 0) rows = panel_rows;
  if (rows > (1L << 21)) rows = 1L << 21;  // the slope kernel's row tiles are a grid dimension (< 65536)
  if (rows > na) rows = na;
  const bool want_a = dA != nullptr, want_b = dB != nullptr;
  const long nsl = cdiv(D, kSliceD), ldl = nsl * kSliceD;
  const long ncb = cdiv(nb, kThreads), nrg = cdiv(rows, kThreads);
  const long nrb_max = kpts_max_blocks(h, ncb * nsl, rows, nb, D, want_b);
  const long nkb_max = kpts_max_blocks(h, nrg * nsl, nb, rows, D, true);
  const long ntx = cdiv(nb, GT), nty_max = cdiv(rows, GT);
  // arena: H | Ht | part_b | part_a | part_l | part_v | accs | accb
  const size_t b_h = al((size_t)rows * nb * 8), b_ht = want_a ? b_h : 0;
  const size_t b_pb = want_b ? al((size_t)nrb_max * nb * D * 8) : 0;
  const size_t b_pa = want_a ? al((size_t)nkb_max * rows * D * 8) : 0;
  const size_t b_pl = al((size_t)nrb_max * ncb * ldl * 8), b_pv = al((size_t)ntx * nty_max * 8);
  const size_t b_as = al((size_t)(ldl + 1) * 8), b_ab = want_b ? al((size_t)nb * D * 8) : 0;
  MGP_TRY(mgp_reserve(h, &h->kgrad, &h->kgrad_bytes, b_h + b_ht + b_pb + b_pa + b_pl + b_pv + b_as + b_ab));
  char* q = (char*)h->kgrad;
  double* H = (double*)q;
  double* Ht = want_a ? (double*)(q + b_h) : nullptr;
  q += b_h + b_ht;
  double* part_b = want_b ? (double*)q : nullptr;
  double* part_a = want_a ? (double*)(q + b_pb) : nullptr;
  double* part_l = (double*)(q + b_pb + b_pa);
  double* part_v = (double*)(q + b_pb + b_pa + b_pl);
  double* accs = (double*)(q + b_pb + b_pa + b_pl + b_pv);
  double* accb = want_b ? (double*)(q + b_pb + b_pa + b_pl + b_pv + b_as) : nullptr;
  MGP_HIP(h, hipMemsetAsync(accs, 0, (size_t)(ldl + 1) * 8, h->stream));
  if (want_b) MGP_HIP(h, hipMemsetAsync(accb, 0, (size_t)nb * D * 8, h->stream));
  MGP_HIP(h, hipMemcpyAsync(h->dparams, inv, (size_t)D * sizeof(double), hipMemcpyHostToDevice, h->stream));
  MGP_HIP(h, hipStreamSynchronize(h->stream));  // inv[] is this frame's
  const double* dinv = h->dparams;
  const SweepParams none = {};
  const double two_var = 2.0 * k->variance;
  for (long i0 = 0; i0 < na; i0 += rows) {
    const long nr = na - i0 < rows ? na - i0 : rows;
    const bool last = i0 + nr >= na;
    const double* Ap = A + i0 * D;
    const double* Gp = G + i0 * ldg;
    const long nty = cdiv(nr, GT);
    const dim3 sgrid((unsigned)ntx, (unsigned)nty);
    if (want_a)
      hipLaunchKernelGGL((kpts_slope_kernel<KIND, true>), sgrid, dim3(256), 0, h->stream, Ap, nr, B, nb, D, dinv, Gp,
                         ldg, H, Ht, part_v);
    else
      hipLaunchKernelGGL((kpts_slope_kernel<KIND, false>), sgrid, dim3(256), 0, h->stream, Ap, nr, B, nb, D, dinv, Gp,
                         ldg, H, Ht, part_v);
    MGP_LAUNCH_CHECK(h);
    long nrb, rpb;
    kpts_blocks(nr, nrb_max, &nrb, &rpb);
    const dim3 cgrid((unsigned)ncb, (unsigned)nsl, (unsigned)nrb);
    if (want_b)
      hipLaunchKernelGGL((kpts_slice_kernel<true, true>), cgrid, dim3(kThreads), 0, h->stream, Ap, nr, B, nb, D, dinv,
                         (const double*)H, nb, rpb, part_l, part_b);
    else
      hipLaunchKernelGGL((kpts_slice_kernel<true, false>), cgrid, dim3(kThreads), 0, h->stream, Ap, nr, B, nb, D, dinv,
                         (const double*)H, nb, rpb, part_l, part_b);
    MGP_LAUNCH_CHECK(h);
    hipLaunchKernelGGL(kpts_fold_scalars_kernel, dim3(1), dim3(256), 0, h->stream, (const double*)part_l, nrb * ncb,
                       (int)ldl, (const double*)part_v, ntx * nty, (int)ldl, accs);
    MGP_LAUNCH_CHECK(h);
    if (want_b) {
      hipLaunchKernelGGL(kpts_fold_kernel, dim3((unsigned)cdiv(nb * D, 256)), dim3(256), 0, h->stream,
                         (const double*)part_b, nrb, nb, D, D, accb, last ? dB : (double*)nullptr, none, dinv,
                         -two_var);
      MGP_LAUNCH_CHECK(h);
    }
    if (want_a) {
      // owners: the panel's rows; streamed: the columns; the kernel sums H (b - a), so the coefficient is dB's
      long nkb, cpb;
      kpts_blocks(nb, nkb_max, &nkb, &cpb);
      const dim3 rgrid((unsigned)cdiv(nr, kThreads), (unsigned)nsl, (unsigned)nkb);
      hipLaunchKernelGGL((kpts_slice_kernel<false, true>), rgrid, dim3(kThreads), 0, h->stream, B, nb, Ap, nr, D, dinv,
                         (const double*)Ht, nr, cpb, (double*)nullptr, part_a);
      MGP_LAUNCH_CHECK(h);
      hipLaunchKernelGGL(kpts_fold_kernel, dim3((unsigned)cdiv(nr * D, 256)), dim3(256), 0, h->stream,
                         (const double*)part_a, nkb, nr, D, D, (double*)nullptr, dA + i0 * D, none, dinv, -two_var);
      MGP_LAUNCH_CHECK(h);
    }
  }
  // accs: ldl lengthscale sums (the first D count), then the variance sum
  return mgp_fold_vjp_partials(h, accs, 1, (int)ldl + 1, k, dvar, dls);
}

}  // namespace

extern "C" int mgp_k_dense_vjp_points(mgp_handle* h, const mgp_kernel* k, const void* A, int64_t na, const void* B,
                                      int64_t nb, const void* G, int64_t ldg, int64_t panel_rows, double* dvariance,
                                      double* dlengthscales, void* dA, void* dB) {
  MGP_TRY(mgp_check_kernel(h, k));
  if (k->dtype != MGP_F64) return mgp_fail(h, MGP_E_DTYPE, "k_dense_vjp_points: fp64 only");
  if (!dvariance || !dlengthscales)
    return mgp_fail(h, MGP_E_BADARG, "k_dense_vjp_points: dvariance and dlengthscales are required");
  if (na < 0 || nb < 0) return mgp_fail(h, MGP_E_SHAPE, "k_dense_vjp_points: na, nb >= 0 required");
  if (ldg < nb) return mgp_fail(h, MGP_E_SHAPE, "k_dense_vjp_points: ldg=%lld < nb=%lld", (long long)ldg, (long long)nb);
  if (panel_rows < 0) return mgp_fail(h, MGP_E_SHAPE, "k_dense_vjp_points: panel_rows >= 0 required");
  if ((na > 0 && !A) || (nb > 0 && !B) || (na > 0 && nb > 0 && !G))
    return mgp_fail(h, MGP_E_BADARG, "k_dense_vjp_points: A, B and G are required");
  const int D = k->D;
  *dvariance = 0.0;
  for (int d = 0; d < D; ++d) dlengthscales[d] = 0.0;
  if (na == 0 || nb == 0) {
    if (dA && na > 0) MGP_HIP(h, hipMemsetAsync(dA, 0, (size_t)na * D * 8, h->stream));
    if (dB && nb > 0) MGP_HIP(h, hipMemsetAsync(dB, 0, (size_t)nb * D * 8, h->stream));
    MGP_HIP(h, hipStreamSynchronize(h->stream));
    return MGP_OK;
  }
  const double *Ad = (const double*)A, *Bd = (const double*)B, *Gd = (const double*)G;
  return mgp_with_kind(k->kind, [&](auto kind) -> int {
    constexpr int KIND = decltype(kind)::value;
    if (D > MGP_FUSED_MAX_D)
      return kpts_generic_run<KIND>(h, k, Ad, na, Bd, nb, Gd, ldg, (long)panel_rows, dvariance, dlengthscales,
                                    (double*)dA, (double*)dB);
    return mgp_with_dp(D, [&](auto dp) -> int {
      return kpts_fused_run<decltype(dp)::value, KIND>(h, k, Ad, na, Bd, nb, Gd, ldg, (long)panel_rows, dvariance,
                                                       dlengthscales, (double*)dA, (double*)dB);
    });
  });
}
