// kmn_grad_generic.hip -- mgp_kmn_knm_vjp_anyd (include/mgp_anyd.h): the VJP of kmn_grad.hip at any input dimension
// D <= MGP_MAX_D, with the row panel as an argument.  D <= MGP_FUSED_MAX_D goes to kmn_grad.hip's implementation
// (a point's coordinates and its 2 DP sums in registers); this file is the route above that, where neither fits.
//
// Same quantities as kmn_grad.hip:4-12 (W = K (Gq + Gq^T) + Y Gb^T; dvariance = sum W f; dl_d and dZ_md the sums of
// H (a_nd - b_md)^2 and H (a_nd - b_md), H = W f', scaled by variance (-2 / l_d)), r2 from direct differences.  Per row
// panel of X:
//   1. K_panel = k(X_panel, Z)                 mgp_k_dense_generic (direct differences, 16 dimensions per LDS stage)
//   2. W_panel = K_panel G2 (+ Y_panel Gb^T)   the fp64 MFMA NT GEMM of dense.hip; Gq == NULL: Y_panel Gb^T alone and
//                                              steps 1 and G2 fall away
//   3. kvjp_slope_generic_kernel<KIND>         64 x 64 tiles, 4 x 4 pairs per thread, as k_dense_vjp_generic_kernel:
//                                              r2 over the dimension slices, the W f share of dvariance per tile, and
//                                              H = W f' written over W (the panel is scratch)
//   4. kvjp_pairs_generic_kernel<DZ>           a lane owns column m and ONE slice of kSliceD = 32 dimensions for the
//                                              whole row block: b = z_m / l of the slice and the 2 x 32 sums live in
//                                              registers, rows are staged through LDS kPairTR at a time and read as
//                                              broadcasts, H_nm is read once per slice (coalesced over m)
//   5. kvjp_fold_generic_kernel                row-block partials added to the running sums in block order
// Tail: dZ = scale_d accz (kvjp_dz_generic_kernel), the D + 1 scalars through mgp_fold_vjp_partials.
//
// Why the slice is the outer loop and H goes through memory: the per-column dZ sums of a strip over all D do not fit
// on chip (64 columns x 512 dimensions = 256 KB), and keeping H in registers while sweeping the slices means adding
// every tile's slice sums into the partial array in memory (a read-modify-write of 16 bytes per 64 pair-dimensions,
// ~0.25 byte per pair-dimension, against a working set of [row blocks][M][D] that lives in HBM).  With the slice
// outermost the sums of a (row block, column, slice) never leave registers until the block is done: no
// read-modify-write, no cross-lane reduction for dZ at all (each lane owns its column: rows are added in ascending
// order), and H costs one store and ceil(D / 32) coalesced loads per pair (~0.25 byte per pair-dimension, read-only).
// Static LDS: 17.4 KB (slope kernel), 9.2 KB (pair kernel).
//
// Arena rule (kgrad): panels as kmn_grad.hip (K and W, at most 256 MiB each, + G2).  Row blocks per panel
//     nrb <= min(ceil(4 CUs / (ncb nsl)), ceil(rows / kPairTR), dZ ? max(1, 128 MiB / (8 M D)) : inf)
// (ncb = ceil(M / 256) column blocks, nsl = ceil(D / 32) slices), rows_per_block = ceil(rows / nrb) rounded up to
// kPairTR: the [nrb][M][D] partials of dZ are capped at 128 MiB (16 MiB each at M = 4096, D = 512: 4 row blocks by the
// first bound, 64 MiB), the running sums [M][D] add one more block, and the lengthscale partials
// [nrb ncb][nsl 32] and the variance partials [tiles] are small: below the 256 MiB of the panel they serve.
//
// Scales: SweepParams::inv_ls holds 32 entries, so the D reciprocals 1 / l_d (and, for the tail, variance (-2 / l_d))
// go through h->dparams, uploaded on the stream after the K panel's kernel (which reads c / l_d from the same buffer).
// Every sum has a fixed order (no float atomics): two calls are bit-identical.
#include <vector>

#include "../../include/mgp_anyd.h"
#include "mgp_common.h"

namespace {

constexpr int GT = 64;          // tile edge of the slope kernel
constexpr int GK = 16;          // dimensions per LDS stage of the slope kernel (as generic.hip: the K panel's order)
constexpr int kSliceD = 32;     // dimensions a lane of the pair kernel owns
constexpr int kPairCols = 256;  // columns per workgroup of the pair kernel
constexpr int kPairTR = 32;     // rows staged per LDS tile of the pair kernel

// In place W -> H = W f'(r2), and part_v[tile] = sum over the tile of W f(r2).  grid (column tiles, row tiles).
template <int KIND>
__global__ __launch_bounds__(256) void kvjp_slope_generic_kernel(const double* __restrict__ Xp, long rows,
                                                                 const double* __restrict__ Z, long M, int D,
                                                                 const double* __restrict__ inv_ls,
                                                                 double* __restrict__ W, double* __restrict__ part_v) {
  __shared__ double As[GT][GK + 1];
  __shared__ double Bs[GT][GK + 1];
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
      As[r][d] = (i0 + r < rows && d0 + d < D) ? Xp[(i0 + r) * D + d0 + d] * sc : 0.0;
      Bs[r][d] = (j0 + r < M && d0 + d < D) ? Z[(j0 + r) * D + d0 + d] * sc : 0.0;
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
      if (i < rows && j < M) {
        const double w = W[i * M + j];
        double f, fp;
        mgp_profile_slope<KIND>(r2[a][b], f, fp);
        gf = mgp_fma(w, f, gf);
        W[i * M + j] = w * fp;
      }
    }
  }
  const double v = mgp_wave_sum(gf);
  if (lane == 0) red[wave] = v;
  __syncthreads();
  if (t == 0) part_v[(long)blockIdx.y * gridDim.x + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// grid (column blocks of kPairCols, slices of kSliceD dimensions, row blocks of rows_per_block rows of the panel).
// part_l[(row block * ncb + column block)][nsl * kSliceD]: the workgroup's lengthscale sums of its slice;
// with DZ part_z[row block][M][D]: the lane's column sums of its slice.
template <bool DZ>
__global__ __launch_bounds__(kPairCols) void kvjp_pairs_generic_kernel(const double* __restrict__ Xp, long rows,
                                                                       const double* __restrict__ Z, long M, int D,
                                                                       const double* __restrict__ inv_ls,
                                                                       const double* __restrict__ H,
                                                                       long rows_per_block,
                                                                       double* __restrict__ part_l,
                                                                       double* __restrict__ part_z) {
  __shared__ double xs[kPairTR * kSliceD];
  __shared__ double red[kPairCols / 64][kSliceD];
  const int t = threadIdx.x;
  const long m = (long)blockIdx.x * kPairCols + t;
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
  for (long i0 = ib; i0 < ie; i0 += kPairTR) {
    __syncthreads();
    for (int e = t; e < kPairTR * kSliceD; e += kPairCols) {
      const long i = i0 + e / kSliceD;
      const int d = d0 + e % kSliceD;
      xs[e] = (i < ie && d < D) ? Xp[i * D + d] * inv_ls[d] : 0.0;
    }
    __syncthreads();
    if (live) {
      const int lim = (ie - i0) < kPairTR ? (int)(ie - i0) : kPairTR;
      const double* hp = H + i0 * M + m;
      for (int ii = 0; ii < lim; ++ii) {
        const double g = hp[(long)ii * M];
        const double* xr = &xs[ii * kSliceD];
#pragma unroll
        for (int d = 0; d < kSliceD; ++d) {
          const double df = xr[d] - b[d];
          const double gd = g * df;
          accl[d] = mgp_fma(gd, df, accl[d]);
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
  // workgroup sum of the slice's lengthscale sums: wave butterflies, then the four waves in order
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

// running sums += the panel's partials, each element summed over its blocks in block order.  accs[0:D] the
// lengthscale sums, accs[D] the variance sum; accz [M, D].  The last workgroup of the grid takes the variance sum: a
// panel has one partial per 64 x 64 tile (8192 at M = 4096), so lane t adds tiles t, t + 256, ... in order, then the
// lanes are added by wave butterflies and the four waves in order -- fixed, but not one thread's chain of loads.
__global__ __launch_bounds__(256) void kvjp_fold_generic_kernel(const double* __restrict__ part_z, long nrb, long MD,
                                                                const double* __restrict__ part_l, long nlb, long ldl,
                                                                int D, const double* __restrict__ part_v, long nvb,
                                                                int dz, double* __restrict__ accs,
                                                                double* __restrict__ accz) {
  __shared__ double red[4];
  if (blockIdx.x == gridDim.x - 1) {
    const int t = threadIdx.x;
    double s = 0.0;
    for (long q = t; q < nvb; q += 256) s += part_v[q];
    s = mgp_wave_sum(s);
    if ((t & 63) == 0) red[t >> 6] = s;
    __syncthreads();
    if (t == 0) accs[D] += (red[0] + red[1]) + (red[2] + red[3]);
    return;
  }
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  const long nz = dz ? MD : 0;
  if (e < nz) {
    double s = 0.0;
    for (long r = 0; r < nrb; ++r) s += part_z[r * MD + e];
    accz[e] += s;
  } else if (e < nz + D) {
    const long d = e - nz;
    double s = 0.0;
    for (long q = 0; q < nlb; ++q) s += part_l[q * ldl + d];
    accs[d] += s;
  }
}

// dZ[m, d] = scale_d accz[m, d]  (scale_d = variance * -2 / l_d, in h->dparams)
__global__ __launch_bounds__(256) void kvjp_dz_generic_kernel(const double* __restrict__ accz, long MD, int D,
                                                              const double* __restrict__ scale,
                                                              double* __restrict__ dZ) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= MD) return;
  dZ[e] = scale[e % D] * accz[e];
}

// D doubles to h->dparams, ordered on the stream behind whatever still reads the buffer
int kvjp_upload(mgp_handle* h, int D, const double* host) {
  MGP_HIP(h, hipMemcpyAsync(h->dparams, host, (size_t)D * sizeof(double), hipMemcpyHostToDevice, h->stream));
  MGP_HIP(h, hipStreamSynchronize(h->stream));  // host[] is the caller's temporary
  return MGP_OK;
}

int kvjp_generic_run(mgp_handle* h, const mgp_kernel* k, const double* X, long N, const double* Z, long M,
                     const double* Gq, const double* Y, const double* Gb, int P, long panel_rows, double* dvar,
                     double* dls, double* dZ) {
  const int D = k->D;
  double inv[MGP_MAX_D], sc[MGP_MAX_D];
  for (int d = 0; d < D; ++d) {
    inv[d] = 1.0 / k->lengthscales[d];  // plain reciprocals, as grad.hip
    sc[d] = k->variance * (-2.0 / k->lengthscales[d]);
  }
  long rows = (long)(((size_t)256 << 20) / ((size_t)M * 8));
  rows = rows < 16 ? 16 : rows / 16 * 16;
  if (panel_rows > 0) rows = panel_rows;
  if (rows > (1L << 21)) rows = 1L << 21;  // the slope kernel's row tiles are a grid dimension (< 65536)
  if (rows > N) rows = N;
  const bool want_dz = dZ != nullptr, with_k = Gq != nullptr;
  const long ncb = (M + kPairCols - 1) / kPairCols, nsl = (D + kSliceD - 1) / kSliceD;
  const long MD = M * D;
  long nrb_max = (4L * h->num_cus + ncb * nsl - 1) / (ncb * nsl);
  const long cap_rows = (rows + kPairTR - 1) / kPairTR;
  if (nrb_max > cap_rows) nrb_max = cap_rows;
  if (want_dz) {
    const long cap_z = (long)(((size_t)128 << 20) / ((size_t)MD * 8));
    if (nrb_max > cap_z) nrb_max = cap_z;
  }
  if (nrb_max < 1) nrb_max = 1;
  const long ntx = (M + GT - 1) / GT, nty_max = (rows + GT - 1) / GT;
  const long ldl = nsl * kSliceD;
  // arena: K panel | W panel | G2 | part_z | part_l | part_v | accs | accz  (each 256-byte aligned)
  auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
  const size_t b_panel = al((size_t)rows * M * 8), b_k = with_k ? b_panel : 0, b_g2 = with_k ? al((size_t)M * M * 8) : 0;
  const size_t b_pz = want_dz ? al((size_t)nrb_max * MD * 8) : 0;
  const size_t b_pl = al((size_t)nrb_max * ncb * ldl * 8), b_pv = al((size_t)ntx * nty_max * 8);
  const size_t b_as = al((size_t)(D + 1) * 8), b_az = want_dz ? al((size_t)MD * 8) : 0;
  MGP_TRY(mgp_reserve(h, &h->kgrad, &h->kgrad_bytes, b_k + b_panel + b_g2 + b_pz + b_pl + b_pv + b_as + b_az));
  char* base = (char*)h->kgrad;
  double* Kp = with_k ? (double*)base : nullptr;
  double* Wp = (double*)(base + b_k);
  double* G2 = with_k ? (double*)(base + b_k + b_panel) : nullptr;
  char* q = base + b_k + b_panel + b_g2;
  double* part_z = want_dz ? (double*)q : nullptr;
  double* part_l = (double*)(q + b_pz);
  double* part_v = (double*)(q + b_pz + b_pl);
  double* accs = (double*)(q + b_pz + b_pl + b_pv);
  double* accz = want_dz ? (double*)(q + b_pz + b_pl + b_pv + b_as) : nullptr;
  MGP_HIP(h, hipMemsetAsync(accs, 0, (size_t)(D + 1) * 8, h->stream));
  if (want_dz) MGP_HIP(h, hipMemsetAsync(accz, 0, (size_t)MD * 8, h->stream));
  if (with_k) MGP_TRY(mgp_kvjp_symmetrize(h, Gq, M, G2));
  else MGP_TRY(kvjp_upload(h, D, inv));
  const double* dinv = h->dparams;
  for (long i0 = 0; i0 < N; i0 += rows) {
    const long nr = N - i0 < rows ? N - i0 : rows;
    const double* Xp = X + i0 * D;
    if (with_k) {
      MGP_TRY(mgp_k_dense_generic(h, k, Xp, nr, Z, M, Kp, M, 0.0, nullptr, nullptr));  // leaves c / l in h->dparams
      MGP_TRY(mgp_gemm_nt(h, MGP_F64, Kp, M, nr, G2, M, M, M, Wp, M, 0, nullptr));
      if (P > 0) MGP_TRY(mgp_gemm_nt(h, MGP_F64, Y + i0 * P, P, nr, Gb, P, M, P, Wp, M, 1, nullptr));
      MGP_TRY(kvjp_upload(h, D, inv));
    } else {
      MGP_TRY(mgp_gemm_nt(h, MGP_F64, Y + i0 * P, P, nr, Gb, P, M, P, Wp, M, 0, nullptr));
    }
    const long nty = (nr + GT - 1) / GT;
    MGP_TRY(mgp_with_kind(k->kind, [&](auto kind) -> int {
      hipLaunchKernelGGL((kvjp_slope_generic_kernel<decltype(kind)::value>), dim3((unsigned)ntx, (unsigned)nty),
                         dim3(256), 0, h->stream, Xp, nr, Z, M, D, dinv, Wp, part_v);
      MGP_LAUNCH_CHECK(h);
      return MGP_OK;
    }));
    long rpb = (nr + nrb_max - 1) / nrb_max;
    rpb = (rpb + kPairTR - 1) / kPairTR * kPairTR;
    const long nrb = (nr + rpb - 1) / rpb;
    const dim3 grid((unsigned)ncb, (unsigned)nsl, (unsigned)nrb);
    if (want_dz)
      hipLaunchKernelGGL((kvjp_pairs_generic_kernel<true>), grid, dim3(kPairCols), 0, h->stream, Xp, nr, Z, M, D, dinv,
                         (const double*)Wp, rpb, part_l, part_z);
    else
      hipLaunchKernelGGL((kvjp_pairs_generic_kernel<false>), grid, dim3(kPairCols), 0, h->stream, Xp, nr, Z, M, D, dinv,
                         (const double*)Wp, rpb, part_l, part_z);
    MGP_LAUNCH_CHECK(h);
    const long nfold = (want_dz ? MD : 0) + D;
    hipLaunchKernelGGL(kvjp_fold_generic_kernel, dim3((unsigned)((nfold + 255) / 256 + 1)), dim3(256), 0, h->stream,
                       (const double*)part_z, nrb, MD, (const double*)part_l, nrb * ncb, ldl, D,
                       (const double*)part_v, ntx * nty, want_dz ? 1 : 0, accs, accz);
    MGP_LAUNCH_CHECK(h);
  }
  if (want_dz) {
    MGP_TRY(kvjp_upload(h, D, sc));
    hipLaunchKernelGGL(kvjp_dz_generic_kernel, dim3((unsigned)((MD + 255) / 256)), dim3(256), 0, h->stream,
                       (const double*)accz, MD, D, (const double*)h->dparams, dZ);
    MGP_LAUNCH_CHECK(h);
  }
  // the D + 1 running sums as one block of partials: *dvar = accs[D], dls[d] = variance (-2 / l_d) accs[d]
  return mgp_fold_vjp_partials(h, accs, 1, D + 1, k, dvar, dls);
}

}  // namespace

extern "C" int mgp_kmn_knm_vjp_anyd(mgp_handle* h, const mgp_kernel* k, const void* X, int64_t N, const void* Z,
                                    int64_t M, const void* Gq, const void* Y, const void* Gb, int32_t P,
                                    int64_t panel_rows, double* dvariance, double* dlengthscales, void* dZ) {
  int done = 0;
  MGP_TRY(mgp_kvjp_check(h, k, X, N, Z, M, Gq, Y, Gb, P, MGP_MAX_D, dvariance, dlengthscales, dZ, &done));
  if (panel_rows < 0) return mgp_fail(h, MGP_E_SHAPE, "kmn_knm_vjp_anyd: panel_rows >= 0 required");
  if (done) return MGP_OK;
  const double *Yd = P > 0 ? (const double*)Y : nullptr, *Gbd = P > 0 ? (const double*)Gb : nullptr;
  if (k->D <= MGP_FUSED_MAX_D)
    return mgp_kvjp_fused_d(h, k, (const double*)X, N, (const double*)Z, M, (const double*)Gq, Yd, Gbd, P,
                            (long)panel_rows, dvariance, dlengthscales, (double*)dZ);
  return kvjp_generic_run(h, k, (const double*)X, N, (const double*)Z, M, (const double*)Gq, Yd, Gbd, P,
                          (long)panel_rows, dvariance, dlengthscales, (double*)dZ);
}
