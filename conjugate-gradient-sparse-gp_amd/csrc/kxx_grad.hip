// kxx_grad.hip -- hyper-parameter bilinear forms of the self-kernel: sum_r u_r^T (dK/dtheta) v_r, K = k(X, X).
//
// The gradient of the exact-GP marginal likelihood needs  1/2 a^T dK a - 1/2 tr(Khat^-1 dK)  (the trace by probes),
// i.e. bilinear forms over all N^2 pairs; mgp_k_dense_vjp would need the [N, N] matrix G = U V^T.  Here nothing N x N
// exists: with c_ij = sum_r (u_ri v_rj + u_rj v_ri) each unordered pair {i, j} is evaluated once and
//     dvariance   += c_ij f(r2_ij)
//     dl_d (pre)  += c_ij f'(r2_ij) (x_id - x_jd)^2 / l_d^2     (the host applies variance * -2 / l_d)
// with f = k / variance of the scaled squared distance r2 and f' as grad.hip forms it (Matern-1/2: 0 at GPflow's
// 1e-36 floor, so duplicate rows add nothing to the lengthscales and never a NaN).  Direct differences, as grad.hip:
// a gradient amplifies the expansion form's cancellation.
//
// Tiling follows kxx.hip: rows are cut into blocks of TB = 256 points and every unordered block pair {I, J} is one tile
// (I, (I + d) mod nb) for d = 0 .. nb/2.  A lane owns one row of block I in registers (scaled x, its RC columns of u
// and v); the TB points of block J are streamed by wave-uniform (scalar) loads.  On the diagonal tile every ordered
// pair is visited, so the owned u, v are halved there (exact) and the diagonal pair counts u_i . v_i once.  A fixed
// grid of workgroups walks the tiles in a fixed stride; lanes accumulate D+1 doubles in registers, each workgroup
// writes D+1 partials and the host adds them in workgroup order: no atomics, two calls are bit-identical.
//
// Per evaluated pair: D sub + D fma (r2) + D mul + D fma (accumulate) + 2 RC fma (c) + the polynomial exp2 of
// mgp_math.h (13 fp64 + cvt + ldexp) + 3 (f, f', the variance term): 4D + 2RC + ~18.  Columns beyond RC = 16 (8 at
// D > 16 and for Matern-1/2) are further passes over the pairs; mgp.h states the scratch bound.
#include <vector>

#include "mgp_common.h"

namespace {

constexpr int kKgThreads = 256;
constexpr int kKgTB = kKgThreads;  // points per block: one owned row per lane
constexpr int kKgWgPerCu = 8;      // grid = 8 workgroups per CU (the tile walk's stride)

// P[j, 0:DP] = x_j / l (zeros for d >= D and for the pad rows j >= N)
template <typename T, int DP>
__global__ __launch_bounds__(256) void kgrad_pack_x_kernel(const T* __restrict__ X, long N, long npad, int D,
                                                           SweepParams prm, double* __restrict__ P) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= npad * DP) return;
  const long j = e / DP;
  const int d = (int)(e - j * DP);
  P[e] = (j < N && d < D) ? (double)X[j * D + d] * prm.inv_ls[d] : 0.0;
}

// UV[j, 0:RC] = U(j, r0 + c), UV[j, RC:2RC] = V(j, r0 + c); zeros for the pad rows
template <typename T>
__global__ __launch_bounds__(256) void kgrad_pack_uv_kernel(const T* __restrict__ U, long u_si, long u_sr,
                                                            const T* __restrict__ V, long v_si, long v_sr, long N,
                                                            long npad, int r0, int RC, double* __restrict__ UV) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= npad * 2 * RC) return;
  const long j = e / (2 * RC);
  const int c = (int)(e - j * 2 * RC);
  double w = 0.0;
  if (j < N) w = c < RC ? (double)U[j * u_si + (long)(r0 + c) * u_sr] : (double)V[j * v_si + (long)(r0 + c - RC) * v_sr];
  UV[e] = w;
}

template <int DP, int KIND, int RC>
__global__ __launch_bounds__(kKgThreads) void kxx_grad_kernel(const double* __restrict__ P,
                                                              const double* __restrict__ UV, long nbk, long ntiles,
                                                              double* __restrict__ part) {
  __shared__ double red[kKgThreads / 64][DP + 1];
  const int t = threadIdx.x;
  double acc[DP + 1];
#pragma unroll
  for (int d = 0; d <= DP; ++d) acc[d] = 0.0;
  for (long tau = blockIdx.x; tau < ntiles; tau += gridDim.x) {
    const long I = tau % nbk, dist = tau / nbk;
    if (dist > 0 && 2 * dist == nbk && I >= nbk / 2) continue;  // that block pair is the tile of I - nbk/2
    const long J = (I + dist) % nbk;
    const double hw = dist == 0 ? 0.5 : 1.0;  // diagonal tile: every ordered pair is visited
    const long i = I * kKgTB + t;
    double a[DP], ui[RC], vi[RC];
#pragma unroll
    for (int d = 0; d < DP; ++d) a[d] = P[i * DP + d];
#pragma unroll
    for (int c = 0; c < RC; ++c) {
      ui[c] = hw * UV[i * 2 * RC + c];
      vi[c] = hw * UV[i * 2 * RC + RC + c];
    }
    const double* rp = P + J * kKgTB * DP;        // wave-uniform: scalar loads
    const double* wp = UV + J * kKgTB * 2 * RC;
    for (int jl = 0; jl < kKgTB; ++jl) {
      double d2[DP], r2 = 0.0;
#pragma unroll
      for (int d = 0; d < DP; ++d) {
        const double df = a[d] - rp[d];
        d2[d] = df * df;
        r2 = mgp_fma(df, df, r2);
      }
      // c in groups of 4 columns, the scalar loads of a group issued behind the previous one's use: all 2 RC streamed
      // column values at once would not fit the SGPR file at RC = 16
      double c = 0.0;
#pragma unroll
      for (int q0 = 0; q0 < RC; q0 += 4) {
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int q = q0; q < q0 + 4 && q < RC; ++q) c = mgp_fma(ui[q], wp[RC + q], c);
#pragma unroll
        for (int q = q0; q < q0 + 4 && q < RC; ++q) c = mgp_fma(wp[q], vi[q], c);
      }
      __builtin_amdgcn_sched_barrier(0);
      double f, fp;
      mgp_profile_slope<KIND>(r2, f, fp);
      acc[DP] = mgp_fma(c, f, acc[DP]);
      const double g = c * fp;
#pragma unroll
      for (int d = 0; d < DP; ++d) acc[d] = mgp_fma(g, d2[d], acc[d]);
      rp += DP;
      wp += 2 * RC;
    }
  }
  // workgroup sum of the DP+1 accumulators: wave butterflies, then the four waves in order
  const int lane = t & 63, wave = t >> 6;
#pragma unroll
  for (int d = 0; d <= DP; ++d) {
    const double v = mgp_wave_sum(acc[d]);
    if (lane == 0) red[wave][d] = v;
  }
  __syncthreads();
  if (t <= DP) part[(long)blockIdx.x * (DP + 1) + t] = (red[0][t] + red[1][t]) + (red[2][t] + red[3][t]);
}

// widest column pass the register budget allows (kernel-resource-usage: no spills; Matern-1/2's division spilled SGPRs
// at 16 columns)
constexpr int kgrad_rc_max(int DP, int KIND) { return DP <= 16 && KIND != 1 ? 16 : 8; }

template <int DP, int KIND, int RC>
int kgrad_pass(mgp_handle* h, const double* P, const double* UV, long nbk, long ntiles, long grid, double* part) {
  hipLaunchKernelGGL((kxx_grad_kernel<DP, KIND, RC>), dim3((unsigned)grid), dim3(kKgThreads), 0, h->stream, P, UV,
                     nbk, ntiles, part);
  MGP_LAUNCH_CHECK(h);
  return MGP_OK;
}

template <typename T, int DP, int KIND>
int kgrad_fused(mgp_handle* h, const mgp_kernel* k, const T* X, long N, VecView U, VecView V, int R, double* dvar,
                double* dls) {
  SweepParams prm = mgp_make_params(k);
  for (int d = 0; d < MGP_FUSED_MAX_D; ++d) prm.inv_ls[d] = d < k->D ? 1.0 / k->lengthscales[d] : 0.0;
  const long nbk = (N + kKgTB - 1) / kKgTB, npad = nbk * kKgTB;
  const long ntiles = nbk * (nbk / 2 + 1);
  long grid = (long)h->num_cus * kKgWgPerCu;
  grid = grid < ntiles ? grid : ntiles;
  constexpr int RCM = kgrad_rc_max(DP, KIND);
  // arena: P [npad DP] | UV [npad 2 RCM] | partials [grid (DP+1)]
  const size_t need = (size_t)npad * DP * 8 + (size_t)npad * 2 * RCM * 8 + (size_t)grid * (DP + 1) * 8;
  MGP_TRY(mgp_reserve(h, &h->kgrad, &h->kgrad_bytes, need));
  double* P = (double*)h->kgrad;
  double* UV = P + npad * DP;
  double* part = UV + npad * 2 * RCM;
  hipLaunchKernelGGL((kgrad_pack_x_kernel<T, DP>), dim3((unsigned)((npad * DP + 255) / 256)), dim3(256), 0, h->stream,
                     X, N, npad, k->D, prm, P);
  MGP_LAUNCH_CHECK(h);
  double tot[DP + 1] = {0.0};  // running sums over the groups' blocks
  int r0 = 0;
  while (r0 < R) {
    const int left = R - r0;
    const int rc = left >= RCM ? RCM : (left >= 8 ? 8 : (left >= 4 ? 4 : (left >= 2 ? 2 : 1)));
    hipLaunchKernelGGL((kgrad_pack_uv_kernel<T>), dim3((unsigned)((npad * 2 * rc + 255) / 256)), dim3(256), 0,
                       h->stream, (const T*)U.base, U.si, U.sr, (const T*)V.base, V.si, V.sr, N, npad, r0, rc, UV);
    MGP_LAUNCH_CHECK(h);
    switch (rc) {
      case 16: MGP_TRY((kgrad_pass<DP, KIND, kgrad_rc_max(DP, KIND)>(h, P, UV, nbk, ntiles, grid, part))); break;
      case 8: MGP_TRY((kgrad_pass<DP, KIND, 8>(h, P, UV, nbk, ntiles, grid, part))); break;
      case 4: MGP_TRY((kgrad_pass<DP, KIND, 4>(h, P, UV, nbk, ntiles, grid, part))); break;
      case 2: MGP_TRY((kgrad_pass<DP, KIND, 2>(h, P, UV, nbk, ntiles, grid, part))); break;
      default: MGP_TRY((kgrad_pass<DP, KIND, 1>(h, P, UV, nbk, ntiles, grid, part))); break;
    }
    MGP_TRY(mgp_fold_vjp_partials(h, part, grid, DP + 1, k, dvar, dls, tot));
    r0 += rc;
  }
  return MGP_OK;
}

// G[ii, j] = sum_r U(i0 + ii, r) V(j, r) for a panel of rows
template <typename T>
__global__ __launch_bounds__(256) void kgrad_outer_kernel(const T* __restrict__ U, long u_si, long u_sr,
                                                          const T* __restrict__ V, long v_si, long v_sr, long i0,
                                                          long rows, long N, int R, T* __restrict__ G) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= rows * N) return;
  const long ii = e / N, j = e - ii * N;
  T s = 0;
  for (int r = 0; r < R; ++r) s = mgp_fma(U[(i0 + ii) * u_si + (long)r * u_sr], V[j * v_si + (long)r * v_sr], s);
  G[e] = s;
}

// Panel route (fp32, D > 32, MGP_KXX_GRAD=panel): row panels of at most ~256 MB of G = U[rows] V^T through
// mgp_k_dense_vjp(X[rows], X, G); the panels' results are added on the host in panel order.
template <typename T>
int kgrad_panel(mgp_handle* h, const mgp_kernel* k, const T* X, long N, VecView U, VecView V, int R, double* dvar,
                double* dls) {
  const long budget = (long)(((size_t)256 << 20) / sizeof(T));
  long rows = budget / N;
  rows = rows < 1 ? 1 : (rows > N ? N : rows);
  MGP_TRY(mgp_reserve(h, &h->kgrad, &h->kgrad_bytes, (size_t)rows * N * sizeof(T)));
  T* G = (T*)h->kgrad;
  const int D = k->D;
  std::vector<double> pl(D);
  for (long i0 = 0; i0 < N; i0 += rows) {
    const long nr = N - i0 < rows ? N - i0 : rows;
    hipLaunchKernelGGL((kgrad_outer_kernel<T>), dim3((unsigned)((nr * N + 255) / 256)), dim3(256), 0, h->stream,
                       (const T*)U.base, U.si, U.sr, (const T*)V.base, V.si, V.sr, i0, nr, N, R, G);
    MGP_LAUNCH_CHECK(h);
    double pv = 0.0;
    MGP_TRY(mgp_k_dense_vjp(h, k, X + i0 * D, nr, X, N, G, N, &pv, pl.data()));  // synchronises
    *dvar += pv;
    for (int d = 0; d < D; ++d) dls[d] += pl[d];
  }
  return MGP_OK;
}

}  // namespace

// Dispatch: the fused pair kernel for fp64 and D <= MGP_FUSED_MAX_D (MGP_KXX_GRAD=panel forces the panel route there
// too, the in-library A/B); fp32 and D > 32 take the panel route.
extern "C" int mgp_kxx_grad(mgp_handle* h, const mgp_kernel* k, const void* X, int64_t N, const void* U, const void* V,
                            int32_t R, int layout, double* dvariance, double* dlengthscales) {
  MGP_TRY(mgp_check_kernel(h, k));
  if (!dvariance || !dlengthscales) return mgp_fail(h, MGP_E_BADARG, "NULL output");
  *dvariance = 0.0;
  for (int d = 0; d < k->D; ++d) dlengthscales[d] = 0.0;
  if (N < 0) return mgp_fail(h, MGP_E_SHAPE, "kxx_grad: N < 0");
  if (R < 1) return mgp_fail(h, MGP_E_BADARG, "kxx_grad: R < 1");
  if (layout != MGP_COLS && layout != MGP_ROWS) return mgp_fail(h, MGP_E_BADARG, "bad layout");
  if (N == 0) return MGP_OK;
  if (!X || !U || !V) return mgp_fail(h, MGP_E_BADARG, "NULL data pointer");
  const VecView Uv = mgp_view(U, N, R, layout), Vv = mgp_view(V, N, R, layout);
  if (k->dtype == MGP_F64 && k->D <= MGP_FUSED_MAX_D && h->kxx_grad_mode != 2) {
    if ((N + kKgTB - 1) / kKgTB > 2147483647L / 2) return mgp_fail(h, MGP_E_SHAPE, "kxx_grad: N too large");
    const double* Xd = (const double*)X;
    return mgp_with_kind(k->kind, [&](auto kind) {
      return mgp_with_dp<4>(k->D, [&](auto dp) {
        return kgrad_fused<double, decltype(dp)::value, decltype(kind)::value>(h, k, Xd, N, Uv, Vv, R, dvariance,
                                                                               dlengthscales);
      });
    });
  }
  return mgp_with_dtype(k->dtype, [&](auto t) {
    using T = decltype(t);
    return kgrad_panel<T>(h, k, (const T*)X, N, Uv, Vv, R, dvariance, dlengthscales);
  });
}
