// rff_grad.hip -- backward pass of mgp_rff_sample (rff.hip): with phi_nl = theta_l . x_n and G(s, n) the cotangent of
// out(s, n) = scale * sum_l (W[s, l] cos phi_nl + W[s, L + l] sin phi_nl),
//     q(n, l)      = scale * sum_s G(s, n) (W[s, L + l] cos phi_nl - W[s, l] sin phi_nl)
//     dtheta[l, d] = sum_n q(n, l) x_n[d]
//     dX[n, d]     = sum_l q(n, l) theta_l[d]
// (include/mgp_pathwise.h has the contract and the error bound).
//
// One kernel template serves both outputs, the two point sets exchanging roles (the fused forward's pattern):
//  - dtheta: a lane owns RPT bases -- theta'_l = theta_l / (2 pi), W[:, l], W[:, L + l] and D accumulators in
//    registers -- and the row records [x_n (DP) | G(:, n)] are streamed wave-uniformly (scalar loads);
//  - dX: a lane owns RPT rows -- x_n, G(:, n) and D accumulators -- and the forward's basis records
//    [theta'_l (DP) | W[:, l] | W[:, L + l]] are streamed; the factor 2 pi of theta = 2 pi theta' joins `scale`.
// The phase t = sum_d x_d theta'_d is the forward's fma chain (products and fmas commute in their factors, so which
// side is owned does not change a bit of t) and rff_math.h turns it into the same sin / cos.
//
// Owners are few where it matters (1024 bases: four workgroups at D > 8), so the streamed side is split over
// blockIdx.y, aiming at 4 workgroups per CU as rff.hip's fused_launch does; each chunk writes a partial and
// rff_vjp_reduce_kernel adds the partials in chunk order.  No atomics: two calls are bit-identical.
#include "../../include/mgp_pathwise.h"
#include "mgp_common.h"
#include "rff_math.h"

namespace {

constexpr int kVjpThreads = 256;
constexpr int kVjpMaxS = 8;
constexpr double kTwoPi = 6.283185307179586476925;

// streamed records.  ROWOWN (dX): record l = [theta'_l (DP, zero padded) | W[s, l] s < S | W[s, L + l] s < S], as
// rff.hip's rff_pack_records_kernel; otherwise (dtheta): record n = [x_n (DP, zero padded) | G(s, n) s < S].
template <bool ROWOWN>
__global__ __launch_bounds__(256) void rff_vjp_pack_kernel(const double* __restrict__ P, long cnt, int D, int DP,
                                                           const double* __restrict__ A, int S, long a_si, long a_ss,
                                                           double* __restrict__ rec) {
  const int REC = DP + (ROWOWN ? 2 * S : S);
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= cnt * REC) return;
  const long i = e / REC;
  const int j = (int)(e - i * REC);
  double v;
  if (j < DP) {
    v = j < D ? (ROWOWN ? P[i * D + j] / kTwoPi : P[i * D + j]) : 0.0;
  } else if (ROWOWN) {
    v = j < DP + S ? A[(long)(j - DP) * 2 * cnt + i] : A[(long)(j - DP - S) * 2 * cnt + cnt + i];
  } else {
    v = A[i * a_si + (long)(j - DP) * a_ss];
  }
  rec[e] = v;
}

// Lane owns points o_k = blockIdx.x * 256 RPT + k * 256 + threadIdx.x of the owned set (NO points); streamed records
// [blockIdx.y * chunk, min(NS, (blockIdx.y + 1) * chunk)).  part == nullptr: out[o, d] = mul * acc; otherwise
// part[(blockIdx.y * NO + o) * D + d] = acc.  ROWOWN: P = X, A = G (element (n, s) at A[n a_si + s a_ss]);
// otherwise P = theta, A = W [S, 2 NO].
template <int DP, int S, int RPT, bool ROWOWN>
__global__ __launch_bounds__(kVjpThreads) void rff_vjp_kernel(const double* __restrict__ P, long NO, int D,
                                                              const double* __restrict__ A, long a_si, long a_ss,
                                                              const double* __restrict__ rec, long NS, long chunk,
                                                              double mul, double* __restrict__ out,
                                                              double* __restrict__ part) {
  constexpr int WS = ROWOWN ? 2 * S : S;  // streamed weights per record
  constexpr int REC = DP + WS;
  const long o0 = (long)blockIdx.x * kVjpThreads * RPT + threadIdx.x;
  double p[RPT][DP], acc[RPT][DP];
  double oc[RPT][S], os[RPT][S];  // ROWOWN: oc = G(:, n), os unused; otherwise W[:, l], W[:, L + l]
#pragma unroll
  for (int k = 0; k < RPT; ++k) {
    const long o = o0 + (long)k * kVjpThreads;
    const bool live = o < NO;
#pragma unroll
    for (int d = 0; d < DP; ++d) {
      const double v = (live && d < D) ? P[o * D + d] : 0.0;
      p[k][d] = ROWOWN ? v : v / kTwoPi;
      acc[k][d] = 0.0;
    }
#pragma unroll
    for (int s = 0; s < S; ++s) {
      if (ROWOWN) {
        oc[k][s] = live ? A[o * a_si + s * a_ss] : 0.0;
        os[k][s] = 0.0;
      } else {
        oc[k][s] = live ? A[(long)s * 2 * NO + o] : 0.0;
        os[k][s] = live ? A[(long)s * 2 * NO + NO + o] : 0.0;
      }
    }
  }
  const long i0 = (long)blockIdx.y * chunk;
  const long i1 = i0 + chunk < NS ? i0 + chunk : NS;
  for (long i = i0; i < i1; ++i) {
    const double* __restrict__ rp = rec + i * REC;  // wave-uniform address: scalar loads
    double r[DP], w[WS];
#pragma unroll
    for (int d = 0; d < DP; ++d) r[d] = rp[d];
#pragma unroll
    for (int s = 0; s < WS; ++s) w[s] = rp[DP + s];
#pragma unroll
    for (int k = 0; k < RPT; ++k) {
      // the forward's chain x_0 theta'_0, then fma(x_d, theta'_d, t): the same bits whichever side is owned
      double t = p[k][0] * r[0];
#pragma unroll
      for (int d = 1; d < DP; ++d) t = mgp_fma(p[k][d], r[d], t);
      double sn, cs;
      rff_sincos_rev(t, sn, cs);
      // a = sum_s G_s W[s, L + l], b = sum_s G_s W[s, l]
      double a, b;
      if (ROWOWN) {
        a = oc[k][0] * w[S];
        b = oc[k][0] * w[0];
#pragma unroll
        for (int s = 1; s < S; ++s) {
          a = mgp_fma(oc[k][s], w[S + s], a);
          b = mgp_fma(oc[k][s], w[s], b);
        }
      } else {
        a = w[0] * os[k][0];
        b = w[0] * oc[k][0];
#pragma unroll
        for (int s = 1; s < S; ++s) {
          a = mgp_fma(w[s], os[k][s], a);
          b = mgp_fma(w[s], oc[k][s], b);
        }
      }
      const double q = mgp_fma(a, cs, -(b * sn));
#pragma unroll
      for (int d = 0; d < DP; ++d) acc[k][d] = mgp_fma(q, r[d], acc[k][d]);
    }
  }
#pragma unroll
  for (int k = 0; k < RPT; ++k) {
    const long o = o0 + (long)k * kVjpThreads;
    if (o >= NO) continue;
#pragma unroll
    for (int d = 0; d < DP; ++d) {
      if (d >= D) continue;
      if (part == nullptr)
        out[o * D + d] = mul * acc[k][d];
      else
        part[((long)blockIdx.y * NO + o) * D + d] = acc[k][d];
    }
  }
}

// out[e] = mul * sum_c part[c, e], chunks in ascending order
__global__ __launch_bounds__(256) void rff_vjp_reduce_kernel(const double* __restrict__ part, long count, int nchunks,
                                                             double mul, double* __restrict__ out) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= count) return;
  double v = 0.0;
  for (int c = 0; c < nchunks; ++c) v += part[(long)c * count + e];
  out[e] = mul * v;
}

// one output: P / A the owned side's data, Q / B the streamed side's (packed into h->gen)
template <int DP, int S, bool ROWOWN>
int vjp_pass(mgp_handle* h, const double* P, long NO, int D, const double* A, long a_si, long a_ss, const double* Q,
             long NS, const double* B, long b_si, long b_ss, double mul, double* out) {
  constexpr int RPT = DP <= 8 ? 2 : 1;
  constexpr int REC = DP + (ROWOWN ? 2 * S : S);
  const long rec_elems = NS * REC;
  MGP_TRY(mgp_reserve(h, &h->gen, &h->gen_bytes, (size_t)rec_elems * sizeof(double) + 256));
  double* rec = (double*)h->gen;
  hipLaunchKernelGGL((rff_vjp_pack_kernel<ROWOWN>), dim3((unsigned)((rec_elems + 255) / 256)), dim3(256), 0, h->stream,
                     Q, NS, D, DP, B, S, b_si, b_ss, rec);
  MGP_LAUNCH_CHECK(h);
  const long per_block = (long)kVjpThreads * RPT;
  const long bx = (NO + per_block - 1) / per_block;
  // split the streamed side while the owner blocks alone leave CUs idle: 4 workgroups per CU, >= 32 records per chunk
  long nchunks = 1;
  const long want = 4L * h->num_cus;
  if (bx < want) {
    nchunks = (want + bx - 1) / bx;
    const long cap = (NS + 31) / 32;
    if (nchunks > cap) nchunks = cap;
    if (nchunks > 256) nchunks = 256;
    if (nchunks < 1) nchunks = 1;
  }
  const long chunk = (NS + nchunks - 1) / nchunks;
  nchunks = (NS + chunk - 1) / chunk;
  double* part = nullptr;
  if (nchunks > 1) {
    MGP_TRY(mgp_reserve(h, &h->ws, &h->ws_bytes, (size_t)nchunks * NO * D * sizeof(double)));
    part = (double*)h->ws;
  }
  hipLaunchKernelGGL((rff_vjp_kernel<DP, S, RPT, ROWOWN>), dim3((unsigned)bx, (unsigned)nchunks), dim3(kVjpThreads), 0,
                     h->stream, P, NO, D, A, a_si, a_ss, (const double*)rec, NS, chunk, mul, out, part);
  MGP_LAUNCH_CHECK(h);
  if (part != nullptr) {
    const long tot = NO * D;
    hipLaunchKernelGGL(rff_vjp_reduce_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, h->stream,
                       (const double*)part, tot, (int)nchunks, mul, out);
    MGP_LAUNCH_CHECK(h);
  }
  return MGP_OK;
}

template <int DP, int S>
int vjp_both(mgp_handle* h, const double* X, long N, int D, const double* theta, long L, const double* W, double scale,
             const double* G, long g_sn, long g_ss, double* dtheta, double* dX) {
  if (dtheta) MGP_TRY((vjp_pass<DP, S, false>(h, theta, L, D, W, 0, 0, X, N, G, g_sn, g_ss, scale, dtheta)));
  if (dX) MGP_TRY((vjp_pass<DP, S, true>(h, X, N, D, G, g_sn, g_ss, theta, L, W, 0, 0, scale * kTwoPi, dX)));
  return MGP_OK;
}

template <int DP>
int vjp_dispatch_s(mgp_handle* h, const double* X, long N, int D, const double* theta, long L, const double* W, int S,
                   double scale, const double* G, long g_sn, long g_ss, double* dtheta, double* dX) {
  switch (S) {
#define MGP_RFF_VJP_S(SV) \
  case SV: return vjp_both<DP, SV>(h, X, N, D, theta, L, W, scale, G, g_sn, g_ss, dtheta, dX)
    MGP_RFF_VJP_S(1); MGP_RFF_VJP_S(2); MGP_RFF_VJP_S(3); MGP_RFF_VJP_S(4);
    MGP_RFF_VJP_S(5); MGP_RFF_VJP_S(6); MGP_RFF_VJP_S(7); MGP_RFF_VJP_S(8);
#undef MGP_RFF_VJP_S
    default: return mgp_fail(h, MGP_E_BADARG, "rff_sample_vjp: S=%d", S);
  }
}

}  // namespace

extern "C" int mgp_rff_sample_vjp(mgp_handle* h, int dtype, const void* X, int64_t N, int32_t D, const void* theta,
                                  int64_t L, const void* W, int32_t S, double scale, const void* G, int g_layout,
                                  void* dtheta, void* dX) {
  if (!h) return MGP_E_BADARG;
  if (dtype != MGP_F64) return mgp_fail(h, MGP_E_DTYPE, "rff_sample_vjp: fp64 only, got dtype %d", dtype);
  if (N < 0 || L < 0) return mgp_fail(h, MGP_E_SHAPE, "rff_sample_vjp: negative size N=%ld L=%ld", (long)N, (long)L);
  const bool anyd = (g_layout & MGP_RFF_ANYD) != 0;  // the flag only picks the route; the layout is checked without it
  g_layout &= ~MGP_RFF_ANYD;
  const int max_d = anyd ? MGP_MAX_D : MGP_FUSED_MAX_D;  // above MGP_FUSED_MAX_D: rff_anyd.hip
  if (D < 1 || D > max_d) return mgp_fail(h, MGP_E_BADARG, "rff_sample_vjp: D = %d outside [1, %d]", D, max_d);
  if (S < 1 || S > kVjpMaxS) return mgp_fail(h, MGP_E_BADARG, "rff_sample_vjp: S = %d outside [1, %d]", S, kVjpMaxS);
  if (g_layout != MGP_COLS && g_layout != MGP_ROWS)
    return mgp_fail(h, MGP_E_BADARG, "rff_sample_vjp: bad g_layout %d", g_layout);
  if (!(scale == scale) || scale - scale != 0.0) return mgp_fail(h, MGP_E_BADARG, "rff_sample_vjp: scale not finite");
  if (!dtheta && !dX) return mgp_fail(h, MGP_E_BADARG, "rff_sample_vjp: dtheta and dX are both NULL");
  if (N == 0 || L == 0) {  // an empty sum on one side, no element on the other
    if (dtheta && L > 0) MGP_HIP(h, hipMemsetAsync(dtheta, 0, (size_t)L * D * sizeof(double), h->stream));
    if (dX && N > 0) MGP_HIP(h, hipMemsetAsync(dX, 0, (size_t)N * D * sizeof(double), h->stream));
    return MGP_OK;
  }
  if (!X || !theta || !W || !G) return mgp_fail(h, MGP_E_BADARG, "rff_sample_vjp: NULL data pointer");
  const long g_sn = g_layout == MGP_COLS ? S : 1, g_ss = g_layout == MGP_COLS ? 1 : N;
  if (D > MGP_FUSED_MAX_D)
    return mgp_rff_anyd_vjp(h, (const double*)X, N, D, (const double*)theta, L, (const double*)W, S, scale,
                            (const double*)G, g_sn, g_ss, (double*)dtheta, (double*)dX);
  return mgp_with_dp<4>(D, [&](auto dp) {
    return vjp_dispatch_s<decltype(dp)::value>(h, (const double*)X, N, D, (const double*)theta, L, (const double*)W, S,
                                               scale, (const double*)G, g_sn, g_ss, (double*)dtheta, (double*)dX);
  });
}
