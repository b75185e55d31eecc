// rff.hip -- random Fourier features of a stationary kernel (the reference's cggp/rff.py:48-73): the feature panel
// Phi[n, :] = [cos(theta x_n) | sin(theta x_n)] and prior function samples out[s, n] = scale * Phi[n, :] . W[s, :].
//
// Phases are kept in revolutions: theta' = theta / (2 pi) is formed once per call (pack kernels below), the phase
// t = sum_d x_d theta'_d is an fma chain, and r = t - rint(t) is exact, so Matern-1/2 phases of 1e4-1e6 rad (the
// Cauchy spectral law) lose nothing beyond the rounding of t itself.  One sin/cos polynomial pair on [-pi/4, pi/4]
// after a quadrant split replaces libm sin/cos per feature (rff_math.h, shared with the VJP of rff_grad.hip).
//
// Two routes for the samples:
//  - fused (D <= 32, S <= 8): the sweep_fast_kernel pattern of sweep.hip -- every lane owns RPT rows of X with their
//    coordinates in registers, the basis records [theta'_l (DP) | W[0..S-1, l] | W[0..S-1, L+l]] are streamed
//    wave-uniformly, S accumulators per row, `scale` applied at the end.  When N leaves CUs idle the bases are split
//    over blockIdx.y into per-chunk partials that rff_reduce_kernel sums in chunk order (deterministic, no atomics).
//  - panel (S > 8 or D > 32): Phi written in row chunks of at most ~256 MB and multiplied against W by mgp_gemm_nt,
//    as generic.hip does for the kernel panels;
//  - MGP_RFF_ANYD in out_layout, fp64, D > 32, S <= 8: rff_anyd.hip, fused on the matrix cores.
#include <cstdlib>

#include "../../include/mgp_pathwise.h"
#include "mgp_common.h"
#include "rff_math.h"

namespace {

constexpr int kRffThreads = 256;
constexpr int kRffMaxS = 8;       // fused route: accumulators per row
constexpr long kPanelBytes = 256L << 20;

// theta'[l, d] = theta[l, d] / (2 pi), the division carried out in double
template <typename T>
__global__ __launch_bounds__(256) void rff_pack_theta_kernel(const T* __restrict__ theta, long count,
                                                             T* __restrict__ th) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e < count) th[e] = (T)((double)theta[e] / 6.283185307179586476925);
}

// record l = [theta'_l (DP, zero padded) | W[s, l] s < S | W[s, L + l] s < S]
template <typename T>
__global__ __launch_bounds__(256) void rff_pack_records_kernel(const T* __restrict__ theta, long L, int D, int DP,
                                                               const T* __restrict__ W, int S, T* __restrict__ rec) {
  const int REC = DP + 2 * S;
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= L * REC) return;
  const long l = e / REC;
  const int j = (int)(e - l * REC);
  T v;
  if (j < DP) {
    v = j < D ? (T)((double)theta[l * D + j] / 6.283185307179586476925) : (T)0;
  } else if (j < DP + S) {
    v = W[(long)(j - DP) * 2 * L + l];
  } else {
    v = W[(long)(j - DP - S) * 2 * L + L + l];
  }
  rec[e] = v;
}

// Fused prior sample.  Lane owns rows n_k = blockIdx.x * 256 RPT + k * 256 + threadIdx.x; bases
// [blockIdx.y * lchunk, min(L, (blockIdx.y + 1) * lchunk)).  part == nullptr: out(n, s) = scale * acc (layout strides);
// otherwise part[(blockIdx.y * S + s) * N + n] = acc.
template <typename T, int DP, int S, int RPT>
__global__ __launch_bounds__(kRffThreads) void rff_fused_kernel(const T* __restrict__ X, long N, int D,
                                                                const T* __restrict__ rec, long L, long lchunk,
                                                                T scale, T* __restrict__ out, long o_sn, long o_ss,
                                                                T* __restrict__ part) {
  constexpr int REC = DP + 2 * S;
  const long n0 = (long)blockIdx.x * kRffThreads * RPT + threadIdx.x;
  T x[RPT][DP];
  T acc[RPT][S];
#pragma unroll
  for (int k = 0; k < RPT; ++k) {
    const long n = n0 + (long)k * kRffThreads;
#pragma unroll
    for (int d = 0; d < DP; ++d) x[k][d] = (n < N && d < D) ? X[n * D + d] : (T)0;
#pragma unroll
    for (int s = 0; s < S; ++s) acc[k][s] = 0;
  }
  const long l0 = (long)blockIdx.y * lchunk;
  const long l1 = l0 + lchunk < L ? l0 + lchunk : L;
  for (long l = l0; l < l1; ++l) {
    const T* __restrict__ rp = rec + l * REC;  // wave-uniform address: scalar loads
    T th[DP], wc[S], ws[S];
#pragma unroll
    for (int d = 0; d < DP; ++d) th[d] = rp[d];
#pragma unroll
    for (int s = 0; s < S; ++s) {
      wc[s] = rp[DP + s];
      ws[s] = rp[DP + S + s];
    }
#pragma unroll
    for (int k = 0; k < RPT; ++k) {
      T t = x[k][0] * th[0];
#pragma unroll
      for (int d = 1; d < DP; ++d) t = mgp_fma(x[k][d], th[d], t);
      T sn, cs;
      rff_sincos_rev(t, sn, cs);
#pragma unroll
      for (int s = 0; s < S; ++s) acc[k][s] = mgp_fma(ws[s], sn, mgp_fma(wc[s], cs, acc[k][s]));
    }
  }
#pragma unroll
  for (int k = 0; k < RPT; ++k) {
    const long n = n0 + (long)k * kRffThreads;
    if (n >= N) continue;
#pragma unroll
    for (int s = 0; s < S; ++s) {
      if (part == nullptr)
        out[n * o_sn + s * o_ss] = scale * acc[k][s];
      else
        part[((long)blockIdx.y * S + s) * N + n] = acc[k][s];
    }
  }
}

// out(n, s) = scale * sum_c part[c, s, n], chunks in ascending order
template <typename T>
__global__ __launch_bounds__(256) void rff_reduce_kernel(const T* __restrict__ part, long N, int S, int nchunks,
                                                         T scale, T* __restrict__ out, long o_sn, long o_ss) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= N * S) return;
  const long s = e / N, n = e - s * N;
  T v = 0;
  for (int c = 0; c < nchunks; ++c) v += part[(long)c * N * S + e];
  out[n * o_sn + s * o_ss] = scale * v;
}

// Phi[n, l] = mul cos(2 pi theta'_l . x_n), Phi[n, L + l] = mul sin(...), rows of `out` ld apart.  Block = 4 rows
// (blockIdx.x) x 64 bases (blockIdx.y); theta' of the block's bases staged through LDS 16 dimensions at a time (any D <= MGP_MAX_D).
constexpr int FB = 64, FR = 4, FK = 16;
template <typename T>
__global__ __launch_bounds__(256) void rff_features_kernel(const T* __restrict__ X, long N, int D,
                                                           const T* __restrict__ th, long L, T mul,
                                                           T* __restrict__ out, long ld) {
  __shared__ T ts[FK][FB + 1];
  __shared__ T xs[FR][FK];
  const int tl = threadIdx.x & (FB - 1), tr = threadIdx.x / FB;
  const long l0 = (long)blockIdx.y * FB, nb = (long)blockIdx.x * FR;
  const long l = l0 + tl, n = nb + tr;
  T t = 0;
  for (int d0 = 0; d0 < D; d0 += FK) {
    __syncthreads();
    for (int e = threadIdx.x; e < FK * FB; e += 256) {
      const int b = e / FK, d = e % FK;
      ts[d][b] = (l0 + b < L && d0 + d < D) ? th[(l0 + b) * D + d0 + d] : (T)0;
    }
    if (threadIdx.x < FR * FK) {
      const int r = threadIdx.x / FK, d = threadIdx.x % FK;
      xs[r][d] = (nb + r < N && d0 + d < D) ? X[(nb + r) * D + d0 + d] : (T)0;
    }
    __syncthreads();
    const int dn = D - d0 < FK ? D - d0 : FK;
    for (int d = 0; d < dn; ++d) t = mgp_fma(xs[tr][d], ts[d][tl], t);
  }
  if (n >= N || l >= L) return;
  T sn, cs;
  rff_sincos_rev(t, sn, cs);
  out[n * ld + l] = mul * cs;
  out[n * ld + L + l] = mul * sn;
}

template <typename T>
int features_launch(mgp_handle* h, const T* X, long N, int D, const T* th, long L, T mul, T* out, long ld) {
  dim3 grid((unsigned)((N + FR - 1) / FR), (unsigned)((L + FB - 1) / FB));  // rows on x: N reaches 2^20+
  hipLaunchKernelGGL((rff_features_kernel<T>), grid, dim3(256), 0, h->stream, X, N, D, th, L, mul, out, ld);
  MGP_LAUNCH_CHECK(h);
  return MGP_OK;
}

template <typename T>
int pack_theta(mgp_handle* h, const T* theta, long L, int D, T* th) {
  const long cnt = L * D;
  hipLaunchKernelGGL((rff_pack_theta_kernel<T>), dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, h->stream, theta,
                     cnt, th);
  MGP_LAUNCH_CHECK(h);
  return MGP_OK;
}

template <typename T>
int features_t(mgp_handle* h, const T* X, long N, int D, const T* theta, long L, T* out, long ld) {
  MGP_TRY(mgp_reserve(h, &h->gen, &h->gen_bytes, (size_t)L * D * sizeof(T) + 256));
  T* th = (T*)h->gen;
  MGP_TRY(pack_theta<T>(h, theta, L, D, th));
  return features_launch<T>(h, X, N, D, th, L, (T)1, out, ld);
}

// panel route: out (S x N rows or N x S cols) in row chunks of Phi, each chunk one NT GEMM against W
template <typename T>
int sample_panel_t(mgp_handle* h, const T* X, long N, int D, const T* theta, long L, const T* W, int S, T scale,
                   T* out, int layout) {
  const long K = 2 * L;
  long rc = kPanelBytes / (K * (long)sizeof(T));
  if (rc > N) rc = N;
  if (rc < 64) rc = N < 64 ? N : 64;
  const size_t th_elems = ((size_t)L * D + 31) / 32 * 32;
  MGP_TRY(mgp_reserve(h, &h->gen, &h->gen_bytes, (th_elems + (size_t)rc * K) * sizeof(T) + 256));
  T* th = (T*)h->gen;
  T* panel = th + th_elems;
  MGP_TRY(pack_theta<T>(h, theta, L, D, th));
  for (long i0 = 0; i0 < N; i0 += rc) {
    const long c = N - i0 < rc ? N - i0 : rc;
    MGP_TRY(features_launch<T>(h, X + i0 * D, c, D, th, L, scale, panel, K));
    if (layout == MGP_ROWS)  // out[S, i0 : i0 + c] = W . panel^T
      MGP_TRY(mgp_gemm_nt(h, sizeof(T) == 8 ? MGP_F64 : MGP_F32, W, K, S, panel, K, c, K, out + i0, N, 0, nullptr));
    else  // out[i0 : i0 + c, S] = panel . W^T
      MGP_TRY(mgp_gemm_nt(h, sizeof(T) == 8 ? MGP_F64 : MGP_F32, panel, K, c, W, K, S, K, out + i0 * S, S, 0,
                          nullptr));
  }
  return MGP_OK;
}

template <typename T, int DP, int S, int RPT>
int fused_launch(mgp_handle* h, const T* X, long N, int D, const T* rec, long L, T scale, T* out, long o_sn,
                 long o_ss) {
  const long per_block = (long)kRffThreads * RPT;
  const long bx = (N + per_block - 1) / per_block;
  // split the bases while the row blocks alone leave CUs idle: aim at 4 workgroups per CU, >= 32 bases per chunk
  long nchunks = 1;
  const long want = 4L * h->num_cus;
  if (bx < want) {
    nchunks = (want + bx - 1) / bx;
    const long cap = (L + 31) / 32;
    if (nchunks > cap) nchunks = cap;
    if (nchunks > 256) nchunks = 256;
    if (nchunks < 1) nchunks = 1;
  }
  const long lchunk = (L + nchunks - 1) / nchunks;
  nchunks = (L + lchunk - 1) / lchunk;
  T* part = nullptr;
  if (nchunks > 1) {
    MGP_TRY(mgp_reserve(h, &h->ws, &h->ws_bytes, (size_t)nchunks * S * N * sizeof(T)));
    part = (T*)h->ws;
  }
  hipLaunchKernelGGL((rff_fused_kernel<T, DP, S, RPT>), dim3((unsigned)bx, (unsigned)nchunks), dim3(kRffThreads), 0,
                     h->stream, X, N, D, rec, L, lchunk, scale, out, o_sn, o_ss, part);
  MGP_LAUNCH_CHECK(h);
  if (part != nullptr) {
    const long tot = N * S;
    hipLaunchKernelGGL((rff_reduce_kernel<T>), dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, h->stream,
                       (const T*)part, N, S, (int)nchunks, scale, out, o_sn, o_ss);
    MGP_LAUNCH_CHECK(h);
  }
  return MGP_OK;
}

template <typename T, int DP>
int fused_dispatch_s(mgp_handle* h, const T* X, long N, int D, const T* rec, long L, int S, T scale, T* out,
                     long o_sn, long o_ss) {
  constexpr int RPT = DP <= 8 ? 4 : (DP <= 16 ? 2 : 1);
  switch (S) {
#define MGP_RFF_S(SV) \
  case SV: return fused_launch<T, DP, SV, RPT>(h, X, N, D, rec, L, scale, out, o_sn, o_ss)
    MGP_RFF_S(1); MGP_RFF_S(2); MGP_RFF_S(3); MGP_RFF_S(4);
    MGP_RFF_S(5); MGP_RFF_S(6); MGP_RFF_S(7); MGP_RFF_S(8);
#undef MGP_RFF_S
    default: return mgp_fail(h, MGP_E_BADARG, "rff fused route: S=%d", S);
  }
}

template <typename T>
int sample_fused_t(mgp_handle* h, const T* X, long N, int D, const T* theta, long L, const T* W, int S, T scale,
                   T* out, int layout) {
  return mgp_with_dp<4>(D, [&](auto dp) {
    constexpr int DP = decltype(dp)::value;
    const long rec_elems = L * (DP + 2L * S);
    MGP_TRY(mgp_reserve(h, &h->gen, &h->gen_bytes, (size_t)rec_elems * sizeof(T) + 256));
    T* rec = (T*)h->gen;
    hipLaunchKernelGGL((rff_pack_records_kernel<T>), dim3((unsigned)((rec_elems + 255) / 256)), dim3(256), 0,
                       h->stream, theta, L, D, DP, W, S, rec);
    MGP_LAUNCH_CHECK(h);
    const long o_sn = layout == MGP_COLS ? S : 1, o_ss = layout == MGP_COLS ? 1 : N;
    return fused_dispatch_s<T, DP>(h, X, N, D, rec, L, S, scale, out, o_sn, o_ss);
  });
}

// MGP_RFF_ROUTE=panel | fused (A/B runs; read per call so one process can alternate); default: fused where eligible
bool rff_use_fused(int D, int S) {
  if (D > MGP_FUSED_MAX_D || S > kRffMaxS) return false;
  const char* e = std::getenv("MGP_RFF_ROUTE");
  return !(e != nullptr && std::strcmp(e, "panel") == 0);
}

int rff_check(mgp_handle* h, int dtype, const void* X, int64_t N, int32_t D, const void* theta, int64_t L) {
  if (!h) return MGP_E_BADARG;
  if (dtype != MGP_F32 && dtype != MGP_F64) return mgp_fail(h, MGP_E_DTYPE, "bad dtype %d", dtype);
  if (N < 0 || L < 0) return mgp_fail(h, MGP_E_SHAPE, "rff: negative size N=%ld L=%ld", (long)N, (long)L);
  if (D < 1 || D > MGP_MAX_D) return mgp_fail(h, MGP_E_SHAPE, "rff: D=%d outside [1,%d]", D, MGP_MAX_D);
  if (N > 0 && L > 0 && (!X || !theta)) return mgp_fail(h, MGP_E_BADARG, "rff: NULL data pointer");
  return MGP_OK;
}

}  // namespace

extern "C" int mgp_rff_features(mgp_handle* h, int dtype, const void* X, int64_t N, int32_t D, const void* theta,
                                int64_t L, void* out, int64_t ld) {
  MGP_TRY(rff_check(h, dtype, X, N, D, theta, L));
  if (ld < 2 * L) return mgp_fail(h, MGP_E_SHAPE, "rff_features: ld=%ld < 2L=%ld", (long)ld, (long)(2 * L));
  if (N == 0 || L == 0) return MGP_OK;
  if (!out) return mgp_fail(h, MGP_E_BADARG, "rff_features: NULL out");
  return mgp_with_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    return features_t<T>(h, (const T*)X, N, D, (const T*)theta, L, (T*)out, ld);
  });
}

extern "C" int mgp_rff_sample(mgp_handle* h, int dtype, const void* X, int64_t N, int32_t D, const void* theta,
                              int64_t L, const void* W, int32_t S, double scale, void* out, int out_layout) {
  MGP_TRY(rff_check(h, dtype, X, N, D, theta, L));
  if (S < 1) return mgp_fail(h, MGP_E_SHAPE, "rff_sample: S=%d < 1", S);
  const bool anyd = (out_layout & MGP_RFF_ANYD) != 0;  // the flag only picks the route; the layout is checked without it
  out_layout &= ~MGP_RFF_ANYD;
  if (out_layout != MGP_COLS && out_layout != MGP_ROWS)
    return mgp_fail(h, MGP_E_BADARG, "rff_sample: bad out_layout %d", out_layout);
  if (!(scale == scale) || scale - scale != 0.0) return mgp_fail(h, MGP_E_BADARG, "rff_sample: scale not finite");
  if (N == 0) return MGP_OK;
  if (!out) return mgp_fail(h, MGP_E_BADARG, "rff_sample: NULL out");
  if (L == 0) {
    MGP_HIP(h, hipMemsetAsync(out, 0, (size_t)N * S * mgp_elem(dtype), h->stream));
    return MGP_OK;
  }
  if (!W) return mgp_fail(h, MGP_E_BADARG, "rff_sample: NULL W");
  if (anyd && mgp_rff_anyd_serves(dtype, D, S))
    return mgp_rff_anyd_sample(h, (const double*)X, N, D, (const double*)theta, L, (const double*)W, S, scale,
                               (double*)out, out_layout);
  const bool fused = rff_use_fused(D, S);
  return mgp_with_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    auto f = fused ? sample_fused_t<T> : sample_panel_t<T>;
    return f(h, (const T*)X, N, D, (const T*)theta, L, (const T*)W, S, (T)scale, (T*)out, out_layout);
  });
}
