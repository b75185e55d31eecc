// quadform.hip -- q[b] = k(xs_b, Z) C k(Z, xs_b) for one symmetric C [M, M] (include/mgp_predict.h): the predictive
// variance of the sparse models over a whole test set, var = k** - q, with C = (K_mm + Lambda)^-1 (CDGP) or
// K_mm^-1 - s2 S^-1 (SGPR).  The upper triangle of C defines the form, q = sum_i C_ii k_i^2 + 2 sum_{i<j} C_ij k_i k_j;
// nothing below the diagonal and nothing past column M of a row is read.
//
// k(Xs, Z) [B, M] is never materialised.  The tiling is project.hip's (MT = 4, NQ = 4): a workgroup of four waves
// (2 x 2) owns QT = 128 test rows and one block J of QC = 128 columns of C, walks i = 0 ... end of block J in steps
// of 16, evaluates the 16 x 128 kernel panel into LDS on the VALU and contracts it with the 16 x 128 panel of C,
// staged masked to i < j, by v_mfma_f64_16x16x4_f64.  A column tile of 16 inside block J is final as soon as the walk
// has passed it (later rows have i > j), and at that step the kernel panel in LDS holds exactly k_bj for its columns:
// the wave that owns the tile forms (acc + acc + C_jj k_bj) k_bj there and adds it to 16 row sums per lane.  After the
// walk the row sums are reduced over the 16 lanes of a row and the two column waves, in a fixed order.
// Block J costs J + 1 block walks, so a workgroup takes block nJ-1-J and then block J: nJ + 1 walks each.  The per-block
// row sums part[nJ][B'] go to the arena; a second kernel adds them in block order and scales by variance^2.  No float
// atomics: two calls are bit-identical.
// The grid is (row tiles, block pairs) with the row tiles fastest, so the workgroups resident together walk the same
// column blocks and share the stream of C in L2 and the Infinity Cache.
//
// fp32 or D > MGP_FUSED_MAX_D: the symmetric matrix from the upper triangle of C, row panels of k(Xs_chunk, Z) by
// mgp_k_dense, the NT GEMM of dense.hip and a row-dot kernel.
#include "mgp_common.h"

#include "../../include/mgp_predict.h"

namespace {

using Acc4 = __attribute__((ext_vector_type(4))) double;

constexpr int QK = 16;        // rows of Z (and of C) per step
constexpr int QKS = QK + 2;   // LDS row stride of the kernel panel
constexpr int QT = 128;       // test rows per workgroup
constexpr int QC = 128;       // columns of C per block
constexpr long QF_CHUNK_B = 1L << 16;  // test rows per launch (bounds the partial arena)

// Zp[i] = (2 z_i / l, -|z_i / l|^2): the streamed side of the expansion-form distance (project.hip's pack)
template <int DP>
__global__ __launch_bounds__(256) void qf_pack_kernel(const double* __restrict__ Z, long M, int D, SweepParams prm,
                                                      double* __restrict__ Zp) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= M) return;
  double s = 0;
#pragma unroll
  for (int d = 0; d < DP; ++d) {
    const double v = d < D ? Z[i * D + d] * prm.inv_ls[d] : 0.0;
    s = mgp_fma(v, v, s);
    Zp[i * (DP + 1) + d] = v + v;
  }
  Zp[i * (DP + 1) + DP] = -s;
}

template <int DP, int KIND>
__global__ __launch_bounds__(256) void knm_quadform_kernel(const double* __restrict__ Xs, long B,
                                                           const double* __restrict__ Zp, long M,
                                                           const double* __restrict__ C, long ldc,
                                                           double* __restrict__ part, long Bpad, int nJ, int D,
                                                           SweepParams prm) {
  constexpr int MT = QT / 32, NQ = QC / 32;
  constexpr int KE = QK * QT / 256;  // kernel values per thread and step
  constexpr int RS = QC + 16;  // row stride of the C panel: the four k rows of an operand read fall in different banks
  constexpr int XE = QK * (DP + 1);     // elements of a staged Z panel
  constexpr int XL = (XE + 255) / 256;  // ... per thread
  constexpr int RL = QK * QC / 256;     // elements of a staged C panel per thread
  __shared__ __attribute__((aligned(16))) double Ka[QT * QKS];     // [b][k]; after a walk, the row sums of the two column waves
  __shared__ __attribute__((aligned(16))) double Cs[2][QK * RS];   // [k][j]
  __shared__ __attribute__((aligned(16))) double Xt[2][XE];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const long b0 = (long)blockIdx.x * QT;

  // this thread's test row (c) and its KE rows of every 16-row step (kg * KE ...; kg is wave-uniform)
  const int c = t % QT, kg = t / QT;
  double xs[DP];
  double xs2 = 0;
  {
    const long jb = b0 + c < B ? b0 + c : B - 1;
#pragma unroll
    for (int d = 0; d < DP; ++d) {
      const double v = d < D ? Xs[jb * D + d] * prm.inv_ls[d] : 0.0;
      xs[d] = v;
      xs2 = mgp_fma(v, v, xs2);
    }
  }
  const double clamp = prm.clamp;

  for (int pass = 0; pass < 2; ++pass) {
    // the heavier block of the pair first; the middle block of an odd nJ has no partner
    const int J = pass == 0 ? nJ - 1 - (int)blockIdx.y : (int)blockIdx.y;
    if (pass == 1 && J == nJ - 1 - (int)blockIdx.y) break;  // uniform
    const long j0 = (long)J * QC;
    const long i_end = j0 + QC < M ? j0 + QC : M;

    Acc4 acc[MT][NQ];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int q = 0; q < NQ; ++q) acc[m][q] = Acc4{0, 0, 0, 0};
    double rp[MT][4];  // row sums of this lane's 16 rows over the finished column tiles
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int g = 0; g < 4; ++g) rp[m][g] = 0;

    double xg[XL], rg[RL];
    // rows past the end are fetched as zeros; of C only i < j < M is read, the rest of the panel is zero
    auto fetch = [&](long i0) {
#pragma unroll
      for (int u = 0; u < XL; ++u) {
        const int e = t + 256 * u;
        const long g = i0 * (DP + 1) + e;
        xg[u] = (e < XE && g < i_end * (DP + 1)) ? Zp[g] : 0.0;
      }
#pragma unroll
      for (int u = 0; u < RL; ++u) {
        const int e = t + 256 * u, k = e / QC, j = e - k * QC;
        const long i = i0 + k, col = j0 + j;
        rg[u] = (col < M && i < col) ? C[i * ldc + col] : 0.0;
      }
    };
    auto stage = [&](int buf) {
#pragma unroll
      for (int u = 0; u < XL; ++u) {
        const int e = t + 256 * u;
        if (e < XE) Xt[buf][e] = xg[u];
      }
#pragma unroll
      for (int u = 0; u < RL; ++u) {
        const int e = t + 256 * u, k = e / QC, j = e - k * QC;
        Cs[buf][k * RS + j] = rg[u];
      }
    };

    int buf = 0;
    fetch(0);
    stage(0);
    __syncthreads();
    for (long i0 = 0; i0 < i_end; i0 += QK) {
      const bool more = i0 + QK < i_end;
      if (more) fetch(i0 + QK);
#pragma unroll
      for (int kk = 0; kk < KE; ++kk) {
        const int k = kg * KE + kk;
        const double* p = &Xt[buf][k * (DP + 1)];
        double s = p[DP] - xs2;
#pragma unroll
        for (int d = 0; d < DP; ++d) s = mgp_fma(xs[d], p[d], s);
        Ka[c * QKS + k] = mgp_profile<KIND, double>(s, clamp);
      }
      __syncthreads();
#pragma unroll
      for (int ks = 0; ks < QK; ks += 4) {
        double af[MT], bf[NQ];
#pragma unroll
        for (int m = 0; m < MT; ++m) af[m] = Ka[(wm * 16 * MT + m * 16 + (lane & 15)) * QKS + ks + (lane >> 4)];
#pragma unroll
        for (int q = 0; q < NQ; ++q) bf[q] = Cs[buf][(ks + (lane >> 4)) * RS + (2 * q + wn) * 16 + (lane & 15)];
#pragma unroll
        for (int q = 0; q < NQ; ++q)
#pragma unroll
          for (int m = 0; m < MT; ++m) acc[m][q] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[m], bf[q], acc[m][q], 0, 0, 0);
      }
      if (i0 >= j0) {  // uniform: inside the diagonal block, column tile ct = columns i0 ... i0 + 15 is final
        const int ct = (int)((i0 - j0) / QK);
        if ((ct & 1) == wn) {  // wave-uniform: the column wave that owns the tile
          const long col = i0 + (lane & 15);
          const double cjj = col < M ? C[col * ldc + col] : 0.0;
#pragma unroll
          for (int q = 0; q < NQ; ++q)
            if (q == (ct >> 1)) {
#pragma unroll
              for (int m = 0; m < MT; ++m)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                  const int row = wm * 16 * MT + m * 16 + (lane >> 4) + 4 * g;  // accumulator layout of the f64 MFMA
                  const double kd = Ka[row * QKS + (lane & 15)];
                  const double a = acc[m][q][g];
                  rp[m][g] = mgp_fma(mgp_fma(cjj, kd, a + a), kd, rp[m][g]);
                }
            }
        }
      }
      if (more) stage(buf ^ 1);
      __syncthreads();
      buf ^= 1;
    }
    // the 16 lanes of a row, then the two column waves (Ka is free: every wave is past the last barrier of the walk)
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        double v = rp[m][g];
#pragma unroll
        for (int off = 8; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
        if ((lane & 15) == 0) Ka[wn * QT + wm * 16 * MT + m * 16 + (lane >> 4) + 4 * g] = v;
      }
    __syncthreads();
    // part[J][B'], B' = gridDim.x * QT (rows past B hold the clamped last row and are never read)
    if (t < QT) part[(long)J * Bpad + b0 + t] = Ka[t] + Ka[QT + t];
    __syncthreads();
  }
}

// q[b] = variance^2 * sum_J part[J][b], in block order
__global__ __launch_bounds__(256) void knm_quadform_reduce_kernel(const double* __restrict__ part, int nJ, long Bpad,
                                                                  long B, double scale, double* __restrict__ q) {
  const long b = (long)blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  double s = 0;
  for (int J = 0; J < nJ; ++J) s += part[(long)J * Bpad + b];
  q[b] = s * scale;
}

template <int KIND, int DP>
int quadform_fused_dp(mgp_handle* h, const mgp_kernel* k, const double* Xs, long B, const double* Z, long M,
                      const double* C, long ldc, double* q) {
  const SweepParams prm = mgp_make_params(k);
  const int D = k->D;
  const long nJ = (M + QC - 1) / QC;
  const long Bmax = B < QF_CHUNK_B ? B : QF_CHUNK_B;
  const long Bpad_max = (Bmax + QT - 1) / QT * QT;
  const size_t part_bytes = ((size_t)nJ * Bpad_max * sizeof(double) + 255) & ~(size_t)255;
  MGP_TRY(mgp_reserve(h, &h->prj, &h->prj_bytes, part_bytes + (size_t)M * (DP + 1) * sizeof(double)));
  double* part = (double*)h->prj;
  double* Zp = (double*)((char*)h->prj + part_bytes);
  hipLaunchKernelGGL((qf_pack_kernel<DP>), dim3((unsigned)((M + 255) / 256)), dim3(256), 0, h->stream, Z, M, D, prm, Zp);
  MGP_LAUNCH_CHECK(h);
  for (long c0 = 0; c0 < B; c0 += QF_CHUNK_B) {
    const long Bc = B - c0 < QF_CHUNK_B ? B - c0 : QF_CHUNK_B;
    const long tiles = (Bc + QT - 1) / QT;
    hipLaunchKernelGGL((knm_quadform_kernel<DP, KIND>), dim3((unsigned)tiles, (unsigned)((nJ + 1) / 2)), dim3(256), 0,
                       h->stream, Xs + c0 * D, Bc, (const double*)Zp, M, C, ldc, part, tiles * QT, (int)nJ, D, prm);
    MGP_LAUNCH_CHECK(h);
    hipLaunchKernelGGL(knm_quadform_reduce_kernel, dim3((unsigned)((Bc + 255) / 256)), dim3(256), 0, h->stream,
                       (const double*)part, (int)nJ, tiles * QT, Bc, k->variance * k->variance, q + c0);
    MGP_LAUNCH_CHECK(h);
  }
  return MGP_OK;
}

// generic route: S(i, j) = C(min(i, j), max(i, j)), the symmetric matrix of the upper triangle
template <typename T>
__global__ __launch_bounds__(256) void qf_symmetrise_kernel(const T* __restrict__ C, long M, long ldc,
                                                            T* __restrict__ S) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= M * M) return;
  const long i = e / M, j = e - i * M;
  S[e] = i <= j ? C[i * ldc + j] : C[j * ldc + i];
}

// generic route: q[b] = sum_j P[b, j] W[b, j], one wave per row
template <typename T>
__global__ __launch_bounds__(256) void qf_row_dot_kernel(const T* __restrict__ P, const T* __restrict__ W, long rows,
                                                         long M, T* __restrict__ q) {
  const int lane = threadIdx.x & 63;
  const long b = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= rows) return;
  T s = 0;
  for (long j = lane; j < M; j += 64) s = mgp_fma(P[b * M + j], W[b * M + j], s);
  s = mgp_wave_sum(s);
  if (lane == 0) q[b] = s;
}

template <typename T>
int quadform_generic(mgp_handle* h, const mgp_kernel* k, const T* Xs, long B, const T* Z, long M, const T* C, long ldc,
                     T* q) {
  // panel [rc, M] <= 256 MiB
  long rc_max = (long)((256ull << 20) / ((size_t)M * sizeof(T)));
  if (rc_max < 64) rc_max = 64;
  if (rc_max > B) rc_max = B;
  const size_t s_elems = (size_t)M * M, panel_elems = (size_t)rc_max * M;
  MGP_TRY(mgp_reserve(h, &h->prj, &h->prj_bytes, (s_elems + 2 * panel_elems) * sizeof(T) + 256));
  T* S = (T*)h->prj;
  T* panel = S + s_elems;
  T* W = panel + panel_elems;
  hipLaunchKernelGGL((qf_symmetrise_kernel<T>), dim3((unsigned)((s_elems + 255) / 256)), dim3(256), 0, h->stream, C, M,
                     ldc, S);
  MGP_LAUNCH_CHECK(h);
  for (long i0 = 0; i0 < B; i0 += rc_max) {
    const long rc = B - i0 < rc_max ? B - i0 : rc_max;
    MGP_TRY(mgp_k_dense(h, k, Xs + i0 * k->D, rc, Z, M, panel, M, 0.0, nullptr));
    // W[rc, M] = panel[rc, M] . S[M, M]^T (S is symmetric)
    MGP_TRY(mgp_gemm_nt(h, k->dtype, panel, M, rc, S, M, M, M, W, M, 0, nullptr));
    hipLaunchKernelGGL((qf_row_dot_kernel<T>), dim3((unsigned)((rc + 3) / 4)), dim3(256), 0, h->stream,
                       (const T*)panel, (const T*)W, rc, M, q + i0);
    MGP_LAUNCH_CHECK(h);
  }
  return MGP_OK;
}

}  // namespace

extern "C" int mgp_knm_quadform(mgp_handle* h, const mgp_kernel* k, const void* Xs, int64_t B, const void* Z, int64_t M,
                                const void* C, int64_t ldc, void* q) {
  MGP_TRY(mgp_check_kernel(h, k));
  if (B < 0 || M < 0) return mgp_fail(h, MGP_E_SHAPE, "negative size");
  if (ldc < M) return mgp_fail(h, MGP_E_BADARG, "ldc=%lld is less than M=%lld", (long long)ldc, (long long)M);
  if (!q) return mgp_fail(h, MGP_E_BADARG, "q is NULL");
  if (B == 0) return MGP_OK;
  if (M == 0) {
    MGP_HIP(h, hipMemsetAsync(q, 0, (size_t)B * mgp_elem(k->dtype), h->stream));
    return MGP_OK;
  }
  if (!Xs || !Z || !C) return mgp_fail(h, MGP_E_BADARG, "NULL data pointer");
  if (k->dtype == MGP_F32 || k->D > MGP_FUSED_MAX_D)
    return mgp_with_dtype(k->dtype, [&](auto t) {
      using T = decltype(t);
      return quadform_generic<T>(h, k, (const T*)Xs, B, (const T*)Z, M, (const T*)C, ldc, (T*)q);
    });
  return mgp_with_kind(k->kind, [&](auto kind) {
    return mgp_with_dp(k->D, [&](auto dp) {
      return quadform_fused_dp<decltype(kind)::value, decltype(dp)::value>(h, k, (const double*)Xs, B, (const double*)Z,
                                                                           M, (const double*)C, ldc, (double*)q);
    });
  });
}
