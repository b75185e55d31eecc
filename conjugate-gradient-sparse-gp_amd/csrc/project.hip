// project.hip -- proj = k(Xs, X) R for a WIDE dense R [N, r] (r = 64 ... 256) and the squared row norms of proj:
// the query of a Lanczos variance cache, var(x*) = k** - |k(x*, X) R|^2 (Pleiss et al. 2018).
//
// k(Xs, X) [B, N] is never materialised.  A workgroup owns a tile of test rows (128 for r <= 128, 64 above) and ALL r
// columns, walks its share of the rows of X in steps of 16, evaluates the kernel panel straight into LDS on the VALU
// (the expansion-form distance and the profile arithmetic of kmn_knm_kernel, contract.hip) and contracts it with the
// 16 x r panel of R by v_mfma_f64_16x16x4_f64.  Because one workgroup holds every column, each kernel value is
// evaluated exactly once (B N evaluations in all; the split over N below partitions the rows of X, it does not
// repeat them) -- the fused K_mn K_nm tiles repeat every value once per 128-column tile of the other side, this
// kernel has no other side.  What is re-read is the panel of R, once per row tile (B / 128 times N r elements, from
// the Infinity Cache at the sizes of a cache).
// N is split over blockIdx.z so that small B still fills the chip; the per-split tiles [split, B', r'] go to an arena
// of the handle and a second kernel adds them in split order, scales by the variance, writes proj and forms the row
// norms (of the summed row: they cannot be formed per split).  No float atomics: two calls are bit-identical.
//
// fp32, D > MGP_FUSED_MAX_D or r > 256: row panels of k(Xs_chunk, X) by mgp_k_dense, the NT GEMM of dense.hip against
// R^T, and a row-square-sum kernel.
#include "mgp_common.h"

namespace {

using Acc4 = __attribute__((ext_vector_type(4))) double;

constexpr int PK = 16;        // rows of X per step
constexpr int PKS = PK + 2;   // LDS row stride of the kernel panel
constexpr int PJ_MAX_R = 256;
constexpr long PJ_CHUNK_B = 1L << 16;  // test rows per launch (bounds the partial arena)

// Xp[i] = (2 x_i / l, -|x_i / l|^2): the streamed side of the expansion-form distance, packed once per call so that a
// step of the main kernel stages its 16 rows with one flat copy
// No gate, or the gate word of a CG solve (MGP_OP_KMM_LAMBDA_WIDE): the last argument of the two kernels below.  An
// empty argument generates no code, so the mgp_knm_project instantiations keep the instruction streams they had before
// the gate existed (a null pointer tested at run time moved that entry point's times by up to 1 % either way).
struct PjNoGate {};
struct PjCgGate {
  const int* word;  // device int: 0 = closed, the kernel reads and writes nothing; may be null (open)
};
template <typename GATE>
__device__ __forceinline__ bool pj_closed(GATE gate) {
  if constexpr (std::is_same<GATE, PjCgGate>::value) return gate.word != nullptr && *gate.word == 0;
  return false;
}

template <int DP, typename GATE>
__global__ __launch_bounds__(256) void pj_pack_kernel(const double* __restrict__ X, long N, int D, SweepParams prm,
                                                      double* __restrict__ Xp, GATE gate) {
  if (pj_closed(gate)) return;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  double s = 0;
#pragma unroll
  for (int d = 0; d < DP; ++d) {
    const double v = d < D ? X[i * D + d] * prm.inv_ls[d] : 0.0;
    s = mgp_fma(v, v, s);
    Xp[i * (DP + 1) + d] = v + v;
  }
  Xp[i * (DP + 1) + DP] = -s;
}

// A workgroup of four waves (2 x 2) owns PB = 32 MT test rows and 32 NQ padded columns: MT x NQ accumulator tiles of
// 16 x 16 per wave.  MT = 4, NQ <= 4 (r <= 128): 128 rows, so that the panel of R is re-read by half as many row
// tiles; MT = 2, NQ = 8 (r <= 256): 64 rows.  Either way at most 64 accumulator doubles per lane.  The 2 NQ column
// tiles are dealt to the two column waves alternately so that a ragged r leaves both with the same number of live
// tiles.  The next step's panels of R and X are fetched into registers before the current step's arithmetic and
// stored to LDS after it, so their latency hides behind the VALU and MFMA work.  NQ <= 4 double-buffers the staged
// panels (two barriers per step); NQ = 8 keeps one set (three barriers) to stay inside 64 KB of static LDS.
template <int DP, int KIND, int MT, int NQ, typename GATE>
__global__ __launch_bounds__(256) void knm_project_kernel(const double* __restrict__ Xs, long B,
                                                          const double* __restrict__ Xp, long N,
                                                          const double* __restrict__ R, long r_si, long r_sj, int r,
                                                          double* __restrict__ part, long rows_per_split, int D, int RP,
                                                          SweepParams prm, GATE gate) {
  if (pj_closed(gate)) return;  // uniform
  constexpr int PB = 32 * MT;        // test rows per workgroup
  constexpr int KE = PK * PB / 256;  // kernel values per thread and step
  constexpr int RC = 32 * NQ;        // padded columns of this instantiation
  constexpr int RS = RC + 16;  // row stride of the R panel: the four k rows of an operand read fall in different banks
  constexpr int NB = NQ <= 4 ? 2 : 1;
  constexpr int XE = PK * (DP + 1);           // elements of a staged X panel
  constexpr int XL = (XE + 255) / 256;        // ... per thread
  constexpr int RL = PK * RC / 256;           // elements of a staged R panel per thread
  __shared__ __attribute__((aligned(16))) double Ka[PB * PKS];      // [b][k]
  __shared__ __attribute__((aligned(16))) double Rs[NB][PK * RS];   // [k][j]
  __shared__ __attribute__((aligned(16))) double Xt[NB][XE];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const long b0 = (long)blockIdx.x * PB;
  const long i_begin = (long)blockIdx.z * rows_per_split;
  const long i_end = i_begin + rows_per_split < N ? i_begin + rows_per_split : N;

  // this thread's test row (c) and its KE rows of every 16-row step (kg * KE ...; kg is wave-uniform)
  const int c = t % PB, kg = t / PB;
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

  Acc4 acc[MT][NQ];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int q = 0; q < NQ; ++q) acc[m][q] = Acc4{0, 0, 0, 0};

  double xg[XL], rg[RL];
  // rows past the end and columns past r are fetched as zeros, so they contribute nothing
  auto fetch = [&](long i0) {
#pragma unroll
    for (int u = 0; u < XL; ++u) {
      const int e = t + 256 * u;
      const long g = i0 * (DP + 1) + e;
      xg[u] = (e < XE && g < i_end * (DP + 1)) ? Xp[g] : 0.0;
    }
    if (r_sj == 1) {
#pragma unroll
      for (int u = 0; u < RL; ++u) {
        const int e = t + 256 * u, k = e / RC, j = e - k * RC;
        const long i = i0 + k;
        rg[u] = (j < r && i < i_end) ? R[i * r_si + j] : 0.0;
      }
    } else {
#pragma unroll
      for (int u = 0; u < RL; ++u) {
        const int e = t + 256 * u, j = e / PK, k = e - j * PK;
        const long i = i0 + k;
        rg[u] = (j < r && i < i_end) ? R[i * r_si + (long)j * r_sj] : 0.0;
      }
    }
  };
  auto stage = [&](int buf) {
#pragma unroll
    for (int u = 0; u < XL; ++u) {
      const int e = t + 256 * u;
      if (e < XE) Xt[buf][e] = xg[u];
    }
    if (r_sj == 1) {
#pragma unroll
      for (int u = 0; u < RL; ++u) {
        const int e = t + 256 * u, k = e / RC, j = e - k * RC;
        Rs[buf][k * RS + j] = rg[u];
      }
    } else {
#pragma unroll
      for (int u = 0; u < RL; ++u) {
        const int e = t + 256 * u, j = e / PK, k = e - j * PK;
        Rs[buf][k * RS + j] = rg[u];
      }
    }
  };

  int buf = 0;
  if (i_begin < i_end) {
    fetch(i_begin);
    stage(0);
  }
  __syncthreads();
  for (long i0 = i_begin; i0 < i_end; i0 += PK) {
    const bool more = i0 + PK < i_end;
    if (more) fetch(i0 + PK);
#pragma unroll
    for (int kk = 0; kk < KE; ++kk) {
      const int k = kg * KE + kk;
      const double* p = &Xt[buf][k * (DP + 1)];
      double s = p[DP] - xs2;
#pragma unroll
      for (int d = 0; d < DP; ++d) s = mgp_fma(xs[d], p[d], s);
      Ka[c * PKS + k] = mgp_profile<KIND, double>(s, clamp);
    }
    __syncthreads();
#pragma unroll
    for (int ks = 0; ks < PK; ks += 4) {
      double af[MT], bf[NQ];
#pragma unroll
      for (int m = 0; m < MT; ++m) af[m] = Ka[(wm * 16 * MT + m * 16 + (lane & 15)) * PKS + ks + (lane >> 4)];
#pragma unroll
      for (int q = 0; q < NQ; ++q) bf[q] = Rs[buf][(ks + (lane >> 4)) * RS + (2 * q + wn) * 16 + (lane & 15)];
#pragma unroll
      for (int q = 0; q < NQ; ++q)
        if ((2 * q + wn) * 16 < r) {  // wave-uniform
#pragma unroll
          for (int m = 0; m < MT; ++m) acc[m][q] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[m], bf[q], acc[m][q], 0, 0, 0);
        }
    }
    if (NB == 1) __syncthreads();  // one set of panels: every wave has read it before it is overwritten
    if (more) stage(NB == 2 ? buf ^ 1 : 0);
    __syncthreads();
    if (NB == 2) buf ^= 1;
  }
  // part[split][B'][RP], B' = gridDim.x * PB (rows past B hold the clamped last row and are never read)
  double* o = part + ((long)blockIdx.z * gridDim.x * PB + b0) * RP;
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int col = (2 * q + wn) * 16 + (lane & 15);
      if (col < RP) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int row = wm * 16 * MT + m * 16 + (lane >> 4) + 4 * g;  // accumulator layout of the f64 MFMA
          o[(long)row * RP + col] = acc[m][q][g];
        }
      }
    }
}

// one wave per test row: proj[b, j] = variance * sum_split part (split order), sqnorm[b] = sum_j proj[b, j]^2
__global__ __launch_bounds__(256) void knm_project_reduce_kernel(const double* __restrict__ part, int nsplit, long Bpad,
                                                                 int RP, long B, int r, double variance,
                                                                 double* __restrict__ proj,
                                                                 double* __restrict__ sqnorm) {
  const int lane = threadIdx.x & 63;
  const long b = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;
  double sq = 0;
  for (int j = lane; j < r; j += 64) {
    double s = 0;
    for (int z = 0; z < nsplit; ++z) s += part[((long)z * Bpad + b) * RP + j];
    s *= variance;
    if (proj != nullptr) proj[b * r + j] = s;
    sq = mgp_fma(s, s, sq);
  }
  sq = mgp_wave_sum(sq);
  if (lane == 0 && sqnorm != nullptr) sqnorm[b] = sq;
}

// generic route: Rt[j, i] = R[i, j]
template <typename T>
__global__ __launch_bounds__(256) void pj_transpose_kernel(const T* __restrict__ R, long N, int r, T* __restrict__ Rt) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= N * r) return;
  const long j = e / N, i = e - j * N;
  Rt[e] = R[i * r + j];
}

// generic route: sqnorm[b] = sum_j P[b, j]^2, one wave per row
template <typename T>
__global__ __launch_bounds__(256) void pj_row_sqsum_kernel(const T* __restrict__ P, long rows, int r,
                                                           T* __restrict__ sqnorm) {
  const int lane = threadIdx.x & 63;
  const long b = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= rows) return;
  T sq = 0;
  for (int j = lane; j < r; j += 64) {
    const T v = P[b * r + j];
    sq = mgp_fma(v, v, sq);
  }
  sq = mgp_wave_sum(sq);
  if (lane == 0) sqnorm[b] = sq;
}

// split of N for a launch of `tiles` row tiles: about four workgroups per CU, at least 1024 rows of X per split
void pj_plan(const mgp_handle* h, long tiles, long N, long* nsplit, long* rows) {
  long ns = (4L * h->num_cus + tiles - 1) / tiles;
  const long max_split = (N + 1023) / 1024;
  if (ns > max_split) ns = max_split;
  if (ns < 1) ns = 1;
  long rw = (N + ns - 1) / ns;
  rw = (rw + PK - 1) / PK * PK;
  ns = (N + rw - 1) / rw;
  *nsplit = ns < 1 ? 1 : ns;
  *rows = rw;
}

template <int KIND, int DP>
int project_fused_dp(mgp_handle* h, const mgp_kernel* k, const double* Xs, long B, const double* X, long N,
                     const double* R, int r, int r_layout, double* proj, double* sqnorm) {
  const SweepParams prm = mgp_make_params(k);
  const int D = k->D, RP = (r + 15) / 16 * 16;
  const int PB = r <= 128 ? 128 : 64;
  const long r_si = r_layout == MGP_COLS ? r : 1, r_sj = r_layout == MGP_COLS ? 1 : N;
  size_t part_bytes = 0;
  for (long c0 = 0; c0 < B; c0 += PJ_CHUNK_B) {
    const long tiles = ((B - c0 < PJ_CHUNK_B ? B - c0 : PJ_CHUNK_B) + PB - 1) / PB;
    long ns, rw;
    pj_plan(h, tiles, N, &ns, &rw);
    const size_t bytes = (size_t)ns * tiles * PB * RP * sizeof(double);
    if (bytes > part_bytes) part_bytes = bytes;
  }
  part_bytes = (part_bytes + 255) & ~(size_t)255;
  MGP_TRY(mgp_reserve(h, &h->prj, &h->prj_bytes, part_bytes + (size_t)N * (DP + 1) * sizeof(double)));
  double* part = (double*)h->prj;
  double* Xp = (double*)((char*)h->prj + part_bytes);
  hipLaunchKernelGGL((pj_pack_kernel<DP, PjNoGate>), dim3((unsigned)((N + 255) / 256)), dim3(256), 0, h->stream, X, N, D, prm,
                     Xp, PjNoGate{});
  MGP_LAUNCH_CHECK(h);
  for (long c0 = 0; c0 < B; c0 += PJ_CHUNK_B) {
    const long Bc = B - c0 < PJ_CHUNK_B ? B - c0 : PJ_CHUNK_B;
    const long tiles = (Bc + PB - 1) / PB;
    long ns, rw;
    pj_plan(h, tiles, N, &ns, &rw);
    const double* xs = Xs + c0 * D;
    dim3 grid((unsigned)tiles, 1, (unsigned)ns);
#define MGP_PJ(MTV, NQV)                                                                                             \
  hipLaunchKernelGGL((knm_project_kernel<DP, KIND, MTV, NQV, PjNoGate>), grid, dim3(256), 0, h->stream, xs, Bc,           \
                     (const double*)Xp, N, R, r_si, r_sj, r, part, rw, D, RP, prm, PjNoGate{})
    if (r <= 32) MGP_PJ(4, 1);
    else if (r <= 64) MGP_PJ(4, 2);
    else if (r <= 128) MGP_PJ(4, 4);
    else MGP_PJ(2, 8);
#undef MGP_PJ
    MGP_LAUNCH_CHECK(h);
    hipLaunchKernelGGL(knm_project_reduce_kernel, dim3((unsigned)((Bc + 3) / 4)), dim3(256), 0, h->stream,
                       (const double*)part, (int)ns, tiles * PB, RP, Bc, r, k->variance,
                       proj ? proj + c0 * r : nullptr, sqnorm ? sqnorm + c0 : nullptr);
    MGP_LAUNCH_CHECK(h);
  }
  return MGP_OK;
}

template <typename T>
int project_generic(mgp_handle* h, const mgp_kernel* k, const T* Xs, long B, const T* X, long N, const T* R, int r,
                    int r_layout, T* proj, T* sqnorm) {
  // test-row chunks x streamed chunks of X; panel [rc, sc] <= 256 MiB
  const long sc_max = N < 16384 ? N : 16384;
  long rc_max = (long)((256ull << 20) / ((size_t)sc_max * sizeof(T)));
  if (rc_max < 64) rc_max = 64;
  if (rc_max > B) rc_max = B;
  const size_t rt_elems = r_layout == MGP_COLS ? (size_t)r * N : 0, panel_elems = (size_t)rc_max * sc_max;
  const size_t pc_elems = proj ? 0 : (size_t)rc_max * r;
  MGP_TRY(mgp_reserve(h, &h->prj, &h->prj_bytes, (rt_elems + panel_elems + pc_elems) * sizeof(T) + 256));
  T* Rt = (T*)h->prj;
  T* panel = Rt + rt_elems;
  T* pc = panel + panel_elems;
  const T* Rrows = R;  // [r, N]
  if (r_layout == MGP_COLS) {
    hipLaunchKernelGGL((pj_transpose_kernel<T>), dim3((unsigned)((rt_elems + 255) / 256)), dim3(256), 0, h->stream, R,
                       N, r, Rt);
    MGP_LAUNCH_CHECK(h);
    Rrows = Rt;
  }
  for (long i0 = 0; i0 < B; i0 += rc_max) {
    const long rc = B - i0 < rc_max ? B - i0 : rc_max;
    T* oc = proj ? proj + i0 * r : pc;
    for (long j0 = 0; j0 < N; j0 += sc_max) {
      const long sc = N - j0 < sc_max ? N - j0 : sc_max;
      MGP_TRY(mgp_k_dense(h, k, Xs + i0 * k->D, rc, X + j0 * k->D, sc, panel, sc, 0.0, nullptr));
      // oc[rc, r] (+)= panel[rc, sc] . Rrows[r, j0:j0+sc]^T
      MGP_TRY(mgp_gemm_nt(h, k->dtype, panel, sc, rc, Rrows + j0, N, r, sc, oc, r, j0 > 0 ? 1 : 0, nullptr));
    }
    if (sqnorm) {
      hipLaunchKernelGGL((pj_row_sqsum_kernel<T>), dim3((unsigned)((rc + 3) / 4)), dim3(256), 0, h->stream,
                         (const T*)oc, rc, r, sqnorm + i0);
      MGP_LAUNCH_CHECK(h);
    }
  }
  return MGP_OK;
}

// ---------------------------------------------------------------- many-column (k(Z, Z) + diag lambda) (MGP_OP_KMM_LAMBDA_WIDE)
// out[Bt, M] = P[Bt, M] (k(Z, Z) + diag lambda) with the kernel above: Xs = Z, the packed Z streamed, R = P in the
// MGP_ROWS layout, the right-hand sides in groups of at most PJ_MAX_R.  Every kernel value is evaluated once per group,
// not once per 8 right-hand sides as by the sweep.  The arena: the pack of Z first (its place does not depend on the
// group width, so one pack serves a whole solve), the split tiles of the widest group behind it.

constexpr int FT_I = 64;  // output rows (elements of one right-hand side) per workgroup of the finish kernel
constexpr int FT_B = 16;  // right-hand sides per workgroup: every padded width RP is a multiple

// out[b, i] = variance * sum_split part[split][i][b] (split order) + lam[i] * P[b, i] for the rows i < rows of one row
// chunk and the right-hand sides b < cols of one group; lam, P and out point at the chunk's first row and the group's
// first right-hand side.  part is b-fastest, out is i-fastest: a 64 x 16 tile goes through LDS, read as 16-element
// (128-byte) runs of part and written as 64-element runs of out.  No atomics; a closed gate writes nothing.
__global__ __launch_bounds__(256) void kmm_wide_finish_kernel(const double* __restrict__ part, int nsplit, long Bpad,
                                                              int RP, long rows, int cols, double variance,
                                                              const double* __restrict__ lam,
                                                              const double* __restrict__ P, double* __restrict__ out,
                                                              long M, const int* __restrict__ gate) {
  if (gate != nullptr && *gate == 0) return;
  __shared__ double tile[FT_B][FT_I + 1];
  const int t = threadIdx.x;
  const long i0 = (long)blockIdx.x * FT_I;
  const int bb = blockIdx.y * FT_B;
  {
    const int b = t & (FT_B - 1), il = t / FT_B;
#pragma unroll
    for (int u = 0; u < FT_I * FT_B / 256; ++u) {
      const int ii = il + (256 / FT_B) * u;
      const long i = i0 + ii;
      double s = 0;
      if (i < rows && bb + b < cols) {
        for (int z = 0; z < nsplit; ++z) s += part[((long)z * Bpad + i) * RP + bb + b];
        s *= variance;
      }
      tile[b][ii] = s;
    }
  }
  __syncthreads();
  const int ii = t & (FT_I - 1), bl = t / FT_I;
  const long i = i0 + ii;
  if (i >= rows) return;
  const double l = lam[i];
#pragma unroll
  for (int u = 0; u < FT_I * FT_B / 256; ++u) {
    const int b = bl + (256 / FT_I) * u;
    if (bb + b < cols) {
      const long e = (long)(bb + b) * M + i;
      out[e] = mgp_fma(l, P[e], tile[b][ii]);
    }
  }
}

inline int wide_dp(int D) { return D <= 2 ? 2 : D <= 4 ? 4 : D <= 8 ? 8 : D <= 16 ? 16 : 32; }
inline size_t wide_pack_bytes(long M, int D) {
  return ((size_t)M * (wide_dp(D) + 1) * sizeof(double) + 255) & ~(size_t)255;
}
// split tiles of the widest group of Bt right-hand sides: the full groups of PJ_MAX_R and the remainder plan differently
size_t wide_part_bytes(const mgp_handle* h, long M, long Bt) {
  size_t part_bytes = 0;
  const long widths[2] = {Bt < PJ_MAX_R ? Bt : (long)PJ_MAX_R, Bt > PJ_MAX_R ? Bt % PJ_MAX_R : 0};
  for (const long g : widths) {
    if (g <= 0) continue;
    const long RP = (g + 15) / 16 * 16, PB = g <= 128 ? 128 : 64;
    for (long c0 = 0; c0 < M; c0 += PJ_CHUNK_B) {
      const long tiles = ((M - c0 < PJ_CHUNK_B ? M - c0 : PJ_CHUNK_B) + PB - 1) / PB;
      long ns, rw;
      pj_plan(h, tiles, M, &ns, &rw);
      const size_t bytes = (size_t)ns * tiles * PB * RP * sizeof(double);
      if (bytes > part_bytes) part_bytes = bytes;
    }
  }
  return (part_bytes + 255) & ~(size_t)255;
}

template <int KIND, int DP>
int kmm_wide_dp(mgp_handle* h, const mgp_kernel* k, const double* Z, long M, const double* lam, const double* P,
                long Bt, double* out, const int* gate) {
  const SweepParams prm = mgp_make_params(k);
  const int D = k->D;
  const double* Xp = (const double*)h->prj;
  double* part = (double*)((char*)h->prj + wide_pack_bytes(M, D));
  for (long g0 = 0; g0 < Bt; g0 += PJ_MAX_R) {
    const int r = (int)(Bt - g0 < PJ_MAX_R ? Bt - g0 : PJ_MAX_R), RP = (r + 15) / 16 * 16;
    const int PB = r <= 128 ? 128 : 64;
    const double* Pg = P + g0 * M;
    double* og = out + g0 * M;
    for (long c0 = 0; c0 < M; c0 += PJ_CHUNK_B) {
      const long Bc = M - c0 < PJ_CHUNK_B ? M - c0 : PJ_CHUNK_B;
      const long tiles = (Bc + PB - 1) / PB;
      long ns, rw;
      pj_plan(h, tiles, M, &ns, &rw);
      const double* xs = Z + c0 * D;
      dim3 grid((unsigned)tiles, 1, (unsigned)ns);
#define MGP_PJ(MTV, NQV)                                                                                            \
  hipLaunchKernelGGL((knm_project_kernel<DP, KIND, MTV, NQV, PjCgGate>), grid, dim3(256), 0, h->stream, xs, Bc, Xp, M, \
                     Pg, 1L, M, r, part, rw, D, RP, prm, PjCgGate{gate})
      if (r <= 32) MGP_PJ(4, 1);
      else if (r <= 64) MGP_PJ(4, 2);
      else if (r <= 128) MGP_PJ(4, 4);
      else MGP_PJ(2, 8);
#undef MGP_PJ
      MGP_LAUNCH_CHECK(h);
      hipLaunchKernelGGL(kmm_wide_finish_kernel, dim3((unsigned)((Bc + FT_I - 1) / FT_I), (unsigned)(RP / FT_B)),
                         dim3(256), 0, h->stream, (const double*)part, (int)ns, tiles * PB, RP, Bc, r, k->variance,
                         lam + c0, Pg + c0, og + c0, M, gate);
      MGP_LAUNCH_CHECK(h);
    }
  }
  return MGP_OK;
}

}  // namespace

bool mgp_kmm_wide_serves(const mgp_kernel* k) { return k->dtype == MGP_F64 && k->D <= MGP_FUSED_MAX_D; }

int mgp_kmm_wide_prepare(mgp_handle* h, const mgp_kernel* k, const void* Z, int64_t M, int64_t Bt, const int* gate) {
  const size_t pack_bytes = wide_pack_bytes(M, k->D);
  MGP_TRY(mgp_reserve(h, &h->prj, &h->prj_bytes, pack_bytes + wide_part_bytes(h, M, Bt)));
  const SweepParams prm = mgp_make_params(k);
  return mgp_with_dp(k->D, [&](auto dp) -> int {
    hipLaunchKernelGGL((pj_pack_kernel<decltype(dp)::value, PjCgGate>), dim3((unsigned)((M + 255) / 256)), dim3(256), 0,
                       h->stream, (const double*)Z, (long)M, k->D, prm, (double*)h->prj, PjCgGate{gate});
    MGP_LAUNCH_CHECK(h);
    return MGP_OK;
  });
}

int mgp_kmm_wide_apply(mgp_handle* h, const mgp_kernel* k, const void* Z, int64_t M, const void* lambda, const void* P,
                       int64_t Bt, void* out, const int* gate) {
  if (h->wide_pack_src == Z && h->wide_pack_m == M) {  // inside a solve: packed before its loop, the arena sized there
    if (wide_pack_bytes(M, k->D) + wide_part_bytes(h, M, Bt) > h->prj_bytes)
      return mgp_fail(h, MGP_E_NOMEM, "many-column operator: %lld right-hand sides do not fit the arena reserved for the solve",
                      (long long)Bt);
  } else {
    MGP_TRY(mgp_kmm_wide_prepare(h, k, Z, M, Bt, gate));
  }
  return mgp_with_kind(k->kind, [&](auto kind) {
    return mgp_with_dp(k->D, [&](auto dp) {
      return kmm_wide_dp<decltype(kind)::value, decltype(dp)::value>(h, k, (const double*)Z, M, (const double*)lambda,
                                                                     (const double*)P, Bt, (double*)out, gate);
    });
  });
}

extern "C" int mgp_knm_project(mgp_handle* h, const mgp_kernel* k, const void* Xs, int64_t B, const void* X, int64_t N,
                               const void* R, int32_t r, int r_layout, void* proj, void* sqnorm) {
  MGP_TRY(mgp_check_kernel(h, k));
  if (B < 0 || N < 0 || r < 0) return mgp_fail(h, MGP_E_SHAPE, "negative size");
  if (r_layout != MGP_COLS && r_layout != MGP_ROWS) return mgp_fail(h, MGP_E_BADARG, "bad r_layout %d", r_layout);
  if (!proj && !sqnorm) return mgp_fail(h, MGP_E_BADARG, "proj and sqnorm are both NULL");
  if (B == 0) return MGP_OK;
  const size_t es = mgp_elem(k->dtype);
  if (N == 0 || r == 0) {
    if (proj && r > 0) MGP_HIP(h, hipMemsetAsync(proj, 0, (size_t)B * r * es, h->stream));
    if (sqnorm) MGP_HIP(h, hipMemsetAsync(sqnorm, 0, (size_t)B * es, h->stream));
    return MGP_OK;
  }
  if (!Xs || !X || !R) return mgp_fail(h, MGP_E_BADARG, "NULL data pointer");
  if (k->dtype == MGP_F32 || k->D > MGP_FUSED_MAX_D || r > PJ_MAX_R)
    return mgp_with_dtype(k->dtype, [&](auto t) {
      using T = decltype(t);
      return project_generic<T>(h, k, (const T*)Xs, B, (const T*)X, N, (const T*)R, r, r_layout, (T*)proj, (T*)sqnorm);
    });
  return mgp_with_kind(k->kind, [&](auto kind) {
    return mgp_with_dp(k->D, [&](auto dp) {
      return project_fused_dp<decltype(kind)::value, decltype(dp)::value>(
          h, k, (const double*)Xs, B, (const double*)X, N, (const double*)R, r, r_layout, (double*)proj, (double*)sqnorm);
    });
  });
}
