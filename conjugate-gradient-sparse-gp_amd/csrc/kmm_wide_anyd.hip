// kmm_wide_anyd.hip -- the many-column (k(Z, Z) + diag lambda) operator at MGP_FUSED_MAX_D < D <= MGP_MAX_D, fp64
// (MGP_OP_KMM_LAMBDA_WIDE_ANYD, include/mgp_sweep_anyd.h):  out[Bt, M] = P[Bt, M] (k(Z, Z) + diag lambda)  with no
// kernel panel in memory and every kernel value evaluated once per group of up to 256 right-hand sides.
//
// Distance: the scheme of sweep_anyd.hip.  A 16 x 16 tile of  -s_ij = 2 a_i.b_j - |a_i|^2 - |b_j|^2  comes out of
// v_mfma_f64_16x16x4_f64 with the K dimension augmented,
//     A row (streamed point i) = [ a_1 .. a_D,  |a|^2,  1,      0.. ]
//     B col (owned point j)    = [2b_1 .. 2b_D, -1,    -|b|^2,  0.. ]      K = 4*KS >= D + 2,  a = z c / l
// walked in slices of kWKSL k-steps (32 columns), k ascending, one accumulator per pair across the slices; the profile
// is applied once, after the last slice.  |a|^2 is an fma chain over d ascending.  Z is packed once per call -- once
// per solve inside mgp_pcg_solve -- in the A form and in MFMA fragment order,
//     pack[(tile * KS + ks) * 64 + kq * 16 + l] = A row of point 16 tile + l, column 4 ks + kq,
// so that a k-step of a tile is one 512-byte run: the streamed side is copied flat into LDS, the owned side is loaded
// by every lane as its own operand (B form: doubled, -1 and -|b|^2 taken from the same pack).  Points past M in the last
// tile are exact zeros in every column.
//
// Contraction: the scheme of project.hip.  A workgroup of four waves owns kWOwn = 64 output columns j (one column
// tile per wave) and ALL r <= 256 right-hand sides of a group, and streams the other side i in steps of kWStep = 32.
// For f64 the MFMA result register v of lane l holds tile row (l >> 4) + 4 v, column l & 15: the B-operand map
// (k = l >> 4, column l & 15) for tile rows 4v .. 4v + 3.  So the profiled tile is fed back as the B operand of
//     out^T[r, j] += sum_i P^T[r, i] K[i, j]
// with no LDS round trip, four instructions per 16-row tile of P^T; the 16 x r panel of P goes through LDS and is the
// only thing re-read.  Streamed points past M meet zeros of P (profile(0) = 1 times 0); owned columns past M are never
// stored.
//
// Split and finish: when ceil(M / 64) workgroups leave CUs idle the streamed side is split over blockIdx.z
// (wide_anyd_plan below); every split writes its tile part[split][j][RP] to the arena and a finish kernel adds them in
// split order, scales by the variance, adds lambda_j P[b, j] and writes out.  No float atomics: two calls give the
// same bits.  Right-hand sides beyond 256 go in groups of 256 plus a remainder.
//
// Scratch: the prj arena alone,
//     bytes = align256(8 * 64 * KS * ceil(M / 16)) + align256(8 * nsplit * 64 * ceil(M / 64) * RP),
// KS = ceil((D + 2) / 4), RP = the widest group padded to 16, nsplit by wide_anyd_plan.  c / l_d go through the
// handle's dparams buffer, read by the pack kernel only.
#include "../../include/mgp_sweep_anyd.h"
#include "mgp_common.h"

namespace {

using Acc4 = __attribute__((ext_vector_type(4))) double;

constexpr int kWThreads = 256;
constexpr int kWOwn = 64;     // output columns per workgroup: one 16-column tile per wave
constexpr int kWStep = 32;    // streamed points per step: two 16-row tiles (one with more than 128 right-hand sides)
constexpr int kWKSL = 8;      // k-steps of 4 per K slice
constexpr int kWMaxR = 256;   // right-hand sides per group

// pack[(tile * KS + ks) * 64 + kq * 16 + l]: the A row of point i = 16 tile + l at column k = 4 ks + kq
__global__ __launch_bounds__(256) void wide_anyd_pack_kernel(const double* __restrict__ Z, long M, int D, int KS,
                                                             const double* __restrict__ sc, double* __restrict__ pack,
                                                             const int* __restrict__ gate) {
  if (gate != nullptr && *gate == 0) return;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  const long Mt = (M + 15) / 16 * 16;
  if (i >= Mt) return;
  double* row = pack + (i >> 4) * (long)KS * 64 + (i & 15);
  if (i >= M) {
    for (int k = 0; k < 4 * KS; ++k) row[(k >> 2) * 64 + (k & 3) * 16] = 0.0;
    return;
  }
  double s = 0;
  for (int d = 0; d < D; ++d) {
    const double v = Z[i * D + d] * sc[d];
    s = mgp_fma(v, v, s);
    row[(d >> 2) * 64 + (d & 3) * 16] = v;
  }
  for (int k = D; k < 4 * KS; ++k) row[(k >> 2) * 64 + (k & 3) * 16] = k == D ? s : (k == D + 1 ? 1.0 : 0.0);
}

// NRT = 16-row tiles of P^T held by a wave: r <= 16 NRT right-hand sides
template <int KIND, int NRT>
__global__ __launch_bounds__(kWThreads) void kmm_wide_anyd_kernel(const double* __restrict__ pack, long M, int D,
                                                                   const double* __restrict__ P, int r,
                                                                   double* __restrict__ part, long rows_per_split,
                                                                   int RP, double clamp, const int* __restrict__ gate) {
  if (gate != nullptr && *gate == 0) return;
  constexpr int RC = 16 * NRT;  // padded right-hand sides of this instantiation
  constexpr int RS = RC + 16;   // row stride of the P panel: the four k rows of an operand read fall in different banks
  constexpr int NIT = NRT <= 8 ? kWStep / 16 : 1;  // 16-row tiles per step: the P panel of a step stays inside 64 KB
  constexpr int STEP = 16 * NIT;
  constexpr int PL = STEP * RC / kWThreads;  // elements of a staged P panel per thread
  constexpr int SWZ = 32 / STEP;
  __shared__ __attribute__((aligned(16))) double frag[NIT * kWKSL * 64];  // one K slice of the streamed step
  // [i][b ^ swz(i)], swz(i) = SWZ (i >> 1) & 15: the staging stores of 32 lanes (i fastest) fall in 32 different banks
  __shared__ __attribute__((aligned(16))) double Ps[STEP * RS];
  __shared__ double e2tab[MGP_EXP2_TAB_SIZE];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int l15 = lane & 15, kq = lane >> 4;
  for (int e = t; e < MGP_EXP2_TAB_SIZE; e += kWThreads) e2tab[e] = mgp_exp2_tab_entry(e);
  const E2Tab<true> e2{e2tab};

  const int KS = (D + 2 + 3) >> 2;
  const long Mt = (M + 15) / 16 * 16;
  const long j0 = (long)blockIdx.x * kWOwn + wave * 16;  // this wave's column tile
  // a column tile wholly past M computes on tile 0 and stores nothing
  const double* own = pack + (j0 < Mt ? j0 >> 4 : 0L) * KS * 64;
  const long i_begin = (long)blockIdx.z * rows_per_split;
  const long i_end = i_begin + rows_per_split < Mt ? i_begin + rows_per_split : Mt;

  Acc4 acc[NRT];
#pragma unroll
  for (int q = 0; q < NRT; ++q) acc[q] = Acc4{0, 0, 0, 0};

  double pg[PL];
  // P panel of a step: rows i0 .. i0 + STEP - 1, right-hand sides 0 .. RC - 1; zeros past M and past r
  auto fetch = [&](long i0) {
#pragma unroll
    for (int u = 0; u < PL; ++u) {
      const int e = t + kWThreads * u, b = e / STEP, ii = e - b * STEP;
      const long i = i0 + ii;
      pg[u] = (b < r && i < M) ? P[(long)b * M + i] : 0.0;
    }
  };
  auto stage = [&]() {
#pragma unroll
    for (int u = 0; u < PL; ++u) {
      const int e = t + kWThreads * u, b = e / STEP, ii = e - b * STEP;
      Ps[ii * RS + (b ^ ((SWZ * (ii >> 1)) & 15))] = pg[u];
    }
  };

  if (i_begin < i_end) fetch(i_begin);
  for (long i0 = i_begin; i0 < i_end; i0 += STEP) {
    Acc4 c[NIT];
#pragma unroll
    for (int it = 0; it < NIT; ++it) c[it] = Acc4{0, 0, 0, 0};
    const int nit = i_end - i0 < STEP ? (int)((i_end - i0) >> 4) : NIT;  // live 16-row tiles (uniform)

    for (int s0 = 0; s0 < KS; s0 += kWKSL) {
      const int nks = KS - s0 < kWKSL ? KS - s0 : kWKSL;
      // the owned operands of this slice: B form of this wave's column tile
      double bf[kWKSL];
#pragma unroll
      for (int ks = 0; ks < kWKSL; ++ks) {
        bf[ks] = 0.0;
        if (ks < nks) {
          const int k = 4 * (s0 + ks) + kq;
          // column D + 1 holds -|b|^2: |b|^2 stands in column D of the A form
          const double v = k == D + 1 ? own[(long)(D >> 2) * 64 + (D & 3) * 16 + l15] : own[(long)(s0 + ks) * 64 + lane];
          bf[ks] = k < D ? v + v : (k == D ? -1.0 : (k == D + 1 ? -v : 0.0));
        }
      }
      __syncthreads();  // the previous slice's fragments, and the previous step's P panel, fully consumed
      // streamed A fragments of the slice: a flat copy, nit tiles x nks k-steps x 64
      for (int e = t; e < NIT * kWKSL * 64; e += kWThreads) {
        const int it = e / (kWKSL * 64), rem = e - it * (kWKSL * 64), ks = rem >> 6;
        if (it < nit && ks < nks) frag[e] = pack[(((i0 >> 4) + it) * KS + s0 + ks) * 64 + (rem & 63)];
      }
      if (s0 == 0) stage();
      __syncthreads();
#pragma unroll
      for (int ks = 0; ks < kWKSL; ++ks)
        if (ks < nks) {
#pragma unroll
          for (int it = 0; it < NIT; ++it)
            if (it < nit) {
              const double af = frag[(it * kWKSL + ks) * 64 + lane];
              c[it] = __builtin_amdgcn_mfma_f64_16x16x4f64(af, bf[ks], c[it], 0, 0, 0);
            }
        }
    }
    if (i0 + STEP < i_end) fetch(i0 + STEP);  // in flight behind the contraction

    // ---- the profile once per pair, then the tile as the B operand of out^T += P^T K
#pragma unroll
    for (int it = 0; it < NIT; ++it)
      if (it < nit) {
        Acc4 kv;
#pragma unroll
        for (int v = 0; v < 4; ++v) kv[v] = mgp_profile<KIND, double, E2Tab<true>>(c[it][v], clamp, e2);
#pragma unroll
        for (int v = 0; v < 4; ++v) {  // tile rows 4v .. 4v + 3, ascending: the order of every output's chain
          const int row = it * 16 + 4 * v + kq;
          const double* prow = &Ps[row * RS + (l15 ^ ((SWZ * (row >> 1)) & 15))];
#pragma unroll
          for (int q = 0; q < NRT; ++q)
            if (q * 16 < r)  // wave-uniform
              acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(prow[q * 16], kv[v], acc[q], 0, 0, 0);
        }
      }
  }

  // part[split][j][RP], j < 64 gridDim.x: result register v of lane l holds right-hand side (l >> 4) + 4 v, column l & 15
  const long Mp = (long)gridDim.x * kWOwn;
  double* o = part + ((long)blockIdx.z * Mp + j0 + l15) * RP;
#pragma unroll
  for (int q = 0; q < NRT; ++q)
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int b = q * 16 + kq + 4 * v;
      if (b < RP) o[b] = acc[q][v];
    }
}

constexpr int kFI = 64;  // output elements per workgroup of the finish kernel
constexpr int kFB = 16;  // right-hand sides per workgroup: every padded width RP is a multiple

// out[b, j] = variance * sum_split part[split][j][b] (split order) + lam[j] * P[b, j]: the tile scheme of
// kmm_wide_finish_kernel (project.hip) -- part is b-fastest, out is j-fastest, a 64 x 16 tile goes through LDS
__global__ __launch_bounds__(256) void kmm_wide_anyd_finish_kernel(const double* __restrict__ part, int nsplit, long Mp,
                                                                   int RP, long M, int cols, double variance,
                                                                   const double* __restrict__ lam,
                                                                   const double* __restrict__ P,
                                                                   double* __restrict__ out,
                                                                   const int* __restrict__ gate) {
  if (gate != nullptr && *gate == 0) return;
  __shared__ double tile[kFB][kFI + 1];
  const int t = threadIdx.x;
  const long j0 = (long)blockIdx.x * kFI;
  const int bb = blockIdx.y * kFB;
  {
    const int b = t & (kFB - 1), jl = t / kFB;
#pragma unroll
    for (int u = 0; u < kFI * kFB / 256; ++u) {
      const int jj = jl + (256 / kFB) * u;
      const long j = j0 + jj;
      double s = 0;
      if (j < M && bb + b < cols) {
        for (int z = 0; z < nsplit; ++z) s += part[((long)z * Mp + j) * RP + bb + b];
        s *= variance;
      }
      tile[b][jj] = s;
    }
  }
  __syncthreads();
  const int jj = t & (kFI - 1), bl = t / kFI;
  const long j = j0 + jj;
  if (j >= M) return;
  const double l = lam[j];
#pragma unroll
  for (int u = 0; u < kFI * kFB / 256; ++u) {
    const int b = bl + (256 / kFI) * u;
    if (bb + b < cols) {
      const long e = (long)(bb + b) * M + j;
      out[e] = mgp_fma(l, P[e], tile[b][jj]);
    }
  }
}

struct WideAnydPlan {
  long nblk, nsplit, rows;
};

// split of the streamed side: about two workgroups per CU, at least 256 streamed points per split, a split a multiple
// of the step
WideAnydPlan wide_anyd_plan(long M, int num_cus) {
  WideAnydPlan p;
  p.nblk = (M + kWOwn - 1) / kWOwn;
  long ns = (2L * num_cus + p.nblk - 1) / p.nblk;
  const long max_split = (M + 255) / 256;
  if (ns > max_split) ns = max_split;
  if (ns < 1) ns = 1;
  long rows = (M + ns - 1) / ns;
  rows = (rows + kWStep - 1) / kWStep * kWStep;
  p.rows = rows;
  p.nsplit = (M + rows - 1) / rows;
  return p;
}

inline int wide_anyd_ks(int D) { return (D + 2 + 3) >> 2; }
inline size_t wide_anyd_pack_bytes(long M, int D) {
  return ((size_t)((M + 15) / 16) * wide_anyd_ks(D) * 64 * sizeof(double) + 255) & ~(size_t)255;
}
// split tiles of the widest group of Bt right-hand sides
size_t wide_anyd_part_bytes(const mgp_handle* h, long M, long Bt) {
  const long g = Bt < kWMaxR ? Bt : (long)kWMaxR;
  const long RP = (g + 15) / 16 * 16;
  const WideAnydPlan pl = wide_anyd_plan(M, h->num_cus);
  return ((size_t)pl.nsplit * pl.nblk * kWOwn * RP * sizeof(double) + 255) & ~(size_t)255;
}

template <int KIND>
int kmm_wide_anyd_run(mgp_handle* h, const mgp_kernel* k, long M, const double* lam, const double* P, long Bt,
                      double* out, const int* gate) {
  const int D = k->D;
  const double c = mgp_profile_scale(k->kind);
  const double clamp = c * c * 1e-36;
  const double* pack = (const double*)h->prj;
  double* part = (double*)((char*)h->prj + wide_anyd_pack_bytes(M, D));
  const WideAnydPlan pl = wide_anyd_plan(M, h->num_cus);
  if (pl.nblk > 2147483647L || pl.nsplit > 65535) return mgp_fail(h, MGP_E_SHAPE, "many-column operator: grid too large");
  for (long g0 = 0; g0 < Bt; g0 += kWMaxR) {
    const int r = (int)(Bt - g0 < kWMaxR ? Bt - g0 : kWMaxR), RP = (r + 15) / 16 * 16;
    const double* Pg = P + g0 * M;
    double* og = out + g0 * M;
    dim3 grid((unsigned)pl.nblk, 1, (unsigned)pl.nsplit);
#define MGP_WA(NRTV)                                                                                                  \
  hipLaunchKernelGGL((kmm_wide_anyd_kernel<KIND, NRTV>), grid, dim3(kWThreads), 0, h->stream, pack, M, D, Pg, r, part, \
                     pl.rows, RP, clamp, gate)
    if (r <= 32) MGP_WA(2);
    else if (r <= 64) MGP_WA(4);
    else if (r <= 128) MGP_WA(8);
    else MGP_WA(16);
#undef MGP_WA
    MGP_LAUNCH_CHECK(h);
    hipLaunchKernelGGL(kmm_wide_anyd_finish_kernel, dim3((unsigned)((M + kFI - 1) / kFI), (unsigned)(RP / kFB)),
                       dim3(256), 0, h->stream, (const double*)part, (int)pl.nsplit, pl.nblk * kWOwn, RP, M, r,
                       k->variance, lam, Pg, og, gate);
    MGP_LAUNCH_CHECK(h);
  }
  return MGP_OK;
}

}  // namespace

bool mgp_kmm_wide_anyd_serves(const mgp_kernel* k) { return k->dtype == MGP_F64 && k->D > MGP_FUSED_MAX_D; }

int mgp_kmm_wide_anyd_prepare(mgp_handle* h, const mgp_kernel* k, const void* Z, int64_t M, int64_t Bt,
                              const int* gate) {
  MGP_TRY(mgp_reserve(h, &h->prj, &h->prj_bytes, wide_anyd_pack_bytes(M, k->D) + wide_anyd_part_bytes(h, M, Bt)));
  double host[MGP_MAX_D];
  const double c = mgp_profile_scale(k->kind);
  for (int d = 0; d < k->D; ++d) host[d] = c / k->lengthscales[d];
  MGP_HIP(h, hipMemcpyAsync(h->dparams, host, (size_t)k->D * sizeof(double), hipMemcpyHostToDevice, h->stream));
  MGP_HIP(h, hipStreamSynchronize(h->stream));  // host[] is a stack temporary
  const long Mt = (M + 15) / 16 * 16;
  hipLaunchKernelGGL(wide_anyd_pack_kernel, dim3((unsigned)((Mt + 255) / 256)), dim3(256), 0, h->stream,
                     (const double*)Z, (long)M, k->D, wide_anyd_ks(k->D), (const double*)h->dparams, (double*)h->prj,
                     gate);
  MGP_LAUNCH_CHECK(h);
  return MGP_OK;
}

int mgp_kmm_wide_anyd_apply(mgp_handle* h, const mgp_kernel* k, const void* Z, int64_t M, const void* lambda,
                            const void* P, int64_t Bt, void* out, const int* gate) {
  if (h->wide_pack_src == Z && h->wide_pack_m == M) {  // inside a solve: packed before its loop, the arena sized there
    if (wide_anyd_pack_bytes(M, k->D) + wide_anyd_part_bytes(h, M, Bt) > h->prj_bytes)
      return mgp_fail(h, MGP_E_NOMEM, "many-column operator: %lld right-hand sides do not fit the arena reserved for the solve",
                      (long long)Bt);
  } else {
    MGP_TRY(mgp_kmm_wide_anyd_prepare(h, k, Z, M, Bt, gate));
  }
  return mgp_with_kind(k->kind, [&](auto kind) {
    return kmm_wide_anyd_run<decltype(kind)::value>(h, k, M, (const double*)lambda, (const double*)P, Bt, (double*)out,
                                                    gate);
  });
}
