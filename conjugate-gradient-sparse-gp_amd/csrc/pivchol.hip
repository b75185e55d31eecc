// pivchol.hip -- matrix-free partial pivoted Cholesky of k(X, X) and the diagonal-plus-low-rank preconditioner
// application built on it (Harbrecht, Peters & Schneider 2012; Gardner et al. 2018, the mBCG preconditioner).
//
// mgp_kxx_pivchol: greedy rank-k factor K ~= L^T L, L [k, N] row-major.  Step i needs the pivot p_i = argmax d, the
// row k(x_p, X) and the i earlier rows of L -- 8 i N bytes streamed once, the whole build about 4 k^2 N bytes.  One
// launch per step, no host round trip: every workgroup of step i first reduces the (max, index, sum) partials that
// the workgroups of step i - 1 left (double-buffered), so all of them know p_i, then forms its own slice of row i,
// updates its slice of d and leaves its own partial for step i + 1.  The argmax (lowest index on ties) and the
// trace are reduced in a fixed order: two calls give the same bits.  No spin waits between workgroups, no
// persistent grid.
//
// mgp_lowrank_apply: z = dinv o r - (r B^T) B for row batches, B [k, n].  Pass 1 is a reduction over n in two
// stages (column-chunk partials, then their sum in chunk order; no float atomics), pass 2 forms z.  Both stream B
// once; they are bandwidth-bound.  The gated form is the MGP_PRE_LOWRANK step of the device CG loop (cg.hip).
//
// MGP_PRE_LOWRANK_WIDE: the same z for batches of many rows, in groups of 256 instead of 16: both products as tiles
// of v_mfma_f64_16x16x4_f64, pass 1 split over n with the per-split tiles added in split order (the sum kernel above),
// pass 2 with the diagonal term fused into its store.  Three launches per 256 rows; no float atomics.
#include "mgp_common.h"

namespace {

constexpr int PC_NT = 256;        // threads per workgroup of the factor kernels
constexpr int PC_MAX_WG = 512;    // workgroups per step (each reads every partial of the step before)
constexpr int PC_MAX_RANK = 1024;

struct PcState {
  int rank;     // rows of L written so far that count (set when the build stops early)
  int stopped;  // a step found the trace under the tolerance or no positive pivot
};

// (max, lowest index of the max, sum) of the workgroup's values; every thread returns the same triple
struct PcTriple {
  double mx;
  long ix;
  double sm;
};

__device__ __forceinline__ void pc_take(PcTriple& a, double mx, long ix) {
  if (mx > a.mx || (mx == a.mx && ix < a.ix)) {
    a.mx = mx;
    a.ix = ix;
  }
}

__device__ __forceinline__ PcTriple pc_block_reduce(PcTriple v, double* smx, long* six, double* ssm) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const double omx = __shfl_xor(v.mx, off, 64);
    const long oix = __shfl_xor(v.ix, off, 64);
    v.sm += __shfl_xor(v.sm, off, 64);
    pc_take(v, omx, oix);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();  // the LDS slots may still be read from the previous reduction
  if (lane == 0) {
    smx[wave] = v.mx;
    six[wave] = v.ix;
    ssm[wave] = v.sm;
  }
  __syncthreads();
  PcTriple r{smx[0], six[0], ssm[0]};
  for (int w = 1; w < PC_NT / 64; ++w) {  // fixed order
    pc_take(r, smx[w], six[w]);
    r.sm += ssm[w];
  }
  return r;
}

// d = variance everywhere, the partials of step 0, the state word
__global__ __launch_bounds__(PC_NT) void pivchol_init_kernel(double* __restrict__ d, long N, long slice, double variance,
                                                              double* __restrict__ pmx, long* __restrict__ pix,
                                                              double* __restrict__ psm, PcState* __restrict__ st,
                                                              int max_rank) {
  __shared__ double smx[PC_NT / 64], ssm[PC_NT / 64];
  __shared__ long six[PC_NT / 64];
  const long c0 = (long)blockIdx.x * slice;
  const long c1 = c0 + slice < N ? c0 + slice : N;
  PcTriple v{-1.0, N, 0.0};
  for (long c = c0 + threadIdx.x; c < c1; c += PC_NT) {
    d[c] = variance;
    pc_take(v, variance, c);
    v.sm += variance;
  }
  v = pc_block_reduce(v, smx, six, ssm);
  if (threadIdx.x == 0) {
    pmx[blockIdx.x] = v.mx;
    pix[blockIdx.x] = v.ix;
    psm[blockIdx.x] = v.sm;
    if (blockIdx.x == 0) {
      st->rank = max_rank;
      st->stopped = 0;
    }
  }
}

// Step i of the factor.  `in` partials come from step i - 1 (or the init kernel), `out` go to step i + 1.
template <int KIND>
__global__ __launch_bounds__(PC_NT) void pivchol_step_kernel(const double* __restrict__ X, long N, int D,
                                                              const double* __restrict__ inv_ls, double variance,
                                                              double stop_sum, int i, double* __restrict__ L,
                                                              double* __restrict__ d, long* __restrict__ piv, long slice,
                                                              const double* __restrict__ in_mx, const long* __restrict__ in_ix,
                                                              const double* __restrict__ in_sm, double* __restrict__ out_mx,
                                                              long* __restrict__ out_ix, double* __restrict__ out_sm,
                                                              PcState* __restrict__ st) {
  if (st->stopped) return;  // written by an earlier launch
  __shared__ double smx[PC_NT / 64], ssm[PC_NT / 64];
  __shared__ long six[PC_NT / 64];
  __shared__ double xp[MGP_MAX_D];   // the pivot's row, scaled
  __shared__ double sinv[MGP_MAX_D];
  __shared__ double lp[PC_MAX_RANK];  // L[j, p] for j < i
  const int t = threadIdx.x;
  // every workgroup reduces all partials of the step before, in the same order: the same pivot and trace everywhere
  PcTriple g{-1.0, N, 0.0};
  for (int w = t; w < (int)gridDim.x; w += PC_NT) {
    pc_take(g, in_mx[w], in_ix[w]);
    g.sm += in_sm[w];
  }
  g = pc_block_reduce(g, smx, six, ssm);
  if (!(g.sm > stop_sum) || !(g.mx > 0.0)) {
    if (blockIdx.x == 0 && t == 0) {
      st->rank = i;
      st->stopped = 1;
    }
    return;
  }
  const long p = g.ix;
  const double inv_root = 1.0 / mgp_sqrt(g.mx);
  for (int e = t; e < D; e += PC_NT) {
    const double s = inv_ls[e];
    sinv[e] = s;
    xp[e] = X[p * D + e] * s;
  }
  for (int j = t; j < i; j += PC_NT) lp[j] = L[(long)j * N + p];
  if (blockIdx.x == 0 && t == 0) piv[i] = p;
  __syncthreads();
  const long c0 = (long)blockIdx.x * slice;
  const long c1 = c0 + slice < N ? c0 + slice : N;
  double* __restrict__ Li = L + (long)i * N;
  PcTriple v{-1.0, N, 0.0};
  for (long c = c0 + t; c < c1; c += PC_NT) {
    const double dc = d[c];
    double lv = 0.0, dn = 0.0;
    // a column whose residual diagonal is exactly 0 -- every earlier pivot, and the pivot itself below -- keeps an
    // exact 0 in this row: its residual row is 0 in exact arithmetic (K is positive semi-definite)
    if (c == p) {
      lv = g.mx * inv_root;  // sqrt(d_p)
    } else if (dc > 0.0) {
      double r2 = 0.0;
      const double* __restrict__ xc = X + c * D;
      for (int e = 0; e < D; ++e) {
        const double df = xc[e] * sinv[e] - xp[e];
        r2 = mgp_fma(df, df, r2);
      }
      // k(x_p, x_c) / variance from direct differences of the rows scaled by 1 / lengthscale; the slope is not used
      double f, fp;
      mgp_profile_slope<KIND>(r2, f, fp);
      double acc = variance * f;
#pragma unroll 8
      for (int j = 0; j < i; ++j) acc = mgp_fma(-lp[j], L[(long)j * N + c], acc);
      lv = acc * inv_root;
      dn = mgp_fma(-lv, lv, dc);
      dn = dn > 0.0 ? dn : 0.0;
    }
    Li[c] = lv;
    d[c] = dn;
    pc_take(v, dn, c);
    v.sm += dn;
  }
  v = pc_block_reduce(v, smx, six, ssm);
  if (t == 0) {
    out_mx[blockIdx.x] = v.mx;
    out_ix[blockIdx.x] = v.ix;
    out_sm[blockIdx.x] = v.sm;
  }
}

// ---- z = dinv o r - (r B^T) B ------------------------------------------------------------------------------------
constexpr int LR_ROWS = 16;      // rows of B per workgroup of pass 1 (four per wavefront)
constexpr int LR_LDS_ELEMS = 2048;  // elements of r a workgroup of pass 1 stages (chunk columns x columns of the batch)
constexpr int LR_TILE = 128;     // rows of B whose coefficients pass 2 stages at a time

// pass 1: part[chunk, b, i] = sum over the chunk's columns j of R[b, j] B[i, j]
template <typename T, int BT>
__global__ __launch_bounds__(256) void lowrank_dot_kernel(const int* __restrict__ gate, const T* __restrict__ B, long k,
                                                          long n, const T* __restrict__ R, int bt, long chunk,
                                                          T* __restrict__ part) {
  if (gate != nullptr && *gate == 0) return;
  __shared__ T rs[LR_LDS_ELEMS];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const long c0 = (long)blockIdx.x * chunk;
  const long cn = (c0 + chunk < n ? c0 + chunk : n) - c0;  // columns of this chunk
  for (long e = t; e < (long)BT * chunk; e += 256) {
    const long b = e / chunk, j = e - b * chunk;
    rs[e] = (b < bt && j < cn) ? R[b * n + c0 + j] : (T)0;
  }
  __syncthreads();
  const long i0 = (long)blockIdx.y * LR_ROWS;
  for (int q = wave; q < LR_ROWS; q += 4) {
    const long i = i0 + q;
    if (i >= k) break;  // wave-uniform
    const T* __restrict__ Bi = B + i * n + c0;
    T acc[BT];
#pragma unroll
    for (int b = 0; b < BT; ++b) acc[b] = 0;
    for (long j = lane; j < cn; j += 64) {
      const T bv = Bi[j];
#pragma unroll
      for (int b = 0; b < BT; ++b) acc[b] = mgp_fma(bv, rs[b * chunk + j], acc[b]);
    }
#pragma unroll
    for (int b = 0; b < BT; ++b) {
      const T v = mgp_wave_sum(acc[b]);
      if (lane == 0 && b < bt) part[((long)blockIdx.x * bt + b) * k + i] = v;
    }
  }
}

// stage 2 of pass 1: tt[b, i] = sum over chunks, in chunk order
template <typename T>
__global__ __launch_bounds__(256) void lowrank_sum_kernel(const int* __restrict__ gate, const T* __restrict__ part,
                                                          long nchunks, long total, T* __restrict__ tt) {
  if (gate != nullptr && *gate == 0) return;
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  T s = 0;
  for (long c = 0; c < nchunks; ++c) s += part[c * total + e];
  tt[e] = s;
}

// pass 2: Z[b, j] = dinv[j] R[b, j] - sum_i tt[b, i] B[i, j]
template <typename T, int BT>
__global__ __launch_bounds__(256) void lowrank_form_kernel(const int* __restrict__ gate, const T* __restrict__ dinv,
                                                           const T* __restrict__ B, long k, long n,
                                                           const T* __restrict__ R, int bt, const T* __restrict__ tt,
                                                           T* __restrict__ Z) {
  if (gate != nullptr && *gate == 0) return;
  __shared__ T ts[BT * LR_TILE];
  const long j = (long)blockIdx.x * 256 + threadIdx.x;
  const long jc = j < n ? j : n - 1;
  T acc[BT];
#pragma unroll
  for (int b = 0; b < BT; ++b) acc[b] = 0;
  for (long i0 = 0; i0 < k; i0 += LR_TILE) {
    const int lim = (int)(k - i0 < LR_TILE ? k - i0 : LR_TILE);
    __syncthreads();
    for (int e = threadIdx.x; e < BT * LR_TILE; e += 256) {
      const int b = e / LR_TILE, q = e - b * LR_TILE;
      ts[e] = (b < bt && q < lim) ? tt[(long)b * k + i0 + q] : (T)0;
    }
    __syncthreads();
    const T* __restrict__ Bc = B + i0 * n + jc;
#pragma unroll 8
    for (int q = 0; q < lim; ++q) {
      const T bv = Bc[(long)q * n];
#pragma unroll
      for (int b = 0; b < BT; ++b) acc[b] = mgp_fma(ts[b * LR_TILE + q], bv, acc[b]);
    }
  }
  if (j >= n) return;
  const T dv = dinv[j];
#pragma unroll
  for (int b = 0; b < BT; ++b)
    if (b < bt) Z[(long)b * n + j] = mgp_fma(dv, R[(long)b * n + j], -acc[b]);
}

// columns of a pass-1 chunk for a batch rounded up to BT columns: a multiple of 64, at most 2048
inline long lr_chunk(int BT) { return LR_LDS_ELEMS / BT; }

template <typename T, int BT>
int lowrank_group(mgp_handle* h, const T* dinv, const T* B, long k, long n, const T* R, int bt, T* Z, const int* gate) {
  const long chunk = lr_chunk(BT);
  const long nchunks = (n + chunk - 1) / chunk;
  const long total = (long)bt * k;
  MGP_TRY(mgp_reserve(h, &h->pch, &h->pch_bytes, (size_t)(nchunks + 1) * total * sizeof(T)));
  T* part = (T*)h->pch;
  T* tt = part + nchunks * total;
  hipLaunchKernelGGL((lowrank_dot_kernel<T, BT>), dim3((unsigned)nchunks, (unsigned)((k + LR_ROWS - 1) / LR_ROWS)),
                     dim3(256), 0, h->stream, gate, B, k, n, R, bt, chunk, part);
  MGP_LAUNCH_CHECK(h);
  hipLaunchKernelGGL((lowrank_sum_kernel<T>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, h->stream, gate,
                     (const T*)part, nchunks, total, tt);
  MGP_LAUNCH_CHECK(h);
  hipLaunchKernelGGL((lowrank_form_kernel<T, BT>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, gate,
                     dinv, B, k, n, R, bt, (const T*)tt, Z);
  MGP_LAUNCH_CHECK(h);
  return MGP_OK;
}

template <typename T>
int lowrank_apply_t(mgp_handle* h, const T* dinv, const T* B, long k, long n, const T* R, long Bt, T* Z,
                    const int* gate) {
  // batches of more than 16 rows go in groups of 16 (B is read once per group)
  for (long b0 = 0; b0 < Bt; b0 += 16) {
    const int bt = (int)(Bt - b0 < 16 ? Bt - b0 : 16);
    const T* Rg = R + b0 * n;
    T* Zg = Z + b0 * n;
    if (bt == 1) MGP_TRY((lowrank_group<T, 1>(h, dinv, B, k, n, Rg, bt, Zg, gate)));
    else if (bt == 2) MGP_TRY((lowrank_group<T, 2>(h, dinv, B, k, n, Rg, bt, Zg, gate)));
    else if (bt <= 4) MGP_TRY((lowrank_group<T, 4>(h, dinv, B, k, n, Rg, bt, Zg, gate)));
    else if (bt <= 8) MGP_TRY((lowrank_group<T, 8>(h, dinv, B, k, n, Rg, bt, Zg, gate)));
    else MGP_TRY((lowrank_group<T, 16>(h, dinv, B, k, n, Rg, bt, Zg, gate)));
  }
  return MGP_OK;
}

// ---- the same z for many rows of R (MGP_PRE_LOWRANK_WIDE): both products on the fp64 matrix cores ------------------
// A workgroup of four waves (2 x 2) owns LW_TB = 32 MT rows of the batch and LW_TN = 64 columns of the product, MT x 2
// accumulator tiles of 16 x 16 per wave, and walks its contraction range in steps of 16 staged through LDS; the next
// step's panels are fetched into registers before the current step's arithmetic (the scheme of project.hip).  Operand
// and accumulator lanes of v_mfma_f64_16x16x4_f64 as in project.hip: A[row = lane & 15][k = lane >> 4],
// B[k = lane >> 4][col = lane & 15], C[row = (lane >> 4) + 4 g][col = lane & 15].
using LwAcc4 = __attribute__((ext_vector_type(4))) double;
constexpr int LW_KC = 16;           // contraction elements per step
constexpr int LW_STR = LW_KC + 2;   // LDS row stride of a panel held contraction-fastest
constexpr int LW_TN = 64;           // columns of the product per workgroup
constexpr int LW_RS = LW_TN + 16;   // LDS row stride of pass 2's panel of B: the four rows of an operand read fall in different banks
constexpr int LW_GROUP = 256;       // rows of the batch per group of launches
constexpr long LW_MIN_SPLIT = 256;  // columns of n a split of pass 1 holds at least

// pass 1: part[split][b][i] = sum over the split's columns j of R[b, j] B[i, j], for b < BP and i < KP (the padded
// extents: rows past bt and past k are staged as zeros and written as zeros)
template <int MT>
__global__ __launch_bounds__(256) void lowrank_wide_dot_kernel(const int* __restrict__ gate, const double* __restrict__ B,
                                                               long k, long n, const double* __restrict__ R, int bt,
                                                               long split_cols, double* __restrict__ part, long BP,
                                                               long KP) {
  if (gate != nullptr && *gate == 0) return;
  constexpr int TB = 32 * MT;
  constexpr int RL = TB * LW_KC / 256, BL = LW_TN * LW_KC / 256;
  __shared__ double Rs[TB * LW_STR];     // [b][j]
  __shared__ double Bs[LW_TN * LW_STR];  // [i][j]
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const long b0 = (long)blockIdx.x * TB, i0 = (long)blockIdx.y * LW_TN;
  const long j_begin = (long)blockIdx.z * split_cols;
  const long j_end = j_begin + split_cols < n ? j_begin + split_cols : n;
  LwAcc4 acc[MT][2];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int q = 0; q < 2; ++q) acc[m][q] = LwAcc4{0, 0, 0, 0};
  double rg[RL], bg[BL];
  // 16 consecutive threads read the 16 columns of one row; what lies past the batch, past k or past the split is zero
  auto fetch = [&](long j0) {
    const int jj = t & (LW_KC - 1);
    const long j = j0 + jj;
#pragma unroll
    for (int u = 0; u < RL; ++u) {
      const long b = b0 + (t >> 4) + 16 * u;
      rg[u] = (b < bt && j < j_end) ? R[b * n + j] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < BL; ++u) {
      const long i = i0 + (t >> 4) + 16 * u;
      bg[u] = (i < k && j < j_end) ? B[i * n + j] : 0.0;
    }
  };
  auto stage = [&]() {
    const int jj = t & (LW_KC - 1);
#pragma unroll
    for (int u = 0; u < RL; ++u) Rs[((t >> 4) + 16 * u) * LW_STR + jj] = rg[u];
#pragma unroll
    for (int u = 0; u < BL; ++u) Bs[((t >> 4) + 16 * u) * LW_STR + jj] = bg[u];
  };
  fetch(j_begin);
  stage();
  __syncthreads();
  for (long j0 = j_begin; j0 < j_end; j0 += LW_KC) {
    const bool more = j0 + LW_KC < j_end;
    if (more) fetch(j0 + LW_KC);
#pragma unroll
    for (int ks = 0; ks < LW_KC; ks += 4) {
      double af[MT], bf[2];
#pragma unroll
      for (int m = 0; m < MT; ++m) af[m] = Rs[(wm * 16 * MT + m * 16 + (lane & 15)) * LW_STR + ks + (lane >> 4)];
#pragma unroll
      for (int q = 0; q < 2; ++q) bf[q] = Bs[((2 * q + wn) * 16 + (lane & 15)) * LW_STR + ks + (lane >> 4)];
#pragma unroll
      for (int q = 0; q < 2; ++q)
#pragma unroll
        for (int m = 0; m < MT; ++m) acc[m][q] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[m], bf[q], acc[m][q], 0, 0, 0);
    }
    __syncthreads();  // every wave has read the panels before they are overwritten
    if (more) stage();
    __syncthreads();
  }
  double* __restrict__ o = part + (long)blockIdx.z * BP * KP;
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const long i = i0 + (2 * q + wn) * 16 + (lane & 15);
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const long b = b0 + wm * 16 * MT + m * 16 + (lane >> 4) + 4 * g;
        o[b * KP + i] = acc[m][q][g];  // b < BP and i < KP: the grid covers exactly the padded extents
      }
    }
}

// pass 2: Z[b, j] = dinv[j] R[b, j] - sum_i tt[b, i] B[i, j]; tt [BP, KP] holds zeros past bt and past k.  The
// coefficients are staged 16 at a time, so any k fits
template <int MT>
__global__ __launch_bounds__(256) void lowrank_wide_form_kernel(const int* __restrict__ gate,
                                                                const double* __restrict__ dinv,
                                                                const double* __restrict__ B, long k, long n,
                                                                const double* __restrict__ R, int bt,
                                                                const double* __restrict__ tt, long KP,
                                                                double* __restrict__ Z) {
  if (gate != nullptr && *gate == 0) return;
  constexpr int TB = 32 * MT;
  constexpr int TL = TB * LW_KC / 256, BL = LW_KC * LW_TN / 256;
  __shared__ double Ts[TB * LW_STR];     // [b][i]
  __shared__ double Bs[LW_KC * LW_RS];   // [i][j]
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const long j0 = (long)blockIdx.x * LW_TN, b0 = (long)blockIdx.y * TB;
  LwAcc4 acc[MT][2];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int q = 0; q < 2; ++q) acc[m][q] = LwAcc4{0, 0, 0, 0};
  double tg[TL], bg[BL];
  auto fetch = [&](long i0) {
    // i0 + 15 < KP and b0 + TB <= BP: the padded tt needs no test
#pragma unroll
    for (int u = 0; u < TL; ++u) tg[u] = tt[(b0 + (t >> 4) + 16 * u) * KP + i0 + (t & (LW_KC - 1))];
    const long j = j0 + (t & (LW_TN - 1));
#pragma unroll
    for (int u = 0; u < BL; ++u) {
      const long i = i0 + (t >> 6) + 4 * u;
      bg[u] = (i < k && j < n) ? B[i * n + j] : 0.0;
    }
  };
  auto stage = [&]() {
#pragma unroll
    for (int u = 0; u < TL; ++u) Ts[((t >> 4) + 16 * u) * LW_STR + (t & (LW_KC - 1))] = tg[u];
#pragma unroll
    for (int u = 0; u < BL; ++u) Bs[((t >> 6) + 4 * u) * LW_RS + (t & (LW_TN - 1))] = bg[u];
  };
  fetch(0);
  stage();
  __syncthreads();
  for (long i0 = 0; i0 < k; i0 += LW_KC) {
    const bool more = i0 + LW_KC < k;
    if (more) fetch(i0 + LW_KC);
#pragma unroll
    for (int ks = 0; ks < LW_KC; ks += 4) {
      double af[MT], bf[2];
#pragma unroll
      for (int m = 0; m < MT; ++m) af[m] = Ts[(wm * 16 * MT + m * 16 + (lane & 15)) * LW_STR + ks + (lane >> 4)];
#pragma unroll
      for (int q = 0; q < 2; ++q) bf[q] = Bs[(ks + (lane >> 4)) * LW_RS + (2 * q + wn) * 16 + (lane & 15)];
#pragma unroll
      for (int q = 0; q < 2; ++q)
#pragma unroll
        for (int m = 0; m < MT; ++m) acc[m][q] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[m], bf[q], acc[m][q], 0, 0, 0);
    }
    __syncthreads();
    if (more) stage();
    __syncthreads();
  }
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const long j = j0 + (2 * q + wn) * 16 + (lane & 15);
    if (j >= n) continue;
    const double dv = dinv[j];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const long b = b0 + wm * 16 * MT + m * 16 + (lane >> 4) + 4 * g;
        if (b < bt) Z[b * n + j] = mgp_fma(dv, R[b * n + j], -acc[m][q][g]);
      }
  }
}

// One group of bt <= LW_GROUP rows: the row tile, the padded extents, the split of n and the bytes of its scratch
// (part [ns][BP][KP], then tt [BP][KP]).  About four workgroups per CU, at least LW_MIN_SPLIT columns per split: the
// partials stay under 8 (4 CUs + tiles) LW_TB LW_TN bytes whatever n
struct LwPlan {
  int mt;
  long BP, KP, ns, split_cols;
  size_t bytes;
};
LwPlan lw_plan(const mgp_handle* h, long bt, long k, long n) {
  LwPlan p;
  p.mt = bt <= 32 ? 1 : bt <= 64 ? 2 : 4;
  const long TB = 32L * p.mt;
  p.BP = (bt + TB - 1) / TB * TB;
  p.KP = (k + LW_TN - 1) / LW_TN * LW_TN;
  const long tiles = (p.BP / TB) * (p.KP / LW_TN);
  long ns = (4L * h->num_cus + tiles - 1) / tiles;
  const long max_split = (n + LW_MIN_SPLIT - 1) / LW_MIN_SPLIT;
  if (ns > max_split) ns = max_split;
  if (ns < 1) ns = 1;
  long cols = (n + ns - 1) / ns;
  cols = (cols + LW_KC - 1) / LW_KC * LW_KC;
  p.split_cols = cols;
  p.ns = (n + cols - 1) / cols;
  p.bytes = (size_t)(p.ns + 1) * p.BP * p.KP * sizeof(double);
  return p;
}

int lowrank_wide_apply(mgp_handle* h, const double* dinv, const double* B, long k, long n, const double* R, long Bt,
                       double* Z, const int* gate) {
  // the arena for the widest group: the full groups and the remainder plan differently
  size_t need = 0;
  const long widths[2] = {Bt < LW_GROUP ? Bt : (long)LW_GROUP, Bt > LW_GROUP ? Bt % LW_GROUP : 0};
  for (const long g : widths)
    if (g > 0) {
      const size_t b = lw_plan(h, g, k, n).bytes;
      if (b > need) need = b;
    }
  MGP_TRY(mgp_reserve(h, &h->pch, &h->pch_bytes, need));
  for (long g0 = 0; g0 < Bt; g0 += LW_GROUP) {
    const int bt = (int)(Bt - g0 < LW_GROUP ? Bt - g0 : LW_GROUP);
    const LwPlan p = lw_plan(h, bt, k, n);
    const long total = p.BP * p.KP, TB = 32L * p.mt;
    double* part = (double*)h->pch;
    double* tt = part + p.ns * total;
    const double* Rg = R + g0 * n;
    double* Zg = Z + g0 * n;
    const dim3 g1((unsigned)(p.BP / TB), (unsigned)(p.KP / LW_TN), (unsigned)p.ns);
    const dim3 g2((unsigned)((n + LW_TN - 1) / LW_TN), (unsigned)(p.BP / TB));
#define MGP_LW(MTV)                                                                                                   \
  do {                                                                                                                \
    hipLaunchKernelGGL((lowrank_wide_dot_kernel<MTV>), g1, dim3(256), 0, h->stream, gate, B, k, n, Rg, bt,            \
                       p.split_cols, part, p.BP, p.KP);                                                               \
    MGP_LAUNCH_CHECK(h);                                                                                              \
    hipLaunchKernelGGL((lowrank_sum_kernel<double>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, h->stream,  \
                       gate, (const double*)part, p.ns, total, tt);                                                   \
    MGP_LAUNCH_CHECK(h);                                                                                              \
    hipLaunchKernelGGL((lowrank_wide_form_kernel<MTV>), g2, dim3(256), 0, h->stream, gate, dinv, B, k, n, Rg, bt,     \
                       (const double*)tt, p.KP, Zg);                                                                  \
    MGP_LAUNCH_CHECK(h);                                                                                              \
  } while (0)
    if (p.mt == 1) MGP_LW(1);
    else if (p.mt == 2) MGP_LW(2);
    else MGP_LW(4);
#undef MGP_LW
  }
  return MGP_OK;
}

}  // namespace

// internal: the many-column form (MGP_PRE_LOWRANK_WIDE); fp32 takes the code of MGP_PRE_LOWRANK
int mgp_lowrank_wide_apply_gated(mgp_handle* h, int dtype, const void* diag_inv, const void* B, int64_t k, int64_t n,
                                 const void* R, int64_t Bt, void* Z, const int* gate) {
  if (dtype != MGP_F64) return mgp_lowrank_apply_gated(h, dtype, diag_inv, B, k, n, R, Bt, Z, gate);
  return lowrank_wide_apply(h, (const double*)diag_inv, (const double*)B, k, n, (const double*)R, Bt, (double*)Z, gate);
}

// internal: the gated form the CG loop enqueues (steps past convergence do nothing)
int mgp_lowrank_apply_gated(mgp_handle* h, int dtype, const void* diag_inv, const void* B, int64_t k, int64_t n,
                            const void* R, int64_t Bt, void* Z, const int* gate) {
  return mgp_with_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    return lowrank_apply_t<T>(h, (const T*)diag_inv, (const T*)B, k, n, (const T*)R, Bt, (T*)Z, gate);
  });
}

extern "C" int mgp_lowrank_apply(mgp_handle* h, int dtype, const void* diag_inv, const void* B, int64_t k, int64_t n,
                                 const void* R, int64_t Bt, void* Z) {
  if (!h) return MGP_E_BADARG;
  if (dtype != MGP_F32 && dtype != MGP_F64) return mgp_fail(h, MGP_E_DTYPE, "bad dtype %d", dtype);
  if (k < 1 || n < 0 || Bt < 0) return mgp_fail(h, MGP_E_SHAPE, "low-rank apply needs k >= 1, n >= 0, Bt >= 0");
  if (n == 0 || Bt == 0) return MGP_OK;
  if (!diag_inv || !B || !R || !Z) return mgp_fail(h, MGP_E_BADARG, "NULL data pointer");
  if (R == Z) return mgp_fail(h, MGP_E_BADARG, "low-rank apply is not in place (R == Z)");
  return mgp_lowrank_apply_gated(h, dtype, diag_inv, B, k, n, R, Bt, Z, nullptr);
}

extern "C" int mgp_kxx_pivchol(mgp_handle* h, const mgp_kernel* k, const void* X, int64_t N, int32_t max_rank,
                               double rel_tol, void* L, int64_t* piv, void* diag, int32_t* rank_out) {
  if (!h) return MGP_E_BADARG;
  MGP_TRY(mgp_check_kernel(h, k));
  if (k->dtype != MGP_F64) return mgp_fail(h, MGP_E_DTYPE, "the pivoted Cholesky factor is fp64 only");
  if (N < 0) return mgp_fail(h, MGP_E_SHAPE, "N < 0");
  if (max_rank < 1 || max_rank > PC_MAX_RANK)
    return mgp_fail(h, MGP_E_BADARG, "max_rank=%d outside [1, %d]", max_rank, PC_MAX_RANK);
  if (!(rel_tol >= 0.0)) return mgp_fail(h, MGP_E_BADARG, "rel_tol must be >= 0");
  if (!rank_out) return mgp_fail(h, MGP_E_BADARG, "rank_out is NULL");
  *rank_out = 0;
  if (N == 0) return MGP_OK;
  if (!X || !L || !piv) return mgp_fail(h, MGP_E_BADARG, "NULL data pointer");
  const int kmax = (int64_t)max_rank > N ? (int)N : max_rank;
  // workgroups: slices of a multiple of 256 columns, at most PC_MAX_WG of them
  long slice = (N + PC_MAX_WG - 1) / PC_MAX_WG;
  slice = (slice + PC_NT - 1) / PC_NT * PC_NT;
  const long G = (N + slice - 1) / slice;
  // arena: d [N] | partials 2 x (max, index, sum) [G] | 1/lengthscale [D] | state
  const size_t nd = ((size_t)N + 31) & ~(size_t)31;
  const size_t need = (nd + 6 * (size_t)PC_MAX_WG + MGP_MAX_D) * sizeof(double) + 256;
  MGP_TRY(mgp_reserve(h, &h->pch, &h->pch_bytes, need));
  double* d = (double*)h->pch;
  double* pmx[2] = {d + nd, d + nd + PC_MAX_WG};
  double* psm[2] = {d + nd + 2 * PC_MAX_WG, d + nd + 3 * PC_MAX_WG};
  long* pix[2] = {(long*)(d + nd + 4 * PC_MAX_WG), (long*)(d + nd + 5 * PC_MAX_WG)};
  double* inv_ls = d + nd + 6 * PC_MAX_WG;
  PcState* st = (PcState*)(inv_ls + MGP_MAX_D);
  hipStream_t s = h->stream;
  double host_inv[MGP_MAX_D];
  for (int e = 0; e < k->D; ++e) host_inv[e] = 1.0 / k->lengthscales[e];
  MGP_HIP(h, hipMemcpyAsync(inv_ls, host_inv, (size_t)k->D * sizeof(double), hipMemcpyHostToDevice, s));
  MGP_HIP(h, hipStreamSynchronize(s));  // host_inv is a stack temporary
  hipLaunchKernelGGL(pivchol_init_kernel, dim3((unsigned)G), dim3(PC_NT), 0, s, d, (long)N, slice, k->variance, pmx[0],
                     pix[0], psm[0], st, kmax);
  MGP_LAUNCH_CHECK(h);
  const double stop_sum = rel_tol * (double)N * k->variance;
  for (int i = 0; i < kmax; ++i) {
    const int a = i & 1, b = a ^ 1;
    MGP_TRY(mgp_with_kind(k->kind, [&](auto kind) {
      hipLaunchKernelGGL((pivchol_step_kernel<decltype(kind)::value>), dim3((unsigned)G), dim3(PC_NT), 0, s,
                         (const double*)X, (long)N, k->D, (const double*)inv_ls, k->variance, stop_sum, i, (double*)L, d,
                         (long*)piv, slice, (const double*)pmx[a], (const long*)pix[a], (const double*)psm[a], pmx[b],
                         pix[b], psm[b], st);
      return MGP_OK;
    }));
    MGP_LAUNCH_CHECK(h);
  }
  if (diag) MGP_HIP(h, hipMemcpyAsync(diag, d, (size_t)N * sizeof(double), hipMemcpyDeviceToDevice, s));
  PcState host_st{0, 0};
  MGP_HIP(h, hipMemcpyAsync(h->host_flag, st, sizeof(PcState), hipMemcpyDeviceToHost, s));
  MGP_HIP(h, hipStreamSynchronize(s));
  memcpy(&host_st, h->host_flag, sizeof(PcState));
  *rank_out = host_st.rank;
  return MGP_OK;
}
