// kxx_sym_anyd.hip -- the symmetric self-kernel operator at MGP_FUSED_MAX_D < D <= MGP_MAX_D, fp64
// (MGP_OP_KXX_NOISE_SYM_ANYD, include/mgp.h):  out[Bt, N] = P[Bt, N] (k(X, X) + s2 I)  with every unordered pair of
// rows evaluated once and all right-hand sides of a group of at most 16 contracted in the same pass.
//
// Pack: the scheme of kmm_wide_anyd.hip.  X is packed once per call -- once per solve inside mgp_pcg_solve -- as
//     A row of point i = [ a_1 .. a_D,  |a|^2,  1,  0.. ]      K = 4*KS >= D + 2,  a = x c / l,
// in MFMA fragment order, pack[(tile * KS + ks) * 64 + kq * 16 + l] = A row of point 16 tile + l, column 4 ks + kq; the
// B form of a point (2b_1 .. 2b_D, -1, -|b|^2) is taken from the same pack.  |a|^2 is an fma chain over d ascending.
// Points past N, up to N' = N rounded up to TB, are exact zeros in every column.
//
// Tiles: rows go in blocks of TB = 128 points and the unordered block pairs are dealt as in kxx.hip: tile
// (I, (I + d) mod nb) for d = 0 .. nb/2, for even nb d = nb/2 only for I < nb/2.  A workgroup of four waves keeps
// block I -- two 16-point tiles per wave, as the B operand in registers -- over the DC consecutive d of its chunk and
// streams block J = (I + d) mod nb through LDS in steps of two 16-point tiles.  Distance: that of sweep_anyd.hip,
// v_mfma_f64_16x16x4_f64 with K in slices of 8 k-steps (32 columns), k ascending, one accumulator per pair across the
// slices; mgp_profile<KIND> once after the last slice.
//
// Two contractions per profiled 16 x 16 tile K[i, j] (i streamed, j kept), four MFMAs each:
//   * kept side: result register v of lane l holds K[(l >> 4) + 4 v, l & 15], the B-operand map for tile rows
//     4v .. 4v + 3, so  out^T[c, j] += sum_i P^T[c, i] K[i, j]  takes the tile straight from the result registers;
//     the accumulator is private to the wave and lives across the streamed block and across the d of the chunk;
//   * streamed side: out^T[c, i] += sum_j P^T[c, j] K[i, j] needs the tile the other way round: it is transposed
//     through LDS (a 16 x 17 buffer per tile and wave: 4 ds_write_b64 + 4 ds_read_b64 per lane) and is the B operand
//     of a second set of MFMAs; at the end of a block pair the four waves' accumulators are added in wave order
//     through LDS and stored.
// The diagonal block (d = 0) is evaluated whole and feeds only the kept side, so diagonal pairs count once.  P enters
// as Wt[N'][16] = P^T, zeros past N and past the r live columns of the group: a 16 x 4 operand is one 512-byte run.
//
// Partials, no float atomics: a launch takes S consecutive d in chunks of DC and fills S + ceil(S / DC) slots
// [N'][r] (live columns only): slot dd < S holds the streamed-side sums of d0 + dd (rows of block J, one writer per
// slot and row; zeros where the diagonal or the idle half of d = nb/2 gives none), slot S + ch the kept-side sums of
// chunk ch (rows of block I).  A finish launch adds them in slot order to a running sum [N'][16]; the last one writes
// variance * sum + s2 P.  Two calls give the same bits.  Right-hand sides beyond 16 go in groups of 16 + a remainder.
//
// Plan (sym_plan): nb = ceil(N / TB), nd = nb/2 + 1 values of d; want = min(max(ceil(2 CUs / nb), 1), nd) chunks over
// all d, DC = ceil(nd / want); slots per launch <= maxs = max(2, 2^29 / (8 N' r)) (the bound of kxx.hip):
// DC = min(DC, maxs - 1), S = min(nd, max(1, maxs / (DC + 1)) DC).
//
// Scratch: the kxx arena alone,
//     bytes = align256(8 * 64 * KS * N' / 16) + 2 * align256(8 * 16 * N') + align256(8 * (S + ceil(S / DC)) * N' * r),
// KS = ceil((D + 2) / 4), r = min(Bt, 16): pack, Wt, running sum, slots (S and DC are those of r; with Bt > 16 and a
// remainder Bt mod 16 > 0 the slot term is the larger of the two widths').  c / l_d go through the handle's dparams
// buffer, read by the pack kernel only.
#include "mgp_common.h"

namespace {

using Acc4 = __attribute__((ext_vector_type(4))) double;

constexpr int kSThreads = 256;
constexpr int kSNJ = 2;               // kept 16-point tiles per wave
constexpr int kSTB = 64 * kSNJ;       // points per block
constexpr int kSNI = kSTB / 16;       // 16-point tiles of a streamed block
constexpr int kSNIT = 2;              // streamed tiles per step
constexpr int kSKSL = 8;              // k-steps of 4 per K slice
constexpr int kSCols = 16;            // right-hand sides per group
constexpr int kSTr = 17;              // row stride of a transposed tile / of the wave sums in LDS
constexpr size_t kSSlotBudget = (size_t)1 << 29;  // bytes of slots one launch may fill (kxx.hip's bound)

// pack[(tile * KS + ks) * 64 + kq * 16 + l]: the A row of point i = 16 tile + l at column k = 4 ks + kq; zeros past N
__global__ __launch_bounds__(256) void sym_anyd_pack_kernel(const double* __restrict__ X, long N, long npad, int D,
                                                            int KS, const double* __restrict__ sc,
                                                            double* __restrict__ pack, const int* __restrict__ gate) {
  if (gate != nullptr && *gate == 0) return;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= npad) return;
  double* row = pack + (i >> 4) * (long)KS * 64 + (i & 15);
  if (i >= N) {
    for (int k = 0; k < 4 * KS; ++k) row[(k >> 2) * 64 + (k & 3) * 16] = 0.0;
    return;
  }
  double s = 0;
  for (int d = 0; d < D; ++d) {
    const double v = X[i * D + d] * sc[d];
    s = mgp_fma(v, v, s);
    row[(d >> 2) * 64 + (d & 3) * 16] = v;
  }
  for (int k = D; k < 4 * KS; ++k) row[(k >> 2) * 64 + (k & 3) * 16] = k == D ? s : (k == D + 1 ? 1.0 : 0.0);
}

// Wt[i][c] = P[c][i] for i < N and c < r, zeros up to npad and up to 16 columns
__global__ __launch_bounds__(256) void sym_anyd_weights_kernel(const double* __restrict__ P, long N, long npad, int r,
                                                               double* __restrict__ Wt, const int* __restrict__ gate) {
  if (gate != nullptr && *gate == 0) return;
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= npad * kSCols) return;
  const long i = e / kSCols;
  const int c = (int)(e - i * kSCols);
  Wt[e] = (i < N && c < r) ? P[(long)c * N + i] : 0.0;
}

template <int KIND>
__global__ __launch_bounds__(kSThreads) void kxx_sym_anyd_kernel(const double* __restrict__ pack,
                                                                 const double* __restrict__ Wt, long nbk, long d0,
                                                                 int nd, int dc, int D, int r,
                                                                 double* __restrict__ slots, long slot_stride, int S,
                                                                 double clamp, const int* __restrict__ gate) {
  if (gate != nullptr && *gate == 0) return;
  constexpr int TRT = 16 * kSTr;  // doubles of one transposed tile
  __shared__ __attribute__((aligned(16))) double frag[kSNIT * kSKSL * 64];  // one K slice of the streamed step
  // transposed tiles [wave][it][jt][16 x 17]; at the end of a block pair the waves' sums [TB][17] stand here instead
  __shared__ double scr[4 * kSNIT * kSNJ * TRT];
  __shared__ double e2tab[MGP_EXP2_TAB_SIZE];
  static_assert(4 * kSNIT * kSNJ * TRT >= kSTB * kSTr, "the wave sums fit the transpose buffers");
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int l15 = lane & 15, kq = lane >> 4;
  for (int e = t; e < MGP_EXP2_TAB_SIZE; e += kSThreads) e2tab[e] = mgp_exp2_tab_entry(e);
  const E2Tab<true> e2{e2tab};

  const int KS = (D + 2 + 3) >> 2;
  const long I = blockIdx.x;
  const int ch = blockIdx.y;
  const int dd0 = ch * dc, dd1 = dd0 + dc < nd ? dd0 + dc : nd;
  const long otile = I * kSNI + wave * kSNJ;  // this wave's first kept tile
  const double* own = pack + otile * KS * 64;
  // the kept points' right-hand sides as the A operand of the streamed-side contraction: P[c = l15][j = 4 kk + kq]
  double pw[kSNJ][4];
#pragma unroll
  for (int jt = 0; jt < kSNJ; ++jt)
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) pw[jt][kk] = Wt[((otile + jt) * 16 + 4 * kk + kq) * kSCols + l15];

  Acc4 accO[kSNJ];
#pragma unroll
  for (int jt = 0; jt < kSNJ; ++jt) accO[jt] = Acc4{0, 0, 0, 0};
  double* trw = scr + wave * (kSNIT * kSNJ * TRT);

  for (int dd = dd0; dd < dd1; ++dd) {
    const long dist = d0 + dd;
    const long J = (I + dist) % nbk;
    const bool diag = dist == 0;
    const bool idle = !diag && 2 * dist == nbk && I >= nbk / 2;  // that block pair is the tile of workgroup J
    double* st = slots + (long)dd * slot_stride + J * kSTB * r;  // streamed-side sums of this d: rows of block J
    if (diag || idle)
      for (int e = t; e < kSTB * r; e += kSThreads) st[e] = 0.0;
    if (idle) continue;

    Acc4 accS[kSNI];
#pragma unroll
    for (int it = 0; it < kSNI; ++it) accS[it] = Acc4{0, 0, 0, 0};

#pragma unroll
    for (int stp = 0; stp < kSNI / kSNIT; ++stp) {
      const long itile = J * kSNI + stp * kSNIT;  // first streamed tile of the step
      // the streamed points' right-hand sides as the A operand of the kept-side contraction: P[c = l15][i = 4 v + kq]
      double pa[kSNIT][4];
#pragma unroll
      for (int it = 0; it < kSNIT; ++it)
#pragma unroll
        for (int v = 0; v < 4; ++v) pa[it][v] = Wt[((itile + it) * 16 + 4 * v + kq) * kSCols + l15];

      Acc4 c[kSNIT][kSNJ];
#pragma unroll
      for (int it = 0; it < kSNIT; ++it)
#pragma unroll
        for (int jt = 0; jt < kSNJ; ++jt) c[it][jt] = Acc4{0, 0, 0, 0};

      for (int s0 = 0; s0 < KS; s0 += kSKSL) {
        const int nks = KS - s0 < kSKSL ? KS - s0 : kSKSL;
        // the kept operands of this slice: B form of this wave's tiles
        double bf[kSNJ][kSKSL];
#pragma unroll
        for (int jt = 0; jt < kSNJ; ++jt)
#pragma unroll
          for (int ks = 0; ks < kSKSL; ++ks) {
            bf[jt][ks] = 0.0;
            if (ks < nks) {
              const int k = 4 * (s0 + ks) + kq;
              const double* o = own + (long)jt * KS * 64;
              // column D + 1 holds -|b|^2: |b|^2 stands in column D of the A form
              const double v = k == D + 1 ? o[(long)(D >> 2) * 64 + (D & 3) * 16 + l15] : o[(long)(s0 + ks) * 64 + lane];
              bf[jt][ks] = k < D ? v + v : (k == D ? -1.0 : (k == D + 1 ? -v : 0.0));
            }
          }
        __syncthreads();  // the previous slice's fragments, and the previous step's transposed tiles, fully consumed
        // streamed A fragments of the slice: a flat copy, kSNIT tiles x nks k-steps x 64
        for (int e = t; e < kSNIT * kSKSL * 64; e += kSThreads) {
          const int it = e / (kSKSL * 64), rem = e - it * (kSKSL * 64), ks = rem >> 6;
          if (ks < nks) frag[e] = pack[((itile + it) * KS + s0 + ks) * 64 + (rem & 63)];
        }
        __syncthreads();
#pragma unroll
        for (int ks = 0; ks < kSKSL; ++ks)
          if (ks < nks) {
#pragma unroll
            for (int it = 0; it < kSNIT; ++it) {
              const double af = frag[(it * kSKSL + ks) * 64 + lane];
#pragma unroll
              for (int jt = 0; jt < kSNJ; ++jt)
                c[it][jt] = __builtin_amdgcn_mfma_f64_16x16x4f64(af, bf[jt][ks], c[it][jt], 0, 0, 0);
            }
          }
      }

      // ---- the profile once per pair; the tile as the B operand of the kept side; its transpose into LDS
#pragma unroll
      for (int it = 0; it < kSNIT; ++it)
#pragma unroll
        for (int jt = 0; jt < kSNJ; ++jt) {
          Acc4 kv;
#pragma unroll
          for (int v = 0; v < 4; ++v) kv[v] = mgp_profile<KIND, double, E2Tab<true>>(c[it][jt][v], clamp, e2);
#pragma unroll
          for (int v = 0; v < 4; ++v)  // tile rows 4v .. 4v + 3, ascending: the order of every output's chain
            accO[jt] = __builtin_amdgcn_mfma_f64_16x16x4f64(pa[it][v], kv[v], accO[jt], 0, 0, 0);
          if (!diag) {
            double* tr = trw + (it * kSNJ + jt) * TRT;
#pragma unroll
            for (int v = 0; v < 4; ++v) tr[(kq + 4 * v) * kSTr + l15] = kv[v];  // [i][j]
          }
        }
      if (!diag) {  // workgroup-uniform
        __syncthreads();
#pragma unroll
        for (int it = 0; it < kSNIT; ++it)
#pragma unroll
          for (int jt = 0; jt < kSNJ; ++jt) {
            const double* tr = trw + (it * kSNJ + jt) * TRT;
#pragma unroll
            for (int kk = 0; kk < 4; ++kk)  // B[k = j = 4 kk + kq][column i = l15]
              accS[stp * kSNIT + it] = __builtin_amdgcn_mfma_f64_16x16x4f64(pw[jt][kk], tr[l15 * kSTr + 4 * kk + kq],
                                                                            accS[stp * kSNIT + it], 0, 0, 0);
          }
      }
    }

    if (!diag) {
      // the four waves' sums of block J, added in wave order: register v of lane l holds column kq + 4 v, row l15
      for (int w = 0; w < 4; ++w) {
        __syncthreads();
        if (wave == w) {
#pragma unroll
          for (int it = 0; it < kSNI; ++it)
#pragma unroll
            for (int v = 0; v < 4; ++v) {
              double* p = &scr[(it * 16 + l15) * kSTr + kq + 4 * v];
              *p = w == 0 ? accS[it][v] : *p + accS[it][v];
            }
        }
      }
      __syncthreads();
      for (int e = t; e < kSTB * r; e += kSThreads) {
        const int il = e / r, cc = e - il * r;
        st[e] = scr[il * kSTr + cc];
      }
    }
  }

  // kept-side sums of the chunk: slot S + ch, rows of block I, live columns only
  double* sd = slots + (long)(S + ch) * slot_stride + otile * 16 * r;
#pragma unroll
  for (int jt = 0; jt < kSNJ; ++jt)
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int cc = kq + 4 * v;
      if (cc < r) sd[(jt * 16 + l15) * r + cc] = accO[jt][v];
    }
}

// sum(i, c) (+)= slots 0 .. nd-1, then S .. S+nch-1, in that order; the last launch writes
// out[c, i] = variance * sum + s2 * P[c, i]
__global__ __launch_bounds__(256) void kxx_sym_anyd_finish_kernel(const double* __restrict__ slots, long slot_stride,
                                                                  int S, int nd, int nch, double* __restrict__ sum,
                                                                  int first, int last, long N, int r, double variance,
                                                                  double s2, const double* __restrict__ P,
                                                                  double* __restrict__ out,
                                                                  const int* __restrict__ gate) {
  if (gate != nullptr && *gate == 0) return;
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= N * r) return;
  double s = first ? 0.0 : sum[e];
  for (int k = 0; k < nd; ++k) s += slots[k * slot_stride + e];
  for (int k = 0; k < nch; ++k) s += slots[(S + k) * slot_stride + e];
  if (!last) {
    sum[e] = s;
    return;
  }
  const long i = e / r, c = e - i * r;
  out[c * N + i] = mgp_fma(s2, P[c * N + i], variance * s);
}

struct SymPlan {
  long nbk, npad, nd_total;
  int S, dc;
};

inline SymPlan sym_plan(long N, int r, int num_cus) {
  SymPlan p;
  p.nbk = (N + kSTB - 1) / kSTB;
  p.npad = p.nbk * kSTB;
  p.nd_total = p.nbk / 2 + 1;
  long want = (2L * num_cus + p.nbk - 1) / p.nbk;
  want = want < 1 ? 1 : (want > p.nd_total ? p.nd_total : want);
  long dc = (p.nd_total + want - 1) / want;
  long maxs = (long)(kSSlotBudget / ((size_t)p.npad * r * sizeof(double)));
  maxs = maxs < 2 ? 2 : (maxs > 32768 ? 32768 : maxs);
  if (dc > maxs - 1) dc = maxs - 1;
  long cpl = maxs / (dc + 1);
  cpl = cpl < 1 ? 1 : cpl;
  const long s = cpl * dc;
  p.S = (int)(s < p.nd_total ? s : p.nd_total);
  p.dc = (int)dc;
  return p;
}

inline size_t sym_align(size_t b) { return (b + 255) & ~(size_t)255; }
inline int sym_ks(int D) { return (D + 2 + 3) >> 2; }
inline size_t sym_pack_bytes(long npad, int D) { return sym_align((size_t)(npad / 16) * sym_ks(D) * 64 * sizeof(double)); }
inline size_t sym_wt_bytes(long npad) { return sym_align((size_t)npad * kSCols * sizeof(double)); }
inline size_t sym_slot_bytes(const SymPlan& pl, int r) {
  return sym_align((size_t)(pl.S + (pl.S + pl.dc - 1) / pl.dc) * pl.npad * r * sizeof(double));
}
// pack | Wt | running sum | slots: the larger need of the call's two group widths (a narrow remainder takes more d per
// launch and may fill more of the budget than the full groups do)
size_t sym_arena_bytes(const mgp_handle* h, long N, int D, long Bt) {
  const int r = (int)(Bt < kSCols ? Bt : kSCols), rem = Bt > kSCols ? (int)(Bt % kSCols) : 0;
  const SymPlan pl = sym_plan(N, r, h->num_cus);
  size_t sb = sym_slot_bytes(pl, r);
  if (rem > 0) {
    const size_t sr = sym_slot_bytes(sym_plan(N, rem, h->num_cus), rem);
    sb = sr > sb ? sr : sb;
  }
  return sym_pack_bytes(pl.npad, D) + 2 * sym_wt_bytes(pl.npad) + sb;
}

template <int KIND>
int kxx_sym_anyd_run(mgp_handle* h, const mgp_kernel* k, long N, double s2, const double* P, long Bt, double* out,
                     const int* gate) {
  const int D = k->D;
  const double c = mgp_profile_scale(k->kind);
  const double clamp = c * c * 1e-36;
  const long npad = (N + kSTB - 1) / kSTB * kSTB;
  char* base = (char*)h->kxx;
  const double* pack = (const double*)base;
  double* Wt = (double*)(base + sym_pack_bytes(npad, D));
  double* sum = (double*)(base + sym_pack_bytes(npad, D) + sym_wt_bytes(npad));
  double* slots = (double*)(base + sym_pack_bytes(npad, D) + 2 * sym_wt_bytes(npad));
  for (long g0 = 0; g0 < Bt; g0 += kSCols) {
    const int r = (int)(Bt - g0 < kSCols ? Bt - g0 : kSCols);
    const SymPlan pl = sym_plan(N, r, h->num_cus);
    if (pl.nbk > 2147483647L) return mgp_fail(h, MGP_E_SHAPE, "symmetric any-D operator: grid too large");
    const double* Pg = P + g0 * N;
    double* og = out + g0 * N;
    hipLaunchKernelGGL(sym_anyd_weights_kernel, dim3((unsigned)((npad * kSCols + 255) / 256)), dim3(256), 0, h->stream,
                       Pg, N, npad, r, Wt, gate);
    MGP_LAUNCH_CHECK(h);
    const long slot_stride = npad * r;
    for (long d0 = 0; d0 < pl.nd_total; d0 += pl.S) {
      const int nd = (int)(pl.nd_total - d0 < pl.S ? pl.nd_total - d0 : pl.S);
      const int nch = (nd + pl.dc - 1) / pl.dc;
      hipLaunchKernelGGL((kxx_sym_anyd_kernel<KIND>), dim3((unsigned)pl.nbk, (unsigned)nch), dim3(kSThreads), 0,
                         h->stream, pack, (const double*)Wt, pl.nbk, d0, nd, pl.dc, D, r, slots, slot_stride, pl.S, clamp,
                         gate);
      MGP_LAUNCH_CHECK(h);
      hipLaunchKernelGGL(kxx_sym_anyd_finish_kernel, dim3((unsigned)((N * r + 255) / 256)), dim3(256), 0, h->stream,
                         (const double*)slots, slot_stride, pl.S, nd, nch, sum, (int)(d0 == 0),
                         (int)(d0 + nd >= pl.nd_total), N, r, k->variance, s2, Pg, og, gate);
      MGP_LAUNCH_CHECK(h);
    }
  }
  return MGP_OK;
}

}  // namespace

bool mgp_kxx_sym_anyd_serves(const mgp_kernel* k) {
  return k != nullptr && k->dtype == MGP_F64 && k->D > MGP_FUSED_MAX_D;
}

int mgp_kxx_sym_anyd_prepare(mgp_handle* h, const mgp_kernel* k, const void* X, int64_t N, int64_t Bt,
                             const int* gate) {
  MGP_TRY(mgp_reserve(h, &h->kxx, &h->kxx_bytes, sym_arena_bytes(h, N, k->D, Bt)));
  double host[MGP_MAX_D];
  const double c = mgp_profile_scale(k->kind);
  for (int d = 0; d < k->D; ++d) host[d] = c / k->lengthscales[d];
  MGP_HIP(h, hipMemcpyAsync(h->dparams, host, (size_t)k->D * sizeof(double), hipMemcpyHostToDevice, h->stream));
  MGP_HIP(h, hipStreamSynchronize(h->stream));  // host[] is a stack temporary
  const long npad = (N + kSTB - 1) / kSTB * kSTB;
  hipLaunchKernelGGL(sym_anyd_pack_kernel, dim3((unsigned)((npad + 255) / 256)), dim3(256), 0, h->stream,
                     (const double*)X, (long)N, npad, k->D, sym_ks(k->D), (const double*)h->dparams, (double*)h->kxx,
                     gate);
  MGP_LAUNCH_CHECK(h);
  return MGP_OK;
}

// out[Bt, N] = P[Bt, N] (k(X, X) + s2 I): mgp_kxx's checks; this file's kernels where they serve, else mgp_kxx itself
int mgp_kxx_sym_anyd(mgp_handle* h, const mgp_kernel* k, const void* X, int64_t N, double s2, const void* P,
                     int64_t Bt, void* out, const int* gate) {
  if (!mgp_kxx_sym_anyd_serves(k))
    return mgp_kxx(h, k, X, N, s2, VecView{P, 1, N}, (int)Bt, VecViewMut{out, 1, N}, gate);
  MGP_TRY(mgp_check_kernel(h, k));
  if (N < 0 || Bt < 0) return mgp_fail(h, MGP_E_SHAPE, "negative size");
  if (N == 0 || Bt == 0) return MGP_OK;
  if (!X || !P || !out) return mgp_fail(h, MGP_E_BADARG, "NULL data pointer");
  if (!(s2 >= 0.0)) return mgp_fail(h, MGP_E_BADARG, "s2 must be >= 0");
  if (h->sym_pack_src == X && h->sym_pack_n == N) {  // inside a solve: packed before its loop, the arena sized there
    if (sym_arena_bytes(h, N, k->D, Bt) > h->kxx_bytes)
      return mgp_fail(h, MGP_E_NOMEM, "symmetric any-D operator: %lld right-hand sides do not fit the arena reserved for the solve",
                      (long long)Bt);
  } else {
    MGP_TRY(mgp_kxx_sym_anyd_prepare(h, k, X, N, Bt, gate));
  }
  return mgp_with_kind(k->kind, [&](auto kind) {
    return kxx_sym_anyd_run<decltype(kind)::value>(h, k, N, s2, (const double*)P, Bt, (double*)out, gate);
  });
}
