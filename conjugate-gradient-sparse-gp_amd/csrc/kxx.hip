// kxx.hip -- symmetric matrix-free self-kernel product: out[N,R] = (k(X,X) + s2 I) V, each unordered pair once.
//
// The fused sweep (sweep.hip) evaluates k(x_i, x_j) and k(x_j, x_i) separately when it is handed Z = X, and it is
// bound by fp64 VALU issue.  Here rows are cut into blocks of TB points (TB = 256 threads x RPT owned points per
// lane) and every unordered block pair {I, J} is one workgroup's tile:
//   * the workgroup owns the TB rows of block I in registers (read from the packed set) and streams the TB points of
//     block J by scalar loads, as the fast sweep streams its points;
//   * each evaluated k(x_i, x_j) feeds the owned row directly (acc_i += k v_j) and the streamed point through a
//     per-lane column partial c_j = sum_q k(x_iq, x_j) v_iq, which each 16-lane DPP row sums on the VALU; one lane per
//     row leaves it in LDS, and every G streamed points the 16 row sums are added in row order and stored;
//   * the diagonal tile (I, I) is evaluated whole and feeds the owned rows only, so diagonal pairs count once.
// Block pairs are dealt cyclically, tile (I, (I + d) mod nb) for d = 0 .. nb/2 (for even nb, d = nb/2 only for
// I < nb/2): every d gives nb tiles whose owned blocks and streamed blocks are both a permutation of the blocks.  A
// launch takes S consecutive d and writes 2 S slots [N', RC] (the direct and the transposed partial of each d, one
// writer per slot and row); a reduce launch adds them in slot order to a running sum [N', RC], the last one writes
// variance * sum + s2 v.  Fixed order throughout: deterministic, no float atomics, O(N R) scratch (mgp.h states the bound).
//
// Per evaluated pair (SE): D fma + the table exp2 of the fast sweep (2048 entries; 3 add, 2 fma, mul, fma and 3
// integer) + 1 fma (direct) + 1 fma (transposed); the row sum (4 x (2 DPP moves + add) per column) is spread over
// the 64 RPT pairs of a wave and point.  The plain sweep spends D + 8 fp64 + 2..3 integer on each ORDERED pair.
#include <type_traits>

#include "mgp_common.h"

namespace {

constexpr int kKxxThreads = 256;
constexpr size_t kKxxSlotBudget = (size_t)1 << 29;  // bytes of slots one launch may fill (mgp.h)
constexpr long kKxxPad = 1024;                      // the packed set is padded to a multiple of every TB

template <int DP, int RC>
struct KxxCfg {
  static constexpr int RPT = (RC == 1 && DP <= 8) ? 4 : ((DP <= 8 || (DP <= 16 && RC <= 4)) ? 2 : 1);
  static constexpr int TB = kKxxThreads * RPT;
  static constexpr int G = RC >= 4 ? 16 : 64 / RC;  // streamed points between two stores of the column sums (LDS: 2 x 16 x G x RC doubles)
};

// sum of v over the 16 lanes of each DPP row, left in every lane of the row: four DPP moves of both halves + adds, all
// on the VALU (a ds_bpermute butterfly put 12 LDS instructions per column and point on the CU's shared LDS pipe and
// bound the product there).  Within a row every lane adds the same values in a lane-dependent order; the caller reads
// one fixed lane per row, so the result is the same from run to run.
template <int CTRL>
__device__ __forceinline__ double kxx_dpp(double v) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xf, 0xf, false);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xf, 0xf, false);
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double kxx_row_sum(double v) {
  v += kxx_dpp<0xb1>(v);   // quad_perm [1,0,3,2]
  v += kxx_dpp<0x4e>(v);   // quad_perm [2,3,0,1]: the quad's sum
  v += kxx_dpp<0x124>(v);  // row_ror:4
  v += kxx_dpp<0x128>(v);  // row_ror:8: the row's sum
  return v;
}

// P[j] = (2 x_j c/l, -|x_j c/l|^2) for j < N, zeros up to npad (the pad rows carry zero weights as well);
// bmax = bit pattern of max |x c/l|^2 (NaN above everything), as pack_points_kernel of sweep.hip
template <int DP>
__global__ __launch_bounds__(256) void kxx_pack_kernel(const double* __restrict__ X, long N, long npad, int D,
                                                       SweepParams prm, double* __restrict__ P,
                                                       unsigned long long* __restrict__ bmax_bits,
                                                       const int* __restrict__ gate) {
  if (gate != nullptr && *gate == 0) return;
  const long j = (long)blockIdx.x * 256 + threadIdx.x;
  double s = 0;
  if (j < npad) {
    double* p = P + j * (DP + 1);
    if (j < N) {
#pragma unroll
      for (int d = 0; d < DP; ++d) {
        const double v = d < D ? X[j * D + d] * prm.inv_ls[d] : 0.0;
        s = mgp_fma(v, v, s);
        p[d] = v + v;
      }
      p[DP] = -s;
    } else {
#pragma unroll
      for (int d = 0; d <= DP; ++d) p[d] = 0.0;
    }
  }
  unsigned long long bits = __builtin_bit_cast(unsigned long long, s) & 0x7fffffffffffffffULL;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long o = __shfl_xor(bits, off, 64);
    bits = o > bits ? o : bits;
  }
  if ((threadIdx.x & 63) == 0 && bits > __hip_atomic_load(bmax_bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
    atomicMax(bmax_bits, bits);
}

// Wt[j][r] = V(j, r) for j < N, 0 up to npad
template <typename T>
__global__ __launch_bounds__(256) void kxx_weights_kernel(const T* __restrict__ V, long v_si, long v_sr, long N,
                                                          long npad, int RC, T* __restrict__ Wt,
                                                          const int* __restrict__ gate) {
  if (gate != nullptr && *gate == 0) return;
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= npad * RC) return;
  const long j = e / RC, r = e - j * RC;
  Wt[e] = j < N ? V[j * v_si + r * v_sr] : (T)0;
}

template <int DP, int KIND, int RC>
__global__ __launch_bounds__(kKxxThreads) void kxx_tile_kernel(const double* __restrict__ P,
                                                               const double* __restrict__ Wt, long nbk, long d0,
                                                               double* __restrict__ slots, long slot_stride, int S,
                                                               const unsigned long long* __restrict__ bmax_bits,
                                                               SweepParams prm, const double* __restrict__ gtab,
                                                               const int* __restrict__ gate) {
  if (gate != nullptr && *gate == 0) return;
  constexpr int RPT = KxxCfg<DP, RC>::RPT, TB = KxxCfg<DP, RC>::TB, NT = kKxxThreads, NROW = NT / 16;
  constexpr int kKxxGroup = KxxCfg<DP, RC>::G;
  constexpr double MAGIC = 0x1.8p+41;  // 2048-entry table: low word of t + MAGIC = round(2048 t)
  constexpr double kTLimit = 1000.0, kNormLimit = KIND == 0 ? kTLimit : kTLimit * kTLimit;
  // The clamped loop writes its exact 0 only below t = -1020: the exponent add on the high word stays normal down to
  // t = -1022, and a Matern-5/2 value is its polynomial (2^17 at q = 1000) times 2^t, so a cut at -1000 dropped values
  // of up to variance * 2^-983 that the ldexp forms return (tests/test_gpu_pair_accuracy.py, the flush floor 2^-990).
  constexpr double kFlushLimit = 1020.0;
  __shared__ double e2tab[MGP_EXP2_TAB_SIZE];
  __shared__ double cb[2][NROW][kKxxGroup][RC];  // per-row column sums of a group of streamed points, two buffers

  const long I = blockIdx.x % nbk, dd = blockIdx.x / nbk, dist = d0 + dd;
  const long J = (I + dist) % nbk;
  const bool diag = dist == 0;
  const bool idle = !diag && 2 * dist == nbk && I >= nbk / 2;  // that block pair is the tile of workgroup J
  const bool trans = !diag && !idle;
  double* sdir = slots + dd * slot_stride;        // direct partial of this d: rows of block I
  double* str = slots + (S + dd) * slot_stride;   // transposed partial of this d: rows of block J
  const int t = threadIdx.x, lane16 = t & 15, row = t >> 4;

  typedef double d2 __attribute__((ext_vector_type(2)));
  for (int e = 2 * t; e < MGP_EXP2_TAB_SIZE; e += 2 * NT)
    *reinterpret_cast<d2*>(&e2tab[e]) = *reinterpret_cast<const d2*>(gtab + e);

  // owned rows: a = (2a)/2 exactly, |a|^2 from the pack (the same fma chain the sweep forms)
  double a[RPT][DP], cq[RPT], acc[RPT][RC], vown[RPT][RC];
#pragma unroll
  for (int q = 0; q < RPT; ++q) {
    const long i = I * TB + q * NT + t;
    const double* p = P + i * (DP + 1);
#pragma unroll
    for (int d = 0; d < DP; ++d) a[q][d] = 0.5 * p[d];
    const double a2 = -p[DP];
    cq[q] = KIND == 0 ? MAGIC - a2 : a2;
    // SE: the sums carry 2^(-rho), rho = (MAGIC - cq) - |a|^2 (what rounding MAGIC - |a|^2 dropped): the owned
    // weights take the 2^rho of their row here, the direct sums at the store
    const double rho = KIND == 0 ? mgp_exp2((MAGIC - cq[q]) - a2) : 1.0;
#pragma unroll
    for (int r = 0; r < RC; ++r) {
      vown[q][r] = Wt[i * RC + r] * rho;
      acc[q][r] = 0;
    }
  }
  __syncthreads();  // table
  const double bb = __builtin_bit_cast(double, *bmax_bits);
  const bool safe = 4.0 * bb < kNormLimit;  // 2 (|a|^2 + |b|^2) over the whole set; NaN compares false
  const double C1 = 0x1.62e42fefa39efp-1, C2 = 0x1.ebfbdff82c58fp-3, C3 = 0x1.c6b08d704a0c0p-5;  // ln2^k / k!
  const double floor_r2 = prm.clamp;
  typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
  const char* tab_bytes = (const char*)e2tab;

  // kernel values of one streamed point against the RPT owned rows: the arithmetic of sweep_fast_kernel's finish
  // (2048-entry table), 2^t up to the SE 2^(-rho) of the owned row
  auto values = [&](auto clamp_tag, const double (&sv)[RPT], double (&kv)[RPT]) {
    constexpr bool CLAMP = decltype(clamp_tag)::value;
    double g[RPT], tq[RPT], qv[KIND == 0 ? 1 : RPT];
    unsigned ex[RPT];
    bool under[RPT];
#pragma unroll
    for (int q = 0; q < RPT; ++q) {
      double u, gg;
      bool low = false;
      if (KIND == 0) {
        const double s = sv[q];
        u = s + cq[q];
        if (CLAMP) {
          const double cmin = MAGIC - kFlushLimit;
          low = u < cmin;
          u = low ? cmin : u;
        }
        gg = s - (u - cq[q]);
      } else {
        double r2 = -sv[q];
        r2 = CLAMP ? (r2 < floor_r2 ? floor_r2 : r2) : __builtin_fmax(r2, floor_r2);
        double qq = mgp_sqrt_pos(r2);
        if (CLAMP) {
          low = qq > kFlushLimit;
          qq = low ? kFlushLimit : qq;
        }
        qv[KIND == 0 ? 0 : q] = qq;
        u = MAGIC - qq;
        gg = -qq - (u - MAGIC);
      }
      under[q] = low;
      const unsigned m = __builtin_bit_cast(u32x2, u).x;
      g[q] = (KIND == 0 && CLAMP) ? (low ? 0.0 : gg) : gg;
      unsigned off;
      asm("v_lshlrev_b32 %0, 3, %1\n\tv_and_b32 %0, 0x3ff8, %0" : "=&v"(off) : "v"(m));
      ex[q] = m;
      tq[q] = *(const double*)(tab_bytes + off);
    }
    double pq[RPT];
#pragma unroll
    for (int q = 0; q < RPT; ++q) pq[q] = mgp_fma(g[q], C3, C2);
#pragma unroll
    for (int q = 0; q < RPT; ++q) pq[q] = mgp_fma(pq[q], g[q], C1);
#pragma unroll
    for (int q = 0; q < RPT; ++q) pq[q] = pq[q] * g[q];
#pragma unroll
    for (int q = 0; q < RPT; ++q) {
      u32x2 tb = __builtin_bit_cast(u32x2, tq[q]);
      asm("v_lshl_add_u32 %0, %1, 9, %0" : "+v"(tb.y) : "v"(ex[q]));  // hi(T') + (m << 9) = hi(T) + (n << 20)
      const double T2 = __builtin_bit_cast(double, tb);
      double k = mgp_fma(T2, pq[q], T2);
      if (KIND == 2) k *= mgp_fma(qv[KIND == 0 ? 0 : q], MGP_LN2, 1.0);
      if (KIND == 3) {
        const double qq = qv[KIND == 0 ? 0 : q];
        k *= mgp_fma(mgp_fma(qq, MGP_LN2 * MGP_LN2 / 3.0, MGP_LN2), qq, 1.0);
      }
      if (CLAMP) k = under[q] ? 0.0 : k;
      kv[q] = k;
    }
  };

  auto tile = [&](auto clamp_tag, auto trans_tag) {
    constexpr bool TRANS = decltype(trans_tag)::value;
    const double* rp = P + J * TB * (DP + 1);
    const double* wp = Wt + J * TB * RC;
    double b[DP], nb2, w[RC];
    auto load = [&](const double* r, const double* wq) {
#pragma unroll
      for (int d = 0; d < DP; ++d) b[d] = r[d];
      nb2 = r[DP];
#pragma unroll
      for (int c = 0; c < RC; ++c) w[c] = wq[c];
    };
    load(rp, wp);
    for (int g0 = 0; g0 < TB; g0 += kKxxGroup) {
      const int buf = (g0 / kKxxGroup) & 1;
      for (int jl = 0; jl < kKxxGroup; ++jl) {
        double sv[RPT];
#pragma unroll
        for (int q = 0; q < RPT; ++q) {
          double s = KIND == 0 ? nb2 : nb2 - cq[q];
#pragma unroll
          for (int d = 0; d < DP; ++d) s = mgp_fma(a[q][d], b[d], s);
          sv[q] = s;
        }
        double wc[RC];
#pragma unroll
        for (int c = 0; c < RC; ++c) wc[c] = w[c];
        const bool more = g0 + jl + 1 < TB;
        rp = more ? rp + (DP + 1) : rp;
        wp = more ? wp + RC : wp;
        __builtin_amdgcn_sched_barrier(0);  // the row is consumed: request the next one now
        load(rp, wp);
        __builtin_amdgcn_sched_barrier(0);
        double kv[RPT];
        values(clamp_tag, sv, kv);
#pragma unroll
        for (int q = 0; q < RPT; ++q)
#pragma unroll
          for (int r = 0; r < RC; ++r) acc[q][r] = mgp_fma(kv[q], wc[r], acc[q][r]);
        if constexpr (TRANS) {
#pragma unroll
          for (int r = 0; r < RC; ++r) {
            double c = kv[0] * vown[0][r];
#pragma unroll
            for (int q = 1; q < RPT; ++q) c = mgp_fma(kv[q], vown[q][r], c);
            c = kxx_row_sum(c);
            if (lane16 == 0) cb[buf][row][jl][r] = c;
          }
        }
      }
      if constexpr (TRANS) {
        __syncthreads();  // this group's row sums are in; the other buffer was read before the previous barrier
        for (int e = t; e < kKxxGroup * RC; e += NT) {
          const int jl = e / RC, r = e - jl * RC;
          double s = cb[buf][0][jl][r];
#pragma unroll
          for (int rw = 1; rw < NROW; ++rw) s += cb[buf][rw][jl][r];
          str[(J * TB + g0) * RC + e] = s;
        }
      }
    }
  };
  if (trans) {
    if (safe) tile(std::false_type{}, std::true_type{});
    else tile(std::true_type{}, std::true_type{});
  } else {
    if (!idle) {
      if (safe) tile(std::false_type{}, std::false_type{});
      else tile(std::true_type{}, std::false_type{});
    }
    // no transposed partial from this tile: its slot rows are zero (diagonal: block I; idle: block J)
    for (int e = t; e < TB * RC; e += NT) str[J * TB * RC + e] = 0.0;
  }
#pragma unroll
  for (int q = 0; q < RPT; ++q) {
    const long i = I * TB + q * NT + t;
    double rho = 1.0;
    if (KIND == 0) {
      const double a2 = -P[i * (DP + 1) + DP];
      rho = mgp_exp2((MAGIC - cq[q]) - a2);
    }
#pragma unroll
    for (int r = 0; r < RC; ++r) sdir[i * RC + r] = acc[q][r] * rho;
  }
}

// sum(i, r) (+)= slots 0 .. nd-1, then S .. S+nd-1, in that order; the last launch writes
// out(i, r) = variance * sum + s2 * v(i, r)
template <typename T>
__global__ __launch_bounds__(256) void kxx_reduce_kernel(const T* __restrict__ slots, long slot_stride, int S, int nd,
                                                         T* __restrict__ sum, int first, int last, long N, int RC,
                                                         double variance, double s2, const T* __restrict__ V, long v_si,
                                                         long v_sr, T* __restrict__ out, long o_si, long o_sr,
                                                         const int* __restrict__ gate) {
  if (gate != nullptr && *gate == 0) return;
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= N * RC) return;
  T s = first ? (T)0 : sum[e];
  for (int k = 0; k < nd; ++k) s += slots[k * slot_stride + e];
  for (int k = 0; k < nd; ++k) s += slots[(S + k) * slot_stride + e];
  if (!last) {
    sum[e] = s;
    return;
  }
  const long i = e / RC, r = e - i * RC;
  out[i * o_si + r * o_sr] = mgp_fma((T)s2, V[i * v_si + r * v_sr], (T)variance * s);
}

struct KxxPlan {
  long TB, nbk, npad, nd_total;
  int S;
};

inline KxxPlan kxx_plan(long N, int TB, int RC) {
  KxxPlan p;
  p.TB = TB;
  p.nbk = (N + TB - 1) / TB;
  p.npad = p.nbk * TB;
  p.nd_total = p.nbk / 2 + 1;
  long s = (long)(kKxxSlotBudget / ((size_t)2 * p.npad * RC * sizeof(double)));
  s = s < 1 ? 1 : s;
  p.S = (int)(s < p.nd_total ? s : p.nd_total);
  return p;
}

// scratch of the product: bmax word | packed set [N' (DP+1)] | weights [N' RCmax] | running sum [N' RCmax] | 2 S
// slots [npad RC] (N' = N rounded up to 1024, RCmax the widest column group of the call)
inline size_t kxx_slot_bytes(const KxxPlan& pl, int RC) { return (size_t)2 * pl.S * pl.npad * RC * sizeof(double); }

template <int DP, int KIND, int RC>
int kxx_group(mgp_handle* h, const SweepParams& prm, const double* P, long N, const double* V,
              long v_si, long v_sr, double* out, long o_si, long o_sr, double s2, double* Wt, double* sum,
              double* slots, const unsigned long long* bmax, const int* gate) {
  const KxxPlan pl = kxx_plan(N, KxxCfg<DP, RC>::TB, RC);
  hipLaunchKernelGGL((kxx_weights_kernel<double>), dim3((unsigned)((pl.npad * RC + 255) / 256)), dim3(256), 0,
                     h->stream, V, v_si, v_sr, N, pl.npad, RC, Wt, gate);
  MGP_LAUNCH_CHECK(h);
    const long slot_stride = pl.npad * RC;
  for (long d0 = 0; d0 < pl.nd_total; d0 += pl.S) {
    const long nd = pl.nd_total - d0 < pl.S ? pl.nd_total - d0 : pl.S;
    if (pl.nbk * nd > 2147483647L) return mgp_fail(h, MGP_E_SHAPE, "kxx: grid too large");
    hipLaunchKernelGGL((kxx_tile_kernel<DP, KIND, RC>), dim3((unsigned)(pl.nbk * nd)), dim3(kKxxThreads), 0,
                       h->stream, P, Wt, pl.nbk, d0, slots, slot_stride, pl.S, bmax, prm,
                       (const double*)h->e2tabs + 8192, gate);
    MGP_LAUNCH_CHECK(h);
    const int last = d0 + nd >= pl.nd_total;
    hipLaunchKernelGGL((kxx_reduce_kernel<double>), dim3((unsigned)((N * RC + 255) / 256)), dim3(256), 0, h->stream,
                       slots, slot_stride, pl.S, (int)nd, sum, (int)(d0 == 0), last, N, RC, prm.variance, s2, V, v_si,
                       v_sr, out, o_si, o_sr, gate);
    MGP_LAUNCH_CHECK(h);
  }
  return MGP_OK;
}

template <int DP, int KIND>
int kxx_dp(mgp_handle* h, const mgp_kernel* k, const double* X, long N, double s2, VecView V, int R, VecViewMut out,
           const int* gate) {
  const SweepParams prm = mgp_make_params(k);
  const long npad_all = (N + kKxxPad - 1) / kKxxPad * kKxxPad;
  // one reservation for every column group of the call (R = 8 a + 4 b + 2 c + d, as the fast sweep groups them)
  const int rcmax = R >= 8 ? 8 : (R >= 4 ? 4 : (R >= 2 ? 2 : 1));
  size_t slot_need = 0;
  {
    const size_t sb[4] = {kxx_slot_bytes(kxx_plan(N, KxxCfg<DP, 8>::TB, 8), 8),
                          kxx_slot_bytes(kxx_plan(N, KxxCfg<DP, 4>::TB, 4), 4),
                          kxx_slot_bytes(kxx_plan(N, KxxCfg<DP, 2>::TB, 2), 2),
                          kxx_slot_bytes(kxx_plan(N, KxxCfg<DP, 1>::TB, 1), 1)};
    const int rcs[4] = {8, 4, 2, 1};
    int left = R;
    for (int g = 0; g < 4; ++g)
      if (left >= rcs[g]) {
        slot_need = sb[g] > slot_need ? sb[g] : slot_need;
        left %= rcs[g];
      }
  }
  const size_t need = 256 + (size_t)npad_all * (DP + 1) * 8 + (size_t)2 * npad_all * rcmax * 8 + slot_need;
  MGP_TRY(mgp_reserve(h, &h->kxx, &h->kxx_bytes, need));
  char* base = (char*)h->kxx;
  unsigned long long* bmax = (unsigned long long*)base;
  double* P = (double*)(base + 256);
  double* Wt = P + npad_all * (DP + 1);
  double* sum = Wt + npad_all * rcmax;
  double* slots = sum + npad_all * rcmax;
  MGP_HIP(h, hipMemsetAsync(bmax, 0, 8, h->stream));
  hipLaunchKernelGGL((kxx_pack_kernel<DP>), dim3((unsigned)(npad_all / 256)), dim3(256), 0, h->stream, X, N, npad_all,
                     k->D, prm, P, bmax, gate);
  MGP_LAUNCH_CHECK(h);
  int r0 = 0;
  while (r0 < R) {
    const int left = R - r0;
    const double* Vr = (const double*)V.base + (long)r0 * V.sr;
    double* outr = (double*)out.base + (long)r0 * out.sr;
#define MGP_KXX_GROUP(RCV) \
  kxx_group<DP, KIND, RCV>(h, prm, P, N, Vr, V.si, V.sr, outr, out.si, out.sr, s2, Wt, sum, slots, bmax, gate)
    int rc;
    if (left >= 8) {
      rc = 8;
      MGP_TRY(MGP_KXX_GROUP(8));
    } else if (left >= 4) {
      rc = 4;
      MGP_TRY(MGP_KXX_GROUP(4));
    } else if (left >= 2) {
      rc = 2;
      MGP_TRY(MGP_KXX_GROUP(2));
    } else {
      rc = 1;
      MGP_TRY(MGP_KXX_GROUP(1));
    }
#undef MGP_KXX_GROUP
    r0 += rc;
  }
  return MGP_OK;
}

}  // namespace

// Dispatch (measured): the symmetric form serves ONE right-hand side, fp64, D <= MGP_FUSED_MAX_D, from
// kxx_min_n rows on.  Below that too few tiles fill the chip (the plain sweep splits its streamed set); with several
// columns the row sums cost 12 RC / RPT VALU instructions per pair and the multi-column sweep is 1.7-1.9x faster.
// Those cases, fp32 and D > 32 take the sweep (mgp_sweep(X, X) with s2 V as its addend).  MGP_KXX=sym / plain force
// one form (A/B runs, tests).
int mgp_kxx(mgp_handle* h, const mgp_kernel* k, const void* X, int64_t N, double s2, VecView V, int32_t R,
            VecViewMut out, const int* gate) {
  MGP_TRY(mgp_check_kernel(h, k));
  if (N < 0 || R < 0) return mgp_fail(h, MGP_E_SHAPE, "negative size");
  if (N == 0 || R == 0) return MGP_OK;
  if (!X || !V.base || !out.base) return mgp_fail(h, MGP_E_BADARG, "NULL data pointer");
  if (!(s2 >= 0.0)) return mgp_fail(h, MGP_E_BADARG, "s2 must be >= 0");
  const bool sym = k->dtype == MGP_F64 && k->D <= MGP_FUSED_MAX_D &&
                   (h->kxx_mode == 1 || (h->kxx_mode == 0 && R == 1 && N >= h->kxx_min_n));
  if (!sym) return mgp_sweep(h, k, X, N, X, N, V, R, out, s2, V, gate);
  const double* Xd = (const double*)X;
  return mgp_with_kind(k->kind, [&](auto kind) {
    return mgp_with_dp<4>(k->D, [&](auto dp) {
      return kxx_dp<decltype(dp)::value, decltype(kind)::value>(h, k, Xd, N, s2, V, R, out, gate);
    });
  });
}

extern "C" int mgp_kxx_matvec(mgp_handle* h, const mgp_kernel* k, const void* X, int64_t N, double s2, const void* V,
                              int32_t R, int v_layout, void* out, int out_layout) {
  if (!h) return MGP_E_BADARG;
  if ((v_layout != MGP_COLS && v_layout != MGP_ROWS) || (out_layout != MGP_COLS && out_layout != MGP_ROWS))
    return mgp_fail(h, MGP_E_BADARG, "bad layout");
  return mgp_kxx(h, k, X, N, s2, mgp_view(V, N, R, v_layout), R, mgp_view_mut(out, N, R, out_layout), nullptr);
}
