// rff_anyd.hip -- the random-Fourier-feature prior sample and its backward pass at MGP_FUSED_MAX_D < D <= MGP_MAX_D,
// fp64, 1 <= S <= 8 (MGP_RFF_ANYD on mgp_rff_sample / mgp_rff_sample_vjp, include/mgp_pathwise.h): no [N, 2L] feature
// panel in memory.  rff.hip and rff_grad.hip only dispatch to this file.
//
// Phases: a 16 x 16 tile of t = sum_d x_d theta'_d (revolutions, theta' = theta / (2 pi) formed once per call) comes
// out of v_mfma_f64_16x16x4_f64.  Both point sets are packed per call in MFMA fragment order,
//     frag[(tile * KS + ks) * 64 + kq * 16 + l] = coordinate 4 ks + kq of point 16 tile + l,   KS = ceil(D / 4),
// zero padded to K = 4 KS columns and to whole tiles, so that a k-step of a tile is one 512-byte run.  K is walked in
// slices of kSL k-steps, k ascending, one accumulator per pair; the streamed side (A operand, tile rows) is copied flat
// into LDS, the owned side (B operand, tile columns) is loaded by every lane as its own operand.  A phase is a plain dot
// product: no K augmentation.  rff_sincos_rev (rff_math.h) turns it into sin / cos, as on every other route.
//
// Contraction: the result register v of lane l holds tile row (l >> 4) + 4 v, column l & 15 -- the B-operand map
// (k = l >> 4, column l & 15) for tile rows 4 v .. 4 v + 3 (kmm_wide_anyd.hip) -- so a tile goes back in as a B operand
// with no LDS round trip.  A workgroup of four waves owns 64 points (one 16-column tile per wave) and streams the other
// side in tiles of 16:
//  - forward (owned rows n, streamed bases l):  out^T[s, n] += Wc^T[s, l] cos[l, n] + Ws^T[s, l] sin[l, n], S padded to
//    16 with exact zeros: eight instructions per tile;
//  - backward (one template, the two point sets exchanging roles):  a = sum_s G_s ws_s and b = sum_s G_s wc_s are two
//    small MFMA products over s (K = 4 or 8), q = cos a - sin b, then  out^T[d, i] += P^T[d, j] q[j, i]  with the
//    streamed points' raw coordinates P (X for dtheta, theta for dX) as the A operand, staged through LDS.  `scale` is
//    applied once at the end.
// A wave's output accumulator is NT tiles of four doubles per lane, NT the smallest of {3, 4, 5, 6, 8, 10, 12, 16} that
// covers the output dimensions (no condition in the loop; a padded tile multiplies zeros).  Up to 256 output dimensions
// fit (NT <= 16, the budget of kmm_wide_anyd_kernel); above, blockIdx.y takes the output dimensions in groups =
// ceil(D / 256) equal groups of 16 NT <= 256 and every group recomputes the phases.
//
// Padding: streamed slots past the end are exact zeros in every fragment, every weight and every raw coordinate
// (cos(0) * 0 = 0), owned slots past the end are zeros too and are never stored; nothing is read behind an array.
//
// Split and finish: when the owned side leaves CUs idle the streamed tiles are split over blockIdx.z (rff_anyd_plan
// below); every split writes its partial and a finish kernel adds them in split order and applies `scale`.  No float
// atomics: two calls give the same bits.  Everything is packed per call; nothing stays on the handle.
//
// Scratch: the gen arena alone, rff_anyd_bytes below (the formula of include/mgp_pathwise.h).
#include "../../include/mgp_pathwise.h"
#include "mgp_common.h"
#include "rff_math.h"

namespace {

using Acc4 = __attribute__((ext_vector_type(4))) double;

constexpr int kAThreads = 256;
constexpr int kAOwn = 64;    // owned points per workgroup: one 16-column tile per wave
constexpr int kSL = 8;       // k-steps of 4 per K slice
constexpr int kAGroup = 256; // most output dimensions per blockIdx.y of the backward pass
constexpr double kTwoPi = 6.283185307179586476925;

// frag[(tile * KS + ks) * 64 + kq * 16 + l] = P[16 tile + l, 4 ks + kq] (REV: / (2 pi)); zeros past cnt and past D
template <bool REV>
__global__ __launch_bounds__(256) void rff_anyd_pack_kernel(const double* __restrict__ P, long cnt, int D, int KS,
                                                            long total, double* __restrict__ frag) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int l = (int)(e & 15), kq = (int)((e >> 4) & 3);
  const long run = e >> 6, tile = run / KS;
  const int k = 4 * (int)(run - tile * KS) + kq;
  const long i = tile * 16 + l;
  double v = 0.0;
  if (i < cnt && k < D) v = REV ? P[i * D + k] / kTwoPi : P[i * D + k];
  frag[e] = v;
}

// backward weights of a point set, in fragment order over s (the A and the B map coincide):
//     wp[(tile * 4 + which * 2 + ks2) * 64 + kq * 16 + l] = A[i a_si + s a_ss + which a_sw],  i = 16 tile + l, s = 4 ks2 + kq
// rows: A = G, a_sw = 0 (both slots the cotangent); bases: A = W + L, a_si = 1, a_ss = 2 L, a_sw = -L (slot 0 the sin
// block, slot 1 the cos block).  Zeros past cnt and past S.
__global__ __launch_bounds__(256) void rff_anyd_pack_w_kernel(const double* __restrict__ A, long cnt, int S, long a_si,
                                                              long a_ss, long a_sw, long total,
                                                              double* __restrict__ wp) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int l = (int)(e & 15), kq = (int)((e >> 4) & 3), ks2 = (int)((e >> 6) & 1), which = (int)((e >> 7) & 1);
  const long i = (e >> 8) * 16 + l;
  const int s = 4 * ks2 + kq;
  wp[e] = (i < cnt && s < S) ? A[i * a_si + s * a_ss + which * a_sw] : 0.0;
}

// forward weights of the bases, as A operands of the contraction over four bases:
//     wf[((tile * 2 + which) * 4 + v) * 64 + kq * 16 + s] = W[s, which L + 16 tile + 4 v + kq];  zeros past L and past S
__global__ __launch_bounds__(256) void rff_anyd_pack_wf_kernel(const double* __restrict__ W, long L, int S, long total,
                                                               double* __restrict__ wf) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int s = (int)(e & 15), kq = (int)((e >> 4) & 3), v = (int)((e >> 6) & 3), which = (int)((e >> 8) & 1);
  const long b = (e >> 9) * 16 + 4 * v + kq;
  wf[e] = (b < L && s < S) ? W[(long)s * 2 * L + which * L + b] : 0.0;
}

// VJP = false: the forward.  ofrag = rows, sfrag = bases, sw = rff_anyd_pack_wf_kernel's, C = S; out element (n, s) at
// out[n o_so + s o_sc].  VJP = true: ow / sw = rff_anyd_pack_w_kernel's of the owned / streamed set, sraw [NS, D] the
// streamed set's raw coordinates, C = D; out element (o, d) at out[o D + d].  NT = output tiles a wave holds.
// Output element (o, c) at out[o o_so + c o_sc] (backward: o_so = D, o_sc = 1).
// part == nullptr: out = mul * acc; otherwise part[(blockIdx.z * NO + o) * PW + c] = acc.
template <bool VJP, int NT>
__global__ __launch_bounds__(kAThreads, NT <= 8 ? 2 : 1) void rff_anyd_kernel(const double* __restrict__ ofrag,
                                                             const double* __restrict__ sfrag,
                                                             const double* __restrict__ ow,
                                                             const double* __restrict__ sw,
                                                             const double* __restrict__ sraw, long NO, long NS, int KS,
                                                             int D, int C, int S, long tps, double mul,
                                                             double* __restrict__ out, long o_so, long o_sc,
                                                             double* __restrict__ part, int PW) {
  constexpr int WN = VJP ? 4 : 8;      // 64-element weight runs per streamed tile
  constexpr int RS = 16 * NT + 16;     // row stride of the raw panel
  __shared__ __attribute__((aligned(16))) double frag[kSL * 64];  // one K slice of the streamed tile
  __shared__ __attribute__((aligned(16))) double wts[WN * 64];
  __shared__ __attribute__((aligned(16))) double raws[VJP ? 16 * RS : 1];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int l15 = lane & 15, kq = lane >> 4;

  const long otiles = (NO + 15) >> 4, stiles = (NS + 15) >> 4;
  const long ot = (long)blockIdx.x * 4 + wave;  // this wave's owned tile; one wholly past NO computes on tile 0, stores nothing
  const double* own = ofrag + (ot < otiles ? ot : 0L) * KS * 64;
  const int d0 = VJP ? (int)blockIdx.y * 16 * NT : 0;  // first output dimension of this group
  const long t_begin = (long)blockIdx.z * tps;
  const long t_end = t_begin + tps < stiles ? t_begin + tps : stiles;

  double oa[2] = {0.0, 0.0}, ob[2] = {0.0, 0.0};  // owned weights: B operands of a and b
  if (VJP) {
    const double* w = ow + (ot < otiles ? ot : 0L) * 256;
    oa[0] = w[lane], oa[1] = w[64 + lane], ob[0] = w[128 + lane], ob[1] = w[192 + lane];
  }
  const bool s_hi = VJP && S > 4;  // a second k-step over s

  Acc4 acc[NT];
#pragma unroll
  for (int q = 0; q < NT; ++q) acc[q] = Acc4{0, 0, 0, 0};

#pragma unroll 1
  for (long ti = t_begin; ti < t_end; ++ti) {
    Acc4 c = Acc4{0, 0, 0, 0};
#pragma unroll 1
    for (int s0 = 0; s0 < KS; s0 += kSL) {
      const int nks = KS - s0 < kSL ? KS - s0 : kSL;
      double bf[kSL];
#pragma unroll
      for (int ks = 0; ks < kSL; ++ks) bf[ks] = ks < nks ? own[(long)(s0 + ks) * 64 + lane] : 0.0;
      __syncthreads();  // the previous slice's fragments, and the previous tile's weights and raw panel, fully consumed
      for (int e = t; e < nks * 64; e += kAThreads) frag[e] = sfrag[(ti * KS + s0) * 64 + e];
      if (s0 == 0) {
        for (int e = t; e < WN * 64; e += kAThreads) wts[e] = sw[ti * (WN * 64) + e];
        if (VJP) {
          constexpr int w = 16 * NT;
#pragma unroll 1
          for (int e = t; e < 16 * w; e += kAThreads) {
            const int r = e / w, cd = e - r * w;
            const long p = ti * 16 + r;
            raws[r * RS + cd] = (p < NS && d0 + cd < D) ? sraw[p * D + d0 + cd] : 0.0;
          }
        }
      }
      __syncthreads();
#pragma unroll
      for (int ks = 0; ks < kSL; ++ks)
        if (ks < nks) c = __builtin_amdgcn_mfma_f64_16x16x4f64(frag[ks * 64 + lane], bf[ks], c, 0, 0, 0);
    }

    double sn[4], cs[4];
#pragma unroll
    for (int v = 0; v < 4; ++v) rff_sincos_rev(c[v], sn[v], cs[v]);

    if (!VJP) {
#pragma unroll
      for (int v = 0; v < 4; ++v) {  // bases 4 v .. 4 v + 3 of the tile, ascending: cos block, then sin block
        acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(wts[v * 64 + lane], cs[v], acc[0], 0, 0, 0);
        acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(wts[(4 + v) * 64 + lane], sn[v], acc[0], 0, 0, 0);
      }
    } else {
      Acc4 a = __builtin_amdgcn_mfma_f64_16x16x4f64(wts[lane], oa[0], Acc4{0, 0, 0, 0}, 0, 0, 0);
      Acc4 b = __builtin_amdgcn_mfma_f64_16x16x4f64(wts[128 + lane], ob[0], Acc4{0, 0, 0, 0}, 0, 0, 0);
      if (s_hi) {  // S > 4: the second k-step over s (wave-uniform)
        a = __builtin_amdgcn_mfma_f64_16x16x4f64(wts[64 + lane], oa[1], a, 0, 0, 0);
        b = __builtin_amdgcn_mfma_f64_16x16x4f64(wts[192 + lane], ob[1], b, 0, 0, 0);
      }
      double q[4];
#pragma unroll
      for (int v = 0; v < 4; ++v) q[v] = mgp_fma(a[v], cs[v], -(b[v] * sn[v]));
      const double* prow = &raws[kq * RS + l15];
#pragma unroll
      for (int qd = 0; qd < NT; ++qd)
#pragma unroll
        for (int v = 0; v < 4; ++v)  // streamed points 4 v .. 4 v + 3 of the tile, ascending
          acc[qd] = __builtin_amdgcn_mfma_f64_16x16x4f64(prow[4 * v * RS + qd * 16], q[v], acc[qd], 0, 0, 0);
    }
  }

  // result register v of lane l: output row (s, or dimension 16 qd + ...) (l >> 4) + 4 v, owned point l & 15
  const long o = ot * 16 + l15;
  if (o >= NO) return;
  double* dst = part != nullptr ? part + ((long)blockIdx.z * NO + o) * PW : out + o * o_so;
  const long stride = part != nullptr ? 1 : o_sc;
  const double m = part != nullptr ? 1.0 : mul;
#pragma unroll
  for (int qd = 0; qd < NT; ++qd)
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int cc = d0 + 16 * qd + kq + 4 * v;
      if (cc < C) dst[cc * stride] = m * acc[qd][v];
    }
}

// out(o, c) = mul * sum_z part[(z NO + o) PW + c], splits in ascending order
__global__ __launch_bounds__(256) void rff_anyd_finish_kernel(const double* __restrict__ part, int nsplit, long NO,
                                                              int PW, int C, double mul, double* __restrict__ out,
                                                              long o_so, long o_sc) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= NO * C) return;
  const long o = e / C;
  const int c = (int)(e - o * C);
  double v = 0.0;
  for (int z = 0; z < nsplit; ++z) v += part[((long)z * NO + o) * PW + c];
  out[o * o_so + c * o_sc] = mul * v;
}

struct RffAnydPlan {
  long nblk, nsplit, tps;
};

// split of the streamed side: about two workgroups per CU, at most one split per 16 streamed tiles (256 points) and at
// most 256 splits; tps = streamed tiles per split
RffAnydPlan rff_anyd_plan(long owned, long streamed, int groups, int num_cus) {
  RffAnydPlan p;
  p.nblk = (owned + kAOwn - 1) / kAOwn;
  const long wg = p.nblk * groups;
  const long stiles = (streamed + 15) / 16;
  long ns = 1;
  if (wg < 2L * num_cus) {
    ns = (2L * num_cus + wg - 1) / wg;
    const long cap = (stiles + 15) / 16;
    if (ns > cap) ns = cap;
    if (ns > 256) ns = 256;
    if (ns < 1) ns = 1;
  }
  p.tps = (stiles + ns - 1) / ns;
  p.nsplit = (stiles + p.tps - 1) / p.tps;
  return p;
}

inline size_t a256(size_t b) { return (b + 255) & ~(size_t)255; }
inline int rff_anyd_ks(int D) { return (D + 3) >> 2; }
inline int rff_anyd_groups(int D) { return (D + kAGroup - 1) / kAGroup; }
// output tiles a wave holds: the 16-wide tiles of D shared evenly among the groups, rounded up the ladder
inline int rff_anyd_nt(int D) {
  const int groups = rff_anyd_groups(D), per = ((D + 15) / 16 + groups - 1) / groups;
  for (int nt : {3, 4, 5, 6, 8, 10, 12}) if (per <= nt) return nt;
  return 16;
}

// scratch of one pass: both fragment packs, the weights, and (nsplit > 1) the partials
size_t rff_anyd_bytes(const mgp_handle* h, long owned, long streamed, int D, bool vjp) {
  const size_t To = (size_t)(owned + 15) / 16, Ts = (size_t)(streamed + 15) / 16, KS = (size_t)rff_anyd_ks(D);
  const RffAnydPlan pl = rff_anyd_plan(owned, streamed, vjp ? rff_anyd_groups(D) : 1, h->num_cus);
  const size_t PW = vjp ? (size_t)(D + 15) / 16 * 16 : 8;
  size_t b = a256(512 * KS * To) + a256(512 * KS * Ts);
  b += vjp ? a256(2048 * To) + a256(2048 * Ts) : a256(4096 * Ts);
  if (pl.nsplit > 1) b += a256(8 * (size_t)pl.nsplit * owned * PW);
  return b;
}

template <bool REV>
int pack_points(mgp_handle* h, const double* P, long cnt, int D, double* frag) {
  const int KS = rff_anyd_ks(D);
  const long total = (cnt + 15) / 16 * KS * 64;
  hipLaunchKernelGGL((rff_anyd_pack_kernel<REV>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, h->stream, P, cnt,
                     D, KS, total, frag);
  MGP_LAUNCH_CHECK(h);
  return MGP_OK;
}

int pack_w(mgp_handle* h, const double* A, long cnt, int S, long a_si, long a_ss, long a_sw, double* wp) {
  const long total = (cnt + 15) / 16 * 256;
  hipLaunchKernelGGL(rff_anyd_pack_w_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, h->stream, A, cnt, S,
                     a_si, a_ss, a_sw, total, wp);
  MGP_LAUNCH_CHECK(h);
  return MGP_OK;
}

int plan_check(mgp_handle* h, const RffAnydPlan& pl, long owned, long streamed) {
  if (pl.nblk > 2147483647L || pl.nsplit > 65535 || owned > (1L << 40) || streamed > (1L << 40))
    return mgp_fail(h, MGP_E_SHAPE, "rff any-D route: grid too large");
  return MGP_OK;
}

// one backward output.  rows_owned: dX (owned rows X with G, streamed bases theta with W); otherwise dtheta.
int vjp_pass(mgp_handle* h, bool rows_owned, const double* X, long N, int D, const double* theta, long L,
             const double* W, int S, double scale, const double* G, long g_sn, long g_ss, double* out) {
  const long NO = rows_owned ? N : L, NS = rows_owned ? L : N;
  const int KS = rff_anyd_ks(D), groups = rff_anyd_groups(D), PW = (D + 15) / 16 * 16;
  const RffAnydPlan pl = rff_anyd_plan(NO, NS, groups, h->num_cus);
  MGP_TRY(plan_check(h, pl, NO, NS));
  const size_t To = (size_t)(NO + 15) / 16, Ts = (size_t)(NS + 15) / 16;
  char* base = (char*)h->gen;
  double* ofrag = (double*)base;
  double* sfrag = (double*)(base += a256(512 * (size_t)KS * To));
  double* owp = (double*)(base += a256(512 * (size_t)KS * Ts));
  double* swp = (double*)(base += a256(2048 * To));
  double* part = pl.nsplit > 1 ? (double*)(base += a256(2048 * Ts)) : nullptr;
  double* xf = rows_owned ? ofrag : sfrag;
  double* tf = rows_owned ? sfrag : ofrag;
  MGP_TRY(pack_points<false>(h, X, N, D, xf));
  MGP_TRY(pack_points<true>(h, theta, L, D, tf));
  MGP_TRY(pack_w(h, G, N, S, g_sn, g_ss, 0, rows_owned ? owp : swp));
  MGP_TRY(pack_w(h, W + L, L, S, 1, 2 * L, -L, rows_owned ? swp : owp));
  const double* sraw = rows_owned ? theta : X;
  dim3 grid((unsigned)pl.nblk, (unsigned)groups, (unsigned)pl.nsplit);
  const int nt = rff_anyd_nt(D);
#define MGP_RA(NTV)                                                                                                  \
  hipLaunchKernelGGL((rff_anyd_kernel<true, NTV>), grid, dim3(kAThreads), 0, h->stream, (const double*)ofrag,         \
                     (const double*)sfrag, (const double*)owp, (const double*)swp, sraw, NO, NS, KS, D, D, S, pl.tps, \
                     scale, out, (long)D, 1L, part, PW)
  switch (nt) {
    case 3: MGP_RA(3); break;
    case 4: MGP_RA(4); break;
    case 5: MGP_RA(5); break;
    case 6: MGP_RA(6); break;
    case 8: MGP_RA(8); break;
    case 10: MGP_RA(10); break;
    case 12: MGP_RA(12); break;
    default: MGP_RA(16); break;
  }
#undef MGP_RA
  MGP_LAUNCH_CHECK(h);
  if (part != nullptr) {
    const long tot = NO * D;
    hipLaunchKernelGGL(rff_anyd_finish_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, h->stream,
                       (const double*)part, (int)pl.nsplit, NO, PW, D, scale, out, (long)D, 1L);
    MGP_LAUNCH_CHECK(h);
  }
  return MGP_OK;
}

}  // namespace

bool mgp_rff_anyd_serves(int dtype, int D, int S) {
  return dtype == MGP_F64 && D > MGP_FUSED_MAX_D && D <= MGP_MAX_D && S >= 1 && S <= 8;
}

int mgp_rff_anyd_sample(mgp_handle* h, const double* X, long N, int D, const double* theta, long L, const double* W,
                        int S, double scale, double* out, int layout) {
  const int KS = rff_anyd_ks(D);
  const RffAnydPlan pl = rff_anyd_plan(N, L, 1, h->num_cus);
  MGP_TRY(plan_check(h, pl, N, L));
  MGP_TRY(mgp_reserve(h, &h->gen, &h->gen_bytes, rff_anyd_bytes(h, N, L, D, false)));
  const size_t To = (size_t)(N + 15) / 16, Ts = (size_t)(L + 15) / 16;
  char* base = (char*)h->gen;
  double* ofrag = (double*)base;
  double* sfrag = (double*)(base += a256(512 * (size_t)KS * To));
  double* wf = (double*)(base += a256(512 * (size_t)KS * Ts));
  double* part = pl.nsplit > 1 ? (double*)(base += a256(4096 * Ts)) : nullptr;
  MGP_TRY(pack_points<false>(h, X, N, D, ofrag));
  MGP_TRY(pack_points<true>(h, theta, L, D, sfrag));
  const long wtot = (long)Ts * 512;
  hipLaunchKernelGGL(rff_anyd_pack_wf_kernel, dim3((unsigned)((wtot + 255) / 256)), dim3(256), 0, h->stream, W, L, S,
                     wtot, wf);
  MGP_LAUNCH_CHECK(h);
  const long o_sn = layout == MGP_COLS ? S : 1, o_ss = layout == MGP_COLS ? 1 : N;
  hipLaunchKernelGGL((rff_anyd_kernel<false, 1>), dim3((unsigned)pl.nblk, 1, (unsigned)pl.nsplit), dim3(kAThreads), 0,
                     h->stream, (const double*)ofrag, (const double*)sfrag, (const double*)nullptr, (const double*)wf,
                     (const double*)nullptr, N, L, KS, D, S, S, pl.tps, scale, out, o_sn, o_ss, part, 8);
  MGP_LAUNCH_CHECK(h);
  if (part != nullptr) {
    const long tot = N * S;
    hipLaunchKernelGGL(rff_anyd_finish_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, h->stream,
                       (const double*)part, (int)pl.nsplit, N, 8, S, scale, out, o_sn, o_ss);
    MGP_LAUNCH_CHECK(h);
  }
  return MGP_OK;
}

int mgp_rff_anyd_vjp(mgp_handle* h, const double* X, long N, int D, const double* theta, long L, const double* W, int S,
                     double scale, const double* G, long g_sn, long g_ss, double* dtheta, double* dX) {
  // one reservation for both passes: a fixed pool hands out a fresh region at every growth
  size_t need = 0;
  if (dtheta) need = rff_anyd_bytes(h, L, N, D, true);
  if (dX) {
    const size_t b = rff_anyd_bytes(h, N, L, D, true);
    if (b > need) need = b;
  }
  MGP_TRY(mgp_reserve(h, &h->gen, &h->gen_bytes, need));
  if (dtheta) MGP_TRY(vjp_pass(h, false, X, N, D, theta, L, W, S, scale, G, g_sn, g_ss, dtheta));
  if (dX) MGP_TRY(vjp_pass(h, true, X, N, D, theta, L, W, S, scale, G, g_sn, g_ss, dX));
  return MGP_OK;
}
